"""-m gpu: the problem classes on the signal spectral ratios (difflexmm_amd/problems.py: TargetSpectrum, TargetTransmission,
TargetHarmonicRatio, TransmissionLimit; DriveWaveformDesign with an objective.SpectrumSpec) on the quads 6x6 of
test_gpu_signal_projection.py's TargetBandPower case: directional derivatives against central differences at that case's bar (relative
step 1e-6, 1e-6), one design with on_device=True against member 0 of a list (1e-13), the host path against the device path (1e-12), a
longer list in chunks with per-member offsets, TransmissionLimit as a state constraint of run_optimization_nlopt for two evaluations; the
sample gradient of a DriveWaveformDesign on a SpectrumSpec against a central difference (the set-up and the 1e-6 bar of
test_gpu_waveform.py's design case)."""
import math

import numpy as np
import pytest

from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from .test_gpu_objective import FOCUS_KW
from .test_gpu_signal_projection import _forward

pytestmark = pytest.mark.gpu

IN, OUT = [(13, 0), (19, 0)], [(16, 0), (22, 0), (21, 2)]
FREQS = [FOCUS_KW["loading_rate"], 1100.0, 1900.0]


def _designs(fw, rng):
    base = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    return base, [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]


@pytest.mark.parametrize("worst_case", [False, True])
def test_target_transmission(hip_lib, worst_case):
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(23)
    base, designs = _designs(fw1, rng)
    probe = P.TargetTransmission(fw3, IN, OUT, "velocity", FREQS, window="hann")
    probe.value(designs)
    spread = np.ptp(probe.last_measures, axis=1)
    beta = float(np.sqrt(200.0 / (spread.min() * spread.max())))
    assert (5.0 <= beta * spread).all() and (beta * spread <= 40.0).all(), beta * spread
    many = P.TargetTransmission(fw3, IN, OUT, "velocity", FREQS, window="hann", worst_case=worst_case, beta=beta)
    sp = many.spec
    assert isinstance(many, P.TargetSpectrum) and sp.n_groups == 3 and sp.basis.shape == (6, 7) and sp.measure == "log"
    assert sp.aggregate == ("ks" if worst_case else "sum") and np.array_equal(sp.group_coef, np.ones(3) if worst_case else np.full(3, 1 / 3))
    assert np.array_equal(sp.basis, O.fourier_basis(fw3.timepoints, FREQS, "hann"))
    assert np.array_equal(sp.num_weights[1, :, 2:4], [[0, 0], [0, 0], [1, 1], [1, 1], [1, 1]]) and np.array_equal(sp.den_weights[1, :, 2:4], [[1, 1], [1, 1], [0, 0], [0, 0], [0, 0]])
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and np.isfinite(v).all() and many.last_measures.shape == (3, 3)
    assert np.allclose(many.value(designs), v, rtol=1e-13, atol=0.0)
    if not worst_case:
        assert np.allclose(v, many.last_measures.mean(1), rtol=1e-13)
    else:
        assert (v >= many.last_measures.max(1)).all() and (v <= many.last_measures.max(1) + math.log(3) / beta).all()
    scale = max(np.abs(a).max() for a in base)
    for trial in range(2):
        dirs = [tuple(rng.normal(size=a.shape) for a in base) for _ in range(3)]
        dirs = [tuple(a / max(np.abs(x).max() for x in d) for a in d) for d in dirs]
        h = 1e-6 * scale
        vp = many.value([tuple(a + h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        vm = many.value([tuple(a - h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        fd = (vp - vm) / (2 * h)
        mine = np.array([sum(float(np.sum(a * e)) for a, e in zip(gm, dd)) for gm, dd in zip(g, dirs)])
        err = np.abs(mine - fd) / np.abs(fd)
        print(f"[signal spectrum] TargetTransmission worst_case={worst_case}, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.TargetTransmission(fw1, IN, OUT, "velocity", FREQS, window="hann", worst_case=worst_case, beta=beta)
    v1, g1 = single.value_and_grad(designs[0], on_device=True)
    e_v = abs(v1 - v[0]) / np.abs(many.last_measures[0]).sum()
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[signal spectrum] TargetTransmission, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13 and single.last_measures.shape == (3,)
    vh, gh = single.value_and_grad(designs[0])
    e_v = abs(vh - v1) / np.abs(single.last_measures).sum()
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(gh, g1))
    print(f"[signal spectrum] TargetTransmission, host path against device path: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert e_v <= 1e-12 and e_g <= 1e-12


def test_chunks_offsets_harmonic_ratio_and_the_constraint(hip_lib):
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(29)
    base, designs = _designs(fw1, rng)
    many = P.TargetTransmission(fw3, IN, OUT, "velocity", FREQS, window="hann")
    # a longer list runs in chunks of the ensemble width; per-member offsets are cut alike
    d0 = rng.uniform(0.5, 2.0, (6, 3)) * 1e-9
    chunked = P.TargetSpectrum(fw3, many.spec.with_offsets(None, d0))
    v6 = chunked.value(designs + designs[::-1])
    halves = [P.TargetSpectrum(fw3, many.spec.with_offsets(None, d0[k:k + 3])).value(d) for k, d in ((0, designs), (3, designs[::-1]))]
    assert v6.shape == (6,) and np.array_equal(v6, np.concatenate(halves)) and not np.array_equal(v6[:3], many.value(designs))
    with pytest.raises(ValueError, match="designs against offsets"):
        chunked.value(designs)
    with pytest.raises(ValueError, match="force components are evaluated on the device only"):
        P.TargetSpectrum(fw1, O.SpectrumSpec(O.SignalSpec([(0, 14, 6, 1.0)], 1), many.spec.basis, np.ones((1, 1, 6)), np.ones((1, 1, 6)))).value_and_grad(designs[0])
    # harmonic generation: the power at 2 f over the power at f
    hr = P.TargetHarmonicRatio(fw1, OUT, "velocity", FOCUS_KW["loading_rate"], window="hann")
    vd, vh = hr.value(designs[0], on_device=True), hr.value(designs[0])
    assert hr.spec.n_groups == 1 and np.isfinite(vd) and abs(vd - vh) <= 1e-12 * (abs(vd) + 1.0)
    # the harmonic's rows (frequency index 1) in the numerator, the fundamental's (index 0) in the denominator, for every signal
    assert np.array_equal(hr.spec.num_weights, np.tile([0.0, 0.0, 1.0, 1.0], (1, 3, 1))) and np.array_equal(hr.spec.den_weights, np.tile([1.0, 1.0, 0.0, 0.0], (1, 3, 1)))
    assert np.array_equal(hr.spec.basis, O.fourier_basis(fw1.timepoints, [FOCUS_KW["loading_rate"], 2 * FOCUS_KW["loading_rate"]], "hann"))
    with pytest.raises(ValueError, match="harmonic"):
        P.TargetHarmonicRatio(fw1, OUT, "velocity", 1000.0, harmonic=1)
    # the constraint: dB against a limit, value and gradient scaled alike
    one = P.TargetTransmission(fw1, IN, OUT, "velocity", FREQS, window="hann", worst_case=True, beta=4.0)
    J, gJ = one.value_and_grad(designs[0])
    limit = P.TransmissionLimit(fw1, IN, OUT, "velocity", FREQS, limit_db=10.0 / math.log(10.0) * J - 1.0, window="hann", beta=4.0)
    c, gc = limit.value_and_grad(designs[0])
    assert abs(c - 1.0) <= 1e-12 and all(np.allclose(a, limit.DB * b, rtol=1e-13, atol=0) for a, b in zip(gc, gJ)) and abs(limit.value(designs[0]) - c) <= 1e-12
    fw = _forward(1)
    prob = P.OptimizationProblem(P.TargetKineticEnergy(fw, (2, 2), (2, 0)), name="transmission-limited")
    prob.run_optimization_nlopt(designs[0], 2, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0, min_edge_length=1.0, verbose=False,
                                state_constraints=[limit])
    state = prob.constraints_violation["state"]
    print(f"[signal spectrum] transmission-limited focusing, 2 evaluations: objective {prob.objective_values}, c {state}")
    assert len(prob.objective_values) == 2 and np.isfinite(state).all() and abs(state[0] - c) <= 1e-12


def test_drive_waveform_design_on_a_spectrum_spec(hip_lib):
    """The samples of a table drive as the design, the objective a SpectrumSpec (log, KS over two groups): value and measures are those of
    DynamicSolver.signal_spectrum_value on the same solve, the sample gradient matches a central difference at 1e-6."""
    from . import waveform_yardstick as wy
    p = wy.problem(None, "disp")
    s = p.solver
    pm = wy.member(p)
    sig = O.SignalSpec.fields_of([(5, 0), (6, 1), (10, 2)], kind="velocity")
    T = wy.TS[-1] - wy.TS[0]
    B = O.fourier_basis(wy.TS, [0.5 / T, 1.0 / T], window="hann")
    wn, wd = O.band_groups(3, 2, [[(1, 0), (2, 0)], [(1, 1), (2, 1)]], [[(0, 0)], [(0, 1)]])
    spec = O.SpectrumSpec(sig, B, wn, wd, None, None, [1.0, 0.8], "log", "ks", 4.0)
    design = P.DriveWaveformDesign(s, p.y0, wy.TS, p.cp(pm), wy.NAME, spec, steps_per_interval=wy.SPI)
    assert design.method == "signal_spectrum_value_and_raw"
    y = wy.VALUES.copy()
    v0, g = design.value_and_grad(y)
    J, l = s.signal_spectrum_value(spec)
    assert np.isfinite(v0) and v0 == J[0] and np.isfinite(l).all() and g.shape == y.shape and np.abs(g).max() > 0
    d = np.random.default_rng(53).normal(size=y.shape)
    eps = 1e-6
    fd = (design.value_and_grad(y + eps * d)[0] - design.value_and_grad(y - eps * d)[0]) / (2 * eps)
    e = abs(float(g @ d) - fd) / abs(fd)
    print(f"[signal spectrum] DriveWaveformDesign on a SpectrumSpec: sample gradient against a central difference {e:.2e}")
    assert e < 1e-6, (float(g @ d), fd)
