"""No GPU: the host layers of the signal spectral ratios (difflexmm_amd/objective.py: SpectrumSpec, band_groups, spectrum_of_projections,
host_spectrum_value_and_cotangent; include/dfx.h: dfx_signal_spectrum*): argument checks, band_groups against a hand-written case, the host
twins against torch.autograd on the formulas of tests/spectrum_yardstick.py on a history of the CPU port, the closed forms (one group, one
row, "ratio" with d0 = 1 and Wd = 0 is twice the projection objective; "log" is invariant under a scaling of all signals), the NaN rule,
and the premise of the GPU cases' synthetic bases: on the CPU port's 70-output histories of both lattices every row of
test_gpu_signal_spectrum.SYNTHETIC_ROWS has kappa = sum_k |B_jk S_ks| / |P_sj| <= 25 for every member and signal (the GPU test asserts
<= 50 on its own history)."""
import functools

import numpy as np
import pytest
import torch

from difflexmm_amd import objective as O

from . import spectrum_yardstick as SY

T, NB = 23, 7
TERMS = [(0, 1, 0, 1.0), (0, 2, 4, -0.5), (1, 3, 2, 2.0), (2, 6, 5, 1e-2), (2, 1, 1, 0.25)]
SIG = O.SignalSpec(TERMS, 3)


def _weights(G=2, n_rows=4, seed=1):
    rng = np.random.default_rng(seed)
    wn, wd = rng.uniform(0.5, 2.0, (G, 3, n_rows)), rng.uniform(0.5, 2.0, (G, 3, n_rows))
    wn[:, :, 0] = 0.0
    wd[:, 1, :] = 0.0
    return rng.normal(size=(n_rows, T)), wn, wd


def test_spectrum_spec_checks_shapes_signs_and_finiteness():
    B, wn, wd = _weights()
    sp = O.SpectrumSpec(SIG, B, wn, wd)
    assert sp.n_groups == 2 and sp.n_rows == 4 and sp.measure == "log" and sp.aggregate == "sum" and np.array_equal(sp.group_coef, [1.0, 1.0])
    family, sig, args, kw = sp.engine_call()
    assert family == "signal_spectrum" and sig is SIG and len(args) == 3 and set(kw) == {"num_offset", "den_offset", "group_coef", "measure", "aggregate", "beta"}
    with pytest.raises(ValueError, match="n_rows >= 1"):
        O.SpectrumSpec(SIG, np.ones((0, T)), np.ones((1, 3, 0)), np.ones((1, 3, 0)))
    with pytest.raises(ValueError, match="targets of the signal spec have T"):
        O.SpectrumSpec(O.SignalSpec(TERMS, 3, np.zeros((T + 1, 3))), B, wn, wd)
    for bad in (np.ones((3, 4)), np.ones((0, 3, 4)), np.ones((2, 4, 3)), np.ones((1, 3, 4))):
        with pytest.raises(ValueError, match="num_weights and den_weights must be"):
            O.SpectrumSpec(SIG, B, bad, wd)
    with pytest.raises(ValueError, match="num_weights and den_weights must be"):
        O.SpectrumSpec(SIG, B, wn, wd[:1])
    for name, kw in (("basis", dict(basis=np.where(np.arange(T) == 3, np.nan, B))), ("num_weights", dict(num_weights=np.where(wn > 1, np.inf, wn))),
                     ("den_weights", dict(den_weights=np.where(wd > 1, np.nan, wd))), ("num_offset", dict(num_offset=[np.nan, 0.0])),
                     ("den_offset", dict(den_offset=[[1.0, np.inf]])), ("group_coef", dict(group_coef=[1.0, np.nan]))):
        with pytest.raises(ValueError, match=f"{name}: non-finite"):
            O.SpectrumSpec(**{**dict(signal_spec=SIG, basis=B, num_weights=wn, den_weights=wd), **kw})
    for name, kw in (("num_weights", dict(num_weights=-wn)), ("den_weights", dict(den_weights=-wd)), ("num_offset", dict(num_offset=[-1.0, 0.0])),
                     ("den_offset", dict(den_offset=[0.0, -1e-300]))):
        with pytest.raises(ValueError, match=f"{name}: negative"):
            O.SpectrumSpec(**{**dict(signal_spec=SIG, basis=B, num_weights=wn, den_weights=wd), **kw})
    for name in ("num_offset", "den_offset"):
        with pytest.raises(ValueError, match=f"{name} must be"):
            O.SpectrumSpec(SIG, B, wn, wd, **{name: np.ones(3)})
    with pytest.raises(ValueError, match="group_coef must be"):
        O.SpectrumSpec(SIG, B, wn, wd, group_coef=np.ones(3))
    with pytest.raises(ValueError, match="members"):
        O.SpectrumSpec(SIG, B, wn, wd, np.ones((3, 2)), np.ones((4, 2)))
    empty = wn.copy()
    empty[1] = 0.0
    with pytest.raises(ValueError, match=r"empty numerator.*\[1\]"):
        O.SpectrumSpec(SIG, B, empty, wd)
    with pytest.raises(ValueError, match=r"empty numerator.*\[1\]"):
        O.SpectrumSpec(SIG, B, empty, wd, num_offset=[[1.0, 1.0], [1.0, 0.0]])
    assert O.SpectrumSpec(SIG, B, empty, wd, num_offset=[0.0, 2.0]).num_offset[1] == 2.0
    with pytest.raises(ValueError, match="measure must be"):
        O.SpectrumSpec(SIG, B, wn, wd, measure="db")
    with pytest.raises(ValueError, match="aggregate must be"):
        O.SpectrumSpec(SIG, B, wn, wd, aggregate="max")
    for beta in (None, 0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="ks aggregate needs a finite beta > 0"):
            O.SpectrumSpec(SIG, B, wn, wd, aggregate="ks", beta=beta)
    per = sp.with_offsets(None, np.ones((5, 2)))
    assert per.den_offset.shape == (5, 2) and per.num_offset is None and np.array_equal(per.num_weights, wn)


def test_band_groups_against_a_hand_written_case():
    wn, wd = O.band_groups(3, 2, [[(2, 0)], [(1, 1), (2, 1)]], [[(0, 0), (0, 0)], []])
    ref_n, ref_d = np.zeros((2, 3, 4)), np.zeros((2, 3, 4))
    ref_n[0, 2, 0:2] = 1.0
    ref_n[1, 1, 2:4] = ref_n[1, 2, 2:4] = 1.0
    ref_d[0, 0, 0:2] = 1.0
    assert np.array_equal(wn, ref_n) and np.array_equal(wd, ref_d)
    with pytest.raises(ValueError, match="out of range"):
        O.band_groups(3, 2, [[(3, 0)]], [[(0, 0)]])
    with pytest.raises(ValueError, match="out of range"):
        O.band_groups(3, 2, [[(0, 0)]], [[(0, 2)]])
    with pytest.raises(ValueError, match="same number"):
        O.band_groups(3, 2, [[(0, 0)]], [])


def _torch_reference(sp, f):
    """J (batch,), l (batch, G), fields_bar by autograd on the yardstick's formulas"""
    ft = torch.tensor(f, requires_grad=True)
    cols = [None] * 3
    for s, b, c, coef in TERMS:
        src = coef * ft[..., c // 3, b, c % 3]
        cols[s] = src if cols[s] is None else cols[s] + src
    S = torch.stack(cols, dim=-1)
    Js, ls = [], []
    for m in range(f.shape[0]):
        n0 = np.zeros(sp.n_groups) if sp.num_offset is None else np.broadcast_to(sp.num_offset, (f.shape[0], sp.n_groups))[m]
        d0 = np.zeros(sp.n_groups) if sp.den_offset is None else np.broadcast_to(sp.den_offset, (f.shape[0], sp.n_groups))[m]
        _, N, D = SY.forms(S[m], sp.basis, sp.num_weights, sp.den_weights, n0, d0)
        l, J = SY.measure_and_value(N, D, sp.group_coef, sp.measure, sp.aggregate, sp.beta)
        Js.append(J)
        ls.append(l.detach().numpy())
    g, = torch.autograd.grad(torch.stack(Js).sum(), ft)
    return np.array([j.item() for j in Js]), np.stack(ls), g.numpy()


@pytest.fixture(scope="module")
def history(cpu_lib):
    """a 3-member history of the CPU port: quads 4x4 with damping, T outputs (three times the same design: the members differ by scale)"""
    from .common import Case
    c = Case("quads", 4, True, False, seed=3, lib=cpu_lib)
    f = np.array(c.solver(np.zeros((2, 16, 3)), np.linspace(0.0, 6e-4, T), c.cp._replace(constraint_params=dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)),
                          steps_per_interval=4))
    assert f.shape == (T, 2, 16, 3) and np.abs(f[:, :, :NB]).max() > 0
    return np.stack([f[:, :, :NB], 0.5 * f[:, :, :NB], -2.0 * f[:, :, :NB]])


@pytest.mark.parametrize("aggregate", ["sum", "ks"])
@pytest.mark.parametrize("measure", ["ratio", "log"])
@pytest.mark.parametrize("offsets", ["none", "shared", "per_member"])
def test_host_twins_are_autograd_of_the_formulas(history, measure, aggregate, offsets):
    f = history
    B, wn, wd = _weights(G=3, seed=4)
    B = O.fourier_basis(np.linspace(0.0, 6e-4, T), [3000.0, 1700.0])
    rng = np.random.default_rng(6)
    P2 = np.einsum("jk,mks->msj", B, O.host_signal_values(SIG, f)) ** 2
    scale = np.einsum("gsj,msj->mg", wd, P2).mean()
    n0 = d0 = None
    if offsets != "none":
        n0, d0 = scale * rng.uniform(0.1, 1.0, (3, 3) if offsets == "per_member" else 3), scale * rng.uniform(0.1, 1.0, (3, 3) if offsets == "per_member" else 3)
    a = np.array([1.0, -0.7, 0.4])
    first = O.SpectrumSpec(SIG, B, wn, wd, n0, d0, a, measure, "sum")
    _, l0, _ = _torch_reference(first, f)
    spread = float(np.ptp(a * l0, axis=1).max())
    sp = O.SpectrumSpec(SIG, B, wn, wd, n0, d0, a, measure, aggregate, 10.0 / spread if aggregate == "ks" else None)
    ref_J, ref_l, ref_g = _torch_reference(sp, f)
    J, l, fb = O.host_spectrum_value_and_cotangent(sp, f)
    N, D, l2 = O.spectrum_of_projections(sp, np.einsum("jk,mks->msj", B, O.host_signal_values(SIG, f)))
    assert J.shape == (3,) and l.shape == (3, 3) and fb.shape == f.shape and np.abs(ref_g).max() > 0 and np.array_equal(l, l2)
    assert (N > 0).all() and (D > 0).all()
    assert np.abs(J - ref_J).max() <= 1e-13 * np.abs(ref_l).max() * np.abs(a).sum()
    assert np.abs(l - ref_l).max() <= 1e-13 * np.abs(ref_l).max()
    assert np.abs(fb - ref_g).max() <= 1e-12 * np.abs(ref_g).max()
    if offsets != "per_member":
        J1, l1, fb1 = O.host_spectrum_value_and_cotangent(sp, f[1])
        assert isinstance(J1, float) and abs(J1 - J[1]) <= 1e-14 * abs(J[1]) and np.allclose(fb1, fb[1], rtol=1e-13, atol=0)
    else:
        with pytest.raises(ValueError, match="per-member offsets"):
            O.host_spectrum_value_and_cotangent(sp, f[1])
    with pytest.raises(ValueError, match="force and hinge-force components"):
        O.host_spectrum_value_and_cotangent(O.SpectrumSpec(O.SignalSpec([(0, 1, 6, 1.0)], 1), B, np.ones((1, 1, 4)), np.ones((1, 1, 4))), f)


def test_ratio_with_unit_denominator_is_twice_the_projection_objective(history):
    f = history
    B = O.fourier_basis(np.linspace(0.0, 6e-4, T), [3000.0])[:1]
    wn = np.array([[[0.0], [1.7], [0.0]]])
    sp = O.SpectrumSpec(SIG, B, wn, np.zeros_like(wn), None, [1.0], None, "ratio", "sum")
    J, l, fb = O.host_spectrum_value_and_cotangent(sp, f)
    Jp, fbp = O.host_projection_value_and_cotangent(O.ProjectionSpec(SIG, B, wn[0]), f)
    assert np.abs(Jp).min() > 0 and np.abs(J - 2 * Jp).max() <= 1e-15 * np.abs(J).max() and np.array_equal(J, l[:, 0])
    assert np.abs(fb - 2 * fbp).max() <= 1e-15 * np.abs(fb).max()


def test_log_ratio_is_invariant_under_a_scaling_of_all_signals(history):
    f = history
    B, wn, wd = _weights(G=2, seed=9)
    B = O.fourier_basis(np.linspace(0.0, 6e-4, T), [3000.0, 1700.0])
    for measure in O.MEASURES:
        sp = O.SpectrumSpec(SIG, B, wn, wd, measure=measure)
        J, l, fb = O.host_spectrum_value_and_cotangent(sp, f[0])
        J3, l3, fb3 = O.host_spectrum_value_and_cotangent(sp, 3.0 * f[0])
        assert abs(J3 - J) <= 1e-13 * np.abs(l).sum() and np.abs(3.0 * fb3 - fb).max() <= 1e-12 * np.abs(fb).max()
    # the members of the history are scaled copies of one another
    assert np.ptp(O.host_spectrum_value_and_cotangent(O.SpectrumSpec(SIG, B, wn, wd), f)[0]) <= 1e-13 * np.abs(l).sum()


def test_a_member_without_a_denominator_gets_nan_and_a_zero_cotangent(history):
    f = history
    B, wn, wd = _weights(G=2, seed=9)
    wd[1] = 0.0
    d0 = np.array([[0.0, 1.0], [0.0, 0.0], [0.0, 1.0]])
    for measure, aggregate, beta in (("ratio", "sum", None), ("log", "ks", 2.0)):
        J, l, fb = O.host_spectrum_value_and_cotangent(O.SpectrumSpec(SIG, B, wn, wd, None, d0, None, measure, aggregate, beta), f)
        Jr, lr, fbr = O.host_spectrum_value_and_cotangent(O.SpectrumSpec(SIG, B, wn, wd, None, np.where(d0 == 0, [0.0, 1.0], d0), None, measure, aggregate, beta), f)
        assert np.isnan(J[1]) and np.isnan(l[1, 1]) and np.isfinite(l[1, 0]) and not fb[1].any()
        assert np.array_equal(J[[0, 2]], Jr[[0, 2]]) and np.array_equal(fb[[0, 2]], fbr[[0, 2]]) and np.isfinite(Jr).all() and fbr[1].any()


def test_the_binding_lists_the_three_entries_with_the_hip_only_names(hip_lib):
    from difflexmm_amd._binding import COMM_EXPORTS
    names = ["dfx_signal_spectrum", "dfx_signal_spectrum_value", "dfx_signal_spectrum_value_and_grad"]
    assert all(n in COMM_EXPORTS and hasattr(hip_lib, n) for n in names)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_the_synthetic_rows_of_the_gpu_cases_do_not_cancel_on_the_cpu_port(cpu_lib, lattice):
    """the premise of test_gpu_signal_spectrum's 16- and 17-row bases, pinned here so that the GPU run cannot hide behind it"""
    from . import projection_yardstick as PY
    from . import test_gpu_objective as TGO
    from .common import Case
    from .test_gpu_signal_misfit import make_terms, member_leaves
    from .test_gpu_signal_spectrum import GRID70, SYNTHETIC_ROWS, synthetic_basis
    old = TGO.Case
    TGO.Case = functools.partial(Case, lib=cpu_lib)
    try:
        e = TGO.Ensemble(lattice)
    finally:
        TGO.Case = old
    terms, _, _ = make_terms(e.c)
    fields = np.array(e.c.solver(np.zeros((2, e.nb, 3)), GRID70[0], e.cps, steps_per_interval=GRID70[1]))
    S = np.stack([PY.MemberGraph(fields[m], member_leaves(e.c, e.cps, m), e.c.bonds, terms, 4).signal_values() for m in range(TGO.BATCH)])
    B = synthetic_basis(lattice, 17)
    assert B.shape == (17, 70) and len({f for f, _ in SYNTHETIC_ROWS[lattice]}) == 17
    k = SY.kappa(B, S, np.einsum("jk,mks->msj", B, S), np.ones((4, 17), dtype=bool))
    print(f"[signal spectrum] {lattice}: kappa of the 17 synthetic rows on the CPU port's history {k.max():.1f}")
    assert np.isfinite(k).all() and k.max() <= 25.0
    # the spec of the GPU case with 65 groups of one pair each over an offset, through the host formulas on these projections, against
    # the yardstick's formulas in torch
    P = np.einsum("jk,mks->msj", B, S)
    Wn = np.zeros((65, 68))
    Wn[np.arange(65), np.arange(65)] = np.random.default_rng(13).uniform(0.5, 2.0, 65)
    Wn = Wn.reshape(65, 4, 17)
    d0 = np.einsum("gsj,msj->mg", Wn, P * P) * np.random.default_rng(3).uniform(0.5, 2.0, (TGO.BATCH, 65))
    a = np.random.default_rng(5).uniform(-1.0, 1.0, 65)
    spec = O.SpectrumSpec(O.SignalSpec(terms, 4), B, Wn, np.zeros_like(Wn), None, d0, a, "log", "ks", 3.0)
    N, D, l = O.spectrum_of_projections(spec, P)
    J, l2, Pbar = O.spectrum_value_and_projection_cotangent(spec, P)
    for m in range(TGO.BATCH):
        Pt = torch.tensor(P[m], requires_grad=True)
        Nt = torch.einsum("gsj,sj->g", torch.tensor(Wn), Pt * Pt)
        lt, Jt = SY.measure_and_value(Nt, torch.tensor(d0[m]), a, "log", "ks", 3.0)
        g, = torch.autograd.grad(Jt, Pt)
        assert np.allclose(N[m], Nt.detach().numpy(), rtol=1e-13, atol=0) and np.array_equal(D[m], d0[m])
        assert np.abs(l[m] - lt.detach().numpy()).max() <= 1e-13 * np.abs(l[m]).max() and abs(J[m] - Jt.item()) <= 1e-13 * np.abs(l[m]).max()
        assert np.abs(Pbar[m] - g.numpy()).max() <= 1e-12 * np.abs(g.numpy()).max()
