"""The host side of the peak ligament-strain objective (difflexmm_amd/objective.py: ``PeakStrainSpec``, ``strain_limit_coefficients``,
``host_strain_measure`` / ``host_peak_strain_value``) against torch through ``oracle.ref_energy`` (tests/peak_strain_yardstick.py) at
1e-13, the bounds that follow from the definitions, the p = 1 identity with ``host_strain_value``, the premises of the cases of
tests/test_gpu_peak_strain.py on the CPU port's solves (tests/peak_strain_cases.py), and ``run_optimization_nlopt(state_constraints=None)``
against a call without the keyword, bit for bit.  No GPU involved."""
import math

import numpy as np
import pytest

from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import objective_shapes as OS
from . import peak_strain_cases as PC
from .peak_strain_yardstick import peak_objective
from .strain_yardstick import T64
from .test_strain_objective_host import _lattice

TOL = 1e-13


# ---- the spec and the coefficients -----------------------------------------------------------------------------------------------------
def test_spec_accepts_and_converts():
    s = O.PeakStrainSpec(np.ones((4, 3)))
    assert s.bond_coef.shape == (4, 3) and s.bond_weights is None and s.time_weights is None and s.aggregate == "ks" and s.sharpness > 0
    s = O.PeakStrainSpec(np.ones((2, 4, 3)), np.eye(4)[:2], [0.0, 1.0, 0.5], "pnorm", 1)
    assert s.bond_coef.shape == (2, 4, 3) and s.bond_weights.shape == (2, 4) and s.time_weights.shape == (3,) and s.sharpness == 1.0


@pytest.mark.parametrize("kw, match", [
    (dict(bond_coef=np.ones(4)), "bond_coef must be"),
    (dict(bond_coef=np.ones((4, 2))), "bond_coef must be"),
    (dict(bond_coef=np.ones((0, 3))), "bond_coef must be"),
    (dict(bond_coef=-np.ones((4, 3))), "finite and non-negative"),
    (dict(bond_coef=np.full((4, 3), np.nan)), "finite and non-negative"),
    (dict(bond_coef=np.ones((4, 3)), bond_weights=np.ones(5)), "bond_weights must be"),
    (dict(bond_coef=np.ones((4, 3)), bond_weights=np.ones((2, 2, 4))), "bond_weights must be"),
    (dict(bond_coef=np.ones((4, 3)), bond_weights=[1.0, -1.0, 0.0, 0.0]), "bond_weights must be finite and non-negative"),
    (dict(bond_coef=np.ones((4, 3)), bond_weights=[1.0, np.inf, 0.0, 0.0]), "bond_weights must be finite and non-negative"),
    (dict(bond_coef=np.ones((4, 3)), bond_weights=[[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]), "all weights are zero for some member"),
    (dict(bond_coef=np.ones((4, 3)), time_weights=np.ones((2, 2))), "time_weights must be"),
    (dict(bond_coef=np.ones((4, 3)), time_weights=[1.0, -0.5]), "time_weights must be finite and non-negative"),
    (dict(bond_coef=np.ones((4, 3)), time_weights=[0.0, 0.0]), "time_weights: all weights are zero"),
    (dict(bond_coef=np.ones((4, 3)), aggregate="max"), "aggregate must be"),
    (dict(bond_coef=np.ones((4, 3)), sharpness=0.0), "sharpness"),
    (dict(bond_coef=np.ones((4, 3)), sharpness=np.inf), "sharpness"),
    (dict(bond_coef=np.ones((4, 3)), aggregate="pnorm", sharpness=0.5), "sharpness"),
])
def test_spec_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        O.PeakStrainSpec(**kw)


def test_strain_limit_coefficients_by_hand():
    """two bonds, l0 = 5 and 2: a = 1 / (l0 eps_lim)^2, s = 1 / (l0 gamma_lim)^2, r = 1 / kappa_lim^2; None and inf give 0"""
    refv = np.array([[3.0, 4.0], [0.0, 2.0]])
    c = O.strain_limit_coefficients(refv, 0.1, [np.inf, 0.5], None)
    assert np.allclose(c, [[4.0, 0.0, 0.0], [25.0, 1.0, 0.0]], rtol=1e-15, atol=0.0)
    c = O.strain_limit_coefficients(refv, None, 0.2, 0.25)
    assert np.allclose(c, [[0.0, 1.0, 16.0], [0.0, 6.25, 16.0]], rtol=1e-15, atol=0.0)
    assert not O.strain_limit_coefficients(refv).any()
    with pytest.raises(ValueError, match="positive"):
        O.strain_limit_coefficients(refv, 0.0)
    with pytest.raises(ValueError, match="positive"):
        O.strain_limit_coefficients(refv, None, -1.0)
    with pytest.raises(ValueError, match="reference_bond_vectors"):
        O.strain_limit_coefficients(np.ones(2), 0.1)


# ---- the NumPy restatement against the yardstick ----------------------------------------------------------------------------------------
def _random_case(lattice):
    geo, cnv, bonds, refv = _lattice(lattice)
    rng = np.random.default_rng(21)
    B, T, nb, nbd = 2, 4, geo.n_blocks, len(bonds)
    fields = rng.normal(size=(B, T, 2, nb, 3)) * np.array([0.4, 0.4, 0.15])
    w = rng.uniform(0.25, 2.0, (B, nbd)) * (rng.random((B, nbd)) < 0.4)
    tau = np.array([0.0, 1.0, 0.37, 2.0])
    refv = np.broadcast_to(refv, (nbd, 2)) * (1 + 0.05 * rng.uniform(-1, 1, (nbd, 1)))
    coef = rng.uniform(0.5, 2.0, (B, nbd, 3))
    return cnv, bonds, refv, fields, w, tau, coef


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
@pytest.mark.parametrize("model", ["nonlinear", "linearized"])
@pytest.mark.parametrize("aggregate", ["ks", "pnorm"])
def test_host_value_against_the_yardstick_and_its_bounds(lattice, model, aggregate):
    cnv, bonds, refv, fields, w, tau, coef = _random_case(lattice)
    B = len(fields)
    q = O.host_strain_measure(coef, fields, cnv, bonds, refv, model)
    qhat = np.array([PC.weighted_pairs(q, w, tau)[m][0] for m in range(B)])
    sharp = PC.choose_beta(qhat) if aggregate == "ks" else PC.P_NORM
    assert aggregate == "pnorm" or PC.in_range(sharp, qhat)
    spec = O.PeakStrainSpec(coef, w, tau, aggregate, sharp)
    J, peak, at = O.host_peak_strain_value(spec, fields, cnv, bonds, refv, model)
    assert J.shape == (B,) and peak.shape == (B,) and at.shape == (B, 2) and at.dtype == np.int32
    worst = 0.0
    for m in range(B):
        Jr, qh, where = peak_objective(T64(fields[m, :, 0]), T64(cnv), bonds, T64(refv), T64(coef[m]), w[m], tau, aggregate, sharp, model)
        worst = max(worst, abs(J[m] - Jr.item()) / abs(Jr.item()), abs(peak[m] - qh) / qh)
        assert tuple(at[m]) == where and tau[where[0]] > 0 and w[m, where[1]] > 0
        # the bounds that follow from the definitions: the sum holds the argmax's own term and at most sum W terms of that size
        W = tau[:, None] * w[m][None, :]
        if aggregate == "ks":
            lo, hi = peak[m] + math.log(W[where]) / sharp, peak[m] + math.log(W.sum()) / sharp
        else:
            lo, hi = peak[m] * W[where] ** (1 / sharp), peak[m] * W.sum() ** (1 / sharp)
        assert lo * (1 - 1e-14) <= J[m] <= hi * (1 + 1e-14), (m, lo, J[m], hi)
    print(f"[peak strain] host value vs torch, {lattice} {model} {aggregate}: {worst:.2e}")
    assert worst <= TOL
    # one member without the member axis, shared coefficients, no weights
    one = O.host_peak_strain_value(O.PeakStrainSpec(coef[0], None, None, aggregate, sharp), fields[1], cnv, bonds, refv, model)
    Jr, qh, where = peak_objective(T64(fields[1, :, 0]), T64(cnv), bonds, T64(refv), T64(coef[0]), np.ones(len(bonds)), np.ones(4), aggregate,
                                   sharp, model)
    assert isinstance(one[0], float) and abs(one[0] - Jr.item()) <= TOL * abs(Jr.item()) and one[1] == pytest.approx(qh, rel=TOL)
    assert tuple(one[2]) == where


def test_ties_take_the_lowest_output_then_the_lowest_bond():
    q = np.zeros((1, 3, 4))
    q[0, 1, 2] = q[0, 1, 3] = q[0, 2, 0] = 2.0
    for agg, sharp in (("ks", 3.0), ("pnorm", 4.0)):
        J, peak, at = O.peak_of_measure(O.PeakStrainSpec(np.ones((4, 3)), None, None, agg, sharp), q)
        assert peak[0] == 2.0 and tuple(at[0]) == (1, 2)
        J, peak, at = O.peak_of_measure(O.PeakStrainSpec(np.ones((4, 3)), [1.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0], agg, sharp), q)
        assert tuple(at[0]) == (1, 3)                                 # bond 2 is not watched
    # at rest: log(sum W) / beta, and 0 without a NaN
    z = np.zeros((1, 3, 4))
    w, tau = np.array([0.5, 0.25, 0.0, 1.0]), np.array([1.0, 0.0, 2.0])
    J, peak, at = O.peak_of_measure(O.PeakStrainSpec(np.ones((4, 3)), w, tau, "ks", 4.0), z)
    assert J[0] == math.log(1.75 * 3.0) / 4.0 and peak[0] == 0.0 and tuple(at[0]) == (0, 0)
    J, peak, at = O.peak_of_measure(O.PeakStrainSpec(np.ones((4, 3)), w, tau, "pnorm", 4.0), z)
    assert J[0] == 0.0 and peak[0] == 0.0


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_p_equal_one_is_twice_the_strain_energy(lattice):
    """q = 2 E with coef_b = parts x k_b, so the p-norm with p = 1 is 2 x host_strain_value (nonlinear ligaments)"""
    cnv, bonds, refv, fields, w, tau, _ = _random_case(lattice)
    rng = np.random.default_rng(3)
    nbd = len(bonds)
    ks, ksh, kr = 120.0 * (1 + 0.1 * rng.uniform(-1, 1, nbd)), 1.19 * np.ones(nbd), 1.5 * (1 + 0.1 * rng.uniform(-1, 1, nbd))
    parts = (1.0, 0.5, 2.0, 0.0)
    coef = np.stack([parts[0] * ks, parts[1] * ksh, parts[2] * kr], 1)
    J, _, _ = O.host_peak_strain_value(O.PeakStrainSpec(coef, w, tau, "pnorm", 1.0), fields, cnv, bonds, refv)
    ref = 2.0 * O.host_strain_value(O.StrainObjectiveSpec(w, tau, parts), fields, cnv, bonds, refv, ks, ksh, kr)
    err = np.abs(J - ref).max() / np.abs(ref).max()
    print(f"[peak strain] p = 1 against 2 x host_strain_value, {lattice}: {err:.2e}")
    assert err <= TOL


def test_host_refusals():
    cnv, bonds, refv, fields, w, tau, coef = _random_case("quads")
    with pytest.raises(ValueError, match="bond_coef"):
        O.host_peak_strain_value(O.PeakStrainSpec(coef[:, :-1]), fields, cnv, bonds, refv)
    with pytest.raises(ValueError, match="time_weights"):
        O.host_peak_strain_value(O.PeakStrainSpec(coef, None, np.ones(7)), fields, cnv, bonds, refv)
    with pytest.raises(ValueError, match="model"):
        O.host_peak_strain_value(O.PeakStrainSpec(coef), fields, cnv, bonds, refv, model="simple_spring")


def test_the_entries_are_exports_of_the_hip_library(hip_lib):
    """HIP-library-only exports of include/dfx.h, like the other objective entries: an engine on a library without them says so."""
    import difflexmm_amd._binding as b
    for name in ("dfx_strain_peak_value", "dfx_strain_peak_value_and_grad"):
        assert name in b.COMM_EXPORTS and name in b.EXPORTS and hasattr(hip_lib, name)


def test_the_cpu_port_says_that_it_has_no_peak_entry(cpu_lib):
    from .common import Case
    c = Case("quads", 4, True, False, seed=3, lib=cpu_lib)
    c.solver(np.zeros((2, 16, 3)), np.linspace(0.0, 1e-4, 3), c.cp, keep_trajectory=True, steps_per_interval=2)
    with pytest.raises(NotImplementedError, match="dfx_strain_peak_value_and_grad"):
        c.solver.peak_strain_value(O.PeakStrainSpec(np.ones((len(c.bonds), 3))))


# ---- the premises of the GPU cases, on the CPU port's solves -----------------------------------------------------------------------------
_SMALL = {}


def _small(lattice, cpu_lib):
    from .test_gpu_objective import SPI, TAU, TS
    if lattice not in _SMALL:
        e = PC.cpu_ensemble(lattice, cpu_lib)
        e.fields = np.array(e.c.solver(np.zeros((2, e.nb, 3)), TS, e.cps, keep_trajectory=True, steps_per_interval=SPI))
        e.coef, e.bw, e.special = PC.small_inputs(e.c)
        e.tau = TAU
        e.q = PC.measure(e.c, e.cps, e.fields, e.coef)
        _SMALL[lattice] = e
    return _SMALL[lattice]


@pytest.fixture(params=["quads", "kagome"])
def small(request, cpu_lib):
    return _small(request.param, cpu_lib)


def test_small_cases_choose_their_sharpness_inside_the_range(small):
    e = small
    assert (e.bw >= 0).all() and (e.bw == 0).mean() > 0.7 and e.tau[0] == 0 and (e.tau != np.round(e.tau)).any()
    assert all((e.bw[:, b] > 0).all() for b in e.special)
    pairs = PC.weighted_pairs(e.q, e.bw, e.tau)
    qhat = np.array([p[0] for p in pairs])
    beta = PC.choose_beta(qhat)
    print(f"[peak strain] {e.c.geo.__class__.__name__}: q_hat {qhat}, beta {beta:.4g}, beta q_hat {beta * qhat}")
    assert (qhat > 0).all() and PC.in_range(beta, qhat)
    assert PC.P_RANGE[0] <= PC.P_NORM <= PC.P_RANGE[1]
    # the softmax is no one-hot here: the second pair carries a share that the bars can see
    assert all(math.exp(beta * (p[1] - p[0])) > 1e-6 for p in pairs)


def test_sharp_case_has_a_gap(cpu_lib):
    e = _small("quads", cpu_lib)
    pairs = PC.weighted_pairs(e.q, e.bw, e.tau)
    gaps = [(p[0] - p[1]) / p[0] for p in pairs]
    print(f"[peak strain] sharp case: relative gap between the two largest q {gaps}, beta {PC.sharp_beta(pairs):.4g}")
    assert min(gaps) > 1e-3
    assert all(math.exp(PC.sharp_beta(pairs) * (p[1] - p[0])) == 0.0 for p in pairs)


@pytest.fixture(scope="module", params=["quads", "kagome"])
def large(request, cpu_lib):
    L = OS.LargeCase(request.param, cpu_lib)
    L.fields = L.solve()
    L.coef, L.pw, L.ptau = PC.large_inputs(L)
    L.q = PC.measure(L.c, L.cps, L.fields, L.coef)
    return L


def test_large_case_spans_many_workgroups_and_its_late_argmax_sits_in_the_last_third(large):
    L = large
    cnt, wg, _ = L.counts()
    assert wg["k_strain_objective"] > 1000 and wg["k_strain_objective"] > OS.ITEMS_WIDE         # the peak kernels share that grid
    assert (OS.N_OUT * cnt["n_act_strain"]) % OS.ITEMS_QUAD != 0
    for name, tau in (("its tau", L.ptau), ("late tau", PC.late_tau(L.ptau))):
        spec = O.PeakStrainSpec(L.coef, L.pw, tau, "ks", 1.0)
        _, qhat, at = O.peak_of_measure(spec, L.q)
        beta = PC.choose_beta(qhat)
        where = [PC.item_of(L, int(k), int(b)) for k, b in at]
        print(f"[peak strain] {L.lattice} large, {name}: q_hat {qhat}, beta q_hat {beta * qhat}, argmax at {at.tolist()}, items {where}")
        assert (qhat > 0).all() and PC.in_range(beta, qhat)
        if name == "late tau":
            assert all(3 * item >= 2 * total for item, total in where)
    for k in OS.ONE_HOT:
        _, qhat, at = O.peak_of_measure(O.PeakStrainSpec(L.coef, L.pw, np.eye(OS.N_OUT)[k], "ks", 1.0), L.q)
        assert (qhat > 0).all() and (at[:, 0] == k).all()


# ---- the optimisation loop without state constraints is the loop as it was -----------------------------------------------------------------
def test_nlopt_loop_without_state_constraints_is_unchanged(cpu_lib):
    import inspect
    assert inspect.signature(P.OptimizationProblem.run_optimization_nlopt).parameters["state_constraints"].default is None

    def run(**kw):
        fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=1e-4 * np.ones((36, 3)), loaded_side="left", input_shift=0,
                                    steps_per_interval=4, _lib=cpu_lib, **_focus_kw())
        fw.setup()
        prob = P.OptimizationProblem(P.TargetKineticEnergy(fw, (2, 2), (2, 0)), name="t")
        x0 = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
        best = prob.run_optimization_nlopt(x0, 3, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0, min_edge_length=1.0,
                                           verbose=False, **kw)
        return prob, best
    a, best_a = run()
    b, best_b = run(state_constraints=None)
    assert len(a.objective_values) == 3 and a.objective_values == b.objective_values
    assert all(np.array_equal(x, y) for da, db in zip(a.design_values, b.design_values) for x, y in zip(da, db))
    assert set(a.constraints_violation) == set(b.constraints_violation) == {"angles", "edge_lengths"}
    assert a.constraints_violation == b.constraints_violation
    assert all(np.array_equal(x, y) for x, y in zip(best_a, best_b))


def _focus_kw():
    from .test_gpu_objective import FOCUS_KW
    return dict(FOCUS_KW)
