"""-m gpu: forward mode along several directions per member (DynamicSolver.jvp_multi / jacfwd -> dfx_forward_tangent_multi,
dfx_forward_tangent_dense_multi): its columns are the single-direction ``jvp``'s, torch.autograd's through the oracle and the transpose
of ``vjp``; batch x directions; the adaptive form; a batch-1 Jacobian against central differences; its contract.  Host side:
tests/test_tangent_multi_host.py.

``jvp`` is ``jvp_multi`` along one direction, and dfx_forward_tangent / dfx_forward_tangent_dense are the ``_multi`` entries at
n_dirs = 1: ONE set of kernels (dfx_tangent.h), instantiated 1, 2 and 4 wide.  "Against ``jvp``" below therefore compares the 4- and
2-wide instances (the chunked form at K >= 2) with the 1-wide one; the K = 1 and the spread-form cases compare the 1-wide kernel with
itself and pass trivially -- they stay as checks of the host's pass planning, slicing and column placement.  The independent check of the
1-wide kernel is the oracle: test_gpu_tangent.py, test_gpu_tangent_adaptive.py and test_gpu_tangent_param_shapes.py through ``jvp``.
Section 8 pins the single-direction C entries to the n_dirs = 1 ones bit for bit.

Tolerances are the suite's: 1e-13 for the primal fields of two kernels that evaluate the same expressions, 1e-12 (the
RHS-level figure) for a column against the 1-wide kernel -- the K-wide epsilon arithmetic is contracted differently --,
RTOL_GRAD against autograd, 1e-11 for the transposition identity, 1e-6 against central differences.  Worst cases measured on the MI355X
are in profiles/r09_tangent_multi.txt."""
import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import _binding as b
from oracle import ref_dynamics as OD

from .common import DENSITY, Case, relerr
from .parity import RTOL_GRAD, T64
from .test_gpu_tangent import CASES, FAST, _case, _explicit_inertia, _grid, _per_bond, _tangent_tree, _tree_dot

pytestmark = pytest.mark.gpu

ZERO = dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None))
WIDEST = 4        # the widest chunk the library ships (kTanMaxWidth): K = 1 below it, 3 no multiple of a width, 5 above it


@pytest.fixture(params=["chunked", "spread"])
def form(request, monkeypatch):
    """Both forms of a pass on lattices of any size: passes of the widest chunk (what a lattice that fills the chip takes), and all
    directions spread over lanes in one pass (what these small lattices take when nothing is forced)."""
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", request.param)
    return request.param


def _columns_equal_jvp(s, fields, fdots, singles, what):
    """fields / columns of jvp_multi against the (fields, fields_dot) pairs of single-direction jvp calls; direction axis 0 of fdots."""
    worst = 0.0
    for k, (f1, d1) in enumerate(singles):
        ef, ed = relerr(fields, f1), relerr(fdots[k], d1)
        worst = max(worst, ed)
        print(what, "column", k, "fields", ef, "fields_dot", ed)
        assert ef < 1e-13, (what, k, ef)
        assert ed < 1e-12, (what, k, ed)
        assert np.abs(d1).max() > 0.0
    return worst


# ---- 1. columns equal the single-direction path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,nonlinear,contact,integrator,unequal", CASES)
def test_columns_equal_single_direction_jvp(lattice, nonlinear, contact, integrator, unequal, form):
    c = _case(lattice, 4, nonlinear, contact, integrator)
    rng = np.random.default_rng(3)
    c.cp = _per_bond(c)
    cp, inertia = _explicit_inertia(c)
    ts = np.linspace(0, 3e-4, 4)
    spi = 4
    st = _grid(ts, spi, unequal)
    y0 = c.random_state(0.05, 0.02, 5.0)
    s = c.solver
    tangents = [(c.random_state(0.05, 0.02, 5.0), _tangent_tree(c, rng, inertia, scale=1.0 + 0.5 * k)) for k in range(5)]
    singles = [s.jvp(y0, ts, cp, y0d, cd, steps_per_interval=spi, step_times=st) for y0d, cd in tangents]
    for K in (1, 3, 5):
        fields, fdots = s.jvp_multi(y0, ts, cp, tangents[:K], steps_per_interval=spi, step_times=st)
        assert fields.shape == (4, 2, c.geo.n_blocks, 3) and fdots.shape == (K, 4, 2, c.geo.n_blocks, 3)
        assert s.stats["step_control"] == "fixed" and s.stats["steps"] == 12
        _columns_equal_jvp(s, fields, fdots, singles[:K], (lattice, nonlinear, contact, integrator, unequal, K))
    # None entries are zero tangents: a zero column, and the columns beside it unmoved
    fields, fdots = s.jvp_multi(y0, ts, cp, [tangents[0], (None, None), (tangents[1][0], None), (None, tangents[1][1])],
                                steps_per_interval=spi, step_times=st)
    assert np.all(fdots[1] == 0.0)
    assert relerr(fdots[0], singles[0][1]) < 1e-12
    assert relerr(fdots[2] + fdots[3], singles[1][1]) < 1e-12          # linear in the direction


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,nonlinear", [("quads", True), ("kagome", False)])
def test_columns_match_autograd_through_the_oracle(lattice, nonlinear):
    integrator = "dopri5"
    c = _case(lattice, 4, nonlinear, True, integrator)
    rng = np.random.default_rng(3)
    c.cp = _per_bond(c)
    cp, inertia = _explicit_inertia(c)
    ts = np.linspace(0, 3e-4, 4)
    spi = 4
    y0 = c.random_state(0.05, 0.02, 5.0)
    tangents = [(c.random_state(0.05, 0.02, 5.0), _tangent_tree(c, rng, inertia, scale=1.0 + k)) for k in range(2)]
    # column 2: column 0 with the contact tangents zeroed
    md0 = tangents[0][1].mechanical_params
    tangents.append((tangents[0][0], tangents[0][1]._replace(mechanical_params=md0._replace(contact_params=dm.ContactParams(0.0, 0.0, 0.0)))))
    fields, fdots = c.solver.jvp_multi(y0, ts, cp, tangents, steps_per_interval=spi)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau=integrator)
    free = osol.free_DOF_ids
    mp = cp.mechanical_params
    names = ["cnv", "refv", "ks", "ksh", "kr", "inertia", "damping", "amplitude", "loading_rate", "input_delay", "state0", "min_angle",
             "cutoff_angle", "k_contact"]
    prim = dict(cnv=c.cnv, refv=np.broadcast_to(c.refv, (len(c.bonds), 2)), ks=mp.bond_params.k_stretch, ksh=mp.bond_params.k_shear,
                kr=mp.bond_params.k_rot, inertia=inertia, damping=mp.damping, state0=y0, min_angle=mp.contact_params.min_angle,
                cutoff_angle=mp.contact_params.cutoff_angle, k_contact=mp.contact_params.k_contact, **FAST)

    def f(*xs):
        lv = dict(zip(names, xs))
        y0t = lv.pop("state0")
        hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(lv), spi, integrator)
        return hist
    n = len(ts)
    for k, (y0d, cd) in enumerate(tangents):
        md = cd.mechanical_params
        tan = dict(cnv=cd.geometrical_params.centroid_node_vectors, refv=md.bond_params.reference_vector, ks=md.bond_params.k_stretch,
                   ksh=md.bond_params.k_shear, kr=md.bond_params.k_rot, inertia=md.inertia, damping=md.damping, state0=y0d,
                   min_angle=md.contact_params.min_angle, cutoff_angle=md.contact_params.cutoff_angle, k_contact=md.contact_params.k_contact,
                   **cd.constraint_params)
        of, ojv = torch.autograd.functional.jvp(f, tuple(T64(prim[x]) for x in names), tuple(T64(tan[x]) for x in names))
        e0 = relerr(fields.reshape(n, 2, -1)[:, :, free], of.detach().numpy())
        e = relerr(fdots[k].reshape(n, 2, -1)[:, :, free], ojv.numpy())
        print(lattice, nonlinear, "column", k, "primal", e0, "tangent", e)
        assert e0 < 1e-10, e0
        assert e < RTOL_GRAD, (lattice, nonlinear, k, e)
    # the contact constants must matter, or the check above says nothing about them
    assert np.abs(fdots[2] - fdots[0]).max() > 1e-6 * np.abs(fdots[0]).max()


# ---- 3. transpose identity --------------------------------------------------------------------------------------------------------------------
def _transpose_check_multi(c, ts, spi, y0, cp, K=4):
    s = c.solver
    rng = np.random.default_rng(11)
    trees = [_tangent_tree(c, rng, scale=1.0 + 0.5 * k) for k in range(K)]
    y0ds = []
    for k in range(K):
        y0d = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.abs(y0).max()
        y0d.reshape(2, -1)[:, s.constrained_DOF_ids] = 0.0          # (state0 of prescribed DOFs is not read)
        y0ds.append(y0d)
    _, fdots = s.jvp_multi(y0, ts, cp, list(zip(y0ds, trees)), steps_per_interval=spi)
    assert fdots.shape[0] == K
    fields = s(y0, ts, cp, keep_trajectory=True, steps_per_interval=spi)
    fb = rng.normal(size=fields.shape)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    bars, s0b = s.vjp(fb)
    for k in range(K):
        lhs = float(np.sum(fb * fdots[k]))
        rhs = _tree_dot(bars, trees[k]) + float(np.sum(np.asarray(s0b) * y0ds[k]))
        gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("transposition gap, column", k, gap, lhs, rhs)
        assert gap <= 1e-11, (k, lhs, rhs, gap)


def test_columns_are_the_transpose_of_the_adjoint_small(form):
    c = _case("kagome", 8, True, True, seed=3)
    c.cp = _per_bond(c)
    _transpose_check_multi(c, np.linspace(0, 3e-4, 4), 12, c.random_state(0.05, 0.02, 5.0), c.cp)


def test_columns_are_the_transpose_of_the_adjoint_128x128_contact(monkeypatch):
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", "chunked")            # (16 384 blocks x 4 directions sit exactly on the spread form's bound)
    c = _case("quads", 128, True, True, batch=1, seed=2)
    c.cp = _per_bond(c)
    _transpose_check_multi(c, np.linspace(0, 3e-4, 3), 250, c.random_state(0.05, 0.02, 5.0), c.cp)        # 500 steps


# ---- 4. batch x directions ------------------------------------------------------------------------------------------------------------------------
def _scaled(cp, f):
    bp = cp.mechanical_params.bond_params
    return cp._replace(mechanical_params=cp.mechanical_params._replace(
        bond_params=bp._replace(k_stretch=bp.k_stretch * f, k_shear=bp.k_shear * f, k_rot=bp.k_rot * f)))


def test_batch_times_directions_with_per_member_tangents_and_grids(form):
    B, K = 3, 3
    c = _case("quads", 8, True, True, batch=B, seed=6)
    c.cp = _per_bond(c)
    rng = np.random.default_rng(7)
    cps = [_scaled(c.cp, f) for f in (1.0, 2.5, 0.4)]                                  # three different designs
    ts = np.stack([np.linspace(0, 3e-4, 4) + 1e-5 * m for m in range(B)])              # every member its own output times
    spi = 12
    st = np.stack([_grid(row, spi, True) for row in ts])
    y0 = np.stack([c.random_state(0.05, 0.02, 5.0) for _ in range(B)])
    s = c.solver
    tangents = [(np.stack([c.random_state(0.05, 0.02, 5.0) for _ in range(B)]),
                 [_tangent_tree(c, rng, scale=1.0 + m + 0.3 * k) for m in range(B)]) for k in range(K)]
    fields, fdots = s.jvp_multi(y0, ts, cps, tangents, steps_per_interval=spi, step_times=st)
    assert fields.shape == (B, 4, 2, c.geo.n_blocks, 3) and fdots.shape == (B, K, 4, 2, c.geo.n_blocks, 3)
    for k, (y0d, trees) in enumerate(tangents):
        f1, d1 = s.jvp(y0, ts, cps, y0d, trees, steps_per_interval=spi, step_times=st)
        for m in range(B):
            ef, ed = relerr(fields[m], f1[m]), relerr(fdots[m, k], d1[m])
            print("member", m, "direction", k, "fields", ef, "fields_dot", ed)
            assert ef < 1e-13 and ed < 1e-12, (m, k, ef, ed)
    # the members really differ, and so do the directions
    assert relerr(fdots[1, 0], fdots[0, 0]) > 1e-3 and relerr(fdots[0, 1], fdots[0, 0]) > 1e-3


# ---- 5. adaptive=True ---------------------------------------------------------------------------------------------------------------------------------
ADAPTIVE_CASES = [(lat, nl, ct) for lat in ("quads", "kagome") for nl in (True, False) for ct in (True, False)]


def _adaptive_columns(s, y0, ts, cp, tangents):
    """jvp_multi(adaptive=True) against the default call's fields and against jvp(adaptive=True) column by column."""
    ref = s(y0, ts, cp)
    assert s.stats["step_control"] == "adaptive"
    fields, fdots = s.jvp_multi(y0, ts, cp, tangents, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense"
    steps = list(s.stats["steps_per_member"])
    e = relerr(fields, ref)
    print("adaptive: steps", steps, "fields against the default call", e)
    assert e < 1e-10, e
    singles = []
    for y0d, cd in tangents:
        singles.append(s.jvp(y0, ts, cp, y0d, cd, adaptive=True))
        assert list(s.stats["steps_per_member"]) == steps
    return fields, fdots, singles


@pytest.mark.parametrize("lattice,nonlinear,contact", ADAPTIVE_CASES)
def test_adaptive_columns_equal_single_direction_jvp(lattice, nonlinear, contact, form):
    c = _case(lattice, 4, nonlinear, contact, seed=9)
    rng = np.random.default_rng(3)
    c.cp = _per_bond(c)
    cp, inertia = _explicit_inertia(c)
    ts = np.linspace(0, 3e-4, 61)
    s = c.solver
    s.rtol = s.atol = 1e-5
    y0 = c.random_state(0.05, 0.02, 5.0)
    K = 5 if (nonlinear and contact) else 3
    tangents = [(c.random_state(0.05, 0.02, 5.0), _tangent_tree(c, rng, inertia, scale=1.0 + 0.5 * k)) for k in range(K)]
    fields, fdots, singles = _adaptive_columns(s, y0, ts, cp, tangents)
    assert fdots.shape == (K, 61, 2, c.geo.n_blocks, 3)
    _columns_equal_jvp(s, fields, fdots, singles, ("adaptive", lattice, nonlinear, contact))


def test_adaptive_distance_contact_columns(form):
    from .test_distance_contact import DistCase
    c = DistCase("quads", None, n=4, seed=5)
    rng = np.random.default_rng(13)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 31)
    y0 = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02]) * np.array([[1.0], [5.0]])[:, :, None]
    tangents = []
    for k in range(3):
        cd = dm.ControlParams(dm.GeometricalParams(0.05 * rng.normal(size=np.shape(c.cen)), 0.02 * rng.normal(size=np.shape(c.cnv))),
                              dm.MechanicalParams(None, None, None, None, dm.ContactParams(0.02, -0.03 * (k + 1), 0.05)),
                              constraint_params=dict(amplitude=0.2 + k))
        tangents.append((rng.normal(size=y0.shape) * np.abs(y0).max(), cd))
    fields, fdots, singles = _adaptive_columns(s, y0, ts, c.cp, tangents)
    assert not s.stats["kept_trajectory"]
    _columns_equal_jvp(s, fields, fdots, singles, "adaptive, distance contact")


def test_adaptive_spring_model_columns(form):
    from .test_spring_models import SpringCase
    c = SpringCase("torsion", None, seed=5)
    rng = np.random.default_rng(17)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 31)
    y0 = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02]) * np.array([[1.0], [5.0]])[:, :, None]
    tangents = []
    for k in range(3):
        cd = dm.ControlParams(dm.GeometricalParams(None, 0.02 * rng.normal(size=np.shape(c.cnv))),
                              dm.MechanicalParams(dm.StretchingTorsionalSpringParams(0.1 * rng.normal(size=c.ks.shape) * c.ks,
                                                                                     0.1 * rng.normal(size=c.kr.shape) * c.kr), None),
                              constraint_params=dict(amplitude=0.2 + k))
        tangents.append((rng.normal(size=y0.shape) * np.abs(y0).max(), cd))
    fields, fdots, singles = _adaptive_columns(s, y0, ts, c.cp, tangents)
    _columns_equal_jvp(s, fields, fdots, singles, "adaptive, stretching + torsional springs")


def _leaves(tree):
    if tree is None:
        return []
    if isinstance(tree, dict):
        return [np.asarray(v, dtype=float) for _, v in sorted(tree.items())]
    if isinstance(tree, tuple) and hasattr(tree, "_fields"):
        return [x for f in tree._fields for x in _leaves(getattr(tree, f))]
    return [np.asarray(tree, dtype=float)]


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_adaptive_members_on_their_own_clocks_and_vjp_on_the_kept_solve(lattice, form):
    B, K = 3, 3
    c = Case(lattice, 4, True, True, seed=9, cutoff_deg=125.0 if lattice == "kagome" else 42.0, batch=B)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    c.cp = _per_bond(c)
    cps = [_scaled(c.cp, f) for f in (1.0, 2.5, 0.4)]
    ts = np.linspace(0, 3e-4, 61)
    s = c.solver
    s.rtol = s.atol = 1e-5
    rng = np.random.default_rng(7)
    y0 = np.stack([c.random_state(0.05, 0.02, 5.0)] * B)
    tangents = [(np.stack([c.random_state(0.05, 0.02, 5.0) for _ in range(B)]),
                 [_tangent_tree(c, rng, scale=1.0 + m + 0.3 * k) for m in range(B)]) for k in range(K)]
    ref = s(y0, ts, cps)
    fields, fdots = s.jvp_multi(y0, ts, cps, tangents, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and s.stats["kept_trajectory"]
    steps = list(s.stats["steps_per_member"])
    assert len(set(steps)) == 3, steps                                  # every member on its own clock
    assert relerr(fields, ref) < 1e-10
    fb = np.random.default_rng(2).normal(size=fields.shape)
    solves = s.solve_count
    bars_multi, s0b_multi = s.vjp(fb)                                   # directly after jvp_multi: the kept adaptive pass
    assert s.solve_count == solves
    for k, (y0d, trees) in enumerate(tangents):
        f1, d1 = s.jvp(y0, ts, cps, y0d, trees, adaptive=True)
        assert list(s.stats["steps_per_member"]) == steps and s.stats["kept_trajectory"]
        for m in range(B):
            ef, ed = relerr(fields[m], f1[m]), relerr(fdots[m, k], d1[m])
            print(lattice, "member", m, "steps", steps[m], "direction", k, "fields", ef, "fields_dot", ed)
            assert ef < 1e-13 and ed < 1e-12, (m, k, ef, ed)
    bars, s0b = s.vjp(fb)                                               # ... and after the single-direction jvp
    assert np.array_equal(np.asarray(s0b_multi), np.asarray(s0b))
    for tm, t1 in zip(bars_multi, bars):
        for a, bb in zip(_leaves(tm), _leaves(t1)):
            assert np.array_equal(a, bb)


# ---- 6. a batch-1 solver returns a Jacobian ------------------------------------------------------------------------------------------------------------
def test_batch_one_jacfwd_matches_central_differences():
    c = _case("quads", 16, True, True, seed=8)
    s = c.solver
    assert s.batch == 1
    ts = np.linspace(0, 2e-4, 3)
    spi = 60
    y0 = c.random_state(0.05, 0.02, 5.0)
    wrt = ["k_stretch", "k_shear", "k_rot", "amplitude"]
    fields, jac = s.jacfwd(y0, ts, c.cp, wrt, steps_per_interval=spi)
    assert sorted(jac) == sorted(wrt) and all(jac[k].shape == fields.shape for k in wrt)
    assert relerr(fields, s(y0, ts, c.cp, steps_per_interval=spi)) < 1e-13
    mp = c.cp.mechanical_params
    free = s.free_DOF_ids
    for name in wrt:
        x = float(FAST[name]) if name in FAST else float(getattr(mp.bond_params, name))
        h = 1e-6 * abs(x)

        def moved(e):
            if name in FAST:
                return c.cp._replace(constraint_params=dict(FAST, **{name: x + e}))
            return c.cp._replace(mechanical_params=mp._replace(bond_params=mp.bond_params._replace(**{name: x + e})))
        fd = (s(y0, ts, moved(h), steps_per_interval=spi) - s(y0, ts, moved(-h), steps_per_interval=spi)) / (2 * h)
        e = relerr(jac[name].reshape(len(ts), 2, -1)[:, :, free], fd.reshape(len(ts), 2, -1)[:, :, free])
        print("jacfwd", name, "against central differences", e)
        assert e < 1e-6, (name, e)
    # the same columns from hand-written unit tangents
    unit = [(None, ZERO._replace(mechanical_params=dm.MechanicalParams(dm.LigamentParams(*[1.0 if j == i else None for j in range(3)], None), None)))
            for i in range(3)] + [(None, ZERO._replace(constraint_params=dict(amplitude=1.0)))]
    _, fdots = s.jvp_multi(y0, ts, c.cp, unit, steps_per_interval=spi)
    for k, name in enumerate(wrt):
        assert np.array_equal(fdots[k], jac[name])


# ---- 7. contract ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_kept_solve_is_left_alone_and_launches_grow_with_passes(monkeypatch):
    c = _case("quads", 4, True, True, seed=14)
    s = c.solver
    ts = np.linspace(0, 1.5e-4, 4)
    y0 = c.random_state(0.05, 0.02, 5.0)
    rng = np.random.default_rng(1)
    K = 6

    def dots():
        return [{"fn_params": np.array([[[1.0 + k, 0.0, 0.0, 0.0, 0.0]]]), "k_bond": rng.normal(size=(1, len(c.bonds), 3))} for k in range(K)]

    seen = {}

    def solve_and_vjp(between, **kw):
        fields = s(y0, ts, c.cp, keep_trajectory=True, **kw)
        fb = np.random.default_rng(2).normal(size=fields.shape)
        between()
        return s.vjp(fb)

    def fixed_in_between():
        seen["fixed"] = s.engine.forward_tangent_multi(y0[None], rng.normal(size=(1, K, 2, c.geo.n_blocks, 3)), dots(), K, ts, 5)

    def dense_in_between():
        e = s.engine
        grid, ns = b.padded_step_times([e.adaptive_step_times(0)], ts[0])
        seen["dense"] = e.forward_tangent_dense_multi(y0[None], None, dots(), K, ts, grid, ns)

    for between, kw in ((fixed_in_between, dict(steps_per_interval=5)), (dense_in_between, dict())):
        if not kw:
            s.rtol = s.atol = 1e-5
        t1, s1 = solve_and_vjp(between, **kw)
        t0, s0 = solve_and_vjp(lambda: None, **kw)
        assert np.array_equal(np.asarray(s1), np.asarray(s0))           # to the bit
        for a, bb in zip(_leaves(t1), _leaves(t0)):
            assert np.array_equal(a, bb)
    assert s.stats["step_control"] == "adaptive-records"
    for key in ("fixed", "dense"):
        f, fd, _ = seen[key]
        assert fd.shape == (1, K, 4, 2, c.geo.n_blocks, 3) and np.abs(fd).max() > 0 and np.all(np.isfinite(f))
    # launches grow with the passes, ceil(K / widest), not with K; a lattice this small takes ONE pass when nothing is forced
    s.prepare(c.cp)
    per_pass = 2 + 15 * 6 + 3
    for forced in ("chunked", None):
        if forced:
            monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", forced)
        else:
            monkeypatch.delenv("DFX_TANGENT_MULTI_FORM")
        launches = {}
        for k in (1, 2, 3, WIDEST, WIDEST + 1, 2 * WIDEST, 2 * WIDEST + 1):
            _, _, st = s.engine.forward_tangent_multi(y0[None], None, dots()[:1] * k, k, ts, 5)
            launches[k] = st["launches"]
        assert all(launches[k] == (-(-k // WIDEST) if forced else 1) * per_pass for k in launches), (forced, launches)
    # n_dirs < 1 is refused with a message
    import ctypes as C
    rc = s.engine.lib.dfx_forward_tangent_multi(s.engine._h, None, None, None, 0, ts.ctypes.data_as(C.POINTER(C.c_double)), 4,
                                                np.full(3, 5, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)), None, 0, None, None, None)
    assert rc == 1 and b"direction" in s.engine.lib.dfx_last_error(s.engine._h)


def test_extra_ligaments_are_refused_before_any_pass():
    c = _case("quads", 4, True, False, seed=12, extra_bonds=[[1, 6], [9, 14]])
    ts = np.linspace(0, 1e-4, 3)
    y0 = c.random_state(0.05, 0.02, 5.0)
    tangents = [(None, ZERO._replace(constraint_params=dict(amplitude=1.0 + k))) for k in range(5)]
    s = c.solver
    s.rtol = s.atol = 1e-5
    for kw in (dict(steps_per_interval=4), dict(adaptive=True), dict()):
        solves = s.solve_count
        with pytest.raises(RuntimeError, match="more than one ligament"):
            s.jvp_multi(y0, ts, c.cp, tangents, **kw)
        assert s.solve_count == solves
    fields = s(y0, ts, c.cp, steps_per_interval=4)
    assert np.all(np.isfinite(fields)) and np.abs(fields).max() > 0
    # and a lattice without them on the same process still runs it
    c2 = _case("quads", 4, True, False, seed=12)
    _, fdots = c2.solver.jvp_multi(y0, ts, c2.cp, tangents, steps_per_interval=4)
    assert np.abs(fdots).max() > 0 and relerr(fdots[1], 2.0 * fdots[0]) < 1e-12


# ---- 8. the single-direction entries are the n_dirs = 1 ones ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_single_direction_entries_are_the_multi_entries_at_one_direction(lattice):
    """dfx_forward_tangent / dfx_forward_tangent_dense against dfx_forward_tangent_multi / dfx_forward_tangent_dense_multi at n_dirs = 1,
    to the bit: the same kernels on the same image, not two that agree to rounding.  4 x 4 quads and the 4-cell kagome lattice (4 and 3
    nodes per block), nonlinear ligaments, angle contact, a driven block, per-bond parameters, a non-zero state0_dot."""
    c = _case(lattice, 4, True, True, "dopri5")
    rng = np.random.default_rng(3)
    c.cp = _per_bond(c)
    cp, inertia = _explicit_inertia(c)
    s, e = c.solver, c.solver.engine
    ts = np.linspace(0, 3e-4, 4)
    y0, y0d = c.random_state(0.05, 0.02, 5.0)[None], c.random_state(0.05, 0.02, 5.0)[None]
    cps, _ = s.prepare(cp)
    params_dot = {k: v[None] for k, v in s._flatten_tangent(cps[0], _tangent_tree(c, rng, inertia)).items()}
    assert all(np.abs(params_dot[k]).max() > 0 for k in ("k_bond", "reference_vector", "void_angle0", "fn_params"))

    def same(one, multi, what):
        (f1, d1, st1), (fm, dm_, stm) = one, multi
        assert dm_.shape == (1, 1) + d1.shape[1:]
        assert np.abs(d1).max() > 0 and np.all(np.isfinite(d1))
        assert np.array_equal(f1, fm), (lattice, what, "fields", relerr(fm, f1))
        assert np.array_equal(d1, dm_[:, 0]), (lattice, what, "fields_dot", relerr(dm_[:, 0], d1))
        for key in ("steps", "rhs_evals", "launches"):
            assert st1[key] == stm[key], (lattice, what, key, st1[key], stm[key])
        return st1
    st = same(e.forward_tangent(y0, y0d, params_dot, ts, 4), e.forward_tangent_multi(y0, y0d[:, None], [params_dot], 1, ts, 4), "fixed grid")
    assert st["steps"] == 12 and st["rhs_evals"] == 12 * 6 and st["launches"] == 2 + 12 * 6 + 3
    # the accepted steps of one adaptive pass
    s.rtol = s.atol = 1e-5
    s(y0[0], ts, cp)
    assert s.stats["step_control"] == "adaptive"
    grid, ns = b.padded_step_times([e.adaptive_step_times(0)], ts[0])
    st = same(e.forward_tangent_dense(y0, y0d, params_dot, ts, grid, ns),
              e.forward_tangent_dense_multi(y0, y0d[:, None], [params_dot], 1, ts, grid, ns), "dense")
    assert st["steps"] == ns[0] > 0 and st["rhs_evals"] == 6 * ns[0] + 1
