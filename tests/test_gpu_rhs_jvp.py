"""dfx_rhs_jvp (Engine.rhs_jvp): forward mode of ONE right-hand-side evaluation, the twin of dfx_rhs_vjp.

Every case is checked in both pass forms (DFX_TANGENT_MULTI_FORM) on K = 5 directions (a pass of width 4 plus a tail of width 1 in the
chunked form), at a state taken from a few steps of a driven solve and a time inside the pulse:
  * dy against dfx_rhs (1e-13), rows of constrained DOFs exactly 0;
  * the transpose identity with dfx_rhs_vjp for a random lam (1e-12);
  * the columns of K = 5 against K = 3 and against five K = 1 calls (1e-12);
  * where the oracle has the leaves (Case / ShapeCase lattices): dy_dots against torch.autograd.functional.jvp through the oracle RHS, the
    one tests/parity.py holds dfx_rhs to, at that suite's bar for one RHS and its VJPs (1e-12 of the largest entry)."""
import ctypes as C

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import _binding as b

from .common import relerr
from .parity import RTOL_RHS, T64, oracle_member_leaves, shape_tangents
from .test_gpu_tangent import FAST, _case, _explicit_inertia, _per_bond, _tangent_tree

pytestmark = pytest.mark.gpu

K = 5                  # 4 + 1: one pass of the widest chunk and a tail
T_EVAL = 1.2e-4        # inside the pulse of FAST (on for 1e-5 < t < 1e-5 + 1 / 3000)
ORACLE_NAMES = ["cnv", "refv", "ks", "ksh", "kr", "inertia", "damping", "amplitude", "loading_rate", "input_delay"]
CONTACT_NAMES = ["min_angle", "cutoff_angle", "k_contact"]


@pytest.fixture(params=["chunked", "spread"])
def form(request, monkeypatch):
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", request.param)
    return request.param


def _driven_states(s, cps, rng, t=T_EVAL, spi=4):
    """(B, 2, nb, 3): every member's state after a few steps of its driven solve from a small random state."""
    B, nb = s.batch, s.n_blocks
    y0 = rng.normal(size=(B, 2, nb, 3)) * np.array([0.05, 0.05, 0.02])
    y0[:, 1] *= 5.0
    out = s(y0 if B > 1 else y0[0], np.array([0.0, t]), cps if B > 1 else cps[0], steps_per_interval=spi)
    return np.asarray(out).reshape(B, 2, 2, nb, 3)[:, -1].copy()


def _random_flat_dots(flats, rng):
    """K directions over every dfx_params array of the members, each entry of the size of the value it perturbs."""
    return [{name: np.stack([rng.normal(size=np.shape(f[name])) * (np.abs(f[name]) + 1e-12) for f in flats]) for name in flats[0]}
            for _ in range(K)]


def _engine_checks(s, flats, y, y_dots, params_dots, rng, expect_contact=False):
    """The checks that need no oracle.  Returns dy_dots (B, K, 2, nb, 3)."""
    e = s.engine
    B, nb = s.batch, s.n_blocks
    e.set_params(**{k: np.stack([f[k] for f in flats]) for k in flats[0]})
    con = s.constrained_DOF_ids
    dy, dd = e.rhs_jvp(y, T_EVAL, y_dots, params_dots, K)
    assert dd.shape == (B, K, 2, nb, 3) and np.all(np.isfinite(dd))
    e_dy = relerr(dy, e.rhs(y, T_EVAL))
    print("dy vs dfx_rhs", e_dy)
    assert e_dy < 1e-13
    assert np.all(dy.reshape(B, 2, -1)[:, :, con] == 0.0) and np.all(dd.reshape(B, K, 2, -1)[:, :, :, con] == 0.0)
    for k in range(K):
        assert np.abs(dd[:, k]).max() > 0.0
    # entries of y and y_dots on constrained DOFs are ignored
    y2, yd2 = y.copy(), y_dots.copy()
    y2.reshape(B, 2, -1)[:, :, con] += 1.0
    yd2.reshape(B, K, 2, -1)[:, :, :, con] += 1.0
    dy2, dd2 = e.rhs_jvp(y2, T_EVAL, yd2, params_dots, K)
    assert np.array_equal(dy2, dy) and np.array_equal(dd2, dd)
    # columns: K = 3 and five K = 1 calls
    dy3, dd3 = e.rhs_jvp(y, T_EVAL, y_dots[:, :3], params_dots[:3], 3)
    e3 = relerr(dd3, dd[:, :3])
    print("K = 3 vs K = 5", e3)
    assert e3 < 1e-12 and relerr(dy3, dy) < 1e-13
    for k in range(K):
        _, dd1 = e.rhs_jvp(y, T_EVAL, y_dots[:, k:k + 1], params_dots[k:k + 1], 1)
        e1 = relerr(dd1[:, 0], dd[:, k])
        print("column", k, "K = 1 vs K = 5", e1)
        assert e1 < 1e-12
    # NULL tangents are zero tangents
    _, dd0 = e.rhs_jvp(y, T_EVAL, None, None, 2)
    assert np.all(dd0 == 0.0)
    # the transpose of dfx_rhs_vjp
    lam = rng.normal(size=y.shape)
    y_bar, g = e.rhs_vjp(y, T_EVAL, lam)
    if expect_contact:
        assert np.abs(g["contact"]).max() > 0, "contact inactive: the test would be vacuous"
    lam_free = lam.copy()
    lam_free.reshape(B, 2, -1)[:, :, con] = 0.0
    for k in range(K):
        lhs = float(np.sum(lam_free * dd[:, k]))
        rhs = float(np.sum(y_bar * y_dots[:, k])) + sum(float(np.sum(g[name] * params_dots[k][name])) for name in g if name in params_dots[k])
        print("transpose, direction", k, lhs, rhs, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)
    return dd


def _oracle_columns(c, prims, tans, y, y_dots):
    """torch.autograd.functional.jvp through the oracle RHS, member by member and direction by direction: (B, K, 2, n_free)."""
    osol = c.oracle_solver()
    free = torch.as_tensor(osol.free_DOF_ids)
    names = ORACLE_NAMES + (CONTACT_NAMES if c.contact else [])
    out = []
    for m, prim in enumerate(prims):
        def f(yf, *xs):
            lv = dict(zip(names, xs))
            inertia = lv.pop("inertia")
            return osol.rhs(yf, T_EVAL, c.oracle_cp(lv), inertia.reshape(-1)[free], create_graph=True)
        cols = []
        for k in range(K):
            tan = tans[m][k]
            args = (T64(y[m].reshape(2, -1)[:, free]),) + tuple(T64(prim[n]) for n in names)
            dots = (T64(y_dots[m, k].reshape(2, -1)[:, free]),) + tuple(T64(np.broadcast_to(tan[n], np.shape(prim[n]))) for n in names)
            cols.append(torch.autograd.functional.jvp(f, args, dots)[1].numpy())
        out.append(np.stack(cols))
    return np.stack(out), np.asarray(osol.free_DOF_ids)


def _tree_leaves(cd, contact):
    md = cd.mechanical_params
    tan = dict(cnv=cd.geometrical_params.centroid_node_vectors, refv=md.bond_params.reference_vector, ks=md.bond_params.k_stretch,
               ksh=md.bond_params.k_shear, kr=md.bond_params.k_rot, inertia=md.inertia, damping=md.damping, **cd.constraint_params)
    if contact:
        tan.update(zip(CONTACT_NAMES, md.contact_params))
    return tan


def _scaled(cp, f):
    bp = cp.mechanical_params.bond_params
    bp = bp._replace(k_stretch=bp.k_stretch * f, k_shear=bp.k_shear / f, k_rot=bp.k_rot * f * f)
    return cp._replace(mechanical_params=cp.mechanical_params._replace(bond_params=bp, inertia=cp.mechanical_params.inertia * f))


def _lattice_check(c, rng):
    """A tests.common.Case of any batch: members with their own stiffnesses and inertia, every leaf seeded in every direction."""
    s = c.solver
    B, nb = s.batch, s.n_blocks
    c.cp = _per_bond(c)
    cp0, inertia = _explicit_inertia(c)
    cps = [_scaled(cp0, 1.0 + 0.1 * m) for m in range(B)]
    y = _driven_states(s, cps, rng)
    y_dots = rng.normal(size=(B, K, 2, nb, 3)) * np.abs(y).max((0, 2, 3))[:, None, None]
    trees = [[_tangent_tree(c, rng, inertia) for _ in range(K)] for _ in range(B)]
    flats = [s._flatten(cp) for cp in cps]
    params_dots = []
    for k in range(K):
        tf = [s._flatten_tangent(cps[m], trees[m][k]) for m in range(B)]
        params_dots.append({name: np.stack([f[name] for f in tf]) for name in tf[0]})
    dd = _engine_checks(s, flats, y, y_dots, params_dots, rng, expect_contact=c.contact)
    prims = []
    for cp in cps:
        mp = cp.mechanical_params
        prim = dict(cnv=c.cnv, refv=np.broadcast_to(c.refv, (len(c.bonds), 2)), ks=mp.bond_params.k_stretch, ksh=mp.bond_params.k_shear,
                    kr=mp.bond_params.k_rot, inertia=mp.inertia, damping=mp.damping, **FAST)
        if c.contact:
            prim.update(zip(CONTACT_NAMES, mp.contact_params))
        prims.append(prim)
    tans = [[_tree_leaves(trees[m][k], c.contact) for k in range(K)] for m in range(B)]
    ref, free = _oracle_columns(c, prims, tans, y, y_dots)
    for m in range(B):
        for k in range(K):
            err = relerr(dd[m, k].reshape(2, -1)[:, free], ref[m, k])
            print("member", m, "direction", k, "dy_dots vs oracle jvp", err)
            assert err < RTOL_RHS, (m, k, err)
    return s, cps, y, y_dots, params_dots, dd


# 8 x 8: more than one wave per member; kagome: 3 nodes per block, 128 blocks
@pytest.mark.parametrize("lattice,nonlinear,contact", [("quads", True, True), ("quads", True, False), ("quads", False, True),
                                                        ("quads", False, False), ("kagome", True, True)])
def test_rhs_jvp_8x8(lattice, nonlinear, contact, form):
    _lattice_check(_case(lattice, 8, nonlinear, contact, seed=21), np.random.default_rng(31))


def test_rhs_jvp_batch_3_of_49_blocks_and_the_pulse_tangent(form):
    """Member boundaries fall inside a wave (3 x 49 lanes); driven and clamped DOFs with a non-zero fn_params tangent inside the pulse."""
    c = _case("quads", 7, True, True, seed=22, batch=3)
    s, cps, y, y_dots, params_dots, dd = _lattice_check(c, np.random.default_rng(32))
    assert s.n_blocks == 49 and len(s.constrained_DOF_ids) > 0
    # the driven DOF moves with the pulse parameters: without their tangent the neighbours' accelerations change
    assert all(np.abs(p["fn_params"][:, 0, :3]).min() > 0 for p in params_dots)
    without = [dict(p, fn_params=np.zeros_like(p["fn_params"])) for p in params_dots]
    _, dd0 = s.engine.rhs_jvp(y, T_EVAL, y_dots, without, K)
    assert np.abs(dd0 - dd).max() > 1e-6 * np.abs(dd).max()


def test_rhs_jvp_non_uniform_image(form):
    """Stiffnesses per ligament (p_k) together with a dictionary of 17 reference vectors (the dictionary in global memory)."""
    from .param_shapes import ShapeCase, n_distinct
    sc = ShapeCase("refv_17", "quads", n=5, contact=True, nonlinear=True, seed=3)
    c, s = sc.c, sc.c.solver
    rng = np.random.default_rng(33)
    nbd = len(c.bonds)
    p = sc.members[0]
    p.update(ks=p["ks"] * (1 + 0.1 * rng.uniform(-1, 1, nbd)), ksh=p["ksh"] * (1 + 0.1 * rng.uniform(-1, 1, nbd)),
             kr=p["kr"] * (1 + 0.1 * rng.uniform(-1, 1, nbd)))
    assert n_distinct(p["refv"]) == 17 and all(np.ptp(p[k]) > 0 for k in ("ks", "ksh", "kr"))
    cp = sc.control_params(p)
    y = _driven_states(s, [cp], rng)
    y_dots = rng.normal(size=(1, K, 2, s.n_blocks, 3)) * np.abs(y).max((0, 2, 3))[:, None, None]
    dirs = [shape_tangents(sc, 40 + k)[0]["all"] for k in range(K)]
    params_dots = [{name: v[None] for name, v in s._flatten_tangent(cp, tree).items()} for _, tree, _ in dirs]
    dd = _engine_checks(s, [s._flatten(cp)], y, y_dots, params_dots, rng, expect_contact=True)
    prim = oracle_member_leaves(sc, p)
    prim.pop("state0")
    tans = [[{n: lv[n] for n in lv if n != "state0"} for _, _, lv in dirs]]
    ref, free = _oracle_columns(c, [prim], tans, y, y_dots)
    for k in range(K):
        err = relerr(dd[0, k].reshape(2, -1)[:, free], ref[0, k])
        print("direction", k, "dy_dots vs oracle jvp", err)
        assert err < RTOL_RHS, (k, err)


def _flat_space_check(c, rng):
    """Cases whose oracle builders do not take every leaf: all checks but the oracle's, on random tangents of every dfx_params array."""
    s = c.solver
    y = _driven_states(s, [c.cp], rng)
    flats = [s._flatten(c.cp)]
    y_dots = rng.normal(size=(1, K, 2, s.n_blocks, 3)) * np.abs(y).max((0, 2, 3))[:, None, None]
    return _engine_checks(s, flats, y, y_dots, _random_flat_dots(flats, rng), rng, expect_contact=bool(s.engine.contact))


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_rhs_jvp_distance_contact(lattice, form):
    from .test_distance_contact import DistCase
    c = DistCase(lattice, None, n=4 if lattice == "quads" else 3, seed=5)
    dd = _flat_space_check(c, np.random.default_rng(34))
    # and against the oracle on the leaves its builder takes: state, node vectors, block centroids, contact constants
    s = c.solver
    rng = np.random.default_rng(35)
    y = _driven_states(s, [c.cp], rng)
    flat = s._flatten(c.cp)
    osol = c.oracle_solver()
    free = torch.as_tensor(osol.free_DOF_ids)
    tan = dict(cnv=0.02 * rng.normal(size=c.cnv.shape), cen=0.05 * rng.normal(size=c.cen.shape), contact=0.05 * rng.normal(size=3))
    yd = rng.normal(size=y.shape) * np.abs(y).max((0, 2, 3))[:, None, None]
    tree = dm.ControlParams(dm.GeometricalParams(tan["cen"], tan["cnv"]), dm.MechanicalParams(None, None, None, None, dm.ContactParams(*tan["contact"])))
    s.engine.set_params(**{k: v[None] for k, v in flat.items()})
    # (inertia follows the node vectors in both: the tree leaves it None, the oracle computes it from cnv)
    _, got = s.engine.rhs_jvp(y, T_EVAL, yd[:, None], [{k: v[None] for k, v in s._flatten_tangent(c.cp, tree).items()}], 1)
    from oracle import ref_geometry as OG

    def f(yf, cnv, cen, c0, c1, c2):
        inertia = OG.compute_inertia(cnv, 6.18e-9)
        return osol.rhs(yf, T_EVAL, c.oracle_cp(cnv=cnv, cen=cen, contact=[c0, c1, c2]), inertia.reshape(-1)[free], create_graph=True)
    args = (T64(y[0].reshape(2, -1)[:, free]), T64(c.cnv), T64(c.cen)) + tuple(T64(v) for v in c.contact_params)
    dots = (T64(yd[0].reshape(2, -1)[:, free]), T64(tan["cnv"]), T64(tan["cen"])) + tuple(T64(v) for v in tan["contact"])
    ref = torch.autograd.functional.jvp(f, args, dots)[1].numpy()
    err = relerr(got[0, 0].reshape(2, -1)[:, free], ref)
    print("distance contact", lattice, "dy_dots vs oracle jvp", err)
    assert err < RTOL_RHS


@pytest.mark.parametrize("model", ["simple", "torsion"])
def test_rhs_jvp_spring_models(model, form):
    from .test_spring_models import SpringCase
    c = SpringCase(model, None, seed=5)
    _flat_space_check(c, np.random.default_rng(36))
    # and against the oracle on the leaves its builder takes: state, node vectors, stiffnesses, reference vectors
    s = c.solver
    rng = np.random.default_rng(37)
    y = _driven_states(s, [c.cp], rng)
    flat = s._flatten(c.cp)
    osol = c.oracle_solver()
    free = torch.as_tensor(osol.free_DOF_ids)
    tan = dict(cnv=0.02 * rng.normal(size=c.cnv.shape), ks=0.1 * rng.normal(size=c.ks.shape) * c.ks, kr=0.1 * rng.normal(size=c.kr.shape) * c.kr,
               refv=0.1 * rng.normal(size=(len(c.bonds), 2)))
    yd = rng.normal(size=y.shape) * np.abs(y).max((0, 2, 3))[:, None, None]
    bd = dm.LigamentParams(tan["ks"], None, None, tan["refv"]) if model == "simple" else dm.StretchingTorsionalSpringParams(tan["ks"], tan["kr"])
    tree = dm.ControlParams(dm.GeometricalParams(None, tan["cnv"]), dm.MechanicalParams(bd, None))
    s.engine.set_params(**{k: v[None] for k, v in flat.items()})
    _, got = s.engine.rhs_jvp(y, T_EVAL, yd[:, None], [{k: v[None] for k, v in s._flatten_tangent(c.cp, tree).items()}], 1)
    from oracle import ref_geometry as OG
    refv0 = np.broadcast_to(c.refv, (len(c.bonds), 2)).copy()

    def f(yf, cnv, ks, kr, refv):
        inertia = OG.compute_inertia(cnv, 6.18e-9)
        return osol.rhs(yf, T_EVAL, c.oracle_cp(cnv=cnv, ks=ks, kr=kr, refv=refv), inertia.reshape(-1)[free], create_graph=True)
    args = (T64(y[0].reshape(2, -1)[:, free]), T64(c.cnv), T64(c.ks), T64(c.kr), T64(refv0))
    dots = (T64(yd[0].reshape(2, -1)[:, free]), T64(tan["cnv"]), T64(tan["ks"]), T64(tan["kr"]), T64(tan["refv"]))
    ref = torch.autograd.functional.jvp(f, args, dots)[1].numpy()
    err = relerr(got[0, 0].reshape(2, -1)[:, free], ref)
    print("springs", model, "dy_dots vs oracle jvp", err)
    assert err < RTOL_RHS


def test_refusals():
    c = _case("quads", 4, True, False, seed=12, extra_bonds=[[1, 6], [9, 14]])
    s = c.solver
    s.prepare(c.cp)
    y = c.random_state(0.05, 0.02, 5.0)[None]
    with pytest.raises(RuntimeError, match="more than one ligament"):
        s.engine.rhs_jvp(y, T_EVAL, None, None, 2)
    c2 = _case("quads", 4, True, False, seed=12)
    e = c2.solver.engine
    c2.solver.prepare(c2.cp)
    dp = C.POINTER(C.c_double)
    dy = np.empty_like(y)
    rc = e.lib.dfx_rhs_jvp(e._h, y.ctypes.data_as(dp), T_EVAL, None, None, 0, dy.ctypes.data_as(dp), None)
    assert rc == 1 and b"direction" in e.lib.dfx_last_error(e._h)
    with pytest.raises(RuntimeError, match="direction"):
        e.rhs_jvp(y, T_EVAL, None, None, 0)
    # a non-finite state is reported
    bad = y.copy()
    bad[0, 0, 5, 0] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        e.rhs_jvp(bad, T_EVAL, None, None, 1)
    assert e.has_rhs_jvp and "dfx_rhs_jvp" in b.COMM_EXPORTS


def test_the_kept_solve_is_left_alone():
    """dfx_adjoint after dfx_rhs_jvp on the same handle: the gradient of the solve kept before it, bit for bit."""
    from .test_gpu_tangent_multi import _leaves
    c = _case("quads", 4, True, True, seed=14)
    s = c.solver
    ts = np.linspace(0, 1.5e-4, 4)
    y0 = c.random_state(0.05, 0.02, 5.0)
    rng = np.random.default_rng(1)

    def solve_and_vjp(between):
        fields = s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=5)
        fb = np.random.default_rng(2).normal(size=fields.shape)
        between(fields)
        return s.vjp(fb)

    def jvp_between(fields):
        dots = [{"k_bond": rng.normal(size=(1, len(c.bonds), 3))} for _ in range(K)]
        _, dd = s.engine.rhs_jvp(fields[-1][None], ts[-1], rng.normal(size=(1, K, 2, c.geo.n_blocks, 3)), dots, K)
        assert np.abs(dd).max() > 0

    t1, s1 = solve_and_vjp(jvp_between)
    t0, s0 = solve_and_vjp(lambda fields: None)
    assert np.array_equal(np.asarray(s1), np.asarray(s0))
    for a, bb in zip(_leaves(t1), _leaves(t0)):
        assert np.array_equal(a, bb)
