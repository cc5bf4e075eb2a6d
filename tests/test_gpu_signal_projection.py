"""-m gpu: signals projected on a time basis, evaluated and differentiated on the device (include/dfx.h: dfx_signal_projections,
dfx_signal_projection_value, dfx_signal_projection_value_and_grad; kernels k_signal_project / k_signal_project_residual in
difflexmm_amd/csrc/dfx_objective.h).

Yardstick (tests/projection_yardstick.py): the signals of tests/signal_yardstick.py on the history downloaded from the same kept solve,
P = B S, J = 1/2 sum W (P - Ptarget)^2 in torch fp64; autograd gives ``fields_bar`` and every explicit term, and ``dfx_adjoint(fields_bar)``
plus the explicit terms is the reference gradient, as tests/test_gpu_signal_misfit.py builds it.  Bars (same history, same fp64 arithmetic,
another summation order): projections 1e-12 of max_sj sum_k |B_jk S_ks|, value 1e-12, every gradient leaf 1e-11 of its largest reference
entry; the identity case (B = I, W = tau x omega, Ptarget = Starget against dfx_signal_misfit_value_and_grad) the same bars.

A time sum can cancel, so every comparison first asserts a condition on its INPUTS, on the yardstick's numbers alone: for every (member,
signal, row) with a non-zero weight kappa = sum_k |B_jk S_ks| / |P_sj - Ptarget_sj| <= 50.  Ptarget = P_yardstick * factor per member,
signal and row, the factors drawn from U(0.5, 1.5) as the signal-misfit test draws its targets; a factor closer to 1 than 0.25 is moved
to that distance (a draw of 1.01 alone makes kappa >= 100 whatever the basis).  The frequencies are chosen per lattice and time grid so that
no cos or sin row cancels by more than a factor 8 for any member and signal (checked on the CPU port's histories): the drive frequency of
the pulse (3000 Hz) and twice it where they qualify, replaced where they do not -- 6000 Hz on the 70-output grid of both lattices (on the
quads its cos row cancels to 1/455 for one signal), both on the 5 outputs of the kagome (sin row at 3000 Hz: 1/31).

Shapes: the ensembles of test_gpu_objective.py (quads 6x6 with the angle contact engaged, kagome 4x4, 3 members with different designs and
different targets), the 4-signal specification of test_gpu_signal_misfit.make_terms; two time grids -- the 5 outputs of that test (fewer
than one wave) and 70 outputs with 1 Dopri5 step per interval (lanes 0..5 carry two terms); bases of 6, 3 and 1 rows ((signal, row) pair
counts 24, 12, 4; the bond-model cases have 3 signals x 6 rows = 18 pairs, no multiple of the 4 waves of a workgroup); W with a zero
row, a negative entry and non-integer entries.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r20_signal_projection.txt):
projections 2.4e-15 of max sum |B S| (kagome, 5 outputs, 1 row); value 8.6e-15 (quads, 70 outputs, 1 row, kappa 11.2); gradient leaves
3.3e-14 (quads, 5 outputs, 3 rows, contact constants, kappa 14.0) over both lattices, both grids, the three bases, the five sweep forms
and the four bond models with and without the angle contact; the largest kappa of any input 28.6 (kagome, adaptive kept steps).  Identity
basis against the signal misfit: value 1.4e-16, every gradient leaf bit-identical.  TargetBandPower: 8.8e-9 for the directional
derivatives against central differences, 0 between one design and member 0 of the list, 1.3e-15 host path against device path.  No bar
was missed."""
import math

import numpy as np
import pytest

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import projection_yardstick as PY
from .common import Case, relerr
from .model_matrix import ModelCase
from .test_gpu_objective import BATCH, FAST, FOCUS_KW, PATHS, SPI, TAU, TS, Ensemble, _spin_damping, _with_env
from .test_gpu_signal_misfit import ALL, DESIGN, MODEL_NAMES, OMEGA, host, make_terms, member_leaves

pytestmark = pytest.mark.gpu

TOL_PROJECTION, TOL_VALUE, TOL_GRAD = 1e-12, 1e-12, 1e-11
WAVES_PER_WORKGROUP = 4                                                                 # kObjWaves: (signal, row) pairs per workgroup
GRIDS = {"5 outputs": (TS, SPI), "70 outputs": (np.linspace(0.0, 4e-4, 70), 1)}
DRIVE_HZ = FAST["loading_rate"]
# (drive frequency, twice it, one incommensurate with both) where those rows do not cancel; replacements where they do (module docstring)
FREQUENCIES = {("quads", "5 outputs"): (DRIVE_HZ, 2 * DRIVE_HZ, 1770.0), ("quads", "70 outputs"): (DRIVE_HZ, 2318.0, 1633.0),
               ("kagome", "5 outputs"): (2318.0, 4373.0, 1496.0), ("kagome", "70 outputs"): (DRIVE_HZ, 1633.0, 811.0)}
# (the adaptive solve of the kagome is another history than its fixed-grid solve: other rows cancel on it)
PATH_FREQUENCIES = {("kagome", "adaptive-kept-steps"): (DRIVE_HZ, 6565.0, 1633.0)}
# (quads 4x4, 5 outputs: neither 3000 Hz nor 6000 Hz qualifies for all three signals under any of the bond models)
MODEL_FREQUENCIES = {"nonlinear": (2318.0, 6839.0, 1085.0), "linearized": (2455.0, 6702.0, 1085.0), "simple": (2318.0, 6565.0, 1359.0),
                     "torsion": (2044.0, 4921.0, 1085.0)}
NS = 4


def solve(e, grid):
    ts, spi = GRIDS[grid] if isinstance(grid, str) else grid
    return e.c.solver(np.zeros((2, e.nb, 3)), ts, e.cps, keep_trajectory=True, steps_per_interval=spi)


def graphs_of(e, fields):
    return [PY.MemberGraph(fields[m], e.leaves[m], e.c.bonds, e.terms, NS) for m in range(BATCH)]


def check_inputs(tag, graphs, B, W, Pt):
    """the condition on the inputs, on the yardstick's numbers; returns (S, P) of the yardstick"""
    S = np.stack([g.signal_values() for g in graphs])
    Pr = np.stack([g.projections(B) for g in graphs])
    k = PY.kappa(B, S, Pr, np.broadcast_to(Pt, Pr.shape), W)
    print(f"[signal projection] {tag}: kappa of the inputs {k.max():.1f} (bound {PY.KAPPA_MAX:.0f})")
    assert np.isfinite(k).all() and k.max() <= PY.KAPPA_MAX, (tag, float(k.max()))
    return S, Pr, float(k.max())


def reference(eng, graphs, B, W, Pt, which):
    """value (B,), raw reference gradients: dfx_adjoint on the autograd cotangent + the autograd explicit terms."""
    Pt = np.broadcast_to(Pt, (len(graphs),) + np.shape(Pt)[-2:])
    res = [g.value_and_grads(B, W, Pt[m]) for m, g in enumerate(graphs)]
    fb = np.stack([r[1] for r in res])
    ref, _ = eng.adjoint(fb, which=which)
    ref = {k: np.array(v) for k, v in ref.items()}
    for m, (_, _, g) in enumerate(res):
        ref["centroid_node_vectors"][m] += g["cnv"]
        if "void_angle0" in ref and "phi0" in g:
            ref["void_angle0"][m] += g["phi0"]
        if "reference_vector" in ref:
            ref["reference_vector"][m] += g["refv"]
        if "k_bond" in ref:
            ref["k_bond"][m] += np.stack([g["ks"], g["ksh"], g["kr"]], 1)
        if "contact" in ref and "am" in g:
            ref["contact"][m] += np.array([g["am"], g["ac"], g["kc"]])
    return np.array([r[0] for r in res]), ref, fb, [r[2] for r in res]


def compare(tag, obj, out, val, ref, kap=None, tol=TOL_GRAD, tol_value=TOL_VALUE):
    worst = {"value": float(np.abs(obj - val).max() / np.abs(val).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[signal projection] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + ("" if kap is None else f" (kappa {kap:.1f})"))
    bad = {k: v for k, v in worst.items() if not v <= (tol_value if k == "value" else tol)}
    assert not bad, (tag, bad, kap)
    return worst


class Inputs:
    """basis, row weights and per-member targets of one (grid, basis): fixed from the first solve on"""

    def __init__(self, B, W, Pt):
        self.B, self.W, self.Pt = B, W, Pt


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    """The ensemble of test_gpu_objective.py with the terms of the signal-misfit test; per grid and basis the targets are the yardstick's
    projections of a first solve times a factor per member, signal and row (fixed inputs from then on)."""
    e = Ensemble(request.param)
    e.lattice = request.param
    e.terms, e.force_blocks, e.listed = make_terms(e.c)
    e.leaves = [member_leaves(e.c, e.cps, m) for m in range(BATCH)]
    e.inputs = {}
    rng = np.random.default_rng(37)
    for grid, (ts, _) in GRIDS.items():
        fields = np.array(_with_env({}, lambda: solve(e, grid)))
        graphs = graphs_of(e, fields)
        for name, (B, W) in PY.make_bases(ts, FREQUENCIES[request.param, grid], NS).items():
            Pr = np.stack([g.projections(B) for g in graphs])
            e.inputs[grid, name] = Inputs(B, W, PY.make_targets(Pr, rng))
    return e


def test_the_inputs_are_the_ones_the_kernels_can_go_wrong_on(ens):
    assert len(GRIDS["5 outputs"][0]) < 64 < len(GRIDS["70 outputs"][0]) and len(GRIDS["70 outputs"][0]) % 64 == 6
    pairs = {name: NS * ens.inputs["5 outputs", name].B.shape[0] for name in ("6 rows", "3 rows", "1 row")}
    assert pairs == {"6 rows": 24, "3 rows": 12, "1 row": 4}
    assert (3 * 6) % WAVES_PER_WORKGROUP != 0                                            # the bond-model cases: a workgroup with idle waves
    for grid in GRIDS:
        for name in pairs:
            i = ens.inputs[grid, name]
            assert i.B.shape == (pairs[name] // NS, len(GRIDS[grid][0])) and i.Pt.shape == (BATCH,) + i.W.shape
            assert (i.W < 0).any() and (i.W == 0).any() and (i.W != np.round(i.W)).any()
            if name != "1 row":
                assert (i.W == 0).all(0).any() and not (i.W == 0).all(0).all()           # a basis row nobody weighs
            assert len(set(np.round(i.Pt[:, 0, 0] / np.abs(i.Pt[:, 0, 0]).max(), 9))) == BATCH


# ---- 1. projections --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_projections(ens, grid):
    c = ens.c

    def run():
        fields = np.array(solve(ens, grid))
        return fields, {name: c.solver.signal_projections(O.ProjectionSpec(O.SignalSpec(ens.terms, NS), ens.inputs[grid, name].B,
                                                                           ens.inputs[grid, name].W)) for name in ("6 rows", "3 rows", "1 row")}
    fields, out = _with_env({}, run)
    graphs = graphs_of(ens, fields)
    S = np.stack([g.signal_values() for g in graphs])
    for name, Pd in out.items():
        B = ens.inputs[grid, name].B
        ref = np.stack([g.projections(B) for g in graphs])
        scale = PY.projection_scale(B, S)
        err = float(np.abs(Pd - ref).max() / scale)
        print(f"[signal projection] {ens.lattice} {grid} {name}: projections against the yardstick {err:.2e} of max sum |B S| = {scale:.3e}")
        assert Pd.shape == ref.shape == (BATCH, NS, B.shape[0]) and np.abs(ref).min() > 0
        assert err <= TOL_PROJECTION
    # the rows of the smaller sets are rows of the 6-row set: the same sums, the same bits
    assert np.array_equal(out["3 rows"], out["6 rows"][:, :, [0, 1, 3]]) and np.array_equal(out["1 row"], out["6 rows"][:, :, [1]])


# ---- 2. value and raw gradients: both grids, the three bases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_value_and_gradients_on_both_grids_and_every_basis(ens, grid):
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(solve(ens, grid))
        graphs = graphs_of(ens, fields)
        res = {}
        for name in ("6 rows", "3 rows", "1 row"):
            i = ens.inputs[grid, name]
            val, ref, fb, explicit = reference(eng, graphs, i.B, i.W, i.Pt, ALL)
            obj, out, _ = eng.signal_projection_value_and_grad(ens.terms, NS, i.B, i.W, i.Pt, which=ALL)
            obj, out = obj.copy(), host(out)
            obj_d, out_d, _ = eng.signal_projection_value_and_grad(ens.terms, NS, i.B, i.W, i.Pt, which=DESIGN)
            res[name] = (val, ref, fb, obj, out, obj_d.copy(), host(out_d), eng.signal_projection_value(ens.terms, NS, i.B, i.W, i.Pt))
        return graphs, res
    graphs, res = _with_env({}, run)
    for name, (val, ref, fb, obj, out, obj_d, out_d, only) in res.items():
        i = ens.inputs[grid, name]
        tag = f"{ens.lattice} {grid} {name}"
        _, _, kap = check_inputs(tag, graphs, i.B, i.W, i.Pt)
        assert np.array_equal(only, obj) and np.array_equal(obj_d, obj)          # one reduction on one history
        assert set(out) == set(ALL) and set(out_d) == set(DESIGN), (tag, sorted(out))
        # position rows (force and displacement terms) and, where signal 2 carries a weight, velocity rows
        assert np.abs(fb[:, :, 0]).max() > 0 and (np.abs(fb[:, :, 1]).max() > 0) == bool((i.W[2] != 0).any())
        engaged = c.geo.n_npb == 4
        assert all(np.abs(ref[k]).max() > 0 for k in ALL if engaged or k not in ("void_angle0", "contact")), tag
        compare(tag, obj, out, val, ref, kap)
        compare(tag + " (design leaves)", obj_d, out_d, val, {k: ref[k] for k in DESIGN}, kap)


# ---- 3. every form of the sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c
    i = Inputs(*PY.make_bases(TS, PATH_FREQUENCIES.get((ens.lattice, path), FREQUENCIES[ens.lattice, "5 outputs"]), NS)["6 rows"], None)

    def run():
        fields = np.array(solve(ens, (TS, spi)))
        st_f = dict(c.solver.stats)
        graphs = graphs_of(ens, fields)
        # (the histories of the sweep forms differ: the targets are drawn around the yardstick's projections of THIS solve)
        Pt = PY.make_targets(np.stack([g.projections(i.B) for g in graphs]), np.random.default_rng(41))
        val, ref, fb, explicit = reference(eng, graphs, i.B, i.W, Pt, ALL)
        obj, out, _ = eng.signal_projection_value_and_grad(ens.terms, NS, i.B, i.W, Pt, which=ALL)
        obj, out = obj.copy(), host(out)
        obj_d, out_d, st = eng.signal_projection_value_and_grad(ens.terms, NS, i.B, i.W, Pt, which=DESIGN)
        return st_f, graphs, Pt, val, ref, explicit, obj, out, obj_d.copy(), host(out_d), st
    st_f, graphs, Pt, val, ref, explicit, obj, out, obj_d, out_d, st = _with_env(env, run)
    tag = f"{ens.lattice} {path}"
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    elif path == "stage-launches":
        assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
    elif path == "persistent":                     # without per-ligament gradients the persistent builds stay eligible
        assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
    elif path == "stages":
        assert st["stage_checkpoint"] == 1, st
    elif path == "segments":
        assert st["checkpoint_records"] == 2, st
    _, _, kap = check_inputs(tag, graphs, i.B, i.W, Pt)
    assert np.array_equal(obj_d, obj) and set(out) == set(ALL) and set(out_d) == set(DESIGN)
    # the moment terms reach the bending stiffness and, on the quads, the contact constants through the EXPLICIT terms
    engaged = c.geo.n_npb == 4
    assert all(np.abs(g["kr"]).max() > 0 for g in explicit) and (not engaged or all(np.abs(g["kc"]) > 0 for g in explicit))
    compare(tag, obj, out, val, ref, kap)
    compare(tag + " (design leaves)", obj_d, out_d, val, {k: ref[k] for k in DESIGN}, kap)


@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_every_bond_model_with_and_without_the_angle_contact(hip_lib, model, contact):
    """Quads 4x4, one member, per-ligament stiffnesses, 3 signals x 6 rows: every leaf against the yardstick written with that model's
    energy."""
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    nbd, p = len(mc.bonds), mc.members[0]
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
    nb = mc.geo.n_blocks
    driven, corner = int(mc.con[0, 0]), nb - 1
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7), (1, 0, 7, -1.3), (1, corner, 8, 0.9), (1, 5, 8, 0.5), (1, 5, 6, -0.2), (2, 6, 1, 2.0), (2, 6, 3, 1e-4)]
    eng = mc.solver.engine
    B, W = PY.make_bases(TS, MODEL_FREQUENCIES[model], 3)["6 rows"]

    def run():
        fields = np.array(mc.solver(np.zeros((2, nb, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
        graphs = [PY.MemberGraph(fields, lv, mc.bonds, terms, 3, MODEL_NAMES[model])]
        Pr = graphs[0].projections(B)[None]
        Pt = PY.make_targets(Pr, np.random.default_rng(3))
        val, ref, fb, explicit = reference(eng, graphs, B, W, Pt, ALL)
        obj, out, _ = eng.signal_projection_value_and_grad(terms, 3, B, W, Pt, which=ALL)
        return graphs, Pt, val, ref, obj.copy(), host(out), eng.signal_projections(terms, 3, B)
    graphs, Pt, val, ref, obj, out, Pd = _with_env({}, run)
    tag = f"quads 4x4 {model} contact={contact}"
    S, Pr, kap = check_inputs(tag, graphs, B, W, Pt)
    e_p = float(np.abs(Pd - Pr).max() / PY.projection_scale(B, S))
    print(f"[signal projection] {tag}: projections {e_p:.2e}")
    assert Pd.shape == (1, 3, 6) and e_p <= TOL_PROJECTION
    assert np.abs(val).max() > 0 and np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
    if contact:
        assert np.abs(ref["contact"]).max() > 0 and np.abs(ref["void_angle0"]).max() > 0
    compare(tag, obj, out, val, ref, kap)


# ---- 4. the identity: B = I, W = tau x omega, Ptarget = Starget is the signal misfit -----------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_identity_basis_is_the_signal_misfit(ens, grid):
    eng = ens.c.solver.engine
    T = len(GRIDS[grid][0])
    rng = np.random.default_rng(11)
    tau = TAU if T == len(TAU) else np.where(np.arange(T) == 0, 0.0, rng.uniform(0.25, 2.0, T))

    def run():
        solve(ens, grid)
        S = eng.signal_values(ens.terms, NS)
        Starget = S * rng.uniform(0.5, 1.5, S.shape)
        a = eng.signal_misfit_value_and_grad(ens.terms, NS, Starget, OMEGA, tau, which=ALL)
        a = (a[0].copy(), host(a[1]))
        b = eng.signal_projection_value_and_grad(ens.terms, NS, np.eye(T), OMEGA[:, None] * tau[None, :], np.swapaxes(Starget, 1, 2), which=ALL)
        return a, (b[0].copy(), host(b[1])), eng.signal_projections(ens.terms, NS, np.eye(T)), S
    a, b, Pd, S = _with_env({}, run)
    assert np.array_equal(Pd, np.swapaxes(S, 1, 2))                            # one term per sum: the signals themselves
    assert np.abs(a[0]).min() > 0 and set(a[1]) == set(b[1]) == set(ALL)
    compare(f"{ens.lattice} {grid} identity basis against the signal misfit", b[0], b[1], a[0], a[1])


# ---- 5. repeatability, shared targets, no targets, nothing left behind -----------------------------------------------------------------------------
def test_two_calls_return_the_same_bits_and_nothing_is_left_behind(ens):
    eng, c = ens.c.solver.engine, ens.c
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    i = ens.inputs["70 outputs", "6 rows"]
    j = ens.inputs["70 outputs", "3 rows"]

    def call(inp, targets, device=False):
        obj, out, _ = eng.signal_projection_value_and_grad(ens.terms, NS, inp.B, inp.W, targets, which=which, device=device)
        return obj.copy(), ({k: x.to_host() for k, x in out.items()} if device else host(out))

    def run():
        fields = np.array(solve(ens, "70 outputs"))
        fb = np.random.default_rng(2).normal(size=fields.shape)
        p1 = eng.signal_projections(ens.terms, NS, i.B)
        r1 = call(i, i.Pt)
        other = call(j, j.Pt)
        p2 = eng.signal_projections(ens.terms, NS, i.B)
        r2, r3 = call(i, i.Pt), call(i, i.Pt, device=True)
        shared, per_member = call(i, i.Pt[1]), call(i, np.broadcast_to(i.Pt[1], i.Pt.shape).copy())
        none, zeros = call(i, None), call(i, np.zeros_like(i.Pt))
        v = eng.signal_projection_value(ens.terms, NS, i.B, i.W, i.Pt)
        after = host(c.solver.vjp_raw(fb, which=which))
        fresh = np.array(solve(ens, "70 outputs"))
        before = host(c.solver.vjp_raw(fb, which=which))
        return fields, fresh, p1, p2, r1, r2, r3, other, shared, per_member, none, zeros, v, after, before
    fields, fresh, p1, p2, r1, r2, r3, other, shared, per_member, none, zeros, v, after, before = _with_env({}, run)
    same = lambda x, y: np.array_equal(x[0], y[0]) and set(x[1]) == set(y[1]) and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])     # noqa: E731
    assert np.abs(r1[0]).min() > 0 and all(np.abs(r1[1][k]).max() > 0 for k in which if k != "void_angle0" or c.geo.n_npb == 4)
    assert np.array_equal(p1, p2) and same(r1, r2) and same(r1, r3), "two identical calls, device views"
    assert np.array_equal(v, r1[0]) and not same(r1, other)
    assert same(shared, per_member), "shared targets against the same targets per member"
    assert same(none, zeros) and not same(none, r1), "targets of None against explicit zeros"
    # a vjp after the calls serves the same kept solve as one on a fresh solve of the same problem
    assert np.array_equal(fields, fresh) and all(np.array_equal(after[k], before[k]) for k in which)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_the_next_adjoint_is_unaffected(ens):
    eng, c = ens.c.solver.engine, ens.c
    T, nb = len(TS), c.geo.n_blocks
    i = ens.inputs["5 outputs", "3 rows"]
    one = [(0, 1, 6, 1.0)]
    B1, W1 = np.ones((2, T)), np.ones((1, 2))
    fresh = Case("quads", 4, True, False, seed=3)
    one_driven = [(0, int(fresh.con[0, 0]), 6, 1.0)]
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.signal_projections(one, 1, B1)
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.signal_projection_value(one, 1, B1, W1)
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        fresh.solver.engine.signal_projection_value_and_grad(one, 1, B1, W1)
    _with_env({}, lambda: fresh.solver(np.zeros((2, 16, 3)), TS, fresh.cp._replace(constraint_params=dict(FAST)), steps_per_interval=SPI))
    assert fresh.solver.engine.signal_projection_value(one_driven, 1, B1, W1)[0] > 0                  # any forward pass serves the value ...
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):          # ... the gradient needs the kept trajectory
        fresh.solver.engine.signal_projection_value_and_grad(one, 1, B1, W1)
    fields = np.array(_with_env({}, lambda: solve(ens, "5 outputs")))
    fb = np.random.default_rng(6).normal(size=fields.shape)
    which = ("centroid_node_vectors", "inertia", "fn_params")
    before = host(eng.adjoint(fb, which=which)[0])
    good = eng.signal_projection_value(ens.terms, NS, i.B, i.W, i.Pt)
    calls = (lambda t, n, B, W, tg=None: eng.signal_projection_value_and_grad(t, n, B, W, tg),
             lambda t, n, B, W, tg=None: eng.signal_projection_value(t, n, B, W, tg),
             lambda t, n, B, W, tg=None: eng.signal_projections(t, n, B))
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="n_rows must be at least 1"):
            call(one, 1, np.zeros((0, T)), np.zeros((1, 0)))
        with pytest.raises(RuntimeError, match="non-finite basis entry"):
            call(one, 1, np.where(np.arange(T) == T - 1, np.nan, B1), W1)
        if k < 2:
            with pytest.raises(RuntimeError, match="non-finite row weight"):
                call(one, 1, B1, np.array([[1.0, np.inf]]))
            with pytest.raises(RuntimeError, match="non-finite target"):
                call(one, 1, B1, W1, np.array([[0.0, np.nan]]))
            with pytest.raises(RuntimeError, match="non-finite target"):
                call(one, 1, B1, W1, np.where(np.arange(BATCH)[:, None, None] == BATCH - 1, np.nan, np.zeros((BATCH, 1, 2))))
        # everything the signal entries refuse
        with pytest.raises(RuntimeError, match=f"names block {nb} out of range"):
            call([(0, nb, 6, 1.0)], 1, B1, W1)
        with pytest.raises(RuntimeError, match="names component 9 out of range"):
            call([(0, 1, 9, 1.0)], 1, B1, W1)
        with pytest.raises(RuntimeError, match="names signal 2 out of range"):
            call([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 2, B1, np.ones((2, 2)))
        with pytest.raises(RuntimeError, match="signal 1 is empty"):
            call([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 3, B1, np.ones((3, 2)))
    # NULL arrays: through the C entries themselves (the binding converts its arrays before it calls)
    args, keep = eng._signal_terms(one, 1)
    from difflexmm_amd._binding import _ptr
    out = np.zeros(BATCH)
    for call, what in ((lambda: eng.lib.dfx_signal_projection_value(eng._h, *args, None, 2, _ptr(W1), None, 0, _ptr(out)), "basis is NULL"),
                       (lambda: eng.lib.dfx_signal_projection_value(eng._h, *args, _ptr(B1), 2, None, None, 0, _ptr(out)), "row_weights is NULL"),
                       (lambda: eng.lib.dfx_signal_projection_value_and_grad(eng._h, *args, _ptr(B1), 2, None, None, 0, _ptr(out), None, None, 0, None),
                        "row_weights is NULL"),
                       (lambda: eng.lib.dfx_signal_projections(eng._h, *args, None, 2, _ptr(np.zeros((BATCH, 1, 2)))), "basis is NULL")):
        rc = call()
        assert rc == 1 and what in eng.lib.dfx_last_error(eng._h).decode(), (rc, what, eng.lib.dfx_last_error(eng._h))
    # shapes the binding can check itself
    with pytest.raises(ValueError):
        eng.signal_projection_value(one, 1, np.ones((2, T + 1)), W1)
    with pytest.raises(ValueError):
        eng.signal_projection_value(one, 1, B1, np.ones((2, 2)))
    with pytest.raises(ValueError):
        eng.signal_projection_value(one, 1, B1, W1, np.zeros((BATCH + 1, 1, 2)))
    # after the refusals the next dfx_adjoint on the handle is unaffected, and the handle still answers and solves
    after = host(eng.adjoint(fb, which=which)[0])
    assert all(np.array_equal(after[k], before[k]) and np.abs(before[k]).max() > 0 for k in which)
    assert np.array_equal(eng.signal_projection_value(ens.terms, NS, i.B, i.W, i.Pt), good)
    obj, out, _ = eng.signal_projection_value_and_grad(ens.terms, NS, i.B, i.W, i.Pt, which=("inertia",))
    assert np.array_equal(obj, good) and np.abs(out["inertia"]).max() > 0
    again = np.array(_with_env({}, lambda: solve(ens, "5 outputs")))
    assert np.array_equal(again, fields)
    # force components with the distance-based contact are refused, field components are served there
    mc = ModelCase("quads", "nonlinear", "distance", 4, "uniform", batch=1)
    _with_env({}, lambda: mc.solver(np.zeros((2, 16, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
    for call in (lambda: mc.solver.engine.signal_projection_value_and_grad(one, 1, B1, W1), lambda: mc.solver.engine.signal_projections(one, 1, B1)):
        with pytest.raises(RuntimeError, match="distance-based contact energy is not part of the signal channels"):
            call()
    v, g, _ = mc.solver.engine.signal_projection_value_and_grad([(0, 5, 0, 1.0), (0, 6, 4, 1e-4)], 1, B1, W1, which=("centroid_node_vectors", "block_centroids"))
    assert v[0] > 0 and np.abs(g["centroid_node_vectors"]).max() > 0


# ---- 7. the problem classes ----------------------------------------------------------------------------------------------------------------------
def _forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **{**FOCUS_KW, "n_timepoints": 7})
    fw.setup()
    return fw


def test_target_band_power_directional_derivatives(hip_lib):
    """TargetBandPower on quads 6x6 (7 outputs, Hann window): the velocity of three block DOFs at the drive frequency (maximised: negative
    weights) and at a second frequency (penalised), for a list of 3 designs as one ensemble: directional derivatives along random design
    directions against central differences of ``value`` with the relative step 1e-6 and the 1e-6 bar of TargetSignalMisfit's case in
    test_gpu_signal_misfit.py; a one-design call with on_device=True equals member 0 of the list call to 1e-13; the host path equals the
    device path to 1e-12."""
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(19)
    base = fw1.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    block_dofs, freqs, weights = [(16, 0), (21, 2), (20, 1)], [FOCUS_KW["loading_rate"], 1100.0], [-1.0, 0.25]
    many = P.TargetBandPower(fw3, block_dofs, "velocity", freqs, weights, window="hann")
    assert isinstance(many, P.TargetSignalProjection) and many.spec.basis.shape == (4, 7) and many.spec.row_weights.shape == (3, 4)
    assert np.array_equal(many.spec.basis, O.fourier_basis(fw3.timepoints, freqs, "hann"))
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and (v != 0).all()
    assert np.allclose(many.value(designs), v, rtol=1e-13, atol=0.0)
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
        print(f"[signal projection] TargetBandPower, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.TargetBandPower(fw1, block_dofs, "velocity", freqs, weights, window="hann")
    v1, g1 = single.value_and_grad(designs[0], on_device=True)
    e_v = abs(v1 - v[0]) / abs(v[0])
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[signal projection] TargetBandPower, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13
    vh, gh = single.value_and_grad(designs[0])
    e_v = abs(vh - v1) / abs(v1)
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(gh, g1))
    print(f"[signal projection] TargetBandPower, host path against device path: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert e_v <= 1e-12 and e_g <= 1e-12
    # a longer list runs in chunks of the ensemble width; per-member targets are cut alike
    tg = rng.normal(size=(6, 3, 4)) * 1e-3
    chunked = P.TargetSignalProjection(fw3, many.spec.with_targets(tg))
    v6 = chunked.value(designs + designs[::-1])
    halves = [P.TargetSignalProjection(fw3, many.spec.with_targets(tg[k:k + 3])).value(d) for k, d in ((0, designs), (3, designs[::-1]))]
    assert v6.shape == (6,) and np.array_equal(v6, np.concatenate(halves))
    with pytest.raises(ValueError, match="force components are evaluated on the device only"):
        P.TargetSignalProjection(fw1, O.ProjectionSpec(O.SignalSpec([(0, 14, 6, 1.0)], 1), many.spec.basis, np.ones((1, 4)))).value_and_grad(designs[0])
    with pytest.raises(ValueError, match="weights must be"):
        P.TargetBandPower(fw1, block_dofs, "velocity", freqs, [1.0, 2.0, 3.0])
