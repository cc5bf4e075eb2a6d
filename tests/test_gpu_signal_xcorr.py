"""-m gpu: the cross-correlation of signal pairs over time lags, its peak and its delay, evaluated and differentiated on the device
(include/dfx.h: dfx_signal_xcorr, dfx_signal_xcorr_value, dfx_signal_xcorr_value_and_grad; kernels k_signal_xcorr / k_signal_xcorr_reduce /
k_signal_xcorr_residual in difflexmm_amd/csrc/dfx_objective.h).

Yardstick (tests/xcorr_yardstick.py): the differentiable signals of tests/projection_yardstick.MemberGraph on the history downloaded from
the same kept solve, R, rho, the reduction and J in torch fp64; autograd gives ``fields_bar`` and every explicit term, and
``dfx_adjoint(fields_bar)`` plus the explicit terms is the reference gradient, as tests/test_gpu_signal_projection.py builds it.  Bars (the
projection test's: same history, same fp64 arithmetic, another summation order): rho 1e-12 of max_d sum |A B| / N, J and M 1e-12, delta
1e-12 x max(D, 1), every gradient leaf 1e-11 of its largest reference entry.

Every comparison first asserts the conditions on its INPUTS, on the yardstick's numbers alone (xcorr_yardstick.conditions): at every lag
with g_d != 0 sum |A B| / |R[d]| <= 50; for "max" a gap of at least 1e-3 of the peak between the two largest rho; for "softmax"
beta (max rho - min rho) <= 30 and (|w_peak| + 2 |w_delay| |delta - delta_target| beta D) max_d sum |A B| / N / |J| <= 50.  The inputs were
chosen on the CPU port's histories so that every case meets them: the pairs below (a force signal against another, two template pairs that
share signal 0, signal 2 with itself); per-member templates = the member's own signals 1 and 0 of a first solve shifted by two outputs,
scaled by a factor from U(0.5, 1.5), plus a smooth bump (seed 40: the correlation peaks at delay 2, no lag of the softmax cases cancels by
more than a factor 12); the softmax over 7 lags on 5 outputs and over 17 lags on 70 outputs (over all 139 lags of the 70 outputs some R[d]
cancels to 1/290: there the "at" and "max" reductions run, which put a cotangent on one lag); beta = 4; w_delay = 1 / (beta D); delta_target
1.5 outputs above the largest delta of the members.

Shapes: the ensembles of test_gpu_objective.py (quads 6x6 with the angle contact engaged, kagome 4x4, 3 members with different designs
and different templates), the 4-signal terms of test_gpu_signal_misfit.make_terms; the 5-output grid (fewer outputs than lanes) and the
70-output grid (lanes 0..5 carry two terms); D = 0; D = 3 on 5 outputs (7 lags, clipped on both sides); D = 69 on 70 outputs (139 lags
+ 2 energy rows = 141 rows, no multiple of the 4 waves of a workgroup).

One member with N == 0: a clamped DOF is clamped in every member, so A = the displacement of a clamped DOF under "reference" makes EVERY
member's N zero (checked: all NaN, all leaves exactly zero); one member alone gets N == 0 under "coefficient" with per-member templates of
which that member's column is all zero (checked: that member NaN with exactly zero leaves, the other two against the yardstick).

Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r22_signal_xcorr.txt): rho 2.1e-15 of
max sum |A B| / N (quads 4x4, nonlinear with the angle contact); J 4.3e-15 and M 4.2e-15 (kagome, 5 outputs, "at" / "none"); delta 1.1e-15 x D;
gradient leaves 5.9e-14 (quads 4x4, torsion springs, fn_params) over both lattices, both grids, the reductions, the five sweep forms and
the four bond models with and without the angle contact; the conditions of the inputs at worst kappa 17.3 (kagome, adaptive kept steps), gap
1.5e-2 (kagome, 70 outputs), beta x spread 4.5, amplification 5.9.  One template pair under "none" against dfx_signal_projections:
bit-identical.  TargetCrossCorrelation: 3.1e-8 for the directional derivatives against central differences, 0 between one design and
member 0 of the list, 1.3e-16 / 9.7e-16 host path against device path.  No bar was missed."""
import math

import numpy as np
import pytest

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import projection_yardstick as PY
from . import xcorr_yardstick as XY
from .common import Case, relerr
from .model_matrix import ModelCase
from .test_gpu_objective import BATCH, FAST, FOCUS_KW, PATHS, SPI, TS, Ensemble, _spin_damping, _with_env
from .test_gpu_signal_misfit import ALL, DESIGN, MODEL_NAMES, host, make_terms, member_leaves

pytestmark = pytest.mark.gpu

TOL_RHO, TOL_VALUE, TOL_DELTA, TOL_GRAD = 1e-12, 1e-12, 1e-12, 1e-11
GRIDS = {"5 outputs": (TS, SPI), "70 outputs": (np.linspace(0.0, 4e-4, 70), 1)}
NS = 4
PAIRS = [(0, 1), (1, -1), (0, -2), (2, 2)]        # signal-signal, two template pairs sharing signal 0, signal 2 with itself
SOURCES = (1, 0)                                  # template column j: the member's signal SOURCES[j], shifted
SEED, BETA, W_PEAK = 40, 4.0, -1.3
D_ALL = {"5 outputs": 3, "70 outputs": 69}        # every lag the grid has
D_SOFT = {"5 outputs": 3, "70 outputs": 8}        # the lags of the softmax cases (module docstring)


def solve(e, grid):
    ts, spi = GRIDS[grid] if isinstance(grid, str) else grid
    return e.c.solver(np.zeros((2, e.nb, 3)), ts, e.cps, keep_trajectory=True, steps_per_interval=spi)


def graphs_of(e, fields):
    return [PY.MemberGraph(fields[m], e.leaves[m], e.c.bonds, e.terms, NS) for m in range(BATCH)]


def templates_of(graphs, seed=SEED):
    rng = np.random.default_rng(seed)
    return np.stack([XY.make_templates(g.signal_values(), rng, SOURCES) for g in graphs])


def spec_of(terms, ns, pairs, D, templates, norm, reduce, lag=None, w_delay=0.0, target=0.0):
    return O.CorrelationSpec(O.SignalSpec(terms, ns), pairs, D, templates, norm, reduce, lag, BETA if reduce == "softmax" else None, W_PEAK,
                             w_delay, target)


def with_delay_term(graphs, spec):
    """the same spec with w_delay = 1 / (beta D) and delta_target 1.5 outputs above the largest delta of the members (yardstick)"""
    deltas = [XY.evaluate(g, spec, spec.templates[m], False).delta for m, g in enumerate(graphs)]
    return O.CorrelationSpec(spec.signal_spec, spec.pairs, spec.max_lag, spec.templates, spec.normalisation, "softmax", None, BETA, W_PEAK,
                             1.0 / (BETA * max(spec.max_lag, 1)), max(deltas) + 1.5)


def cases_of(e, grid, graphs):
    """tag -> spec: "at", "max", "softmax" without and with the delay term, and D = 0"""
    tp, Da, Ds = e.templates[grid], D_ALL[grid], D_SOFT[grid]
    out = {"at none": spec_of(e.terms, NS, PAIRS, Da, tp, "none", "at", 2),
           "max reference": spec_of(e.terms, NS, PAIRS, Da, tp, "reference", "max"),
           "softmax coefficient": spec_of(e.terms, NS, PAIRS, Ds, tp, "coefficient", "softmax"),
           "D=0 at coefficient": spec_of(e.terms, NS, PAIRS, 0, tp, "coefficient", "at", 0)}
    out["softmax+delay reference"] = with_delay_term(graphs, spec_of(e.terms, NS, PAIRS, Ds, tp, "reference", "softmax"))
    return out


def templates_m(spec, m):
    return None if spec.templates is None else spec.templates[m] if spec.templates.ndim == 3 else spec.templates


def check_inputs(tag, graphs, spec, members=None):
    """the conditions on the inputs, on the yardstick's numbers; returns the yardstick's Results (with gradients)"""
    res, worst = {}, {}
    for m, g in enumerate(graphs):
        if members is not None and m not in members:
            continue
        res[m] = XY.evaluate(g, spec, templates_m(spec, m))
        c = XY.conditions(res[m], spec)
        for k, v in c.items():
            worst[k] = min(worst.get(k, v), v) if k == "gap" else max(worst.get(k, v), v)
        assert XY.conditions_hold(c), (tag, m, c)
        if spec.w_delay:
            assert abs(res[m].delta - spec.delay_target) >= 1.0, (tag, m, res[m].delta, spec.delay_target)
    print(f"[signal xcorr] {tag}: conditions of the inputs " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return res


def reference(eng, graphs, res, which):
    """raw reference gradients: dfx_adjoint on the autograd cotangent + the autograd explicit terms; members without a Result get zeros"""
    fb = np.stack([res[m].fb if m in res else np.zeros_like(g.fields) for m, g in enumerate(graphs)])
    ref, _ = eng.adjoint(fb, which=which)
    ref = {k: np.array(v) for k, v in ref.items()}
    for m, r in res.items():
        g = r.explicit
        ref["centroid_node_vectors"][m] += g["cnv"]
        if "void_angle0" in ref and "phi0" in g:
            ref["void_angle0"][m] += g["phi0"]
        if "reference_vector" in ref:
            ref["reference_vector"][m] += g["refv"]
        if "k_bond" in ref:
            ref["k_bond"][m] += np.stack([g["ks"], g["ksh"], g["kr"]], 1)
        if "contact" in ref and "am" in g:
            ref["contact"][m] += np.array([g["am"], g["ac"], g["kc"]])
    return ref


def call(eng, spec, which=ALL, device=False):
    kw = dict(templates=spec.templates, normalisation=spec.normalisation, reduce=spec.reduce, lag=spec.lag, beta=spec.beta, w_peak=spec.w_peak,
              w_delay=spec.w_delay, delay_target=spec.delay_target)
    J, M, d, out, st = eng.signal_xcorr_value_and_grad(spec.signal_spec.terms, spec.signal_spec.n_signals, spec.pairs, spec.max_lag, which=which,
                                                       device=device, **kw)
    return J.copy(), M.copy(), d.copy(), ({k: x.to_host() for k, x in out.items()} if device else host(out)), st


def value_only(eng, spec):
    return eng.signal_xcorr_value(spec.signal_spec.terms, spec.signal_spec.n_signals, spec.pairs, spec.max_lag, templates=spec.templates,
                                  normalisation=spec.normalisation, reduce=spec.reduce, lag=spec.lag, beta=spec.beta, w_peak=spec.w_peak,
                                  w_delay=spec.w_delay, delay_target=spec.delay_target)


def compare(tag, spec, got, res, ref, members=None):
    J, M, d, out = got[:4]
    ms = sorted(res)
    worst = {"J": max(abs(J[m] - res[m].J) / abs(res[m].J) for m in ms), "M": max(abs(M[m] - res[m].M) / abs(res[m].M) for m in ms),
             "delta": max(abs(d[m] - res[m].delta) for m in ms) / max(spec.max_lag, 1)}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[signal xcorr] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bars = {"J": TOL_VALUE, "M": TOL_VALUE, "delta": TOL_DELTA}
    bad = {k: v for k, v in worst.items() if not v <= bars.get(k, TOL_GRAD)}
    assert not bad, (tag, bad)
    return worst


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    """The ensemble of test_gpu_objective.py with the terms of the signal-misfit test; per grid the per-member templates are built from the
    yardstick's signals of a first solve (fixed inputs from then on)."""
    e = Ensemble(request.param)
    e.lattice = request.param
    e.terms, e.force_blocks, e.listed = make_terms(e.c)
    e.leaves = [member_leaves(e.c, e.cps, m) for m in range(BATCH)]
    e.templates = {}
    for grid in GRIDS:
        fields = np.array(_with_env({}, lambda: solve(e, grid)))
        e.templates[grid] = templates_of(graphs_of(e, fields))
    return e


def test_the_inputs_are_the_ones_the_kernels_can_go_wrong_on(ens):
    assert len(GRIDS["5 outputs"][0]) < 64 < len(GRIDS["70 outputs"][0]) and len(GRIDS["70 outputs"][0]) % 64 == 6
    assert D_ALL["5 outputs"] == 3 and 2 * D_ALL["70 outputs"] + 3 == 141 and 141 % 4 != 0 and D_ALL["70 outputs"] == len(GRIDS["70 outputs"][0]) - 1
    a, b = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    assert any(x == y for x, y in PAIRS) and a.count(0) == 2 and sum(y < 0 for y in b) == 2 and any(y >= 0 and x != y for x, y in PAIRS)
    for grid in GRIDS:
        tp = ens.templates[grid]
        assert tp.shape == (BATCH, len(GRIDS[grid][0]), 2) and len(set(np.round(tp[:, -1, 0] / np.abs(tp[:, -1, 0]).max(), 9))) == BATCH


# ---- 1. rho ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_rho_for_the_three_normalisations(ens, grid):
    c = ens.c
    specs = {(norm, D): spec_of(ens.terms, NS, PAIRS, D, ens.templates[grid], norm, "at", 0) for norm in O.NORMALISATIONS for D in (0, D_ALL[grid])}

    def run():
        fields = np.array(solve(ens, grid))
        return fields, {k: c.solver.signal_xcorr(s) for k, s in specs.items()}
    fields, out = _with_env({}, run)
    graphs = graphs_of(ens, fields)
    for (norm, D), rho in out.items():
        res = [XY.evaluate(g, specs[norm, D], ens.templates[grid][m], False) for m, g in enumerate(graphs)]
        err = max(float(np.abs(rho[m] - r.rho).max() / XY.rho_scale(r)) for m, r in enumerate(res))
        print(f"[signal xcorr] {ens.lattice} {grid} {norm} D={D}: rho against the yardstick {err:.2e} of max sum |A B| / N")
        assert rho.shape == (BATCH, 2 * D + 1) and all(np.abs(r.rho).max() > 0 for r in res)
        assert err <= TOL_RHO
        # the narrower window is the middle of the wider one: the same sums, the same bits
        assert np.array_equal(out[norm, 0][:, 0], out[norm, D_ALL[grid]][:, D_ALL[grid]])


# ---- 2. value and raw gradients: both grids, every reduction ---------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_value_and_gradients_for_every_reduction(ens, grid):
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(solve(ens, grid))
        graphs = graphs_of(ens, fields)
        out = {}
        for tag, spec in cases_of(ens, grid, graphs).items():
            res = check_inputs(f"{ens.lattice} {grid} {tag}", graphs, spec)
            out[tag] = (spec, res, reference(eng, graphs, res, ALL), call(eng, spec), call(eng, spec, DESIGN), value_only(eng, spec))
        return out
    for tag, (spec, res, ref, got, got_d, only) in _with_env({}, run).items():
        name = f"{ens.lattice} {grid} {tag}"
        assert all(np.array_equal(a, b) for a, b in zip(only, got[:3])) and all(np.array_equal(a, b) for a, b in zip(got_d[:3], got[:3]))
        assert set(got[3]) == set(ALL) and set(got_d[3]) == set(DESIGN), (name, sorted(got[3]))
        engaged = c.geo.n_npb == 4
        assert all(np.abs(ref[k]).max() > 0 for k in ALL if engaged or k not in ("void_angle0", "contact")), name
        if spec.reduce == "max":
            assert all(r.delta == 2.0 for r in res.values()), name                     # the off-centre peak of the shifted templates
        compare(name, spec, got, res, ref)
        compare(name + " (design leaves)", spec, got_d, res, {k: ref[k] for k in DESIGN})


# ---- 3. every form of the sweep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(solve(ens, (TS, spi)))
        st_f = dict(c.solver.stats)
        graphs = graphs_of(ens, fields)
        spec = with_delay_term(graphs, spec_of(ens.terms, NS, PAIRS, 3, ens.templates["5 outputs"], "coefficient", "softmax"))
        res = check_inputs(f"{ens.lattice} {path}", graphs, spec)
        return st_f, spec, res, reference(eng, graphs, res, ALL), call(eng, spec), call(eng, spec, DESIGN)
    st_f, spec, res, ref, got, got_d = _with_env(env, run)
    st = got_d[4]
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
    assert all(np.array_equal(a, b) for a, b in zip(got_d[:3], got[:3])) and set(got[3]) == set(ALL) and set(got_d[3]) == set(DESIGN)
    compare(f"{ens.lattice} {path}", spec, got, res, ref)
    compare(f"{ens.lattice} {path} (design leaves)", spec, got_d, res, {k: ref[k] for k in DESIGN})


@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_every_bond_model_with_and_without_the_angle_contact(hip_lib, model, contact):
    """Quads 4x4, one member, per-ligament stiffnesses, 3 signals, softmax with the delay term over 7 lags: every leaf against the
    yardstick written with that model's energy."""
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    nbd, p = len(mc.bonds), mc.members[0]
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
    nb = mc.geo.n_blocks
    driven, corner = int(mc.con[0, 0]), nb - 1
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7), (1, 0, 7, -1.3), (1, corner, 8, 0.9), (1, 5, 8, 0.5), (1, 5, 6, -0.2), (2, 6, 1, 2.0), (2, 6, 3, 1e-4)]
    eng = mc.solver.engine

    def run():
        fields = np.array(mc.solver(np.zeros((2, nb, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
        graphs = [PY.MemberGraph(fields, lv, mc.bonds, terms, 3, MODEL_NAMES[model])]
        tp = templates_of(graphs)
        spec = with_delay_term(graphs, spec_of(terms, 3, PAIRS, 3, tp, "coefficient", "softmax"))
        res = check_inputs(f"quads 4x4 {model} contact={contact}", graphs, spec)
        return spec, res, reference(eng, graphs, res, ALL), call(eng, spec), mc.solver.signal_xcorr(spec)
    spec, res, ref, got, rho = _with_env({}, run)
    tag = f"quads 4x4 {model} contact={contact}"
    e_r = float(np.abs(rho[0] - res[0].rho).max() / XY.rho_scale(res[0]))
    print(f"[signal xcorr] {tag}: rho {e_r:.2e}")
    assert rho.shape == (1, 7) and e_r <= TOL_RHO
    assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
    if contact:
        assert np.abs(ref["contact"]).max() > 0 and np.abs(ref["void_angle0"]).max() > 0
    compare(tag, spec, got, res, ref)


# ---- 4. repeatability, device views, the projection with one template row ---------------------------------------------------------------
def test_two_calls_return_the_same_bits_device_views_and_the_one_row_projection(ens):
    eng, c = ens.c.solver.engine, ens.c
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    grid = "70 outputs"
    tp = ens.templates[grid]
    a = spec_of(ens.terms, NS, PAIRS, D_SOFT[grid], tp, "coefficient", "softmax")
    b = spec_of(ens.terms, NS, PAIRS, D_ALL[grid], tp, "reference", "max")
    row = np.ascontiguousarray(tp[0, :, :1])                                         # one shared template column
    one = spec_of(ens.terms, NS, [(1, -1)], 0, row, "none", "at", 0)

    def run():
        fields = np.array(solve(ens, grid))
        fb = np.random.default_rng(2).normal(size=fields.shape)
        r1, other, r2, r3 = call(eng, a, which), call(eng, b, which), call(eng, a, which), call(eng, a, which, device=True)
        shared, per_member = call(eng, one, which), call(eng, one.with_templates(np.broadcast_to(row, (BATCH,) + row.shape).copy()), which)
        rho1, rho2 = c.solver.signal_xcorr(one), c.solver.signal_xcorr(one)
        proj = eng.signal_projections(ens.terms, NS, np.ascontiguousarray(row.T))
        S = eng.signal_values(ens.terms, NS)
        after = host(c.solver.vjp_raw(fb, which=which))
        fresh = np.array(solve(ens, grid))
        before = host(c.solver.vjp_raw(fb, which=which))
        return fields, fresh, r1, r2, r3, other, shared, per_member, rho1, rho2, proj, S, after, before
    fields, fresh, r1, r2, r3, other, shared, per_member, rho1, rho2, proj, S, after, before = _with_env({}, run)
    same = lambda x, y: all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and set(x[3]) == set(y[3]) and all(np.array_equal(x[3][k], y[3][k]) for k in x[3])     # noqa: E731
    assert np.abs(r1[0]).min() > 0 and all(np.abs(r1[3][k]).max() > 0 for k in which if k != "void_angle0" or c.geo.n_npb == 4)
    assert same(r1, r2) and same(r1, r3), "two identical calls, device views"
    assert not same(r1, other) and np.array_equal(rho1, rho2)
    assert same(shared, per_member), "a shared template against the same template per member"
    # "none", D = 0, one template pair: rho[0] is the projection of signal 1 on that template as the one basis row
    scale = float(np.einsum("k,mk->m", np.abs(row[:, 0]), np.abs(S[:, :, 1])).max())
    err = float(np.abs(rho1[:, 0] - proj[:, 1, 0]).max() / scale)
    print(f"[signal xcorr] {ens.lattice}: rho[0] of one template pair against dfx_signal_projections {err:.2e} of sum |B S| = {scale:.3e}")
    assert rho1.shape == (BATCH, 1) and err <= 1e-14 and np.array_equal(shared[1], rho1[:, 0])
    # a vjp after the calls serves the same kept solve as one on a fresh solve of the same problem
    assert np.array_equal(fields, fresh) and all(np.array_equal(after[k], before[k]) for k in which)


# ---- 5. a member whose normalisation is zero ----------------------------------------------------------------------------------------------
def test_zero_normalisation_gives_nan_and_exactly_zero_gradients(ens):
    eng = ens.c.solver.engine
    grid = "5 outputs"
    terms5 = list(ens.terms) + [(4, 0, 1, 1.0)]                                      # signal 4: the y displacement of the clamped block 0
    clamped = O.CorrelationSpec(O.SignalSpec(terms5, 5), [(4, 0)], 3, None, "reference", "max", None, None, W_PEAK)
    tp = ens.templates[grid].copy()
    tp[1] = 0.0                                                                      # member 1: EB = 0 under "coefficient"
    dead = spec_of(ens.terms, NS, [(1, -1), (0, -2)], 3, tp, "coefficient", "max")

    def run():
        fields = np.array(solve(ens, grid))
        graphs = graphs_of(ens, fields)
        res = check_inputs(f"{ens.lattice} member 1 without a template", graphs, dead, members=(0, 2))
        return fields, res, reference(eng, graphs, res, ALL), call(eng, clamped), call(eng, dead), value_only(eng, dead), ens.c.solver.signal_xcorr(dead)
    fields, res, ref, got_c, got_d, only, rho = _with_env({}, run)
    assert not fields[:, :, 0, 0, 1].any()                                           # the DOF is clamped in every member
    assert all(np.isnan(x).all() for x in got_c[:3]) and all(not a.any() for a in got_c[3].values()) and set(got_c[3]) == set(ALL)
    for x, y in zip(got_d[:3], only):
        assert np.isnan(x[1]) and np.isfinite(x[[0, 2]]).all() and np.array_equal(x, y, equal_nan=True)
    assert np.isnan(rho[1]).all() and np.isfinite(rho[[0, 2]]).all()
    assert all(not np.asarray(a)[1].any() for a in got_d[3].values()) and all(np.asarray(a)[[0, 2]].any() for k, a in got_d[3].items() if np.abs(ref[k]).max() > 0)
    compare(f"{ens.lattice} member 1 without a template (members 0 and 2)", dead, got_d, res, ref)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_the_next_adjoint_is_unaffected(ens):
    eng, c = ens.c.solver.engine, ens.c
    T, nb = len(TS), c.geo.n_blocks
    one, two = [(0, 1, 6, 1.0)], [(0, 1, 6, 1.0), (1, 2, 0, 1.0)]
    tp1 = np.ones((T, 1))
    fresh = Case("quads", 4, True, False, seed=3)
    feng = fresh.solver.engine
    with pytest.raises(RuntimeError, match="run forward first"):
        feng.signal_xcorr(one, 1, [(0, 0)], 0)
    with pytest.raises(RuntimeError, match="run forward first"):
        feng.signal_xcorr_value(one, 1, [(0, 0)], 0)
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        feng.signal_xcorr_value_and_grad(one, 1, [(0, 0)], 0)
    _with_env({}, lambda: fresh.solver(np.zeros((2, 16, 3)), TS, fresh.cp._replace(constraint_params=dict(FAST)), steps_per_interval=SPI))
    J, M, d = feng.signal_xcorr_value([(0, int(fresh.con[0, 0]), 6, 1.0)], 1, [(0, 0)], 2)
    assert J[0] == M[0] == 1.0 and d[0] == 0.0                                        # any forward pass serves the value: an auto-correlation ...
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):          # ... the gradient needs the kept trajectory
        feng.signal_xcorr_value_and_grad(one, 1, [(0, 0)], 0)
    fields = np.array(_with_env({}, lambda: solve(ens, "5 outputs")))
    fb = np.random.default_rng(6).normal(size=fields.shape)
    which = ("centroid_node_vectors", "inertia", "fn_params")
    before = host(eng.adjoint(fb, which=which)[0])
    good_spec = spec_of(ens.terms, NS, PAIRS, 3, ens.templates["5 outputs"], "coefficient", "softmax")
    good = value_only(eng, good_spec)
    calls = (lambda t, n, p, D, **kw: eng.signal_xcorr_value_and_grad(t, n, p, D, **kw), lambda t, n, p, D, **kw: eng.signal_xcorr_value(t, n, p, D, **kw),
             lambda t, n, p, D, **kw: eng.signal_xcorr(t, n, p, D, **{k: v for k, v in kw.items() if k in ("templates", "normalisation")}))
    for k, f in enumerate(calls):
        with pytest.raises(RuntimeError, match="n_pairs must be at least 1"):
            f(one, 1, np.zeros((0, 2)), 0)
        with pytest.raises(RuntimeError, match="pair 0 names signal 1 out of range"):
            f(one, 1, [(1, 0)], 0)
        with pytest.raises(RuntimeError, match="pair 1 names signal 2 out of range"):
            f(two, 2, [(0, 1), (1, 2)], 0)
        with pytest.raises(RuntimeError, match="pair 0 names signal -1 out of range"):
            f(one, 1, [(-1, 0)], 0)
        with pytest.raises(RuntimeError, match="names template column 0 but templates is NULL"):
            f(one, 1, [(0, -1)], 0)
        with pytest.raises(RuntimeError, match="names template column 1 out of range"):
            f(one, 1, [(0, -2)], 0, templates=tp1)
        with pytest.raises(RuntimeError, match=r"max_lag 5 outside \[0, T - 1\]"):
            f(one, 1, [(0, 0)], T)
        with pytest.raises(RuntimeError, match=r"max_lag -1 outside \[0, T - 1\]"):
            f(one, 1, [(0, 0)], -1)
        with pytest.raises(RuntimeError, match="unknown normalisation 3"):
            f(one, 1, [(0, 0)], 0, normalisation=3)
        with pytest.raises(RuntimeError, match="non-finite template"):
            f(one, 1, [(0, -1)], 0, templates=np.where(np.arange(T)[:, None] == T - 1, np.nan, tp1))
        with pytest.raises(RuntimeError, match="non-finite template"):
            f(one, 1, [(0, -1)], 0, templates=np.where(np.arange(BATCH)[:, None, None] == BATCH - 1, np.inf, np.ones((BATCH, T, 1))))
        if k < 2:
            with pytest.raises(RuntimeError, match="unknown reduction 3"):
                f(one, 1, [(0, 0)], 0, reduce=3)
            with pytest.raises(RuntimeError, match=r"lag0 3 outside \[-max_lag, max_lag\]"):
                f(one, 1, [(0, 0)], 2, reduce="at", lag=3)
            with pytest.raises(RuntimeError, match=r"lag0 -3 outside \[-max_lag, max_lag\]"):
                f(one, 1, [(0, 0)], 2, reduce="at", lag=-3)
            for beta in (0.0, -1.0, np.nan, np.inf):
                with pytest.raises(RuntimeError, match="beta must be positive and finite"):
                    f(one, 1, [(0, 0)], 2, reduce="softmax", beta=beta)
            for red in ("at", "max"):
                with pytest.raises(RuntimeError, match="w_delay != 0 needs the softmax reduction"):
                    f(one, 1, [(0, 0)], 2, reduce=red, w_delay=0.5)
            with pytest.raises(RuntimeError, match="non-finite weight"):
                f(one, 1, [(0, 0)], 2, w_peak=np.nan)
            with pytest.raises(RuntimeError, match="non-finite weight"):
                f(one, 1, [(0, 0)], 2, reduce="softmax", beta=1.0, w_delay=np.inf)
            with pytest.raises(RuntimeError, match="non-finite delay_target"):
                f(one, 1, [(0, 0)], 2, reduce="softmax", beta=1.0, w_delay=1.0, delay_target=np.nan)
        # everything the signal entries refuse
        with pytest.raises(RuntimeError, match=f"names block {nb} out of range"):
            f([(0, nb, 6, 1.0)], 1, [(0, 0)], 0)
        with pytest.raises(RuntimeError, match="names component 9 out of range"):
            f([(0, 1, 9, 1.0)], 1, [(0, 0)], 0)
        with pytest.raises(RuntimeError, match="signal 1 is empty"):
            f([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 3, [(0, 0)], 0)
    # NULL arrays: through the C entries themselves (the binding converts its arrays before it calls)
    args, keep = eng._signal_terms(one, 1)
    from difflexmm_amd._binding import _ptr
    out = np.zeros(BATCH)
    rc = eng.lib.dfx_signal_xcorr_value(eng._h, *args, 1, None, None, None, 0, 0, 0, 0, 1, 0, 1.0, 1.0, 0.0, 0.0, _ptr(out), None, None)
    assert rc == 1 and "pair_a or pair_b is NULL" in eng.lib.dfx_last_error(eng._h).decode()
    pa = np.zeros(1, dtype=np.int32)
    ip = pa.ctypes.data_as(args[1].__class__)
    rc = eng.lib.dfx_signal_xcorr(eng._h, *args, 1, ip, ip, None, 0, 0, 0, 0, None)
    assert rc == 1 and "values is NULL" in eng.lib.dfx_last_error(eng._h).decode()
    rc = eng.lib.dfx_signal_xcorr_value(eng._h, *args, 1, ip, ip, None, 0, 0, 0, 0, 1, 0, 1.0, 1.0, 0.0, 0.0, None, None, None)
    assert rc == 1 and "objective is NULL" in eng.lib.dfx_last_error(eng._h).decode()
    # shapes the binding can check itself
    with pytest.raises(ValueError):
        eng.signal_xcorr_value(one, 1, [(0, -1)], 0, templates=np.ones((T + 1, 1)))
    with pytest.raises(ValueError):
        eng.signal_xcorr_value(one, 1, [(0, -1)], 0, templates=np.ones((BATCH + 1, T, 1)))
    # after the refusals the next dfx_adjoint on the handle is unaffected, and the handle still answers and solves
    after = host(eng.adjoint(fb, which=which)[0])
    assert all(np.array_equal(after[k], before[k]) and np.abs(before[k]).max() > 0 for k in which)
    assert all(np.array_equal(a, b) for a, b in zip(value_only(eng, good_spec), good))
    got = call(eng, good_spec, ("inertia",))
    assert np.array_equal(got[0], good[0]) and np.abs(got[3]["inertia"]).max() > 0
    assert np.array_equal(np.array(_with_env({}, lambda: solve(ens, "5 outputs"))), fields)
    # force components with the distance-based contact are refused, field components are served there
    mc = ModelCase("quads", "nonlinear", "distance", 4, "uniform", batch=1)
    _with_env({}, lambda: mc.solver(np.zeros((2, 16, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
    for f in (lambda: mc.solver.engine.signal_xcorr_value_and_grad(one, 1, [(0, 0)], 0), lambda: mc.solver.engine.signal_xcorr(one, 1, [(0, 0)], 0)):
        with pytest.raises(RuntimeError, match="distance-based contact energy is not part of the signal channels"):
            f()
    J, M, d, g, _ = mc.solver.engine.signal_xcorr_value_and_grad([(0, 5, 0, 1.0), (1, 6, 4, 1e-4)], 2, [(0, 1)], 2, normalisation="coefficient",
                                                                 which=("centroid_node_vectors", "block_centroids"))
    assert np.isfinite(J[0]) and np.abs(g["centroid_node_vectors"]).max() > 0


# ---- 7. the problem classes ------------------------------------------------------------------------------------------------------------------
def _forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **{**FOCUS_KW, "n_timepoints": 7})
    fw.setup()
    return fw


def test_target_cross_correlation_directional_derivatives(hip_lib):
    """TargetCrossCorrelation on quads 6x6 (7 outputs): velocities of three block DOFs, two signal pairs and a template pair with
    per-member templates, the softmax peak of the correlation coefficient over 7 lags with a delay term, for a list of 3 designs as one
    ensemble: directional derivatives along random design directions against central differences of ``value`` with the relative step
    1e-6 and the 1e-6 bar of TargetSignalMisfit's case in test_gpu_signal_misfit.py; a one-design call with on_device=True equals member 0
    of the list call to 1e-13; the host path equals the device path to 1e-12."""
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(19)
    base = fw1.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    sig = O.SignalSpec.fields_of([(16, 0), (21, 2), (20, 1)], "velocity")
    k = np.arange(7)
    tp = np.stack([np.exp(-0.5 * ((k - 3.0 - 0.5 * m) / 1.5) ** 2)[:, None] * (1.0 + 0.3 * m) for m in range(3)])
    spec = O.CorrelationSpec(sig, [(0, 1), (1, 2), (0, -1)], 3, tp, "coefficient", "softmax", None, 4.0, -1.0, 0.05, 1.0)
    many = P.TargetCrossCorrelation(fw3, spec)
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and np.isfinite(v).all() and (v != 0).all()
    assert many.last_peak.shape == many.last_delay.shape == (3,) and (np.abs(many.last_delay) < 3).all()
    assert np.allclose(many.value(designs), v, rtol=1e-13, atol=0.0)
    scale = max(np.abs(a).max() for a in base)
    for trial in range(3):
        dirs = [tuple(rng.normal(size=a.shape) for a in base) for _ in range(3)]
        dirs = [tuple(a / max(np.abs(x).max() for x in d) for a in d) for d in dirs]
        h = 1e-6 * scale
        vp = many.value([tuple(a + h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        vm = many.value([tuple(a - h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        fd = (vp - vm) / (2 * h)
        mine = np.array([sum(float(np.sum(a * e)) for a, e in zip(gm, dd)) for gm, dd in zip(g, dirs)])
        err = np.abs(mine - fd) / np.abs(fd)
        print(f"[signal xcorr] TargetCrossCorrelation, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.TargetCrossCorrelation(fw1, spec.with_templates(tp[0]))
    v1, g1 = single.value_and_grad(designs[0], on_device=True)
    e_v = abs(v1 - v[0]) / abs(v[0])
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[signal xcorr] TargetCrossCorrelation, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13
    peak_d, delay_d = single.last_peak, single.last_delay
    vh, gh = single.value_and_grad(designs[0])
    e_v = abs(vh - v1) / abs(v1)
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(gh, g1))
    print(f"[signal xcorr] TargetCrossCorrelation, host path against device path: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert e_v <= 1e-12 and e_g <= 1e-12 and abs(single.last_peak - peak_d) <= 1e-12 * abs(peak_d) and abs(single.last_delay - delay_d) <= 3e-12
    # a longer list runs in chunks of the ensemble width; per-member templates are cut alike
    tp6 = np.concatenate([tp, tp[::-1] * 1.1])
    v6 = P.TargetCrossCorrelation(fw3, spec.with_templates(tp6)).value(designs + designs[::-1])
    halves = [P.TargetCrossCorrelation(fw3, spec.with_templates(tp6[i:i + 3])).value(d) for i, d in ((0, designs), (3, designs[::-1]))]
    assert v6.shape == (6,) and np.array_equal(v6, np.concatenate(halves))
    with pytest.raises(ValueError, match="force components are evaluated on the device only"):
        P.TargetCrossCorrelation(fw1, O.CorrelationSpec(O.SignalSpec([(0, 14, 6, 1.0)], 1), [(0, 0)], 2)).value_and_grad(designs[0])
    # TargetWaveDelay: source i against target i, seconds into outputs; output times that are not uniform are refused
    wd = P.TargetWaveDelay(fw3, [(16, 0), (16, 1)], [(20, 0), (20, 1)], "velocity", 3, 4.0, delay_target_seconds=1.5e-4, w_delay=0.1)
    dt = float(np.diff(fw3.timepoints).mean())
    assert isinstance(wd, P.TargetCrossCorrelation) and wd.spec.pairs == [(0, 2), (1, 3)] and wd.spec.reduce == "softmax"
    assert wd.spec.normalisation == "coefficient" and wd.spec.w_peak == -1.0 and abs(wd.spec.delay_target - 1.5e-4 / dt) <= 1e-12
    assert np.isfinite(wd.value(designs)).all()
    fw_bad = _forward(1)
    fw_bad.timepoints = np.array(fw_bad.timepoints) * (1.0 + 1e-6 * np.arange(7))
    with pytest.raises(ValueError, match="not uniformly spaced"):
        P.TargetWaveDelay(fw_bad, [(16, 0)], [(20, 0)], "velocity", 3, 4.0)
    fw_bad.timepoints = np.stack([fw1.timepoints] * 2)
    with pytest.raises(ValueError, match="per-member timepoints"):
        P.TargetWaveDelay(fw_bad, [(16, 0)], [(20, 0)], "velocity", 3, 4.0)
