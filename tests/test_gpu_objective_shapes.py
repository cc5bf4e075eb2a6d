"""-m gpu: the three device objectives (weighted kinetic energy / angular momentum, ligament strain energy, signal misfit; kernels in
difflexmm_amd/csrc/dfx_objective.h, launches in engine_objective.hip) at shapes where a launch spans MANY workgroups.  The sibling files
(test_gpu_objective.py, test_gpu_strain_objective.py, test_gpu_signal_misfit.py) are careful about physics, sweep forms, bond models and
refusals on launches of 30 items; here the cases of tests/objective_shapes.py put 66 049 and more items into every kernel: 259 workgroups
of k_objective and k_signal_residual (more than 256 partials: the loop of k_objective_finish makes a second trip), 1 033 to 1 161 workgroups
of the 64-item kernels, 5 to 19 of the explicit kernels, k = item / n_act crossing every workgroup boundary inside an output time, a
compaction list that is no arange, and zero weights inside a full launch.  The premises of the cases (finite solves in regime, few
negligible items, the counts) are checked without a GPU in tests/test_objective_shapes_host.py.

References and bars.  Gradients: the yardsticks of the sibling files, imported -- the host cotangent (NumPy for the weighted kinds, autograd
through tests/strain_yardstick.py and tests/signal_yardstick.py for the others) pushed through the SAME reverse sweep (dfx_adjoint) plus the
explicit terms -- at the siblings' own bars: 1e-12 of the largest entry of a leaf for the weighted kinds, 1e-11 for strain and signal.
Should a leaf exceed its bar the test measures the floor of that reference before it fails: the host cotangent through dfx_adjoint as it is
and with every entry multiplied by 1 + 1e-16 N(0, 1); both figures are printed.  Values: math.fsum of the host's per-item terms, the error
measured against the sum of the ABSOLUTE terms (with weights of both signs the value is 2e-3 to 0.14 of it; a bar on the value would be a
bar on summation order): 1e-13 of it.  A term carries a handful of roundings and a summation tree over 66 049 terms adds at most 17 u, so
honest arithmetic stays below 1e-14; one lost item of median size is 1e-5.  Signal values: 1e-12 of the largest signal, as the sibling.
Sweep forms: the fixed grid at the records level with the default environment, and the adaptive kept steps, on both lattices (none dropped).
The one-hot checks (tau = e_k, k in {0, 1, 128, 255, 256}: item ranges that straddle workgroups 0/1/2, 128/129 and 257/258) go through
the value-only entries on the quads and compare with the host's sum over that output alone; output 0 with the initial state's own terms.
The exact-boundary cases run on the ensemble of test_gpu_objective.py with T x n_act = 256 (one full workgroup of k_objective, four of the
64-item kernels, no padded lane anywhere), 64 and 65, with the comparisons of the siblings' case 1 on stage launches at the records level.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X: profiles/r19_objective_shapes.txt."""
import math

import numpy as np
import pytest

from difflexmm_amd import objective as O

from . import objective_shapes as OS
from . import test_gpu_objective as TO
from . import test_gpu_signal_misfit as TG
from . import test_gpu_strain_objective as TS_
from .common import relerr
from .signal_yardstick import signal_misfit
from .test_gpu_objective import PATHS, _with_env

pytestmark = pytest.mark.gpu

FORMS = {"fixed-records": (dict(DFX_CHECKPOINT="records"), OS.SPI), "adaptive-kept-steps": PATHS["adaptive-kept-steps"]}
TOL_WEIGHTED = TO.TOL                                     # 1e-12
TOL_GRAD = TS_.TOL_GRAD                                   # 1e-11, strain and signal
TOL_SIGNAL = TG.TOL_SIGNAL                                # 1e-12 of the largest signal
TOL_VALUE = 1e-13                                         # of the sum of the absolute terms


def host(out):
    return {k: np.array(v) for k, v in out.items()}


def value_error(obj, units, tau):
    """worst over the members of |device value - fsum(items)| / fsum(|items|), and the smallest |value| / sum |term|"""
    worst, ratio = 0.0, np.inf
    for m, unit in enumerate(units):
        value, total = OS.fsum_value(unit, tau)
        assert total > 0
        worst, ratio = max(worst, abs(float(obj[m]) - value) / total), min(ratio, abs(value) / total)
    return worst, ratio


def sweep_floor(eng, fb, which):
    """the reference's own floor: the host cotangent through the sweep as it is, and with every entry multiplied by 1 + 1e-16 N(0, 1)"""
    a, _ = eng.adjoint(fb, which=which)
    a = host(a)
    b, _ = eng.adjoint(fb * (1.0 + 1e-16 * np.random.default_rng(1).normal(size=fb.shape)), which=which)
    b = host(b)
    return {k: relerr(b[k], a[k]) for k in a if np.abs(a[k]).max() > 0}


def check(tag, obj, out, ref, units, tau, tol, floor=None):
    """value against fsum of the items, every leaf against the reference; prints before it asserts"""
    e_v, ratio = value_error(obj, units, tau)
    worst = {}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    top = max(worst, key=worst.get)
    print(f"[objective shapes] {tag}: value {e_v:.2e} of sum |term| (|value| {ratio:.1e} of it); worst leaf {top} {worst[top]:.2e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= tol}
    if bad and floor is not None:
        fl = floor()
        print(f"[objective shapes] {tag}: over the bar {tol:.0e}: {bad}; floor of the reference (perturbed cotangent through the same sweep): "
              + ", ".join(f"{k} {fl.get(k, 0.0):.2e}" for k in bad))
    assert e_v <= TOL_VALUE, (tag, e_v)
    assert not bad, (tag, bad)


@pytest.fixture(scope="module", params=["quads", "kagome"])
def big(request, hip_lib):
    L = OS.LargeCase(request.param)
    cnt, wg, sig = L.counts()
    # the case spans what this file is there for (the exact numbers are pinned in tests/test_objective_shapes_host.py)
    assert cnt == OS.COUNTS[L.lattice] and wg == OS.WORKGROUPS[L.lattice]
    OS.check_spans_many_workgroups(OS.N_OUT, cnt, wg)
    assert sig["longest_uc"] == 2 and sig["n_distinct"] < sig["n_terms"]
    return L


def solve(L, form):
    fields = L.solve(FORMS[form][1])
    st = dict(L.c.solver.stats)
    if form == "adaptive-kept-steps":
        assert st["step_control"] == "adaptive-records", st
    assert fields.shape == (OS.BATCH, OS.N_OUT, 2, L.nb, 3) and np.isfinite(fields).all()
    assert np.abs(fields[:, :, 0, :, 2]).max() < 0.5
    return fields


# ---- 1. the large case through the sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_weighted_objectives_across_many_workgroups(big, form):
    L, eng = big, big.c.solver.engine

    def run():
        fields = solve(L, form)
        res = {}
        for kind in (O.KINETIC, O.ANGULAR_MOMENTUM):
            spec = L.spec(kind)
            _, fb, _, _ = O.host_value_and_cotangent(spec, fields, L.inertia)
            val, ref = TO.host_reference(eng, spec, fields, L.inertia)
            obj, out, st = eng.objective_value_and_grad(kind, spec.block_weights, spec.time_weights, spec.lever0, which=TO.WHICH)
            obj, out = obj.copy(), host(out)
            only = eng.objective_value(kind, spec.block_weights, spec.time_weights, spec.lever0)
            units = OS.weighted_unit_terms(kind, L.w, L.lever0, fields, L.inertia)
            assert np.array_equal(only, obj)                          # the value-only entry: the same reduction on the same history
            assert set(out) == set(TO.WHICH) - ({"block_centroids"} if kind == O.KINETIC else set())
            assert all(np.abs(ref[k]).max() > 0 for k in out if k != "void_angle0" or L.npb == 4)
            assert all(np.abs(ref["inertia"][m]).max() > 0 for m in range(OS.BATCH))
            if form == "fixed-records":
                assert st["checkpoint_records"] == 1, st
            # (the host's np.sum of the same terms, for the record: within 1e-13 of sum |term| as well)
            assert value_error(val, units, L.tau)[0] <= TOL_VALUE
            check(f"{L.lattice} {form} weighted kind={kind}", obj, out, ref, units, L.tau, TOL_WEIGHTED,
                  lambda fb=fb: sweep_floor(eng, fb, TO.WHICH))
            res[kind] = obj
        return res
    res = _with_env(FORMS[form][0], run)
    assert not np.array_equal(res[O.KINETIC], res[O.ANGULAR_MOMENTUM])


@pytest.mark.parametrize("form", list(FORMS))
def test_strain_energy_across_many_workgroups(big, form):
    """parts (0, 0.5, 2, 1.5): the contact part is on; with (ALL) and without (DESIGN) the per-ligament gradients."""
    L, eng, c = big, big.c.solver.engine, big.c
    parts = OS.STRAIN_PARTS

    def run():
        fields = solve(L, form)
        val, ref, fb = TS_.yardstick(eng, c, L.cps, fields, L.bw, L.tau, parts, TS_.ALL)
        obj, out, _ = eng.strain_objective_value_and_grad(L.bw, L.tau, parts, which=TS_.ALL)
        obj, out = obj.copy(), host(out)
        obj_d, out_d, _ = eng.strain_objective_value_and_grad(L.bw, L.tau, parts, which=TS_.DESIGN)
        obj_d, out_d = obj_d.copy(), host(out_d)
        only = eng.strain_objective_value(L.bw, L.tau, parts)
        return fields, val, ref, fb, obj, out, obj_d, out_d, only
    fields, val, ref, fb, obj, out, obj_d, out_d, only = _with_env(FORMS[form][0], run)
    assert np.array_equal(only, obj) and np.array_equal(obj_d, obj)          # one reduction on one history
    assert set(out) == set(TS_.ALL) and set(out_d) == set(TS_.DESIGN)
    assert not fb[:, 0].any() and not fb[:, :, 1].any()                       # tau[0] = 0; a strain energy has no velocity cotangent
    lv = L.leaves()
    units, contact = zip(*(OS.strain_unit_terms(fields[m, :, 0], lv[m], c.bonds, L.bw[m], parts) for m in range(OS.BATCH)))
    if L.lattice == "quads":
        assert all(ce.sum() > 0 for ce in contact)                            # the contact energy of the reference
    assert all(np.abs(ref[k]).max() > 0 for k in TS_.ALL if L.npb == 4 or k not in ("void_angle0", "contact"))
    assert value_error(val, units, L.tau)[0] <= TOL_VALUE                     # the yardstick's own value is the sum of these items
    floor = lambda: _with_env(FORMS[form][0], lambda: (solve(L, form), sweep_floor(eng, fb, TS_.ALL))[1])      # noqa: E731
    check(f"{L.lattice} {form} strain (ALL)", obj, out, ref, units, L.tau, TOL_GRAD, floor)
    check(f"{L.lattice} {form} strain (DESIGN)", obj_d, out_d, {k: ref[k] for k in TS_.DESIGN}, units, L.tau, TOL_GRAD, floor)


@pytest.mark.parametrize("form", list(FORMS))
def test_signal_misfit_across_many_workgroups(big, form):
    """257 signals of three terms each; the targets are fixed inputs: the device's own signals times U(0.5, 1.5), shifted (OS.signal_targets);
    the signals themselves are compared with the yardstick's below."""
    L, eng, c = big, big.c.solver.engine, big.c
    lv = L.leaves()

    def run():
        fields = solve(L, form)
        S = eng.signal_values(L.terms, L.ns)
        targets = L.targets(S)
        val, S_ref, ref, fb, explicit = TG.yardstick(eng, c, lv, fields, L.terms, L.ns, targets, L.omega, L.tau, TG.ALL)
        obj, out, _ = eng.signal_misfit_value_and_grad(L.terms, L.ns, targets, L.omega, L.tau, which=TG.ALL)
        obj, out = obj.copy(), host(out)
        obj_d, out_d, _ = eng.signal_misfit_value_and_grad(L.terms, L.ns, targets, L.omega, L.tau, which=TG.DESIGN)
        obj_d, out_d = obj_d.copy(), host(out_d)
        only = eng.signal_misfit_value(L.terms, L.ns, targets, L.omega, L.tau)
        S2 = eng.signal_values(L.terms, L.ns)
        return fields, S, S2, targets, val, S_ref, ref, fb, obj, out, obj_d, out_d, only
    fields, S, S2, targets, val, S_ref, ref, fb, obj, out, obj_d, out_d, only = _with_env(FORMS[form][0], run)
    assert S.shape == (OS.BATCH, OS.N_OUT, L.ns) and np.array_equal(S, S2)
    e_s = float(np.abs(S - S_ref).max() / np.abs(S_ref).max())
    per = max(float(np.abs(S[..., s] - S_ref[..., s]).max() / np.abs(S_ref[..., s]).max()) for s in range(L.ns))
    print(f"[objective shapes] {L.lattice} {form} signal values: {e_s:.2e} of the largest signal; worst signal of its own largest entry {per:.2e}")
    assert all(np.abs(S_ref[..., s]).max() > 0 for s in range(L.ns)) and e_s <= TOL_SIGNAL and per <= 1e-11
    assert np.array_equal(only, obj) and np.array_equal(obj_d, obj)
    assert set(out) == set(TG.ALL) and set(out_d) == set(TG.DESIGN)
    assert np.abs(fb[:, :, 0]).max() > 0 and np.abs(fb[:, :, 1]).max() > 0 and not fb[:, 0].any()
    assert all(np.abs(ref[k]).max() > 0 for k in TG.ALL if L.npb == 4 or k not in ("void_angle0", "contact"))
    units = [OS.signal_unit_terms(S_ref[m], targets[m], L.omega) for m in range(OS.BATCH)]
    assert value_error(val, units, L.tau)[0] <= TOL_VALUE
    floor = lambda: _with_env(FORMS[form][0], lambda: (solve(L, form), sweep_floor(eng, fb, TG.ALL))[1])      # noqa: E731
    check(f"{L.lattice} {form} signal (ALL)", obj, out, ref, units, L.tau, TOL_GRAD, floor)
    check(f"{L.lattice} {form} signal (DESIGN)", obj_d, out_d, {k: ref[k] for k in TG.DESIGN}, units, L.tau, TOL_GRAD, floor)


# ---- 2. routing checks that do not go through the sweep -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quads(hip_lib):
    L = OS.LargeCase("quads")
    L.fields = _with_env(FORMS["fixed-records"][0], lambda: solve(L, "fixed-records"))
    y = L.state0_as_output()
    assert all(np.array_equal(L.fields[m, 0], y) for m in range(OS.BATCH))
    L.first = np.broadcast_to(y, (OS.BATCH, 1) + y.shape)                      # the initial state as a history of one output
    return L


def one_hot_check(tag, L, value_of, units, first_units):
    """value_of(tau) -> (batch,) on the resident history; units[m][k, ...] the host's unit terms; first_units[m][0, ...] those of the initial state"""
    worst = 0.0
    for k in OS.ONE_HOT:
        obj = value_of(np.eye(OS.N_OUT)[k])
        for m in range(OS.BATCH):
            for src in ([units[m][k]] + ([first_units[m][0]] if k == 0 else [])):
                value, total = math.fsum(src.ravel()), math.fsum(np.abs(src).ravel())
                assert total > 0
                err = abs(float(obj[m]) - value) / total
                worst = max(worst, err)
                assert err <= TOL_VALUE, (tag, k, m, err)
    print(f"[objective shapes] quads one-hot tau, {tag}: worst value error over outputs {OS.ONE_HOT} {worst:.2e} of that output's sum |term|")


@pytest.mark.parametrize("kind", [O.KINETIC, O.ANGULAR_MOMENTUM])
def test_one_output_at_a_time_weighted(quads, kind):
    L, eng = quads, quads.c.solver.engine
    _with_env(FORMS["fixed-records"][0], lambda: solve(L, "fixed-records"))
    lever = L.lever0 if kind == O.ANGULAR_MOMENTUM else None
    units = OS.weighted_unit_terms(kind, L.w, L.lever0, L.fields, L.inertia)
    first = OS.weighted_unit_terms(kind, L.w, L.lever0, L.first, L.inertia)
    one_hot_check(f"weighted kind={kind}", L, lambda tau: eng.objective_value(kind, L.w, tau, lever), units, first)


def test_one_output_at_a_time_strain(quads):
    L, eng = quads, quads.c.solver.engine
    _with_env(FORMS["fixed-records"][0], lambda: solve(L, "fixed-records"))
    lv = L.leaves()
    units = [OS.strain_unit_terms(L.fields[m, :, 0], lv[m], L.c.bonds, L.bw[m], OS.STRAIN_PARTS)[0] for m in range(OS.BATCH)]
    first = [OS.strain_unit_terms(L.first[m, :, 0], lv[m], L.c.bonds, L.bw[m], OS.STRAIN_PARTS)[0] for m in range(OS.BATCH)]
    one_hot_check("strain", L, lambda tau: eng.strain_objective_value(L.bw, tau, OS.STRAIN_PARTS), units, first)


def test_one_output_at_a_time_signal(quads):
    L, eng = quads, quads.c.solver.engine
    _with_env(FORMS["fixed-records"][0], lambda: solve(L, "fixed-records"))
    lv = L.leaves()
    zeros = np.zeros((OS.N_OUT, L.ns))
    S = np.stack([signal_misfit(L.fields[m], lv[m], L.c.bonds, L.terms, L.ns, zeros, None, None)[1] for m in range(OS.BATCH)])
    S0 = np.stack([signal_misfit(L.first[m], lv[m], L.c.bonds, L.terms, L.ns, zeros[:1], None, None)[1] for m in range(OS.BATCH)])
    targets = L.targets(S)
    units = [OS.signal_unit_terms(S[m], targets[m], L.omega) for m in range(OS.BATCH)]
    first = [OS.signal_unit_terms(S0[m], targets[m, :1], L.omega) for m in range(OS.BATCH)]
    one_hot_check("signal", L, lambda tau: eng.signal_misfit_value(L.terms, L.ns, targets, L.omega, tau), units, first)


# ---- 3. exact-boundary small cases ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    e = TO.Ensemble(request.param)
    e.leaves = [TG.member_leaves(e.c, e.cps, m) for m in range(TO.BATCH)]
    return e


@pytest.mark.parametrize("name", list(OS.SMALL))
def test_items_that_fill_their_workgroups_exactly(ens, name):
    """T x n_act = 256, 64 and 65 on the siblings' ensemble (pulse drive from rest, 3 members): the comparisons of their case 1, all three
    families, stage launches at the records level."""
    T, n = OS.SMALL[name]
    c, eng = ens.c, ens.c.solver.engine
    lattice = "quads" if c.geo.n_npb == 4 else "kagome"
    assert int(c.con[0, 0]) == OS.SMALL_CENTRE[lattice]
    blocks, inside = OS.small_blocks(c.bonds, c.geo.n_npb, ens.nb, n, OS.SMALL_CENTRE[lattice])
    rng = np.random.default_rng(13)
    ts = np.linspace(0.0, 1e-4 * (T - 1), T)
    tau = rng.uniform(0.25, 2.0, T)
    tau[0] = 0.0
    w = np.zeros((TO.BATCH, ens.nb))
    w[:, blocks] = OS.signed(rng, (TO.BATCH, n))
    bw = np.zeros((TO.BATCH, len(c.bonds)))
    bw[:, inside] = OS.signed(rng, (TO.BATCH, len(inside)))
    terms = OS.small_terms(blocks)
    omega = rng.uniform(0.25, 2.0, n)
    factor = rng.uniform(0.5, 1.5, (TO.BATCH, T, n))
    lever0 = ens.cen - ens.cen[0][blocks].mean(0)
    sig = OS.signal_tables(c.bonds, c.geo.n_npb, terms)
    assert len(OS.objective_blocks(w)) == n and len(OS.strain_blocks(c.bonds, c.geo.n_npb, bw)) == n and sig["n_fb"] == n and sig["n_sig"] == n
    assert T * n == {"exactly-256": 256, "exactly-64": 64, "65": 65}[name]
    env, spi = PATHS["stage-launches"]

    def run():
        fields = np.array(c.solver(np.zeros((2, ens.nb, 3)), ts, ens.cps, keep_trajectory=True, steps_per_interval=spi))
        res = {}
        for kind in (O.KINETIC, O.ANGULAR_MOMENTUM):
            spec = O.ObjectiveSpec(kind, w, tau, lever0 if kind == O.ANGULAR_MOMENTUM else None)
            val, ref = TO.host_reference(eng, spec, fields, ens.inertia)
            obj, out, st = eng.objective_value_and_grad(kind, spec.block_weights, spec.time_weights, spec.lever0, which=TO.WHICH)
            assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
            res[kind] = (val, ref, obj.copy(), host(out), eng.objective_value(kind, spec.block_weights, spec.time_weights, spec.lever0))
        val, ref, _ = TS_.yardstick(eng, c, ens.cps, fields, bw, tau, OS.STRAIN_PARTS, TS_.ALL)
        obj, out, _ = eng.strain_objective_value_and_grad(bw, tau, OS.STRAIN_PARTS, which=TS_.ALL)
        res["strain"] = (val, ref, obj.copy(), host(out), eng.strain_objective_value(bw, tau, OS.STRAIN_PARTS))
        S = eng.signal_values(terms, n)
        targets = S * factor
        val, S_ref, ref, _, _ = TG.yardstick(eng, c, ens.leaves, fields, terms, n, targets, omega, tau, TG.ALL)
        obj, out, _ = eng.signal_misfit_value_and_grad(terms, n, targets, omega, tau, which=TG.ALL)
        res["signal"] = (val, ref, obj.copy(), host(out), eng.signal_misfit_value(terms, n, targets, omega, tau))
        return res, S, S_ref
    res, S, S_ref = _with_env(env, run)
    tag = f"{lattice} T x n = {T} x {n}"
    for kind in (O.KINETIC, O.ANGULAR_MOMENTUM):
        val, ref, obj, out, only = res[kind]
        assert np.array_equal(only, obj) and np.abs(val).min() > 0
        TO.compare(f"{tag} kind={kind}", obj, out, val, ref)
    val, ref, obj, out, only = res["strain"]
    assert np.array_equal(only, obj) and np.abs(val).min() > 0
    TS_.compare(f"{tag} strain", obj, out, val, ref)
    e_s = float(np.abs(S - S_ref).max() / np.abs(S_ref).max())
    print(f"[signal misfit] {tag}: signal values {e_s:.2e}")
    assert e_s <= TOL_SIGNAL
    val, ref, obj, out, only = res["signal"]
    assert np.array_equal(only, obj) and np.abs(val).min() > 0
    TG.compare(f"{tag} signal", obj, out, val, ref)
