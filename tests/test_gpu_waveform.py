"""-m gpu: the samples of a table drive as a differentiable leaf (loading.Table with named values; include/dfx.h: dfx_fn_table_values,
dfx_fn_table_grads, dfx_fn_table_grad, dfx_drive_cotangent, dfx_fn_table_tangents; kernels: the TRACE builds of the reverse stage in
csrc/dfx_kernels.h, k_stage_times / k_table_grad in csrc/dfx_drive.h, tan_drive_n in csrc/dfx_tangent.h).  The case, the twin and the
premises are tests/waveform_yardstick.py.

  1 sample gradient of vjp against oracle autograd on the fixed grid: displacement drive, force load, kagome; sample 6 an exact zero
  2 the same with cotangents on the prescribed output rows (the host's hat weights of value and rate)
  3 the four checkpoint levels give the same sample gradient (1e-12)
  4 the kept adaptive solve against autograd through the replay of its accepted steps
  5 a batch of 3 with different waveforms, member by member against batch 1; new values on the same handle; the sweep as replayed
    hipGraphs: a long solve, a shorter one, the request toggled, on one handle of batch 2
  6 the trace: sum gbar dg/dp reproduces the sweep's own amplitude and delay gradients (1e-12) and the sample gradient
  7 forward mode: jvp_multi along 5 sample directions against oracle tangents; the transpose identity, fixed grid and adaptive=True
  8 linearity: with linearised ligaments and no contact, S(y) = S(0) + J y with J from signal_jacfwd over (name, j)
  9 a DriveWaveformDesign step lowers a misfit; value_and_grad against a central difference"""
import numpy as np
import pytest

from difflexmm_amd import objective as O
from difflexmm_amd import problems as P
from difflexmm_amd.dynamics import setup_dynamic_solver

from . import waveform_yardstick as wy
from .common import Case
from .time_functions import with_env

pytestmark = pytest.mark.gpu

PATH_ENV = ("DFX_PERSIST", "DFX_FN_TABLE", "DFX_CHECKPOINT", "DFX_STAGE_CHECKPOINT", "DFX_STAGE_BUILDS", "DFX_WT", "DFX_TANGENT_MULTI_FORM",
            "DFX_EAGER_STEPS", "DFX_STREAMS", "DFX_ADAPTIVE_RECORDS", "DFX_PERSIST_MAX_WG")
TS, SPI = wy.TS, wy.SPI


@pytest.fixture(autouse=True)
def _paths_are_chosen_here(monkeypatch, hip_lib):
    for k in PATH_ENV:
        monkeypatch.delenv(k, raising=False)


def _solve_and_vjp(p, pm, fb, ts=TS, **grid):
    s = p.solver
    grid = grid or dict(steps_per_interval=SPI)
    fields = s(p.y0, ts, p.cp(pm), keep_trajectory=True, **grid)
    tree, s0 = s.vjp(fb)
    return np.asarray(fields), tree, s0


def _free_cotangent(p, n_t=len(TS), member=0):
    return wy.fields_bar(p, n_t, seed=3 + member)[0]


def _check_against_oracle(label, p, pm, fb, fields, tree, ref, rtol_fields=wy.RTOL_TRAJ):
    free = p.solver.free_DOF_ids
    n_t = fields.shape[0]
    errs = {"fields": wy.rel(fields.reshape(n_t, 2, -1)[:, :, free], ref["hist"])}
    mine = wy.engine_grads(p, tree)
    for nk, e in wy.grad_errors(mine, ref["grad"]).items():
        errs["d/d" + nk[1]] = e
    print(f"waveform: {label}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["fields"] < rtol_fields, (label, errs)
    bad = {k: v for k, v in errs.items() if k != "fields" and not v < wy.RTOL_GRAD}
    assert not bad, (label, bad)
    return mine


# -- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role,lattice,n", [("disp", "quads", 4), ("force", "quads", 4), ("disp", "kagome", 3)])
def test_sample_gradient_against_oracle_autograd(role, lattice, n):
    wy.check_premises()
    p = wy.problem(None, role, lattice, n)
    pm = wy.member(p)
    fb = _free_cotangent(p)
    fields, tree, _ = _solve_and_vjp(p, pm, fb)
    assert p.solver.adjoint_stats["tile_kernels"] == 0, p.solver.adjoint_stats          # stage launches, generic builds: dfx_stats says what ran
    ref = wy.oracle(p, pm, TS, fb.reshape(len(TS), 2, -1))
    mine = _check_against_oracle(f"{role}/{lattice}", p, pm, fb, fields, tree, ref)
    sl = wy.slot_of(p)
    g, og = mine[(sl, wy.NAME)], ref["grad"][(sl, wy.NAME)]
    assert g.shape == (len(wy.BREAKS),) and np.count_nonzero(og) == len(wy.BREAKS) - 1
    assert g[6] == 0.0 and og[6] == 0.0          # its support holds no evaluation time


# -- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_cotangents_on_the_prescribed_output_rows():
    wy.check_premises()
    p = wy.problem(None, "disp")
    pm = wy.member(p)
    fb = np.random.default_rng(41).normal(size=(len(TS), 2, p.c.geo.n_blocks, 3))
    con = p.solver.constrained_DOF_ids
    assert np.abs(fb.reshape(len(TS), 2, -1)[:, :, con]).min() > 0.0
    fields, tree, _ = _solve_and_vjp(p, pm, fb)
    ref = wy.oracle(p, pm, TS, fb.reshape(len(TS), 2, -1))
    mine = _check_against_oracle("output rows", p, pm, fb, fields, tree, ref)
    # the rows matter: the same cotangent without them gives another sample gradient
    fb0 = fb.copy()
    fb0.reshape(len(TS), 2, -1)[:, :, con] = 0.0
    _, tree0, _ = _solve_and_vjp(p, pm, fb0)
    assert wy.rel(wy.engine_grads(p, tree0)[(0, wy.NAME)], mine[(0, wy.NAME)]) > 1e-6


# -- 3 ---------------------------------------------------------------------------------------------------------------------------------
LEVELS = {"records": (1, 0), "stages": (0, 1), "state": (0, 0), "segments": (2, 0)}


def test_checkpoint_levels_give_the_same_sample_gradient():
    wy.check_premises()
    out = {}
    for level, codes in LEVELS.items():
        def run():
            p = wy.problem(None, "disp")
            fields, tree, _ = _solve_and_vjp(p, wy.member(p), _free_cotangent(p))
            st = p.solver.stats
            assert (st["checkpoint_records"], st["stage_checkpoint"]) == codes, (level, st)
            assert p.solver.adjoint_stats["tile_kernels"] == 0, (level, p.solver.adjoint_stats)
            return fields, wy.engine_grads(p, tree)
        out[level] = with_env({"DFX_CHECKPOINT": level}, run)
    ref_f, ref_g = out["records"]
    assert np.abs(ref_g[(0, wy.NAME)]).max() > 0.0
    for level, (f, g) in out.items():
        errs = {nk: wy.rel(np.atleast_1d(g[nk]), np.atleast_1d(ref_g[nk])) for nk in ref_g}
        print(f"waveform: DFX_CHECKPOINT={level}: fields {wy.rel(f, ref_f):.2e}, " + ", ".join(f"d/d{k[1]} {v:.2e}" for k, v in errs.items()))
        assert wy.rel(f, ref_f) < 1e-13 and all(v < 1e-12 for v in errs.values()), (level, errs)


# -- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_default_adaptive_call_against_the_replay_of_its_accepted_steps():
    p = wy.problem(None, "disp")
    s = p.solver
    pm = wy.member(p)
    ts = np.linspace(0.0, wy.HORIZON, 41)
    s.rtol = s.atol = 1e-5
    fb = _free_cotangent(p, len(ts))
    fields = np.asarray(s(p.y0, ts, p.cp(pm), keep_trajectory=True))
    assert s.stats["step_control"] == "adaptive-records", s.stats
    st = np.concatenate([ts[:1], s.engine.adaptive_step_times(0)])
    wy.check_step_premises(st, ts)
    tree, _ = s.vjp(fb)
    assert s.adjoint_stats["tile_kernels"] == 0, s.adjoint_stats
    ref = wy.oracle(p, pm, ts, fb.reshape(len(ts), 2, -1), adaptive_steps=st)
    _check_against_oracle(f"adaptive records, {len(st) - 1} steps", p, pm, fb, fields, tree, ref, rtol_fields=1e-11)


# -- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_with_different_waveforms():
    wy.check_premises()
    rng = np.random.default_rng(5)
    waves = [wy.VALUES, rng.normal(size=len(wy.BREAKS)), 0.3 * rng.normal(size=len(wy.BREAKS))]
    p3 = wy.problem(None, "disp", batch=3)
    s3 = p3.solver
    members = [wy.member(p3, w) for w in waves]
    fb3 = wy.fields_bar(p3, len(TS))
    fields3 = np.asarray(s3(p3.y0, TS, [p3.cp(pm) for pm in members], keep_trajectory=True, steps_per_interval=SPI))
    trees3, _ = s3.vjp(fb3)
    p1 = wy.problem(None, "disp")
    for m, pm in enumerate(members):
        fields, tree, _ = _solve_and_vjp(p1, wy.member(p1, waves[m]), fb3[m])
        g3, g1 = wy.engine_grads(p3, trees3[m]), wy.engine_grads(p1, tree)
        errs = {nk: wy.rel(np.atleast_1d(g3[nk]), np.atleast_1d(g1[nk])) for nk in g1}
        errs["cnv"] = wy.rel(trees3[m].geometrical_params.centroid_node_vectors, tree.geometrical_params.centroid_node_vectors)
        e_f = wy.rel(fields3[m], fields)
        print(f"waveform: batch of 3, member {m}: fields {e_f:.2e}, " + ", ".join(f"{k if isinstance(k, str) else k[1]} {v:.2e}" for k, v in errs.items()))
        assert e_f < 1e-13 and all(v < 1e-12 for v in errs.values()), (m, e_f, errs)
    assert wy.rel(fields3[1], fields3[0]) > 1e-3
    # new values on the same handle: the next solve follows them
    turned = np.asarray(s3(p3.y0, TS, [p3.cp(members[(m + 1) % 3]) for m in range(3)], keep_trajectory=True, steps_per_interval=SPI))
    for m in range(3):
        assert wy.rel(turned[m], fields3[(m + 1) % 3]) < 1e-13, m


def test_replayed_graphs_follow_the_trace():
    """The sweep as cached hipGraphs (DFX_EAGER_STEPS=0: what solves of more than 128 steps on small lattices take by default), whose kernel
    nodes hold the trace buffer and its row count by value: a batch of 2 on ONE handle through a long solve, a shorter one with the same
    steps per segment, and the request switched off and on again, every sample gradient against the eager sweep of a fresh handle
    (1e-12).  A replay of a graph captured for another row count, or without the trace kernels, gives wrong or zero gradients for every
    (member, function) but the first."""
    wy.check_premises()
    rng = np.random.default_rng(61)
    waves = [wy.VALUES, rng.normal(size=len(wy.BREAKS))]
    grids = {"long": TS, "short": TS[:3]}

    def sweep(p, ts):
        members = [wy.member(p, w) for w in waves]
        fb = wy.fields_bar(p, len(ts))
        p.solver(p.y0, ts, [p.cp(pm) for pm in members], keep_trajectory=True, steps_per_interval=SPI)
        trees, _ = p.solver.vjp(fb)
        return [wy.engine_grads(p, t) for t in trees]
    eager = {k: sweep(wy.problem(None, "disp", batch=2), ts) for k, ts in grids.items()}

    def graphs():
        p = wy.problem(None, "disp", batch=2)
        out = {"long": sweep(p, grids["long"]), "short": sweep(p, grids["short"])}
        p.solver.engine.fn_table_grads(False)
        p.solver.engine.adjoint(wy.fields_bar(p, 3))            # the same sweep without the trace (per-ligament gradients wanted as before)
        p.solver.engine.fn_table_grads(True)
        out["short again"] = sweep(p, grids["short"])
        out["long again"] = sweep(p, grids["long"])
        return out
    out = with_env({"DFX_EAGER_STEPS": "0"}, graphs)
    for k, got in out.items():
        ref = eager[k.split()[0]]
        for m in range(2):
            assert np.abs(ref[m][(0, wy.NAME)]).max() > 0.0
            errs = {nk[1]: wy.rel(np.atleast_1d(got[m][nk]), np.atleast_1d(ref[m][nk])) for nk in ref[m]}
            print(f"waveform: graphs, {k}, member {m}: " + ", ".join(f"{n} {v:.2e}" for n, v in errs.items()))
            assert all(v < 1e-12 for v in errs.values()), (k, m, errs)


# -- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["disp", "force"])
def test_trace_reproduces_the_sweeps_own_parameter_gradients(role):
    times_ = wy.check_premises()
    p = wy.problem(None, role)
    s = p.solver
    pm = wy.member(p)
    s(p.y0, TS, p.cp(pm), keep_trajectory=True, steps_per_interval=SPI)
    raw = s.vjp_raw(_free_cotangent(p), which=("centroid_node_vectors", "fn_params"))
    times, gbar = s.drive_cotangent(0)
    assert times.shape == (24 * 6,) and gbar.shape == (1, 24 * 6)
    assert np.allclose(np.sort(times), np.sort(times_[:-1]), rtol=0, atol=1e-18)
    d = pm[wy.slot_of(p)]
    amp, delay, Y = d["amplitude"], d["delay"], d[wy.NAME]
    term = (s.con_terms + s.load_terms)[0]
    hats = np.stack([term.hat_weights(t - delay) for t in times])            # (n, n_tab)
    rates = np.stack([term.rate_weights(t - delay) for t in times])
    want = {"amplitude": float(gbar[0] @ (hats @ Y)), "delay": float(gbar[0] @ (-amp * (rates @ Y)))}
    got = {"amplitude": raw["fn_params"][0, 0, 0], "delay": raw["fn_params"][0, 0, 1]}
    samples = amp * (gbar[0] @ hats)
    errs = {k: abs(got[k] - want[k]) / abs(want[k]) for k in want}
    errs["samples"] = wy.rel(raw["fn_table_values"][0][0], samples)
    print(f"waveform: trace identity ({role}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(abs(v) > 0 for v in want.values()) and all(v < 1e-12 for v in errs.values()), errs


# -- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_jvp_multi_along_five_sample_directions_against_oracle_tangents():
    wy.check_premises()
    p = wy.problem(None, "disp")
    s = p.solver
    pm = wy.member(p)
    dirs = wy.sample_directions(5)
    fields, fdot = s.jvp_multi(p.y0, TS, p.cp(pm), [(None, wy.sample_tangent_tree(p, d)) for d in dirs], steps_per_interval=SPI)
    free = s.free_DOF_ids
    fb = _free_cotangent(p)
    ref = wy.oracle(p, pm, TS, fb.reshape(len(TS), 2, -1), tangents=[{(0, wy.NAME): d} for d in dirs])
    assert wy.rel(np.asarray(fields).reshape(len(TS), 2, -1)[:, :, free], ref["hist"]) < wy.RTOL_TRAJ
    for k in range(5):
        assert np.abs(ref["dots"][k]).max() > 0
        e = wy.rel(np.asarray(fdot)[k].reshape(len(TS), 2, -1)[:, :, free], ref["dots"][k])
        print(f"waveform: jvp_multi direction {k}: {e:.2e}")
        assert e < wy.RTOL_GRAD, (k, e)


@pytest.mark.parametrize("adaptive", [False, True])
def test_tangent_is_the_transpose_of_the_sample_gradient(adaptive):
    p = wy.problem(None, "disp")
    s = p.solver
    pm = wy.member(p)
    dirs = wy.sample_directions(5, seed=37)
    tans = [(None, wy.sample_tangent_tree(p, d)) for d in dirs]
    rng = np.random.default_rng(43)
    if adaptive:
        ts = np.linspace(0.0, wy.HORIZON, 41)
        s.rtol = s.atol = 1e-5
        fields, fdot = s.jvp_multi(p.y0, ts, p.cp(pm), tans, adaptive=True)
        assert s.stats["step_control"] == "adaptive-dense" and s.stats["kept_trajectory"], s.stats
    else:
        ts = TS
        wy.check_premises()
        fields, fdot = s.jvp_multi(p.y0, ts, p.cp(pm), tans, steps_per_interval=SPI)
        s(p.y0, ts, p.cp(pm), keep_trajectory=True, steps_per_interval=SPI)
    fb = rng.normal(size=np.shape(fields))          # every row, the prescribed ones included: the host's hat weights on both sides
    tree, _ = s.vjp(fb)
    g = wy.engine_grads(p, tree)[(0, wy.NAME)]
    for k, d in enumerate(dirs):
        lhs, rhs = float(np.sum(fb * np.asarray(fdot)[k])), float(g @ d)
        print(f"waveform: transpose identity ({'adaptive' if adaptive else 'fixed'}), direction {k}: {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
        assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)


# -- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_signals_are_affine_in_the_samples_of_a_linear_lattice():
    """S(y) = S(0) + J y with J from signal_jacfwd over the (name, j) leaves, on the random initial state of the shared case.  The
    "linearised" ligament linearises the strain measures, not the kinematics: the node vectors (length <= r = 15 / sqrt 2) still turn
    with the exact R(theta), so the response is affine in the samples only up to a remainder r d_theta^2 / 2, d_theta <= A |y| / l the
    rotation the drive adds (l = 2.25, the shortest length of the lattice).  The size of y is therefore part of the case: samples of order
    5e-8 (|y| <= 2e-7 asserted) keep the remainder under 3e-13 mm, against a bar of RTOL_TRAJ x max|S| > 1e-12 mm (the signals are of the
    size of the initial displacements, 0.05 mm; asserted), while J y is > 1e-6 of max|S| (asserted; 1.8e-6 measured): an error of a part in
    ten thousand in J y fails.  Much smaller samples would drown in the rounding of the forward solve's strain differences (measured: samples of
    order 1e-12 on a lattice at rest give 8.5e-5 relative to J y); samples of order one give 0.23 (printed): that is the model, not the
    Jacobian -- test 7 holds the tangents against the oracle's."""
    c = Case("quads", 4, False, False, seed=7, lib=None)
    term = wy.WaveTerm(np.array([1.0] + [0.0] * 6))
    s = setup_dynamic_solver(c.geo, c.energy, constrained_block_DOF_pairs=c.con, constrained_DOFs_fn=term.lib(), damped_blocks=c.damped)
    y0 = c.random_state(0.05, 0.02, 5.0)
    spec = O.SignalSpec.fields_of([(5, 0), (6, 1), (10, 2), (9, 0)], kind="displacement")
    unit = np.random.default_rng(47).normal(size=len(wy.BREAKS))
    y = 5e-8 * unit
    assert np.abs(y).max() <= 2e-7 and 15 / np.sqrt(2) * (wy.AMPLITUDE * 2e-7 / 2.25) ** 2 / 2 < 3e-13

    def cp(values):
        return c.cp._replace(constraint_params={"amplitude": wy.AMPLITUDE, "delay": wy.DELAY, wy.NAME: np.asarray(values, dtype=float)})

    def signals(values):
        s(y0, TS, cp(values), steps_per_interval=SPI)
        return s.signal_values(spec)[0]
    wrt = [(wy.NAME, j) for j in range(len(wy.BREAKS))]
    S0, cols = s.signal_jacfwd(y0, TS, cp(np.zeros(len(wy.BREAKS))), wrt, spec, steps_per_interval=SPI)
    assert wy.rel(S0, signals(np.zeros(len(wy.BREAKS)))) < 1e-13
    J = np.stack([cols[name] for name in wrt], axis=-1)           # (T, n_signals, n_tab)
    assert np.all(J[..., 6] == 0.0) and all(np.abs(J[..., j]).max() > 0.0 for j in range(len(wy.BREAKS)) if j != 6)
    Sy = signals(y)
    assert wy.RTOL_TRAJ * np.abs(Sy).max() > 1e-12 and np.abs(J @ y).max() > 1e-6 * np.abs(Sy).max()
    e = wy.rel(Sy, S0 + J @ y)
    print(f"waveform: S(y) = S(0) + J y: {e:.2e} (J y: {np.abs(J @ y).max() / np.abs(Sy).max():.1e} of S); "
          f"{wy.rel(signals(unit), S0 + J @ unit):.2e} with samples of order one")
    assert e < wy.RTOL_TRAJ, e


# -- 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_design_step_lowers_a_misfit_and_its_gradient_matches_a_central_difference():
    p = wy.problem(None, "disp")
    s = p.solver
    pm = wy.member(p)
    blocks = [(5, 0), (6, 1), (10, 2)]
    goal = wy.VALUES + 2e-3 * np.random.default_rng(59).normal(size=len(wy.BREAKS))
    s(p.y0, TS, p.cp(wy.member(p, goal)), steps_per_interval=SPI)
    spec = O.SignalSpec.fields_of(blocks, kind="velocity")
    spec = spec.with_targets(s.signal_values(spec)[0])               # the motion a waveform nearby produces
    design = P.DriveWaveformDesign(s, p.y0, TS, p.cp(pm), wy.NAME, spec, steps_per_interval=SPI)
    y = wy.VALUES.copy()
    v0, g = design.value_and_grad(y)
    assert v0 > 0.0 and g.shape == y.shape and g[6] == 0.0
    d = np.random.default_rng(53).normal(size=y.shape)
    eps = 1e-6
    fd = (design.value_and_grad(y + eps * d)[0] - design.value_and_grad(y - eps * d)[0]) / (2 * eps)
    e = abs(float(g @ d) - fd) / abs(fd)
    print(f"waveform: design gradient against a central difference: {e:.2e}")
    assert e < 1e-6, (float(g @ d), fd)
    # MMA's first move is of the size of the box: one that reaches half way to the goal (breakpoints 2e-6 s apart make the velocity
    # signals steep in the samples between them: the goal is a waveform nearby)
    best = design.run_mma(y, 6, lower_bound=y - 1e-3, upper_bound=y + 1e-3)
    assert best[0] == y[0] and best[-1] == y[-1]
    assert np.all(np.abs(best - y) <= 1e-3 * (1 + 1e-12)) and len(design.objective_values) <= 6
    v1 = design.value_and_grad(best)[0]
    print(f"waveform: misfit {v0:.4e} -> {v1:.4e} in {len(design.objective_values)} evaluations")
    assert v1 < v0
