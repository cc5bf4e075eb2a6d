"""-m gpu: every time function of the closed library (eval_time_fn, csrc/dfx_physics.h) on every piece of device code that evaluates it.
The cases, twins and checkers are tests/time_functions.py; tests/test_time_functions.py validates them on the CPU port.

The matrix.  Rows: function x role (disp = prescribed displacement, force = load).  Columns: what the HIP engine's result is compared with.
"oracle" = the torch oracle driven by the function's torch twin (fields RTOL_TRAJ; every parameter gradient and fields_dot RTOL_GRAD);
"paths" = the same case on another kernel path, engine against engine; "-" = not covered.

  function x role      slot  default path (persistent loop)      adaptive (kept steps)   other paths (see PATHS)   rhs / rhs_vjp / rhs_jvp
                             fields   vjp      jvp               vjp vs replay
  Pulse      disp      0     oracle   oracle   oracle            (test_gpu_parity)       (rest of the suite)       (test_gpu_parity, test_gpu_rhs_jvp)
  Pulse      force     1*    oracle   oracle   oracle            -                       -                         -
  Harmonic   disp      0     oracle   oracle   oracle            -                       paths (two-slot case)     oracle (two-slot case)
  Harmonic   force     1*    oracle   oracle   oracle            -                       -                         -
  Ramp       disp      0     oracle   oracle   oracle            -                       -                         -
  Ramp       force     1     oracle   oracle   oracle            -                       paths (two-slot case)     oracle (two-slot case)
  Sech2Tanh  disp      0     oracle   oracle   oracle            -                       -                         -
  Sech2Tanh  force     1*    oracle   oracle   oracle            oracle                  paths                     oracle
  Constant   disp      0     oracle   oracle   oracle            -                       -                         -
  Constant   force     1*    oracle   oracle   oracle            -                       -                         -
  CappedRamp disp      0     oracle   oracle   oracle            oracle                  paths (chip-filling)      oracle (with DelayedPulse)
  CappedRamp force     1*    oracle   oracle   oracle            -                       -                         -
  DelayedPulse disp    1     oracle   oracle   oracle            -                       paths (chip-filling)      oracle (with CappedRamp)
  Table      disp      0     oracle   oracle   oracle            oracle                  paths                     oracle
  Table      force     1*    oracle   oracle   oracle            -                       -                         -
  (* a force alone sits in slot 0 of the engine; it is slot 1 in the two-slot cases: Harmonic disp + Ramp force, Pulse disp + Sech2Tanh force
  on two DOFs of ONE block.  Slot-1 gradients against the oracle: those two cases and CappedRamp + DelayedPulse, whose chain reaches
  compressive_strain and compressive_strain_rate.)

  Also against the oracle: both lattices (kagome: Table disp, Sech2Tanh force); a pulse that ends exactly on an output time; a batch of 3 whose
  members are before / inside / after their pulse (ramp) at one output time, member by member; amplitude 0 for every function in both
  roles (fields = the undriven solve, finite gradients and tangents equal to autograd's, a non-zero amplitude gradient) and as one member
  of a batch (the others bit-identical to a batch without it); Table with 2 breakpoints and with the whole horizon past its end;
  Constant as a force.

PATHS, engine against engine, for Table disp, Sech2Tanh force and Harmonic disp + Ramp force (fields 1e-13, gradient leaves 1e-12, tangent
columns 1e-12; every run asserts from the solver's stats that it took the path it names):
  persistent loop (default) | DFX_PERSIST=0 with the per-segment table | DFX_PERSIST=0 DFX_FN_TABLE=0 (inline evaluation; one launch per
  segment fewer) | DFX_CHECKPOINT=records, stages, state, segments | caller-chosen unequal steps on all three | per-member grids in a batch
  of 2 against each member alone | the adaptive loop and the stage-launch controller, each with vjp and the raw sweep on the kept steps and
  jvp(adaptive=True), each against the oracle's replay of its own accepted steps, and against each other where both controllers took the
  same decisions (bars of test_adaptive_controller_in_the_loop_equals_the_stage_launch_controller) | jvp_multi K = 3, 5
  in both DFX_TANGENT_MULTI_FORMs against single jvps | jacfwd over the function's own names against jvp columns | 128 x 128 quads with
  CappedRamp + DelayedPulse: the per-stage builds against DFX_STAGE_BUILDS=0.
Not covered: more than two functions per problem; the cotangents / tangents of prescribed-DOF OUTPUTS (host-side central differences)."""
import numpy as np
import pytest

from . import time_functions as tf
from .parity import RTOL_RHS

pytestmark = pytest.mark.gpu

ROLES = [(fn, role) for fn in tf.VALUES for role in ("disp", "force")]
TS = np.linspace(0, tf.HORIZON, tf.N_OUT)
PATH_ENV = ("DFX_PERSIST", "DFX_FN_TABLE", "DFX_CHECKPOINT", "DFX_STAGE_CHECKPOINT", "DFX_STAGE_BUILDS", "DFX_WT", "DFX_TANGENT_MULTI_FORM",
            "DFX_EAGER_STEPS", "DFX_STREAMS", "DFX_ADAPTIVE_RECORDS", "DFX_PERSIST_MAX_WG")


@pytest.fixture(autouse=True)
def _paths_are_chosen_here(monkeypatch, hip_lib):
    """Every test names its path itself: a suite run with one of these set must not move the default underneath them."""
    for k in PATH_ENV:
        monkeypatch.delenv(k, raising=False)


# -- against the oracle (the same checks as on the CPU port, plus forward mode) ------------------------------------------------------------
@pytest.mark.parametrize("fn,role", ROLES)
def test_every_function_in_both_roles_against_the_oracle(fn, role):
    errs, out = tf.check_fixed(tf.single(None, fn, role), f"{fn}/{role}")
    assert out["stats"]["tile_kernels"] == 3 and (0, "fields_dot") in errs         # the default path; forward mode ran


@pytest.mark.parametrize("fn,role", [("Table", "disp"), ("Sech2Tanh", "force")])
def test_kagome_lattice(fn, role):
    tf.check_fixed(tf.single(None, fn, role, lattice="kagome", n=3), f"kagome/{fn}/{role}")


@pytest.mark.parametrize("role", ["disp", "force"])
def test_pulse_that_ends_exactly_on_an_output_time(role):
    tf.check_pulse_end_on_output(None, role)


def test_two_slots_harmonic_drive_and_ramp_force():
    tf.check_fixed(tf.harmonic_plus_ramp(None), "Harmonic+Ramp")


def test_two_slots_capped_ramp_and_delayed_pulse():
    errs, out = tf.check_fixed(tf.static_tuning(None), "CappedRamp+DelayedPulse")
    assert {"d/dcompressive_strain", "d/dcompressive_strain_rate", "d/damplitude", "d/dloading_rate", "d/dinput_delay"} <= {k[1] for k in errs}
    assert all(v != 0.0 for v in out["grads"][0].values())


def test_one_block_constrained_in_x_and_loaded_in_y():
    tf.check_fixed(tf.two_roles_in_one_block(None), "Pulse(x)+Sech2Tanh(y) on one block")


@pytest.mark.parametrize("fn,role", [("Pulse", "disp"), ("Ramp", "force")])
def test_batch_of_three_members_before_inside_and_after(fn, role):
    p = tf.single(None, fn, role, batch=3)
    tf.check_fixed(p, f"{fn}/{role}/batch3", members=tf.staggered_members(p, fn, TS[2]), branches=False)


@pytest.mark.parametrize("fn,role", ROLES)
def test_zero_amplitude(fn, role):
    tf.check_zero_amplitude(None, fn, role)


@pytest.mark.parametrize("role", ["disp", "force"])
def test_zero_amplitude_member_in_a_batch(role):
    tf.check_zero_member_in_batch(None, "Sech2Tanh", role)


@pytest.mark.parametrize("role", ["disp", "force"])
@pytest.mark.parametrize("edge", ["two breakpoints", "past the end"])
def test_table_edges(edge, role):
    tf.check_table_edge(None, edge, role)


def test_constant_force_gradient_is_the_response_to_a_static_load():
    tf.check_constant_force(None)


@pytest.mark.parametrize("family,fn,role", [("smooth", "Sech2Tanh", "force"), ("kinked", "CappedRamp", "disp"), ("table", "Table", "disp")])
def test_adaptive_solve_against_the_replay_of_its_accepted_steps(family, fn, role):
    tf.check_adaptive(tf.single(None, fn, role), f"adaptive/{fn}/{role}")


@pytest.mark.parametrize("case", sorted(tf.RHS_CASES))
def test_rhs_hooks_inside_and_after_the_active_window(case):
    make, times = tf.RHS_CASES[case]
    for t in times:
        errs = tf.check_rhs(make(None), f"rhs/{case}/{t:.3e}", t, RTOL_RHS)
        assert (0, "rhs_dot1") in errs


# -- the same numbers on every path -----------------------------------------------------------------------------------------------------------
PATH_CASES = {"Table disp": lambda: tf.single(None, "Table", "disp"), "Sech2Tanh force": lambda: tf.single(None, "Sech2Tanh", "force"),
              "Harmonic disp + Ramp force": lambda: tf.harmonic_plus_ramp(None)}
STAGE, INLINE = {"DFX_PERSIST": "0"}, {"DFX_PERSIST": "0", "DFX_FN_TABLE": "0"}
LEVELS = {"records": (1, 0), "stages": (0, 1), "state": (0, 0), "segments": (2, 0)}

_DEFAULT = {}


def _default(case):
    """The default path of a case on the 4 x 6 grid: run once, compared with by every path test."""
    if case not in _DEFAULT:
        out = tf.run_path(PATH_CASES[case], {}, TS)
        assert out["stats"]["tile_kernels"] == 3 and out["raw_stats"]["tile_kernels"] == 3, (out["stats"], out["raw_stats"])      # the persistent loops
        _DEFAULT[case] = out
    return _DEFAULT[case]


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_stage_launches_with_the_table_and_with_inline_evaluation(case):
    ref = _default(case)
    table, inline = tf.run_path(PATH_CASES[case], STAGE, TS), tf.run_path(PATH_CASES[case], INLINE, TS)
    assert table["stats"]["tile_kernels"] != 3 and inline["stats"]["tile_kernels"] != 3
    assert table["raw_stats"]["tile_kernels"] != 3 and inline["raw_stats"]["tile_kernels"] != 3
    # k_fn_table is one launch per segment (here: per output interval)
    assert table["stats"]["launches"] - inline["stats"]["launches"] == len(TS) - 1, (table["stats"], inline["stats"])
    assert table["adjoint_stats"]["launches"] > inline["adjoint_stats"]["launches"], (table["adjoint_stats"], inline["adjoint_stats"])
    tf.compare_paths(f"{case}: stage launches + table vs persistent loop", ref, table)
    tf.compare_paths(f"{case}: stage launches, inline vs persistent loop", ref, inline)


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_checkpoint_levels(case):
    """Several segments, so the table is refreshed per segment -- and, at the segments level, again and out of order by the reverse sweep."""
    ref = _default(case)
    for level, codes in LEVELS.items():
        for arm, env in (("loop", {}), ("stage", STAGE)):
            out = tf.run_path(PATH_CASES[case], dict(env, DFX_CHECKPOINT=level), TS, jvp=False)
            assert (out["stats"]["checkpoint_records"], out["stats"]["stage_checkpoint"]) == codes, (level, out["stats"])
            assert (out["stats"]["tile_kernels"] == 3) == (arm == "loop"), (level, arm, out["stats"])
            assert (out["raw_stats"]["tile_kernels"] == 3) == (arm == "loop" and level in ("records", "segments")), (level, arm, out["raw_stats"])
            tf.compare_paths(f"{case}: DFX_CHECKPOINT={level}, {arm}", ref, out)


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_caller_chosen_unequal_steps(case):
    st = tf.unequal_steps(TS, tf.SPI)
    p = PATH_CASES[case]()
    tf.check_premises(p, p.params(), tf.stage_times(st), TS)
    ref = tf.run_path(PATH_CASES[case], {}, TS, step_times=st)
    eq = _default(case)
    assert tf.rel(ref["fields"], eq["fields"]) > 1e-9                      # another grid, another answer
    for name, env in (("table", STAGE), ("inline", INLINE)):
        out = tf.run_path(PATH_CASES[case], env, TS, step_times=st)
        assert out["stats"]["tile_kernels"] != 3
        tf.compare_paths(f"{case}: unequal steps, stage launches ({name}) vs default", ref, out)


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_per_member_grids_in_a_batch_of_two(case):
    """Two members with the same parameters on time grids of their own in one call, each against the same member alone on its grid."""
    grids = np.stack([TS, np.linspace(0.07e-4, 2.83e-4, tf.N_OUT)])
    make2 = lambda: _with_batch(case, 2)        # noqa: E731
    p = PATH_CASES[case]()
    for row in grids:
        tf.check_premises(p, p.params(), tf.stage_times(tf.fixed_step_bounds(row, tf.SPI)), row, branches=False)
    both = tf.run_path(make2, {}, grids)
    for m, row in enumerate(grids):
        alone = tf.run_path(PATH_CASES[case], {}, row, as_member=m)
        tf.compare_paths(f"{case}: member {m} of a batch on its own grid vs alone", alone, tf.member_view(both, m))


def _with_batch(case, batch):
    if case == "Harmonic disp + Ramp force":
        return tf.harmonic_plus_ramp(None, batch=batch)
    fn, role = case.split()
    return tf.single(None, fn, role, batch=batch)


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_adaptive_loop_against_the_stage_launch_controller(case):
    """k_adaptive_fwd_loop (inline evaluation at the controller's trial times) with the dense reverse loop, and the stage-launch controller
    (DFX_PERSIST=0), each followed by vjp and the raw sweep on the kept steps and by jvp(adaptive=True).

    Each path is held to the oracle's replay of the steps it accepted itself (fields 1e-11, gradients and fields_dot RTOL_GRAD): that does
    not depend on what the other controller decided.  The two against each other is a comparison of two controllers: rounding moves their
    step sizes by ~1e-8, and a function with kinks amplifies that until an accept / reject decision differs (Table: 43 accepted steps in the
    loop, 44 on stage launches, in the CPU port and in the oracle's own odeint, boundaries apart by 1e-7 before the first kink and by 1e-5
    after the third; profiles/r12_time_functions.txt).  Such a difference is undecidable in the same sense as a stage time on a kink, so
    the pair is compared where both took the same decisions -- which a function without kinks must -- at the bars of
    test_adaptive_controller_in_the_loop_equals_the_stage_launch_controller (fields 1e-6, gradients 1e-4; tangents as gradients)."""
    ts = np.linspace(0, tf.HORIZON, 31)
    loop = tf.run_path(PATH_CASES[case], {}, ts, adaptive=True)
    stage = tf.run_path(PATH_CASES[case], STAGE, ts, adaptive=True)
    for out, persistent in ((loop, True), (stage, False)):
        assert out["stats"]["step_control"] == "adaptive-records" and out["jvp_stats"]["step_control"] == "adaptive-dense"
        # (the raw sweep: the dense reverse loop; the whole-tree sweep accumulates ligament gradients and stays on stage launches)
        assert (out["stats"]["tile_kernels"] == 3) == persistent and (out["raw_stats"]["tile_kernels"] == 3) == persistent, (out["stats"], out["raw_stats"])
        assert out["adjoint_stats"]["tile_kernels"] != 3
        tf.check_adaptive_path(f"{case}: adaptive, {'loop' if persistent else 'stage launches'} vs replay of its own steps", PATH_CASES[case], out, ts)
    same_decisions = loop["stats"]["steps"] == stage["stats"]["steps"] and loop["stats"]["rhs_evals"] == stage["stats"]["rhs_evals"]
    p = PATH_CASES[case]()
    kinked = any(t.kinks(p.params()[slot]) for t, slot in p.terms())
    print(f"time_functions: {case}: accepted steps loop {loop['stats']['steps']}, stage launches {stage['stats']['steps']}; fields loop vs stage launches "
          f"{tf.rel(loop['fields'], stage['fields']):.2e}")
    assert same_decisions or kinked, (loop["stats"], stage["stats"])
    if same_decisions:
        tf.compare_paths(f"{case}: adaptive loop vs stage-launch controller", stage, loop, tol_fields=1e-6, tol_grad=1e-4, tol_dot=1e-4)


@pytest.mark.parametrize("form", ["chunked", "spread"])
@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_jvp_multi_columns_equal_single_jvps(case, form):
    out = tf.run_path(PATH_CASES[case], {"DFX_TANGENT_MULTI_FORM": form}, TS, multi=(3, 5))
    for K in (3, 5):
        fd, cols, _ = out[f"multi{K}"]
        assert fd.shape == cols.shape == (K,) + out["fields"].shape[1:]
        worst = max(tf.rel(fd[k], cols[k]) for k in range(K))
        print(f"time_functions: {case}: jvp_multi K = {K} ({form}) vs single jvps {worst:.2e}")
        assert worst < 1e-12 and all(np.abs(cols[k]).max() > 0 for k in range(K))


@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_jacfwd_over_the_functions_own_parameters(case):
    p = PATH_CASES[case]()
    pm = p.params()
    cp = p.cp(pm)
    names = [k for d in pm for k in d]
    fields, jac = p.solver.jacfwd(p.y0, TS, cp, names, steps_per_interval=tf.SPI)
    assert tf.rel(fields, _default(case)["fields"][0]) < 1e-13
    for sl, d in enumerate(pm):
        for k in d:
            unit = ({k: 1.0} if sl == 0 else {}, {k: 1.0} if sl == 1 else {})
            _, col = p.solver.jvp(p.y0, TS, cp, None, tf.tangent_tree(p, unit), steps_per_interval=tf.SPI)
            e = tf.rel(jac[k], col)
            print(f"time_functions: {case}: jacfwd column {k} vs jvp {e:.2e}")
            assert e < 1e-12 and np.abs(col).max() > 0, (k, e)


def test_chip_filling_per_stage_builds_with_capped_ramp_and_delayed_pulse():
    """128 x 128 quads, one design, 12 steps: the per-stage builds of the stage kernels (build code 2; write-through stores forced, one
    design is half of what switches them on by itself) against the generic build, both on stage launches and reading the table."""
    ts = np.linspace(0, 1.5e-4, 3)
    make = lambda: tf.static_tuning(None, n=128)      # noqa: E731
    p = make()
    tf.check_premises(p, p.params(), tf.stage_times(tf.fixed_step_bounds(ts, tf.SPI)), ts, branches=False)
    env = {"DFX_PERSIST": "0", "DFX_WT": "1"}
    builds = tf.run_path(make, env, ts, jvp=False)
    generic = tf.run_path(make, dict(env, DFX_STAGE_BUILDS="0"), ts, jvp=False)
    assert builds["stats"]["steps"] == 12 and builds["stats"]["tile_kernels"] == 2 and generic["stats"]["tile_kernels"] == 0, (builds["stats"], generic["stats"])
    assert np.abs(builds["grads"]["0:0:compressive_strain"]) > 0 and np.abs(builds["grads"]["0:0:amplitude"]) > 0
    tf.compare_paths("128 x 128, CappedRamp + DelayedPulse: per-stage builds vs generic", generic, builds)
