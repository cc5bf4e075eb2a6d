"""Every time function of difflexmm_amd/loading.py on the CPU port of the engine (no GPU): the inputs and premises of
tests/test_gpu_time_functions.py -- the torch twins restate the library, the stage times of every grid keep clear of the functions' kinks and
visit all their branches -- and, for every entry point the CPU port has (fixed-grid and adaptive forward, the reverse sweep, the rhs and
rhs_vjp hooks; it has no forward mode), the same comparisons with the oracle that the HIP engine gets there.  eval_time_fn
(csrc/dfx_physics.h) is shared by both engines."""
import numpy as np
import pytest
import torch

from . import time_functions as tf
from .parity import RTOL_RHS

ROLES = [(fn, role) for fn in tf.VALUES for role in ("disp", "force")]
TS = np.linspace(0, tf.HORIZON, tf.N_OUT)


@pytest.mark.parametrize("fn", sorted(tf.VALUES) + ["DelayedPulse"])
def test_twin_restates_the_library_function(fn):
    """The torch twin and the library's own host evaluation (``TimeFunction.value`` / ``resolve``) agree at times on every branch."""
    vals = tf.VALUES[fn]["disp"] if fn in tf.VALUES else (3.0, 8000.0, 0.2137e-4, 0.004, 41.3)
    term = tf.Term(fn, vals, 1.0)
    lib, d = term.lib(), term.params()
    times = np.linspace(-0.2e-4, 3.3e-4, 57)
    assert {term.branch(float(t), d) for t in times} == term.spec["branches"]
    dt = {k: torch.tensor(v, dtype=torch.float64) for k, v in d.items()}
    mine = np.array([float(lib.value(float(t), lib.resolve(d))) for t in times])
    ref = np.array([float(term.value(float(t), dt)) for t in times])
    # (in units of the function's peak: 1 - tanh^2 in the tails of Sech2Tanh carries the rounding of tanh, not of the small difference)
    assert np.abs(ref).max() > 0 and np.abs(mine - ref).max() <= 1e-14 * np.abs(ref).max(), (fn, np.abs(mine - ref).max(), np.abs(ref).max())


def test_fixed_grids_keep_clear_of_kinks_and_visit_every_branch():
    """The premises of every fixed-grid comparison, from the stage times themselves: equal steps, the unequal caller-chosen steps and the
    per-member grids of the path tests."""
    grids = {"equal": tf.fixed_step_bounds(TS, tf.SPI), "unequal": tf.unequal_steps(TS, tf.SPI)}
    for name, bounds in grids.items():
        times = tf.stage_times(bounds)
        assert len(times) == 6 * 4 * tf.SPI
        for fn, role in ROLES:
            term = tf.Term(fn, tf.VALUES[fn][role], 1.0)
            p = type("P", (), {"terms": lambda self, t=term: [(t, 0)]})()
            tf.check_premises(p, (term.params(), {}), times, TS)
    # a kink ON a stage time is refused
    term = tf.Term("Ramp", (1.0, 1 / (TS[1] + 0.3 * (TS[1] / tf.SPI))), 1.0)
    p = type("P", (), {"terms": lambda self: [(term, 0)]})()
    with pytest.raises(AssertionError, match="kink"):
        tf.check_premises(p, (term.params(), {}), tf.stage_times(grids["equal"]), TS)


@pytest.mark.parametrize("fn,role", ROLES)
def test_every_function_in_both_roles_against_the_oracle(cpu_lib, fn, role):
    tf.check_fixed(tf.single(cpu_lib, fn, role), f"{fn}/{role}")


@pytest.mark.parametrize("fn,role", [("Table", "disp"), ("Sech2Tanh", "force")])
def test_kagome_lattice(cpu_lib, fn, role):
    tf.check_fixed(tf.single(cpu_lib, fn, role, lattice="kagome", n=3), f"kagome/{fn}/{role}")


@pytest.mark.parametrize("role", ["disp", "force"])
def test_pulse_that_ends_exactly_on_an_output_time(cpu_lib, role):
    tf.check_pulse_end_on_output(cpu_lib, role)


def test_two_slots_harmonic_drive_and_ramp_force(cpu_lib):
    tf.check_fixed(tf.harmonic_plus_ramp(cpu_lib), "Harmonic+Ramp")


def test_two_slots_capped_ramp_and_delayed_pulse(cpu_lib):
    """Both slots on the constraint side; the DelayedPulse chain reaches compressive_strain and compressive_strain_rate."""
    errs, out = tf.check_fixed(tf.static_tuning(cpu_lib), "CappedRamp+DelayedPulse")
    assert {"d/dcompressive_strain", "d/dcompressive_strain_rate", "d/damplitude", "d/dloading_rate", "d/dinput_delay"} <= {k[1] for k in errs}
    assert all(v != 0.0 for v in out["grads"][0].values())


def test_one_block_constrained_in_x_and_loaded_in_y(cpu_lib):
    tf.check_fixed(tf.two_roles_in_one_block(cpu_lib), "Pulse(x)+Sech2Tanh(y) on one block")


@pytest.mark.parametrize("fn,role", [("Pulse", "disp"), ("Ramp", "force")])
def test_batch_of_three_members_before_inside_and_after(cpu_lib, fn, role):
    p = tf.single(cpu_lib, fn, role, batch=3)
    members = tf.staggered_members(p, fn, TS[2])
    tf.check_fixed(p, f"{fn}/{role}/batch3", members=members, branches=False)


@pytest.mark.parametrize("fn,role", ROLES)
def test_zero_amplitude(cpu_lib, fn, role):
    tf.check_zero_amplitude(cpu_lib, fn, role)


@pytest.mark.parametrize("role", ["disp", "force"])
def test_zero_amplitude_member_in_a_batch(cpu_lib, role):
    tf.check_zero_member_in_batch(cpu_lib, "Sech2Tanh", role)


@pytest.mark.parametrize("role", ["disp", "force"])
@pytest.mark.parametrize("edge", ["two breakpoints", "past the end"])
def test_table_edges(cpu_lib, edge, role):
    tf.check_table_edge(cpu_lib, edge, role)


def test_constant_force_gradient_is_the_response_to_a_static_load(cpu_lib):
    tf.check_constant_force(cpu_lib)


@pytest.mark.parametrize("family,fn,role", [("smooth", "Sech2Tanh", "force"), ("kinked", "CappedRamp", "disp"), ("table", "Table", "disp")])
def test_adaptive_solve_against_the_replay_of_its_accepted_steps(cpu_lib, family, fn, role):
    tf.check_adaptive(tf.single(cpu_lib, fn, role), f"adaptive/{fn}/{role}")


@pytest.mark.parametrize("case", sorted(tf.RHS_CASES))
def test_rhs_hooks_inside_and_after_the_active_window(cpu_lib, case):
    make, times = tf.RHS_CASES[case]
    for t in times:
        tf.check_rhs(make(cpu_lib), f"rhs/{case}/{t:.3e}", t, RTOL_RHS)
