"""Host side of the differentiable drive waveform (no GPU): loading.Table with named values, its hat weights, the (name, j) leaves of
dynamics.unit_tangent / with_leaf, the binding of the new entries of include/dfx.h, the refusal on a library without them, and
problems.DriveWaveformDesign on a stub solver.  The device side: tests/test_gpu_waveform.py."""
import os
import re

import numpy as np
import pytest

from difflexmm_amd import _binding as b
from difflexmm_amd import loading as ld
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P
from difflexmm_amd.dynamics import setup_dynamic_solver, unit_tangent, with_leaf

from .common import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = np.array([0.0, 0.21, 0.46, 0.71, 0.91, 1.10, 1.12, 1.14, 1.51, 1.91, 2.31]) * 1e-4
NEW = ["dfx_fn_table_values", "dfx_fn_table_grads", "dfx_fn_table_grad", "dfx_drive_cotangent", "dfx_fn_table_tangents"]


def test_table_with_named_values_resolves_and_validates():
    Y = np.random.default_rng(0).normal(size=len(T))
    tab = ld.Table(T, "wave", vector=np.array([1.0, 0.0, -2.0]), amplitude="amp", delay=2e-5)
    assert tab.values_name == "wave" and tab.values is None and np.array_equal(tab.table[1], np.zeros(len(T)))
    params = dict(amp=2.5, wave=Y)
    assert np.array_equal(tab.resolve(params), [2.5, 2e-5, 0.0, 0.0, 0.0])
    assert tab.resolve_values(params) is not None and np.array_equal(tab.resolve_values(params), Y)
    t = 1.3e-4
    want = 2.5 * np.interp(t - 2e-5, T, Y) * np.array([1.0, 0.0, -2.0])
    assert np.allclose(tab(t, **params), want, rtol=1e-15, atol=0)
    assert np.allclose(tab.bind(params).value(t, tab.resolve(params)), 2.5 * np.interp(t - 2e-5, T, Y), rtol=1e-15, atol=0)
    with pytest.raises(KeyError, match="wave"):
        tab.resolve_values(dict(amp=2.5))
    with pytest.raises(ValueError, match="shape"):
        tab.resolve_values(dict(amp=2.5, wave=Y[:-1]))
    with pytest.raises(ValueError, match="not finite"):
        tab.resolve_values(dict(amp=2.5, wave=np.where(np.arange(len(T)) == 3, np.nan, Y)))
    with pytest.raises(ValueError, match="bind"):
        tab.value(t, tab.resolve(params))
    # an array keeps the behaviour it had: static data, no name
    old = ld.Table(T, Y, amplitude="amp", delay=2e-5)
    assert old.values_name is None and old.bind(params) is old and np.array_equal(old.table[1], Y)
    assert old(t, amp=2.5) == 2.5 * np.interp(t - 2e-5, T, Y)
    with pytest.raises(ValueError, match="strictly increasing"):
        ld.Table(T[::-1], "wave")


def test_hat_weights_of_value_and_rate_match_finite_differences_of_interp():
    rng = np.random.default_rng(1)
    Y = rng.normal(size=len(T))
    tab = ld.Table(T, "wave")
    taus = np.concatenate([rng.uniform(-0.5e-4, 3e-4, 40), [T[0], T[4], T[-1], T[0] - 1e-6, T[-1] + 1e-6]])
    for tau in taus:
        w, r = tab.hat_weights(tau), tab.rate_weights(tau)
        assert abs(w.sum() - 1.0) < 1e-15 and abs(r.sum()) < 1e-9
        assert abs(w @ Y - np.interp(tau, T, Y)) < 1e-14
        near = np.abs(tau - T).min() < 1e-9
        for j in range(len(T)):
            e = np.zeros(len(T))
            e[j] = 1.0
            fd = (np.interp(tau, T, Y + e) - np.interp(tau, T, Y - e)) / 2          # (linear in Y: exact)
            assert abs(w[j] - fd) < 1e-14, (tau, j)
            if not near:         # the rate jumps at a breakpoint
                h = 1e-9
                fr = ((np.interp(tau + h, T, Y + e) - np.interp(tau - h, T, Y + e)) - (np.interp(tau + h, T, Y - e) - np.interp(tau - h, T, Y - e))) / (4 * h)
                assert abs(r[j] - fr) < 1e-6 * max(1.0, abs(r).max()), (tau, j, r[j], fr)
    # a breakpoint belongs to the piece that starts there; the ends are held
    assert np.array_equal(tab.hat_weights(T[4]), np.eye(len(T))[4]) and tab.rate_weights(T[4])[5] > 0
    assert np.array_equal(tab.hat_weights(T[0] - 1.0), np.eye(len(T))[0]) and not tab.rate_weights(T[0]).any()
    assert np.array_equal(tab.hat_weights(T[-1]), np.eye(len(T))[-1]) and not tab.rate_weights(T[-1]).any()


def test_unit_tangent_and_with_leaf_address_one_sample():
    from difflexmm_amd.utils import ControlParams, GeometricalParams, MechanicalParams
    Y = np.arange(5.0)
    cp = ControlParams(GeometricalParams(None, None), MechanicalParams(None, 1.0), constraint_params=dict(amplitude=2.0, wave=Y),
                       loading_params=dict(push=np.ones(3), both=np.zeros(2)))
    cp = cp._replace(constraint_params=dict(cp.constraint_params, both=np.zeros(2)))
    t = unit_tangent(cp, ("wave", 3))
    assert np.array_equal(t.constraint_params["wave"], [0, 0, 0, 1, 0]) and t.loading_params in (None, {}) and t.geometrical_params.centroid_node_vectors is None
    assert np.array_equal(unit_tangent(cp, ("push", 0)).loading_params["push"], [1, 0, 0])
    cp2 = with_leaf(cp, ("wave", 1), 7.5)
    assert np.array_equal(cp2.constraint_params["wave"], [0, 7.5, 2, 3, 4]) and np.array_equal(Y, np.arange(5.0))          # a copy
    assert cp2.constraint_params["amplitude"] == 2.0 and cp2.loading_params is cp.loading_params
    assert unit_tangent(cp, "amplitude").constraint_params == {"amplitude": 1.0}          # scalar names as before
    for bad, msg in ((("wave", 5), "out of range"), (("wave", -1), "out of range"), (("wave", 1.5), "out of range"), (("nope", 0), "not a key"),
                     (("both", 0), "both"), (("amplitude", 0), "1-D"), (("wave",), "addressed"), ((3, 1), "addressed")):
        with pytest.raises(ValueError, match=msg):
            unit_tangent(cp, bad)
        with pytest.raises(ValueError, match=msg):
            with_leaf(cp, bad, 1.0)
    with pytest.raises(ValueError, match="not a scalar leaf"):
        unit_tangent(cp, "wave")


def test_new_entries_are_declared_bound_and_exported(hip_lib):
    text = open(os.path.join(ROOT, "include", "dfx.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in b.COMM_EXPORTS and name in b.EXPORTS and hasattr(hip_lib, name), name
        assert getattr(hip_lib, name).argtypes, name


def test_named_values_need_the_hip_engine(cpu_lib):
    c = Case("quads", 3, True, False, seed=1, lib=cpu_lib)
    assert not any(hasattr(cpu_lib, name) for name in NEW)
    drive = ld.Table(T, "wave", vector=c.vec)
    with pytest.raises(NotImplementedError, match="dfx_fn_table_grads"):
        setup_dynamic_solver(c.geo, c.energy, constrained_block_DOF_pairs=c.con, constrained_DOFs_fn=drive, damped_blocks=c.damped, _lib=cpu_lib)
    # an array table is served there as before
    s = setup_dynamic_solver(c.geo, c.energy, constrained_block_DOF_pairs=c.con, constrained_DOFs_fn=ld.Table(T, np.ones(len(T)), vector=c.vec),
                             damped_blocks=c.damped, _lib=cpu_lib)
    assert s._table_leaves == []
    with pytest.raises(NotImplementedError, match="dfx_drive_cotangent"):
        s.drive_cotangent()


class _StubSolver:
    """value = 1/2 |y - goal|^2 through the solver interface DriveWaveformDesign uses."""
    batch = 1

    def __init__(self, goal, slot=1):
        self.goal = np.asarray(goal, dtype=float)
        self._table_leaves = [(slot, ld.Table(np.arange(len(self.goal), dtype=float), "wave"), "loading_params")]
        self.slot, self.calls, self.y = slot, [], None

    def __call__(self, state0, timepoints, control_params, keep_trajectory=False, want_fields=True, **grid):
        assert keep_trajectory and not want_fields
        self.y = np.array(control_params.loading_params["wave"])
        self.calls.append((self.y, grid))

    def signal_misfit_value_and_raw(self, spec, which=()):
        r = self.y - self.goal
        return np.array([0.5 * float(r @ r)]), {"fn_params": np.zeros((1, 2, 5)), "fn_table_values": {self.slot: r[None].copy()}}


def test_design_loop_holds_the_fixed_samples_and_respects_the_bounds():
    from difflexmm_amd.utils import ControlParams, GeometricalParams, MechanicalParams
    goal = np.array([3.0, -2.0, 0.4, 5.0, -0.7, 1.0])
    y0 = np.array([0.5, 0.0, 0.0, 0.0, 0.0, -0.25])
    cp = ControlParams(GeometricalParams(None, None), MechanicalParams(None, 1.0), loading_params=dict(wave=y0, amplitude=1.0))
    spec = O.SignalSpec.fields_of([(0, 0)], targets=np.zeros((2, 1)))
    stub = _StubSolver(goal)
    d = P.DriveWaveformDesign(stub, None, np.array([0.0, 1.0]), cp, "wave", spec, steps_per_interval=3)
    assert d.fixed == [0, 5] and list(d.free) == [1, 2, 3, 4] and d.slot == 1 and d.field == "loading_params"
    v, g = d.value_and_grad(y0)
    assert v == 0.5 * np.sum((y0 - goal) ** 2) and np.array_equal(g, y0 - goal) and stub.calls[-1][1] == dict(steps_per_interval=3)
    best = d.run_mma(y0, 30, lower_bound=-1.5, upper_bound=1.5)
    assert best[0] == y0[0] and best[-1] == y0[-1]                                   # held, although the goal pulls at them
    assert all(np.array_equal(y[[0, 5]], y0[[0, 5]]) for y in d.design_values)
    assert all(np.all(np.abs(y[1:5]) <= 1.5) for y in d.design_values)
    assert np.allclose(best[1:5], np.clip(goal[1:5], -1.5, 1.5), atol=1e-3)
    assert d.objective_values[-1] < d.objective_values[0] and len(d.objective_values) <= 30
    # maximising turns the sign; other samples held
    d2 = P.DriveWaveformDesign(_StubSolver(goal), None, np.array([0.0, 1.0]), cp, "wave", spec, fixed=(2,), maximize=True)
    far = d2.run_mma(y0, 10, lower_bound=-1.0, upper_bound=1.0)
    assert far[2] == y0[2] and d2.objective_values[-1] > d2.objective_values[0]
    with pytest.raises(ValueError, match="no loading.Table"):
        P.DriveWaveformDesign(stub, None, np.array([0.0, 1.0]), cp, "other", spec)
    with pytest.raises(TypeError, match="device objective specs"):
        P.DriveWaveformDesign(stub, None, np.array([0.0, 1.0]), cp, "wave", object())
    with pytest.raises(ValueError, match="no targets"):
        P.DriveWaveformDesign(stub, None, np.array([0.0, 1.0]), cp, "wave", O.SignalSpec.fields_of([(0, 0)]))
