"""Forward mode through the adaptive solve, host side (no GPU): the routine that places the outputs inside the frozen accepted steps
(``dfx_dense_output_map``, pure host code of the HIP library) against a brute-force search, on step times of a CPU-port adaptive solve,
and the interface's refusals.  The kernel side is tests/test_gpu_tangent_adaptive.py."""
import os
import re

import numpy as np
import pytest

from difflexmm_amd import _binding as b

from .common import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)


def brute_force(step_times, n_steps, ts):
    """The controller's rule (k_control) and the oracle replay's: output k belongs to the FIRST step with ts[k] <= t_{n+1};
    theta = (ts[k] - t_n) / (t_{n+1} - t_n), those two operations and no others."""
    B, stride = step_times.shape
    out_ptr = np.zeros((B, stride), dtype=np.int32)
    theta = np.zeros((B, len(ts)))
    for m in range(B):
        t, N = step_times[m], int(n_steps[m])
        step_of = np.full(len(ts), -1)
        for k in range(1, len(ts)):
            for n in range(N):
                if ts[k] <= t[n + 1]:
                    step_of[k] = n
                    break
            assert step_of[k] >= 0
            n = step_of[k]
            theta[m, k] = (ts[k] - t[n]) / (t[n + 1] - t[n])
        for n in range(stride):
            out_ptr[m, n] = 1 + np.count_nonzero(step_of[1:] < min(n, N))
    return out_ptr, theta


def _padded(rows, t0):
    return b.padded_step_times([np.asarray(r, dtype=float) for r in rows], t0)


def test_map_matches_brute_force_on_random_steps(hip_lib):
    rng = np.random.default_rng(0)
    ts = np.sort(rng.uniform(0.0, 1.0, 40))
    ts[0] = 0.0
    rows = []
    for N in (5, 23, 90, 1):                    # different step counts in one padded array; a single step over everything
        inner = np.sort(rng.uniform(0.0, 1.0, N - 1))
        rows.append(np.concatenate([inner, [1.0 + rng.uniform(0.0, 0.2)]]))
    # output times ON step boundaries belong to the step that ends there
    rows[1][3], rows[1][7] = ts[5], ts[20]
    rows[1].sort()
    st, ns = _padded(rows, ts[0])
    assert st.shape == (4, 91) and list(ns) == [5, 23, 90, 1]
    op, th = b.dense_output_map(st, ns, ts, lib=hip_lib)
    op_ref, th_ref = brute_force(st, ns, ts)
    assert np.array_equal(op, op_ref)
    assert np.array_equal(th, th_ref)           # the same bits
    k5 = int(np.searchsorted(st[1, :24], ts[5]))
    assert st[1, k5] == ts[5] and op[1, k5 - 1] <= 5 < op[1, k5] and th[1, 5] == 1.0
    assert np.all(op[:, 0] == 1) and all(op[m, ns[m]] == len(ts) for m in range(4))
    assert np.all((th[:, 1:] > 0.0) & (th[:, 1:] <= 1.0)) and np.all(th[:, 0] == 0.0)


def test_last_step_ending_exactly_at_the_last_timepoint_and_a_single_timepoint(hip_lib):
    ts = np.linspace(0.0, 1e-3, 11)
    st, ns = _padded([[4e-4, 1e-3], [2.5e-4, 5e-4, 7.5e-4, ts[-1]]], ts[0])
    op, th = b.dense_output_map(st, ns, ts, lib=hip_lib)
    op_ref, th_ref = brute_force(st, ns, ts)
    assert np.array_equal(op, op_ref) and np.array_equal(th, th_ref)
    assert th[0, -1] == 1.0 and th[1, -1] == 1.0 and op[0, 2] == 11 and op[1, 4] == 11
    # one timepoint: no step at all, the only output is the initial state
    st1, ns1 = _padded([[], []], 0.3)
    assert st1.shape == (2, 1) and list(ns1) == [0, 0]
    op, th = b.dense_output_map(st1, ns1, np.array([0.3]), lib=hip_lib)
    assert np.array_equal(op, [[1], [1]]) and np.array_equal(th, [[0.0], [0.0]])


def test_map_refuses_what_is_not_a_solve(hip_lib):
    ts = np.linspace(0.0, 1.0, 5)
    for rows, t0, msg in (([[0.5, 0.5, 1.1]], 0.0, "strictly increasing"), ([[0.5, 1.1]], 0.1, "t_0"), ([[0.5, 0.9]], 0.0, "last step")):
        st, ns = _padded(rows, t0)
        with pytest.raises(ValueError, match=msg):
            b.dense_output_map(st, ns, ts, lib=hip_lib)
    st, ns = _padded([[0.5, 1.1]], 0.0)
    with pytest.raises(ValueError, match="stride"):
        b.dense_output_map(st, np.array([3]), ts, lib=hip_lib)


def _batch3(lattice, lib):
    c = Case(lattice, 4, True, True, seed=9, lib=lib, cutoff_deg=125.0 if lattice == "kagome" else 42.0, batch=3)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    bp = c.cp.mechanical_params.bond_params
    cps = [c.cp._replace(mechanical_params=c.cp.mechanical_params._replace(
        bond_params=bp._replace(k_stretch=bp.k_stretch * f, k_shear=bp.k_shear * f, k_rot=bp.k_rot * f))) for f in (1.0, 2.5, 0.4)]
    ts = np.linspace(0, 3e-4, 61)
    c.solver.rtol = c.solver.atol = 1e-5
    return c, cps, ts, c.random_state(0.05, 0.02, 5.0)


@pytest.mark.parametrize("lattice,steps,most,empty", [("quads", (38, 54, 33), (3, 2, 4), (4, 7, 5)),
                                                      ("kagome", (51, 74, 39), (2, 2, 3), (4, 16, 3))])
def test_map_on_the_steps_of_an_adaptive_solve(lattice, steps, most, empty, cpu_lib, hip_lib):
    """Step times of the CPU port's adaptive solve of the three-member case of tests/test_gpu_tangent_adaptive.py: members with different
    step counts, steps with no, one and several outputs, every last step ending beyond the last output time."""
    c, cps, ts, y0 = _batch3(lattice, cpu_lib)
    c.solver(y0, ts, cps, keep_trajectory=True)
    assert c.solver.stats["step_control"] == "adaptive-records"
    st, ns = b.padded_step_times([c.solver.engine.adaptive_step_times(m) for m in range(3)], ts[0])
    op, th = b.dense_output_map(st, ns, ts, lib=hip_lib)
    op_ref, th_ref = brute_force(st, ns, ts)
    assert np.array_equal(op, op_ref) and np.array_equal(th, th_ref)
    per_step = [np.diff(op[m, :ns[m] + 1]) for m in range(3)]
    assert tuple(int(n) for n in ns) == steps
    assert tuple(int(p.max()) for p in per_step) == most
    assert tuple(int((p == 0).sum()) for p in per_step) == empty
    assert all((p == 1).any() for p in per_step)
    assert all(st[m, ns[m]] > ts[-1] for m in range(3))


def test_adaptive_jvp_on_the_cpu_port_and_with_a_grid(cpu_lib):
    c = Case("quads", 4, True, True, seed=3, lib=cpu_lib, cutoff_deg=42.0)
    ts = np.linspace(0.0, 1e-4, 3)
    y0 = np.zeros((2, 16, 3))
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent"):
        c.solver.jvp(y0, ts, c.cp, None, c.cp, adaptive=True)
    # a grid of any kind is refused before any library call (the engine is not even looked at)
    engine, c.solver.engine = c.solver.engine, None
    try:
        for kw in (dict(steps_per_interval=2), dict(steps_per_interval=2, step_times=np.linspace(0.0, 1e-4, 5))):
            with pytest.raises(ValueError, match="adaptive=True"):
                c.solver.jvp(y0, ts, c.cp, None, c.cp, adaptive=True, **kw)
        with pytest.raises(ValueError, match="per-member timepoints"):
            c.solver.jvp(y0, np.stack([ts]), c.cp, None, c.cp, adaptive=True)
        c.solver.grid_refine = 2
        with pytest.raises(ValueError, match="grid_refine"):
            c.solver.jvp(y0, ts, c.cp, None, c.cp, adaptive=True)
        c.solver.grid_refine = 1
        c.solver.steps_per_interval = 4
        with pytest.raises(ValueError, match="default grid"):
            c.solver.jvp(y0, ts, c.cp, None, c.cp, adaptive=True)
    finally:
        c.solver.engine, c.solver.steps_per_interval, c.solver.grid_refine = engine, None, 1


def test_header_declares_the_entry_and_the_binding_takes_a_library_without_it(cpu_lib, hip_lib):
    text = open(os.path.join(ROOT, "include", "dfx.h")).read()
    for name in ("dfx_forward_tangent_dense", "dfx_dense_output_map"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in b.COMM_EXPORTS and hasattr(hip_lib, name)
        assert not hasattr(cpu_lib, name)                   # (declare() accepted the CPU port: the cpu_lib fixture went through it)
    import ctypes
    raw = b.declare(ctypes.CDLL(os.path.join(ROOT, "oracle", "cpu", "libdfx_cpu.so")))
    assert not hasattr(raw, "dfx_forward_tangent_dense")
    assert hip_lib.dfx_forward_tangent_dense.argtypes is not None and len(hip_lib.dfx_forward_tangent_dense.argtypes) == 12
