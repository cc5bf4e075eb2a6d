"""-m gpu: the persistent loops (k_adj_persist, k_adj_dense_loop; k_fwd_persist in the last test) with their lean launch context, its stepped addresses and its
per-stage coefficient rows (dfx_persist_api.h: PersistCtx, PersistAdjTab) against the reverse sweep on one launch per stage
(DFX_PERSIST=0).  In the reverse tests both sweeps read the SAME stage records -- one forward solve at the records level, then the sweep twice -- so the
objective is equal bit for bit and the gradients differ only by how the two kernel families fuse multiply-adds: 1e-11 of the largest
entry, the bar tests/test_gpu_persistent.py and test_gpu_persistent_wide.py hold them to; equal bit for bit in the build without
floating-point contraction (DFX_LIBRARY=variants/libdfx_nocontract.so).  The 64 x 64 x 10-member case follows
test_gpu_persistent_wide.py as it stands: two full solves, the forward on stage launches in both.

The cases are the places where a stepped address or a base moved on to the launch's first member can go wrong: output intervals of
different lengths in one solve (a segment per interval: the record pointer, the table row and the W parity start anew each launch),
more steps than a segment holds, launches that do not start at member 0 and a narrower last launch, members on time grids of their
own, stiffness and damping images that differ per ligament / block, the void-angle accumulator (contact engaged), the time functions'
parameter gradients of the driven block, the angular-momentum objective, packed 3-node blocks, and the dense reverse of an adaptive
solve whose members finish in different segments (a member's sweep starts in an earlier launch; of its last step only stage 0 runs)."""
import os

import numpy as np
import pytest

from difflexmm_amd import objective as O

from .common import Case, relerr
from .param_shapes import ShapeCase

pytestmark = pytest.mark.gpu

EXACT = "nocontract" in os.environ.get("DFX_LIBRARY", "")
FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
RAW = ("centroid_node_vectors", "void_angle0", "inertia", "damping", "fn_params")      # what the persistent reverse serves
TOL = 1e-11
KNOBS = ("DFX_PERSIST", "DFX_PERSIST_ADJ_CHUNKS", "DFX_PERSIST_CHUNKS", "DFX_PERSIST_MAX_WG", "DFX_CHECKPOINT", "DFX_STREAMS")


@pytest.fixture(autouse=True)
def _no_knobs_from_outside(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _targets(c):
    mid = c.geo.n_blocks // 2
    return np.array([mid + 1, mid + 2], dtype=np.int32)


def _kinetic(c):
    return lambda: c.solver.engine.kinetic_value_and_grad(_targets(c), which=RAW)


def _two_sweeps(grad, env=None):
    """The reverse sweep of the trajectory the solver holds, on stage launches and on the loop: (objective, gradients, stats) of each."""
    out = {}
    for arm, e in (("stage", {"DFX_PERSIST": "0"}), ("loop", {})):
        obj, g, st = _with_env(dict(env or {}, **e), grad)
        out[arm] = (np.array(np.atleast_1d(obj), dtype=float), {k: np.array(v) for k, v in g.items()}, dict(st))
    return out["stage"], out["loop"]


def _check(tag, ref, out, nonzero=RAW, exact=EXACT):
    assert out[2]["tile_kernels"] == 3 and ref[2]["tile_kernels"] != 3, (tag, ref[2], out[2])      # the loop really ran, and only there
    assert np.array_equal(out[0], ref[0]) and (ref[0] != 0).all(), tag
    assert set(out[1]) == set(ref[1])
    errs = {k: relerr(out[1][k], ref[1][k]) for k in ref[1]}
    print(f"[lean] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in ref[1]:
        assert np.array_equal(out[1][k], ref[1][k]) if exact else errs[k] < TOL, (tag, k, errs[k])
    for k in nonzero:
        assert np.abs(ref[1][k]).max() > 0, (tag, k)


def _solve(c, ts, cps, spi):
    return _with_env({"DFX_CHECKPOINT": "records"},
                     lambda: c.solver(np.zeros((2, c.geo.n_blocks, 3)), ts, cps, keep_trajectory=True, steps_per_interval=spi))


def _members(c, n):
    cps = [c.cp._replace(constraint_params=dict(FAST, amplitude=7.5 * (1 + 0.05 * m))) for m in range(n)]
    return cps if n > 1 else cps[0]


@pytest.mark.parametrize("lattice,n,batch", [("quads", 8, 1), ("quads", 16, 3), ("kagome", 4, 2)])
def test_intervals_of_1_2_and_7_steps(hip_lib, lattice, n, batch):
    """Three output intervals of 1, 2 and 7 steps: three launches per sweep of 6, 12 and 42 stages, the shortest shorter than the ring."""
    c = Case(lattice, n, True, True, seed=31, cutoff_deg=42.0 if lattice == "quads" else 125.0, batch=batch)
    _solve(c, np.array([0.0, 0.2e-4, 0.6e-4, 2.0e-4]), _members(c, batch), [1, 2, 7])
    assert c.solver.stats["checkpoint_records"] == 1
    ref, out = _two_sweeps(_kinetic(c))
    assert out[2]["checkpoint_records"] == 1
    _check(f"{lattice} {n} x {batch}, intervals of 1, 2, 7 steps", ref, out, nonzero=RAW if lattice == "quads" else tuple(k for k in RAW if k != "void_angle0"))


def test_more_steps_than_a_segment(hip_lib):
    """300 steps in one interval: segments of 256 and 44 steps -- the second launch of the sweep starts from what the first left in
    LAM, W and the accumulators."""
    c = Case("quads", 8, True, True, seed=4, cutoff_deg=42.0, batch=2)
    _solve(c, np.array([0.0, 3e-4, 4e-4]), _members(c, 2), [300, 10])
    ref, out = _two_sweeps(_kinetic(c))
    _check("quads 8 x 2, 300 + 10 steps", ref, out)


def test_launches_that_do_not_start_at_member_zero(hip_lib):
    """64 x 64 x 10 members, one workgroup per compute unit: launches of at most four members, the last narrower, every launch but the
    first with m0 > 0 (tests/test_gpu_persistent_wide.py's comparison: two solves, the forward on stage launches in both)."""
    B = 10
    env = {"DFX_PERSIST_MAX_WG": "1"}
    c = Case("quads", 64, True, True, seed=7, cutoff_deg=42.0, batch=B)
    cps = _members(c, B)
    ts = np.linspace(0.0, 1.2e-4, 3)

    def run():
        fields = np.array(c.solver(np.zeros((2, c.geo.n_blocks, 3)), ts, cps, keep_trajectory=True, steps_per_interval=[5, 7]))
        st = dict(c.solver.stats)
        obj, g, sa = c.solver.engine.kinetic_value_and_grad(_targets(c), which=RAW)
        return fields, st, (np.array(np.atleast_1d(obj), dtype=float), {k: np.array(v) for k, v in g.items()}, dict(sa))
    ref = _with_env(dict(env, DFX_PERSIST="0"), run)
    out = _with_env(env, run)
    assert ref[1]["tile_kernels"] != 3 and out[1]["tile_kernels"] != 3 and out[2][2]["checkpoint_records"] == 1
    assert out[2][2]["launches"] >= 2 * 2 * 3                # (per segment at least three launches, each with its ring poison)
    assert np.array_equal(out[0], ref[0])
    _check("quads 64 x 10, launches of <= 4 members", ref[2], out[2], exact=False)
    if EXACT:
        for k in ref[2][1]:
            assert np.array_equal(out[2][1][k], ref[2][1][k]), k


def test_members_on_time_grids_of_their_own(hip_lib):
    """Two members, the second on a shifted and stretched grid: every member reads the step sizes of its own row."""
    c = Case("quads", 8, True, True, seed=9, cutoff_deg=42.0, batch=2)
    grids = np.stack([np.linspace(0.0, 2.4e-4, 4), np.linspace(0.07e-4, 2.83e-4, 4)])
    _solve(c, grids, _members(c, 2), [3, 2, 5])
    ref, out = _two_sweeps(_kinetic(c))
    _check("quads 8 x 2, per-member grids", ref, out)
    assert relerr(ref[1]["inertia"][1], ref[1]["inertia"][0]) > 1e-3        # the grids matter


@pytest.mark.parametrize("shape", ["k_per_bond", "damping_per_block"])
def test_parameter_images_that_differ_inside_a_member(hip_lib, shape):
    """Stiffnesses per ligament / damping per block (some blocks undamped), different in the two members: the loop reads the images
    of ITS member (k_uniform / damping_uniform off)."""
    sc = ShapeCase(shape, "quads", 8)
    c = sc.c
    _with_env({"DFX_CHECKPOINT": "records"}, lambda: c.solver(np.zeros((2, c.geo.n_blocks, 3)), np.linspace(0.0, 2e-4, 3), sc.engine_params(),
                                                              keep_trajectory=True, steps_per_interval=[4, 9]))
    ref, out = _two_sweeps(_kinetic(c))
    _check(f"quads 8 x {len(sc.cps)}, {shape}", ref, out)


@pytest.mark.parametrize("lattice,n", [("quads", 16), ("kagome", 4)])
def test_angular_momentum_objective(hip_lib, lattice, n):
    """The weighted angular-momentum objective on the resident history (per-member weights of both signs, a non-integer time weight):
    its cotangent enters the same sweep; damping and time-function gradients asked for."""
    B = 2
    c = Case(lattice, n, True, True, seed=41, cutoff_deg=42.0 if lattice == "quads" else 125.0, batch=B)
    nb = c.geo.n_blocks
    _solve(c, np.linspace(0.0, 3e-4, 4), _members(c, B), 6)
    mid = nb // 2
    targets = [np.array([mid, mid + 1]), np.array([mid + 1, mid + 2, mid + 3])]
    w = O.block_weights_from_targets(nb, targets, np.array([[1.0, -0.5], [0.25, 2.0]]))
    tau = np.array([0.0, 1.0, 0.37, 2.0])
    lever0 = np.broadcast_to(c.cen - c.cen[targets[0]].mean(0), (B,) + c.cen.shape).copy()
    which = RAW + ("block_centroids",)
    eng = c.solver.engine
    ref, out = _two_sweeps(lambda: eng.objective_value_and_grad(O.ANGULAR_MOMENTUM, w, tau, lever0, which=which))
    _check(f"{lattice} {n} x {B}, angular momentum", ref, out, nonzero=tuple(k for k in RAW if lattice == "quads" or k != "void_angle0"))


@pytest.mark.parametrize("lattice,n", [("quads", 8), ("kagome", 4)])
def test_dense_reverse_of_members_that_finish_in_different_segments(hip_lib, lattice, n):
    """The adaptive solve that keeps its accepted steps, three members with different drives: the first takes a segment of 256 steps
    more than the last, so in the sweep's first launch the others' waves have nothing to do, and every member's sweep opens with the
    lone stage 0 of its step N_m."""
    B = 3
    c = Case(lattice, n, True, True, seed=17, cutoff_deg=42.0 if lattice == "quads" else 125.0, batch=B)
    cps = [c.cp._replace(constraint_params=dict(FAST, amplitude=7.5 / (1 + 2.0 * m))) for m in range(B)]
    s = c.solver
    s.rtol = s.atol = 1e-9
    s(np.zeros((2, c.geo.n_blocks, 3)), np.linspace(0.0, 6e-4, 13), cps, keep_trajectory=True)
    assert s.stats["step_control"] == "adaptive-records", s.stats
    steps = s.engine.adaptive_step_counts().sum(axis=1)
    print(f"[lean] {lattice} {n}: accepted steps {steps.tolist()}")
    assert len({(int(k) + 255) // 256 for k in steps}) > 1, steps
    ref, out = _two_sweeps(_kinetic(c))
    # (3-node blocks: the loop packs five triangles per 16 lanes, the DENSE stage launches keep the quad mapping -- the block sums add
    # in another order, so not even the contraction-free build is bit-identical there: tests/test_gpu_persistent.py)
    _check(f"{lattice} {n} x {B}, dense reverse", ref, out, nonzero=tuple(k for k in RAW if lattice == "quads" or k != "void_angle0"),
           exact=EXACT and lattice == "quads")


@pytest.mark.parametrize("level", ["records", "stages", "state"])
def test_forward_loop_on_member_grids_with_a_driven_block(hip_lib, level):
    """k_fwd_persist against the forward stage launches, two full solves: two members on time grids of their own (the driven block reads
    the NEXT row of its member's time-function table, stepped with the stage), intervals of 3, 2 and 5 steps, at the level that stores
    every stage record (the stepped record pointer), the one that stores stage accelerations and the one that stores step states.
    Fields to 1e-13 of the largest entry (the two kernel families fuse multiply-adds differently; equal in the contraction-free build),
    and the gradients that the reverse sweep makes of each checkpoint to 1e-11."""
    c = Case("quads", 8, True, True, seed=9, cutoff_deg=42.0, batch=2)
    grids = np.stack([np.linspace(0.0, 2.4e-4, 4), np.linspace(0.07e-4, 2.83e-4, 4)])
    cps = _members(c, 2)

    def run():
        fields = np.array(c.solver(np.zeros((2, c.geo.n_blocks, 3)), grids, cps, keep_trajectory=True, steps_per_interval=[3, 2, 5]))
        st = dict(c.solver.stats)
        obj, g, _ = c.solver.engine.kinetic_value_and_grad(_targets(c), which=RAW)
        return fields, st, np.array(np.atleast_1d(obj), dtype=float), {k: np.array(v) for k, v in g.items()}
    ref = _with_env({"DFX_PERSIST": "0", "DFX_CHECKPOINT": level}, run)
    out = _with_env({"DFX_PERSIST": "1", "DFX_CHECKPOINT": level}, run)
    assert ref[1]["tile_kernels"] != 3 and out[1]["tile_kernels"] == 3, (level, ref[1], out[1])
    e_f = relerr(out[0], ref[0])
    errs = {k: relerr(out[3][k], ref[3][k]) for k in ref[3]}
    print(f"[lean] forward loop, {level}: fields {e_f:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    driven = int(c.con[0, 0])
    assert np.abs(ref[0][:, -1, 0, driven, 0]).min() > 0                      # the drive really moved the driven block, in both members
    assert relerr(ref[0][1], ref[0][0]) > 1e-3                                # ... and the grids matter
    assert np.array_equal(out[0], ref[0]) if EXACT else e_f < 1e-13, (level, e_f)
    for k in ref[3]:
        assert np.array_equal(out[3][k], ref[3][k]) if EXACT else errs[k] < TOL, (level, k, errs[k])
