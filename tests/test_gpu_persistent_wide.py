"""-m gpu: the persistent reverse sweep (k_adj_persist) of an ensemble wider than one launch holds -- the records level cut into balanced
launches per segment, on one member group or several (engine_launch.hip: persist_plan_adj, enqueue_interleaved) -- against the reverse
sweep on one launch per stage (DFX_PERSIST=0).  DFX_PERSIST_MAX_WG=1 lets a 64 x 64 lattice stand in for the full-size one: one
workgroup per compute unit, so a launch holds a few members only and ten members take three or four launches, the last ones narrower.
The forward pass stays on stage launches in both arms, so fields and objectives are equal bit for bit; the gradients agree to rounding
(the persistent and the stage kernels fuse multiply-adds differently: tests/test_gpu_persistent.py)."""
import os

import numpy as np
import pytest

from .common import Case, relerr

pytestmark = pytest.mark.gpu

FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
B = 10
NARROW = {"DFX_PERSIST_MAX_WG": "1"}


@pytest.fixture(autouse=True)
def _persistent_loop_not_switched_off(monkeypatch):
    monkeypatch.delenv("DFX_PERSIST", raising=False)
    monkeypatch.delenv("DFX_PERSIST_ADJ_CHUNKS", raising=False)
    monkeypatch.delenv("DFX_PERSIST_CHUNKS", raising=False)
    monkeypatch.delenv("DFX_CHECKPOINT", raising=False)


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _CASES.clear()


def _case(streams):
    """Member groups are fixed when the engine is created: one Case per DFX_STREAMS value."""
    if streams not in _CASES:
        old = os.environ.get("DFX_STREAMS")
        os.environ["DFX_STREAMS"] = streams
        try:
            c = Case("quads", 64, True, True, seed=7, cutoff_deg=42.0, batch=B)
        finally:
            os.environ.pop("DFX_STREAMS") if old is None else os.environ.__setitem__("DFX_STREAMS", old)
        mid = c.geo.n_blocks // 2
        c.target = np.array([mid + 1, mid + 2], dtype=np.int32)
        c.cps = [c.cp._replace(constraint_params=dict(FAST, amplitude=7.5 * (1 + 0.05 * m))) for m in range(B)]
        _CASES[streams] = c
    return _CASES[streams]


def _solve(c, cps, ts, spi, env, isolate=False):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c.solver.engine.set_failure_policy(isolate)
        fields = np.array(c.solver(np.zeros((2, c.geo.n_blocks, 3)), ts, cps, keep_trajectory=True, steps_per_interval=spi))
        st = dict(c.solver.stats)
        status = c.solver.engine.member_status().tolist()
        obj, raw = c.solver.kinetic_energy_value_and_raw(c.target)
        st["adjoint"] = dict(c.solver.adjoint_stats)
        return fields, np.array(np.atleast_1d(obj), dtype=float), {k: np.array(v) for k, v in raw.items()}, st, status
    finally:
        c.solver.engine.set_failure_policy(False)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _check(ref, out):
    assert out[3]["adjoint"]["tile_kernels"] == 3, out[3]["adjoint"]                  # the persistent reverse really ran
    assert ref[3]["adjoint"]["tile_kernels"] != 3 and ref[3]["tile_kernels"] != 3 and out[3]["tile_kernels"] != 3
    assert out[3]["adjoint"]["checkpoint_records"] == 1
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])            # the forward pass is the same launches
    for k in ref[2]:
        assert relerr(out[2][k], ref[2][k]) < 1e-11, (k, relerr(out[2][k], ref[2][k]))
    assert np.abs(ref[0][:, -1]).max() > 0 and (ref[1] > 0).all()


@pytest.mark.parametrize("streams", ["1", "2"])
def test_uneven_launches_equal_stage_launches(hip_lib, streams):
    """Ten members in launches of at most four (the narrowest three): one member group, and two groups whose reverse sweep runs as one
    sequence of launches over the whole batch after both groups' forward stage launches."""
    wide = _case(streams)
    ts = np.linspace(0.0, 2e-4, 3)
    env = NARROW
    ref = _solve(wide, wide.cps, ts, 20, dict(env, DFX_PERSIST="0"))
    out = _solve(wide, wide.cps, ts, 20, env)
    _check(ref, out)
    assert out[3]["adjoint"]["streams"] == int(streams)
    # the same sweep with the forward's cap of two launches per segment: back on stage launches
    cap2 = _solve(wide, wide.cps, ts, 20, dict(env, DFX_PERSIST_ADJ_CHUNKS="2"))
    assert cap2[3]["adjoint"]["tile_kernels"] != 3
    for k in ref[2]:
        assert np.array_equal(cap2[2][k], ref[2][k]), k


def test_several_segments(hip_lib):
    """More steps than one segment holds (256 per launch): every segment's launches start from the adjoint state the later segment's
    launches left, and the accumulators add across segments."""
    wide = _case("2")
    ts = np.linspace(0.0, 6e-4, 3)
    env = NARROW
    ref = _solve(wide, wide.cps, ts, 150, dict(env, DFX_PERSIST="0"))
    out = _solve(wide, wide.cps, ts, 150, env)
    _check(ref, out)


@pytest.mark.parametrize("streams", ["1", "2"])
def test_segments_level_keeps_its_rule(hip_lib, streams):
    """The segments level also reads stage records, but keeps the forward's rule: one member group and at most two launches per segment.
    Ten members that take three launches, or two member groups, stay on stage launches there, bit for bit as with DFX_PERSIST=0."""
    wide = _case(streams)
    ts = np.linspace(0.0, 2e-4, 3)
    env = dict(NARROW, DFX_CHECKPOINT="segments")
    ref = _solve(wide, wide.cps, ts, 20, dict(env, DFX_PERSIST="0"))
    out = _solve(wide, wide.cps, ts, 20, env)
    assert out[3]["adjoint"]["checkpoint_records"] == 2 and out[3]["adjoint"]["tile_kernels"] != 3, out[3]["adjoint"]
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    for k in ref[2]:
        assert np.array_equal(out[2][k], ref[2][k]), k


def test_a_diverging_member_stays_alone(hip_lib):
    """Member 8 (in the last, narrower launch) overflows: under the isolating policy it is flagged and its gradient is not finite; every
    other member's gradient equals that of the batch without the bad member bit for bit, and agrees with the stage launches."""
    wide = _case("2")
    ts = np.linspace(0.0, 2e-4, 3)
    env = NARROW
    bad = list(wide.cps)
    bad[8] = wide.cps[8]._replace(constraint_params=dict(FAST, amplitude=1e200))
    good = _solve(wide, wide.cps, ts, 20, env, isolate=True)
    out = _solve(wide, bad, ts, 20, env, isolate=True)
    ref = _solve(wide, bad, ts, 20, dict(env, DFX_PERSIST="0"), isolate=True)
    assert out[3]["adjoint"]["tile_kernels"] == 3 and ref[3]["adjoint"]["tile_kernels"] != 3
    assert out[4] == ref[4] and out[4][8] != 0 and [s for m, s in enumerate(out[4]) if m != 8] == [0] * (B - 1), out[4]
    assert not np.isfinite(out[1][8])
    keep = [m for m in range(B) if m != 8]
    for k in good[2]:
        assert np.array_equal(np.isfinite(out[2][k][8]), np.isfinite(ref[2][k][8])), k
        assert np.array_equal(out[2][k][keep], good[2][k][keep]), k
        assert relerr(out[2][k][keep], ref[2][k][keep]) < 1e-11, k
