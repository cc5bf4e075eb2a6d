"""-m gpu: every kernel build on non-uniform parameter images (tests/param_shapes.py) against the oracle and against each other.

pack_params (dfx_plan.h) derives three properties from the DATA and the kernels branch on them: uniform stiffnesses (else p_k per slot),
uniform damping (else c.damping per DOF) and the number of distinct reference vectors (<= 16: a per-wave dictionary in LDS, 17..256: the
dictionary in global memory, > 256: p_l per slot).  Each shape runs on
  * the persistent loop (DFX_PERSIST=1: build code 3 forward, and 3 for the reverse sweep of vjp_raw, which asks for no ligament gradients),
  * the generic stage kernels (DFX_PERSIST=0: not 3),
  * the stage kernels with write-through stores (DFX_PERSIST=0 DFX_WT=1: the per-stage builds, code 2, for the common shape only --
    uniform stiffnesses and damping within each member, every dictionary in LDS: uniform, refv_16, mixed_batch -- and 0 for
    every other shape),
and every arm is compared with torch.autograd through the oracle on every parameter leaf, member by member (tests/parity.py), and with the
generic stage arm at the bars of test_gpu_persistent.py (1e-13 fields, 1e-11 gradients; equality in a build without contraction).
Lattices leave a partial last wave: 13 x 13 quads (676 slots = 10.6 waves), 11 x 11 kagome (242 triangles = 12.1 packed waves)."""
import os

import numpy as np
import pytest

from .common import relerr
from .param_shapes import ShapeCase
from .parity import RTOL_GRAD, compare_param_leaves, oracle_param_leaves, run_engine_param_leaves
from .stale_params import check_in_place_change, check_read_only_view_of_writeable_base

pytestmark = pytest.mark.gpu

EXACT = "nocontract" in os.environ.get("DFX_LIBRARY", "")
TS = np.linspace(0.0, 3e-4, 3)
SPI = 8
ARMS = {"persistent": {"DFX_PERSIST": "1"}, "stage": {"DFX_PERSIST": "0"}, "stage_wt": {"DFX_PERSIST": "0", "DFX_WT": "1"}}
SIZES = {"quads": 13, "kagome": 11}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    """The arms set what they test themselves: a suite run with any of these in the environment must not change them underneath."""
    for k in ("DFX_PERSIST", "DFX_WT", "DFX_CHECKPOINT", "DFX_DICT_LDS", "DFX_STAGE_BUILDS", "DFX_PACK3"):
        monkeypatch.delenv(k, raising=False)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(shape, lattice, n, env, batch=None, adaptive=False, ts=TS, seed=1):
    """A fresh solver created under ``env`` (DFX_WT is read when a handle is created, the others per solve) and its run."""
    def go():
        sc = ShapeCase(shape, lattice, n, seed=seed, batch=batch)
        return sc, run_engine_param_leaves(sc, ts, spi=None if adaptive else SPI, adaptive=adaptive)
    return _with_env(env, go)


def _same_as(eng, ref_eng):
    """An arm against the generic stage arm: fields 1e-13, gradients 1e-11 (equality without contraction)."""
    for a, b in zip(eng["members"], ref_eng["members"]):
        for k in b:
            for kk, bv in (b[k].items() if k == "raw" else [(k, b[k])]):
                av = a[k][kk] if k == "raw" else a[k]
                if EXACT:
                    assert np.array_equal(av, bv), (k, kk)
                else:
                    assert relerr(av, bv) < (1e-13 if "fields" in k else 1e-11), (k, kk, relerr(av, bv))


def _codes(eng):
    return eng["fwd_stats"]["tile_kernels"], eng["raw_stats"]["tile_kernels"], eng["tree_stats"]["tile_kernels"]


def common_shape(sc):
    """The parameter shape the per-stage builds compile in (dfx_builds.h, stage_build_ok): every member's stiffnesses and damping uniform
    (each member its own values) and every member's dictionary in LDS."""
    return sc.expect["k_uniform"] and sc.expect["damping_uniform"] and sc.dict_layout == "lds"


def _check_codes(arm, sc, eng):
    shape = sc.shape
    fwd, raw, tree = _codes(eng)
    assert eng["fwd_stats_again"]["tile_kernels"] == fwd
    if arm == "persistent":
        assert fwd == 3 and raw == 3, (arm, shape, fwd, raw, tree)
    elif arm == "stage":
        assert fwd != 3 and raw != 3 and tree != 3, (arm, shape, fwd, raw, tree)
    elif arm == "stage_wt":
        want = 2 if common_shape(sc) else 0          # (the reverse build that accumulates ligament gradients has no per-stage twin)
        assert fwd == want and raw == want and tree == 0, (arm, shape, fwd, raw, tree)


FIXED = [("uniform", "quads"), ("k_per_bond", "quads"), ("damping_per_block", "kagome"), ("refv_16", "quads"), ("refv_17", "kagome"),
         ("refv_256", "quads"), ("refv_257", "kagome"), ("refv_257", "quads"), ("mixed_batch", "quads"), ("mixed_batch_17", "kagome")]


@pytest.mark.parametrize("shape,lattice", FIXED)
def test_param_shape_every_arm_matches_the_oracle(hip_lib, shape, lattice):
    n = SIZES[lattice]
    runs = {arm: _run(shape, lattice, n, env) for arm, env in ARMS.items()}
    sc = runs["stage"][0]
    want_layout = {"uniform": "lds", "k_per_bond": "lds", "damping_per_block": "lds", "refv_16": "lds", "refv_17": "global",
                   "refv_256": "global", "refv_257": "none", "mixed_batch": "lds", "mixed_batch_17": "global"}[shape]
    assert sc.dict_layout == want_layout, (shape, sc.n_dict)
    ref = oracle_param_leaves(sc, TS, spi=SPI)
    assert common_shape(sc) == (shape in ("uniform", "refv_16", "mixed_batch")), (shape, sc.expect)
    for arm, (sc_arm, eng) in runs.items():
        _check_codes(arm, sc_arm, eng)
        compare_param_leaves(eng, ref)
        _same_as(eng, runs["stage"][1])


@pytest.mark.parametrize("shape,lattice", [("k_per_bond", "quads"), ("damping_per_block", "kagome"), ("refv_257", "quads")])
def test_param_shape_checkpoint_levels(hip_lib, shape, lattice):
    """The four checkpoint levels, persistent and stage launches: the reverse sweep reads what each level kept (records, stage values,
    states, segment starts re-run) of a non-uniform image."""
    n = SIZES[lattice]
    ref = None
    base = None
    for level in ("records", "stages", "state", "segments"):
        for arm in ("stage", "persistent"):
            sc, eng = _run(shape, lattice, n, dict(ARMS[arm], DFX_CHECKPOINT=level))
            if ref is None:
                ref = oracle_param_leaves(sc, TS, spi=SPI)
                base = eng
            assert (eng["fwd_stats"]["tile_kernels"] == 3) == (arm == "persistent"), (level, arm, _codes(eng))
            assert (eng["raw_stats"]["tile_kernels"] == 3) == (arm == "persistent" and level in ("records", "segments")), (level, arm, _codes(eng))
            compare_param_leaves(eng, ref)
            _same_as(eng, base)


def test_dictionary_in_global_memory_on_the_common_shape(hip_lib):
    """DFX_DICT_LDS=0: the common shape read through the global-memory dictionary (and so not the per-stage builds)."""
    sc, eng = _run("uniform", "quads", 13, dict(ARMS["stage_wt"], DFX_DICT_LDS="0"))
    _, base = _run("uniform", "quads", 13, ARMS["stage"])
    assert eng["fwd_stats"]["tile_kernels"] == 0, _codes(eng)
    compare_param_leaves(eng, oracle_param_leaves(sc, TS, spi=SPI))
    _same_as(eng, base)
    _, eng_p = _run("uniform", "quads", 13, dict(ARMS["persistent"], DFX_DICT_LDS="0"))
    assert _codes(eng_p)[:2] == (3, 3)
    _same_as(eng_p, base)


def test_persistent_loop_more_members_than_xcds(hip_lib):
    """Ten members with stiffnesses of their own on the persistent loop (more than one member per XCD), each against the oracle."""
    sc, eng = _run("k_per_bond", "quads", 7, ARMS["persistent"], batch=10)
    assert _codes(eng)[:2] == (3, 3)
    _, base = _run("k_per_bond", "quads", 7, ARMS["stage"], batch=10)
    compare_param_leaves(eng, oracle_param_leaves(sc, TS, spi=SPI))
    _same_as(eng, base)


@pytest.mark.parametrize("shape,lattice,n", [("k_per_bond", "quads", 7), ("damping_per_block", "kagome", 5), ("refv_17", "quads", 7),
                                             ("refv_257", "quads", 13), ("mixed_batch_17", "kagome", 5)])
def test_param_shape_adaptive_loop_and_stage_controller(hip_lib, shape, lattice, n):
    """The adaptive controller (k_adaptive_fwd_loop / k_adj_dense_loop, and their stage-launch twins) on a non-uniform image: each run
    against the oracle's replay of the steps it accepted, every leaf; both controllers take the same steps (their boundaries agree to the
    bar of test_gpu_persistent.py: the error estimate amplifies rounding)."""
    ts = np.linspace(0.0, 1.5e-4 if n > 10 else 3e-4, 7)
    out = {}
    for arm in ("persistent", "stage"):
        sc, eng = _run(shape, lattice, n, ARMS[arm], adaptive=True, ts=ts)
        assert eng["fwd_stats"]["step_control"] == "adaptive-records"
        loop = arm == "persistent"
        assert (eng["fwd_stats"]["tile_kernels"] == 3) == loop and (eng["raw_stats"]["tile_kernels"] == 3) == loop, (arm, _codes(eng))
        ref = oracle_param_leaves(sc, ts, step_times=eng["step_times"])
        compare_param_leaves(eng, ref, rtol_grad=RTOL_GRAD)
        out[arm] = eng
    assert out["persistent"]["fwd_stats"]["rhs_evals"] == out["stage"]["fwd_stats"]["rhs_evals"]      # same accepts, same rejects
    for a, b in zip(out["persistent"]["step_times"], out["stage"]["step_times"]):
        assert len(a) == len(b) and (np.array_equal(a, b) if EXACT else relerr(a, b) < 1e-5), (len(a), len(b), relerr(a, b))


@pytest.mark.parametrize("leaf", ["damping", "reference_vector", "k_stretch"])
def test_leaf_changed_in_place_reaches_the_next_solve_gpu(hip_lib, leaf):
    check_in_place_change(None, leaf)


def test_read_only_view_of_a_writeable_base_is_not_trusted_gpu(hip_lib):
    check_read_only_view_of_writeable_base(None)
