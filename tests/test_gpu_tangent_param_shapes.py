"""-m gpu: forward mode (jvp, jvp(adaptive=True), jvp_multi) on the non-uniform parameter images of tests/param_shapes.py.

The tangent kernels do not read the packed image: multi_image (engine_tangent.hip; jvp takes it at one direction) rebuilds a
per-slot image from it on the host and branches on the flags pack_params derives from the DATA -- the reference vector out of the member's
dictionary or out of p_l, the stiffnesses out of the member's constants or out of p_k, damping per block and DOF.  Every other forward-mode
test runs on a uniform image (k_uniform, a dictionary of at most four entries, one damping value on every block).  Here, at the sizes, grid,
seed and ShapeCases of tests/test_gpu_param_shapes.py (13 x 13 quads, 11 x 11 kagome: member boundaries inside a wave, a partial last wave):

  a. every image against torch.autograd.functional.jvp through the oracle, member by member, along ``all`` (every leaf) and ``leaf`` (only
     the leaf the shape is named after: its column would sit decades under the all-leaf column) -- RTOL_TRAJ fields, RTOL_GRAD tangents;
  b. jvp_multi, both forms of a pass, K = 3 (all, leaf, all - leaf) and K = 5: columns equal the single-direction jvp (1e-12; 1e-13 fields;
     the 4- and 2-wide kernels against the 1-wide one) and are linear in the direction;
  c. ten members of 49 blocks with stiffnesses of their own (490 threads): the transposition identity with vjp on the same solve per
     member (1e-11), jvp and jvp_multi in both forms, and members 0 and 9 against the oracle;
  d. jvp(adaptive=True) on the images of test_param_shape_adaptive_loop_and_stage_controller, members leaving the dense pass on their own
     clocks, against the oracle's replay of the steps the engine accepted;
  e. an image whose SHAPE changes in place between two calls (tests/stale_params.py).

Host side (the helpers against the oracle alone, and the premise that every image moves the fields): tests/test_tangent_param_shapes_host.py.
Worst cases measured on the MI355X: profiles/r10_tangent_param_shapes.txt."""
import functools

import numpy as np
import pytest

from .common import relerr
from .param_shapes import ShapeCase
from .parity import RTOL_GRAD, RTOL_TRAJ, _fields_bar, _y0, oracle_param_jvp, shape_leaf_names, shape_tangents, tangent_tree_of
from .stale_params import check_image_shape_change_reaches_jvp
from .test_gpu_param_shapes import FIXED, SIZES, SPI, TS
from .test_gpu_tangent import _tree_dot

pytestmark = pytest.mark.gpu

TANGENT_SEED = 5
WANT_LAYOUT = {"uniform": "lds", "k_per_bond": "lds", "damping_per_block": "lds", "refv_16": "lds", "refv_17": "global",
               "refv_256": "global", "refv_257": "none", "mixed_batch": "lds", "mixed_batch_17": "global"}
FORMS = ("chunked", "spread")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    """The tests set what they test themselves: a suite run with any of these in the environment must not change them underneath."""
    for k in ("DFX_PERSIST", "DFX_WT", "DFX_CHECKPOINT", "DFX_DICT_LDS", "DFX_STAGE_BUILDS", "DFX_PACK3", "DFX_TANGENT_MULTI_FORM"):
        monkeypatch.delenv(k, raising=False)


def _direction(sc, dirs, name):
    """(state0_dot, trees) of one named direction as jvp / jvp_multi take them for the whole batch."""
    B = len(sc.members)
    if name == "rest":          # all - leaf: the leaf direction holds the values `all` has there
        pairs = [tangent_tree_of(sc, {k: v for k, v in d["all"][2].items() if k not in shape_leaf_names(sc.shape)}) for d in dirs]
    else:
        pairs = [d[name][:2] for d in dirs]
    y0d = None
    if any(p[0] is not None for p in pairs):
        y0d = np.stack([np.zeros((2, sc.c.geo.n_blocks, 3)) if p[0] is None else p[0] for p in pairs])
    trees = [p[1] for p in pairs]
    return (y0d, trees) if B > 1 else (None if y0d is None else y0d[0], trees[0])


def _jvp(sc, dirs, name, ts, **kw):
    s, B = sc.c.solver, len(sc.members)
    y0d, trees = _direction(sc, dirs, name)
    fields, fdot = s.jvp(_y0(sc), ts, sc.engine_params(), y0d, trees, **kw)
    shape = (B, len(ts), 2, sc.c.geo.n_blocks, 3)
    return np.array(fields).reshape(shape), np.array(fdot).reshape(shape)


def _jvp_multi(sc, dirs, names, ts, **kw):
    s, B = sc.c.solver, len(sc.members)
    fields, fdots = s.jvp_multi(_y0(sc), ts, sc.engine_params(), [_direction(sc, dirs, name) for name in names], **kw)
    nb = sc.c.geo.n_blocks
    return np.array(fields).reshape(B, len(ts), 2, nb, 3), np.array(fdots).reshape(B, len(names), len(ts), 2, nb, 3)


@functools.lru_cache(maxsize=None)
def _single_direction_runs(shape, lattice):
    """One ShapeCase per image of FIXED and its single-direction jvp along all / leaf, shared by (a) and (b); read-only."""
    sc = ShapeCase(shape, lattice, SIZES[lattice], seed=1)
    dirs = shape_tangents(sc, TANGENT_SEED)
    out = {}
    for name in ("all", "leaf"):
        fields, out[name] = _jvp(sc, dirs, name, TS, steps_per_interval=SPI)
        assert sc.c.solver.stats["step_control"] == "fixed" and sc.c.solver.stats["steps"] == SPI * (len(TS) - 1)
    for v in (fields, *out.values()):
        v.flags.writeable = False
    return sc, dirs, fields, out


def _against_oracle(sc, fields, fdots, ref, what):
    """Every member on its own (a global maximum over the batch would hide a member smaller than its neighbours): fields RTOL_TRAJ,
    every named fields_dot RTOL_GRAD, on the free DOFs."""
    free = sc.c.solver.free_DOF_ids
    bad = {}
    for m, r in enumerate(ref):
        if r is None:
            continue
        T = len(r["fields"])
        ef = relerr(fields[m].reshape(T, 2, -1)[:, :, free], r["fields"])
        print(*what, "member", m, "fields", ef)
        if not ef < RTOL_TRAJ:
            bad[(m, "fields")] = ef
        for name, fd in fdots.items():
            ed = relerr(fd[m].reshape(T, 2, -1)[:, :, free], r[name])
            print(*what, "member", m, "direction", name, "fields_dot", ed, "max", float(np.abs(r[name]).max()))
            if not ed < RTOL_GRAD:
                bad[(m, name)] = ed
    assert not bad, (what, bad)


# ---- a. every image against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lattice", FIXED)
def test_tangent_on_every_parameter_image_matches_autograd(hip_lib, shape, lattice):
    sc, dirs, fields, fdots = _single_direction_runs(shape, lattice)
    assert sc.dict_layout == WANT_LAYOUT[shape], (shape, sc.n_dict)
    for m in range(len(sc.members)):
        assert np.abs(fdots["leaf"][m]).max() > 0, (shape, m)
    ref = oracle_param_jvp(sc, TS, dirs, spi=SPI)
    _against_oracle(sc, fields, fdots, ref, (shape, lattice))


# ---- b. several directions in one pass ---------------------------------------------------------------------------------------------------------
def _check_columns(sc, fields, fdots, fields_1, singles, what, fields_bar=1e-13):
    """fdots (B, K, ...): column k against the single-direction result singles[k] (None: against column 0 - column 1), member by member."""
    for m in range(len(sc.members)):
        ef = relerr(fields[m], fields_1[m])
        print(*what, "member", m, "fields", ef)
        assert ef < fields_bar, (what, m, ef)
        for k, one in enumerate(singles):
            want = fdots[m, 0] - fdots[m, 1] if one is None else one[m]
            ed = relerr(fdots[m, k], want)
            print(*what, "member", m, "column", k, "all - leaf" if one is None else "single", ed)
            assert ed < 1e-12, (what, m, k, ed)
            assert np.abs(want).max() > 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape,lattice", FIXED)
def test_multi_columns_on_every_parameter_image(hip_lib, monkeypatch, shape, lattice, form):
    sc, dirs, fields_1, singles = _single_direction_runs(shape, lattice)
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", form)
    fields, fdots = _jvp_multi(sc, dirs, ["all", "leaf", "rest"], TS, steps_per_interval=SPI)         # one pass of width 4, or 3 slices
    _check_columns(sc, fields, fdots, fields_1, [singles["all"], singles["leaf"], None], (shape, lattice, form, "K=3"))
    if (shape, lattice) == ("refv_257", "quads"):
        fields, fdots = _jvp_multi(sc, dirs, ["all", "leaf", "rest", "rest", "leaf"], TS, steps_per_interval=SPI)    # passes of width 4 and 1
        _check_columns(sc, fields, fdots, fields_1, [singles["all"], singles["leaf"], None, None, singles["leaf"]], (shape, lattice, form, "K=5"))


# ---- c. member boundaries inside a wave ---------------------------------------------------------------------------------------------------------
def _member_gaps(sc, fb, fdot, bars, s0b, dirs, name):
    """Per member |<fb, fields_dot> - (<tree_bar, tangent> + <state0_bar, state0_dot>)| / max(|lhs|, |rhs|) along one named direction."""
    y0d, trees = _direction(sc, dirs, name)
    gaps = []
    for m in range(len(sc.members)):
        lhs = float(np.sum(fb[m] * fdot[m]))
        rhs = _tree_dot(bars[m], trees[m]) + (0.0 if y0d is None else float(np.sum(np.asarray(s0b[m]) * y0d[m])))
        gaps.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    return gaps


def test_member_boundaries_inside_a_wave(hip_lib, monkeypatch):
    """k_per_bond, 7 x 7 quads, ten members: 490 threads of one block per thread, a member boundary every 49 lanes, every member its own
    stiffnesses (the adjoint of this case is pinned to the oracle by test_persistent_loop_more_members_than_xcds)."""
    sc = ShapeCase("k_per_bond", "quads", 7, seed=1, batch=10)
    assert sc.c.geo.n_blocks == 49 and len(sc.members) == 10 and not sc.expect["k_uniform"]
    dirs = shape_tangents(sc, TANGENT_SEED)
    s = sc.c.solver
    names = ["all", "leaf", "rest"]
    fields, fdot = _jvp(sc, dirs, "all", TS, steps_per_interval=SPI)
    multi = {}
    for form in FORMS:
        monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", form)
        multi[form] = _jvp_multi(sc, dirs, names, TS, steps_per_interval=SPI)
    monkeypatch.delenv("DFX_TANGENT_MULTI_FORM")
    kept = np.array(s(_y0(sc), TS, sc.engine_params(), keep_trajectory=True, steps_per_interval=SPI))
    fb = _fields_bar(sc, len(TS))
    bars, s0b = s.vjp(fb)
    assert relerr(fields, kept) < 1e-13
    gaps = {"jvp": _member_gaps(sc, fb, fdot, bars, s0b, dirs, "all")}
    for form in FORMS:
        assert relerr(multi[form][0], kept) < 1e-13
        for k, name in enumerate(names):
            gaps[f"jvp_multi {form} {name}"] = _member_gaps(sc, fb, multi[form][1][:, k], bars, s0b, dirs, name)
    for what, g in gaps.items():
        print("transposition gap per member,", what, ["%.1e" % x for x in g])
    bad = {(what, m): x for what, g in gaps.items() for m, x in enumerate(g) if not x <= 1e-11}
    assert not bad, bad
    ref = oracle_param_jvp(sc, TS, dirs, spi=SPI, names=("all",), members=(0, 9))
    _against_oracle(sc, fields, {"all": fdot}, ref, ("k_per_bond", "quads 7", "batch 10"))


# ---- d. the adaptive solve, members on their own clocks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lattice,n", [("k_per_bond", "quads", 7), ("damping_per_block", "kagome", 5), ("refv_17", "quads", 7),
                                             ("refv_257", "quads", 13), ("mixed_batch_17", "kagome", 5)])
def test_adaptive_tangent_on_parameter_images(hip_lib, shape, lattice, n):
    ts = np.linspace(0.0, 1.5e-4 if n > 10 else 3e-4, 7)
    sc = ShapeCase(shape, lattice, n, seed=1)
    dirs = shape_tangents(sc, TANGENT_SEED)
    s = sc.c.solver
    s.rtol = s.atol = 1e-5
    B = len(sc.members)
    default = np.array(s(_y0(sc), ts, sc.engine_params())).reshape(B, len(ts), 2, -1, 3)
    assert s.stats["step_control"] == "adaptive"
    names = ["all", "leaf"] if shape in ("mixed_batch_17", "damping_per_block") else ["all"]
    fdots, steps, step_times = {}, None, None
    for name in names:
        fields, fdots[name] = _jvp(sc, dirs, name, ts, adaptive=True)
        assert s.stats["step_control"] == "adaptive-dense"
        if steps is None:
            steps = list(s.stats["steps_per_member"])
            step_times = [np.concatenate([ts[:1], s.engine.adaptive_step_times(m)]) for m in range(B)]
            assert [len(t) - 1 for t in step_times] == steps
        assert list(s.stats["steps_per_member"]) == steps
        e = relerr(fields, default)
        print(shape, lattice, n, "steps", steps, name, "fields against the default call", e)
        assert e < 1e-10, e
    if shape == "mixed_batch_17":
        assert len(set(steps)) >= 2, steps              # a member really leaves the dense pass before the others
    f_multi, d_multi = _jvp_multi(sc, dirs, names, ts, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and list(s.stats["steps_per_member"]) == steps
    _check_columns(sc, f_multi, d_multi, fields, [fdots[name] for name in names], (shape, lattice, n, "adaptive"))
    ref = oracle_param_jvp(sc, ts, dirs, step_times=step_times, names=names)
    _against_oracle(sc, fields, fdots, ref, (shape, lattice, n, "adaptive"))


# ---- e. the shape of the image changes in place -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ["k_stretch", "reference_vector"])
def test_image_shape_change_in_place_reaches_jvp(hip_lib, leaf):
    check_image_shape_change_reaches_jvp(None, leaf)
