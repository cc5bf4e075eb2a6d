"""-m gpu: every bond model with every contact model (tests/model_matrix.py) on every build and checkpoint level of the stage kernels.

The kernels are compiled once per (MODEL, CONTACT) pair -- nonlinear / linearised ligaments, the simple spring, the stretching + torsional
spring, each with no contact, angle contact and distance contact -- and again per NPB, TAB, WT, ISTAGE, RECS, BOND_GRADS, REBUILD and for
the persistent and adaptive loops (dfx_builds.h select_fwd_build / select_adj_build / build_code, engine_launch.hip persist_shape_ok,
stage_builds_adj.hip, dfx_persist.hip, dfx_persist_dense.hip, engine_adaptive.hip).  The rest of the suite takes nonlinear ligaments with
angle contact everywhere and the other pairs on 4 x 4 blocks, undamped, on the default arm.  Here all 24 lattice x model x contact
combinations run on 13 x 13 quads (676 slots) and 11 x 11 kagome (242 triangles) -- a partial last wave --, damped, on

  arm          environment                              what it reaches
  stage        DFX_PERSIST=0 DFX_WT=0                   the generic table builds (the baseline); DFX_CHECKPOINT=records|stages|state|segments
  stage_wt     DFX_PERSIST=0 DFX_WT=1                   write-through stores and, for the ligament models without distance contact, ISTAGE builds
  stage_notab  DFX_PERSIST=0 DFX_WT=0 DFX_FN_TABLE=0    the TAB = 0 builds (time functions evaluated in the kernel)
  persistent   DFX_PERSIST=1                            the persistent loops (also at the segments level), or their fallback
  quadmap      DFX_PERSIST=0 DFX_WT=0 DFX_PACK3=0       kagome without distance contact: NPB = 4 on triangles
  quadmap_wt   DFX_PERSIST=0 DFX_WT=1 DFX_PACK3=0       kagome, the ligament models without distance contact: the NPB = 4 ISTAGE builds on triangles

each against torch.autograd through the oracle on every leaf the model has (fields RTOL_TRAJ -- 1e-9 with distance contact, the bar of
test_distance_contact.py --, gradients RTOL_GRAD, member by member), against the stage arm (fields 1e-13, gradients 1e-11; equality where
the same kernels ran and in a build without contraction), with the build code the dispatch implies and with exact zeros for the leaves the
model does not own.  Then the per-ligament image on the two stage arms, k_energy<MODEL, CONTACT> for all 12 pairs on both lattices, and the
adaptive call per model: 9 x 9 quads (5.06 waves: the error norm reduces across waves) and 5 x 5 kagome under DFX_PERSIST=1 and 0 -- the
plain call against the oracle's odeint, the kept steps ("adaptive-records", the ligament models without distance contact) against the
replay of the accepted steps, and the frozen grid ("adaptive-grid", springs and distance contact) against the oracle on that grid.

Measured errors: profiles/r16_model_matrix.txt."""
import os

import numpy as np
import pytest

from . import model_matrix as mm

pytestmark = pytest.mark.gpu

EXACT = "nocontract" in os.environ.get("DFX_LIBRARY", "")
TS = np.linspace(0.0, 3e-4, 3)
SPI = 8
TS_ADAPTIVE = np.linspace(0.0, 3e-4, 7)
STAGE = {"DFX_PERSIST": "0", "DFX_WT": "0"}
ARMS = {"stage": STAGE, "stage_wt": {"DFX_PERSIST": "0", "DFX_WT": "1"}, "stage_notab": dict(STAGE, DFX_FN_TABLE="0"),
        "persistent": {"DFX_PERSIST": "1"}, "quadmap": dict(STAGE, DFX_PACK3="0"),
        "quadmap_wt": {"DFX_PERSIST": "0", "DFX_WT": "1", "DFX_PACK3": "0"}}
LEVELS = ("records", "stages", "state", "segments")
SWITCHES = ("DFX_PERSIST", "DFX_WT", "DFX_FN_TABLE", "DFX_PACK3", "DFX_CHECKPOINT", "DFX_STAGE_CHECKPOINT", "DFX_STAGE_BUILDS", "DFX_DICT_LDS",
            "DFX_ADAPTIVE_RECORDS", "DFX_PERSIST_MAX_WG", "DFX_PERSIST_CHUNKS", "DFX_STREAMS", "DFX_EAGER_STEPS")
GRID = [(lattice, model, contact) for lattice in ("quads", "kagome") for model in mm.MODELS for contact in mm.CONTACTS]
PAIRS = [(model, contact) for model in mm.MODELS for contact in mm.CONTACTS]
PER_BOND = [("quads", m, c) for m, c in mm.rotating_contacts(start=0)] + [("kagome", m, c) for m, c in mm.rotating_contacts(start=1)]
ADAPTIVE = [("quads", 9, m, c) for m, c in PAIRS] + [("kagome", 5, m, c) for m, c in mm.rotating_contacts(start=0)]


def _ids(cases):
    return [mm.case_id(*c) if len(c) == 3 else mm.case_id(c[0], c[2], c[3]) for c in cases]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch, hip_lib):
    """The arms set what they test themselves: a suite run with any of these in the environment must not change them underneath."""
    for k in SWITCHES:
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


def _run(lattice, model, contact, env, image="uniform", seed=0):
    """A fresh solver created under ``env`` (DFX_WT is read when a handle is created, the others per solve) and its run."""
    def go():
        mc = mm.ModelCase(lattice, model, contact, mm.SIZES[lattice], image, seed=seed)
        return mc, mc.run_engine(TS, spi=SPI)
    return _with_env(env, go)


def _codes(eng):
    return eng["fwd_stats"]["tile_kernels"], eng["raw_stats"]["tile_kernels"], eng["tree_stats"]["tile_kernels"]


def _check_codes(arm, level, mc, eng):
    """The build code the dispatch implies (engine_launch.hip): 3 the persistent loops (persist_shape_ok: the ligament models without
    distance contact; the reverse loop at the records and segments levels), 2 the per-stage builds (build_code, dfx_builds.h: the same physics, write-
    through stores, the table, the common parameter shape -- the ``uniform`` image), 0 the generic builds."""
    fwd, raw, tree = _codes(eng)
    what = (arm, level, mc.model, mc.contact, fwd, raw, tree)
    serves = mm.loop_serves(mc.model, mc.contact)
    assert eng["fwd_stats_again"]["tile_kernels"] == fwd, what
    if arm == "persistent" and serves:
        assert fwd == 3 and raw == 3, what
    elif arm in ("stage_wt", "quadmap_wt"):
        want = 2 if serves and mc.image == "uniform" else 0
        assert fwd == want and raw == want and tree == 0, what          # (the build that accumulates ligament gradients has no per-stage twin)
    else:
        assert fwd != 3 and raw != 3 and tree != 3, what
    if level is not None:
        records, stages = {"records": (1, 0), "stages": (0, 1), "state": (0, 0), "segments": (2, 0)}[level]
        assert (eng["fwd_stats"]["checkpoint_records"], eng["fwd_stats"]["stage_checkpoint"]) == (records, stages), (what, eng["fwd_stats"])


def _check_arm(label, mc, eng, ref, base, same_kernels=False):
    f, g = mm.worst(mm.compare(mc, eng, ref))
    df, dg = mm.same_as(eng, base, EXACT or same_kernels)
    print(f"model_matrix: {mm.case_id(mc.lattice, mc.model, mc.contact)} {mc.image} {label}: vs oracle fields {f:.1e} gradients {g:.1e}; "
          f"vs stage arm fields {df:.1e} gradients {dg:.1e}; codes {_codes(eng)}")


@pytest.mark.parametrize("lattice,model,contact", GRID, ids=_ids(GRID))
def test_fixed_grid_on_every_arm_and_level(lattice, model, contact):
    serves = mm.loop_serves(model, contact)
    mc, base = _run(lattice, model, contact, ARMS["stage"])
    mc.assert_partial_last_wave()
    ref = mc.oracle(TS, spi=SPI)
    _check_codes("stage", None, mc, base)
    _check_arm("stage", mc, base, ref, base)
    runs = [("stage", level) for level in LEVELS] + [("stage_wt", None), ("stage_notab", None), ("persistent", None)]
    if serves:
        runs.append(("persistent", "segments"))
    if lattice == "kagome" and contact != "distance":
        runs.append(("quadmap", None))
        if serves:
            runs.append(("quadmap_wt", None))
    for arm, level in runs:
        mc_arm, eng = _run(lattice, model, contact, dict(ARMS[arm], **({"DFX_CHECKPOINT": level} if level else {})))
        _check_codes(arm, level, mc_arm, eng)
        # springs and distance contact leave the persistent loop: the stage arm's kernels ran, bit for bit
        _check_arm(arm + (f"/{level}" if level else ""), mc_arm, eng, ref, base, same_kernels=arm == "persistent" and not serves)


@pytest.mark.parametrize("lattice,model,contact", PER_BOND, ids=_ids(PER_BOND))
def test_per_ligament_stiffnesses_on_the_stage_arms(lattice, model, contact):
    mc, base = _run(lattice, model, contact, ARMS["stage"], image="per_bond", seed=1)
    ref = mc.oracle(TS, spi=SPI)
    _check_codes("stage", None, mc, base)
    _check_arm("stage", mc, base, ref, base)
    mc_wt, eng = _run(lattice, model, contact, ARMS["stage_wt"], image="per_bond", seed=1)
    _check_codes("stage_wt", None, mc_wt, eng)
    assert _codes(eng) == (0, 0, 0)
    _check_arm("stage_wt", mc_wt, eng, ref, base)


def test_per_bond_cases_cover_every_model_on_both_lattices_and_every_contact_twice():
    assert {(l, m) for l, m, _ in PER_BOND} == {(l, m) for l in ("quads", "kagome") for m in mm.MODELS}
    assert all(sum(c == contact for _, _, c in PER_BOND) >= 2 for contact in mm.CONTACTS)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
@pytest.mark.parametrize("model,contact", PAIRS, ids=[mm.case_id("e", m, c)[2:] for m, c in PAIRS])
def test_energy_kernel_of_every_pair(lattice, model, contact):
    e = mm.ModelCase(lattice, model, contact, mm.SIZES[lattice], "uniform").check_energy()
    print(f"model_matrix: {mm.case_id(lattice, model, contact)} k_energy vs oracle {e:.1e}")


# -- the adaptive call ------------------------------------------------------------------------------------------------------------------------
_ORACLE_PLAIN, _ORACLE_KEPT = {}, {}


@pytest.mark.parametrize("persist", ["1", "0"], ids=["loop", "stage_launches"])
@pytest.mark.parametrize("lattice,n,model,contact", ADAPTIVE, ids=_ids(ADAPTIVE))
def test_adaptive_call_against_the_oracle(lattice, n, model, contact, persist):
    """The plain call against the oracle's odeint (fields 1e-8, the same accepted steps), then ``keep_trajectory=True`` and both reverse
    sweeps against autograd through the oracle on the steps the engine kept or froze (model_matrix.check_kept_adaptive)."""
    key = (lattice, n, model, contact)
    serves = mm.loop_serves(model, contact)

    def go():
        mc = mm.ModelCase(lattice, model, contact, n, "uniform", batch=1)
        if key not in _ORACLE_PLAIN:
            _ORACLE_PLAIN[key] = mc.oracle_plain_adaptive(TS_ADAPTIVE)
        e_plain, steps = mm.check_plain_adaptive(mc, TS_ADAPTIVE, oracle=_ORACLE_PLAIN[key])
        eng, errs = mm.check_kept_adaptive(mc, TS_ADAPTIVE, "adaptive-records" if serves else "adaptive-grid",
                                           ref_cache=_ORACLE_KEPT.setdefault(key, {}))
        return e_plain, steps, eng, errs
    e_plain, steps, eng, errs = _with_env({"DFX_PERSIST": persist}, go)
    fwd, raw, tree = _codes(eng)
    if serves:          # the adaptive loop and the dense reverse loop under DFX_PERSIST=1, their stage-launch twins otherwise
        assert (fwd == 3) == (persist == "1") and (raw == 3) == (persist == "1") and tree != 3, (persist, fwd, raw, tree)
    else:
        assert fwd != 3 and raw != 3 and tree != 3, (persist, fwd, raw, tree)
    print(f"model_matrix: {mm.case_id(lattice, model, contact)} adaptive DFX_PERSIST={persist}: {steps} steps, plain fields vs odeint {e_plain:.1e}; "
          f"{eng['fwd_stats']['step_control']} ({eng['fwd_stats']['steps']} steps): fields %.1e gradients %.1e; codes {(fwd, raw, tree)}" % mm.worst(errs))


@pytest.mark.parametrize("lattice,n,model,contact", ADAPTIVE, ids=_ids(ADAPTIVE))
def test_adaptive_call_takes_the_same_rhs_evaluations_with_and_without_the_loop(lattice, n, model, contact):
    """Same accepts, same rejects under DFX_PERSIST=1 and 0: the plain call and the pass that keeps (or freezes) the steps."""
    serves = mm.loop_serves(model, contact)
    out = {}
    for persist in ("1", "0"):
        def go():
            mc = mm.ModelCase(lattice, model, contact, n, "uniform", batch=1)
            _, steps, st = mc.run_plain_adaptive(TS_ADAPTIVE)
            s = mc.solver
            s(mm._y0(mc), TS_ADAPTIVE, mc.engine_params(), keep_trajectory=True)
            assert s.stats["step_control"] == ("adaptive-records" if serves else "adaptive-grid"), s.stats["step_control"]
            kept = s.stats if serves else s.adaptive_stats
            return steps, st["rhs_evals"], kept["steps"], kept["rhs_evals"]
        out[persist] = _with_env({"DFX_PERSIST": persist}, go)
    assert out["1"] == out["0"] and out["1"][1] >= 6 * out["1"][0][0], out
