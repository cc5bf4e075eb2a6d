"""-m gpu: the persistent loops with member-ranked issue priority (dfx_persist_prio.h) and with the angle contact evaluated only beyond the
culling bound (dfx_persist.h, dfx_persist_dense.h).

Priority changes which wave a SIMD issues for, never what a wave computes: with co-resident members -- ten 64 x 64 designs are 640
workgroups, two or three per compute unit, in one launch; DFX_PERSIST_MAX_WG=2 makes it two launches of five at two per compute unit; 24
designs of the 32 x 32-cell kagome lattice take the packed 3-node mapping with one member per XCD -- every result with the priority on is
equal bit for bit to the same run under DFX_PERSIST_PRIO=0, and agrees with the stage launches (DFX_PERSIST=0) at the bars of
tests/test_gpu_persistent_lean.py: fields 1e-13, gradients 1e-11 of the largest entry (the two kernel families fuse multiply-adds
differently).

The cull.  The void angles of this design (squares rotated by 25 degrees, perturbed) start at 35.5 degrees, so with the cutoff at 42 degrees
(tests/test_gpu_persistent_wide.py's contact) the culling bound of dfx_plan.h is negative: no ligament is ever inside it, every lane takes
the branch that evaluates the contact with the ligament's own void angles.  At the benchmark's -10 / -15 degrees every ligament is inside
it.  Both sides in one wave need a cutoff between the two: at 30 degrees the bound is 0.095 rad, a dozen ligaments around the driven block
turn further (a few of them into contact) and the rest stay inside.  The priority checks run on the 42-degree and the -10-degree case; on
the 30-degree case every gradient leaf of the loop agrees with the stage launches (1e-11) and, for the member driven hardest, with
torch.autograd through the oracle at RTOL_GRAD, the bar tests/test_gpu_model_matrix.py holds the kernels to against the oracle.  (One
member against the oracle: the unrolled 40-step solve of a 64 x 64 lattice takes the oracle some twenty seconds per member on the CPU,
and the ten members differ in their drive's amplitude only; all ten are held to the stage launches.)  The premise -- some ligament beyond the bound, some block with all four inside it -- is
asserted from the fields with the bound of dfx_plan.h."""
import math
import os

import numpy as np
import pytest
import torch

from difflexmm_amd import geometry as geo_mod
from oracle import ref_dynamics as OD
from oracle import ref_geometry as OG

from .common import DENSITY, Case, relerr
from .parity import RTOL_GRAD, T64

pytestmark = pytest.mark.gpu

FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
RAW = ("centroid_node_vectors", "void_angle0", "inertia", "damping", "fn_params")
KNOBS = ("DFX_PERSIST", "DFX_PERSIST_PRIO", "DFX_PERSIST_ADJ_CHUNKS", "DFX_PERSIST_CHUNKS", "DFX_PERSIST_MAX_WG", "DFX_PERSIST_XCD", "DFX_CHECKPOINT",
         "DFX_STREAMS")
TS = np.linspace(0.0, 2e-4, 3)
SPI = 20
SETUPS = {"engaged": dict(lattice="quads", n=64, batch=10, cutoff_deg=42.0),          # no ligament inside the culling bound
          "mixed": dict(lattice="quads", n=64, batch=10, cutoff_deg=30.0),            # contact active on some ligaments, culled on most
          "culled": dict(lattice="quads", n=64, batch=10, cutoff_deg=-10.0),          # the benchmark's contact: culled everywhere
          "kagome": dict(lattice="kagome", n=32, batch=24, cutoff_deg=125.0)}
_CASES, _RUNS = {}, {}


@pytest.fixture(autouse=True)
def _no_knobs_from_outside(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _RUNS.clear()
    _CASES.clear()


def _case(name):
    if name not in _CASES:
        s = SETUPS[name]
        c = Case(s["lattice"], s["n"], True, True, seed=7, cutoff_deg=s["cutoff_deg"], batch=s["batch"])
        mid = c.geo.n_blocks // 2
        c.target = np.array([mid + 1, mid + 2], dtype=np.int32)
        c.cps = [c.cp._replace(constraint_params=dict(FAST, amplitude=7.5 * (1 + 0.05 * m))) for m in range(s["batch"])]
        _CASES[name] = c
    return _CASES[name]


def _solve(name, env):
    """(fields, objective, raw gradients, forward stats, adjoint stats) of one full solve under ``env``; every (case, env) runs once."""
    key = (name, tuple(sorted(env.items())))
    if key not in _RUNS:
        c = _case(name)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            fields = np.array(c.solver(np.zeros((2, c.geo.n_blocks, 3)), TS, c.cps, keep_trajectory=True, steps_per_interval=SPI))
            st = dict(c.solver.stats)
            obj, g, sa = c.solver.engine.kinetic_value_and_grad(c.target, which=RAW)
            _RUNS[key] = (fields, np.array(np.atleast_1d(obj), dtype=float), {k: np.array(v) for k, v in g.items()}, st, dict(sa))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return _RUNS[key]


def _same_bits(tag, on, off):
    assert on[4]["tile_kernels"] == 3 and off[4]["tile_kernels"] == 3, (tag, on[4], off[4])       # the reverse loop ran in both
    assert on[3]["tile_kernels"] == off[3]["tile_kernels"], (tag, on[3], off[3])
    assert on[4]["launches"] == off[4]["launches"], (tag, on[4], off[4])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]), tag
    assert set(on[2]) == set(off[2]) == set(RAW), (tag, sorted(on[2]))
    for k in on[2]:
        assert np.array_equal(on[2][k], off[2][k]), (tag, k, relerr(on[2][k], off[2][k]))
    assert (on[1] != 0).all() and np.abs(on[2]["centroid_node_vectors"]).max() > 0, tag


def _against_stage_launches(tag, out, ref, nonzero=RAW):
    assert out[4]["tile_kernels"] == 3 and ref[4]["tile_kernels"] != 3 and ref[3]["tile_kernels"] != 3, (tag, out[4], ref[4], ref[3])
    assert out[4]["checkpoint_records"] == 1, (tag, out[4])
    e_f = relerr(out[0], ref[0])
    errs = {k: relerr(out[2][k], ref[2][k]) for k in ref[2]}
    print(f"[prio] {tag}: forward build {out[3]['tile_kernels']}, fields {e_f:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # the forward pass ran on the loop as well (build 3) or on the same stage launches: the bars of tests/test_gpu_persistent_lean.py
    assert np.array_equal(out[0], ref[0]) if out[3]["tile_kernels"] != 3 else e_f < 1e-13, (tag, e_f)
    for k in ref[2]:
        assert errs[k] < 1e-11, (tag, k, errs[k])
    for k in nonzero:
        assert np.abs(ref[2][k]).max() > 0, (tag, k)


@pytest.mark.parametrize("name", ["engaged", "culled"])
def test_one_launch_of_co_resident_members(hip_lib, name):
    """640 workgroups in one launch, two or three per compute unit: the rule is armed, and changes no bit."""
    on, off = _solve(name, {}), _solve(name, {"DFX_PERSIST_PRIO": "0"})
    assert on[4]["launches"] >= 2 * 2, on[4]              # per segment one launch and its ring poison
    _same_bits(f"{name}, one launch", on, off)


@pytest.mark.parametrize("name", ["engaged", "culled"])
def test_two_launches_at_two_workgroups_per_compute_unit(hip_lib, name):
    env = {"DFX_PERSIST_MAX_WG": "2"}
    on, off = _solve(name, env), _solve(name, dict(env, DFX_PERSIST_PRIO="0"))
    assert on[4]["launches"] == _solve(name, {})[4]["launches"] + 2 * 2, on[4]      # per segment one launch more, with its ring poison
    _same_bits(f"{name}, two launches", on, off)
    _against_stage_launches(f"{name}, two launches", on, _solve(name, {"DFX_PERSIST": "0"}),
                            nonzero=RAW if name == "engaged" else tuple(k for k in RAW if k != "void_angle0"))


def test_forward_loop(hip_lib):
    """DFX_PERSIST_CHUNKS=16: the forward pass takes the loop whatever the width; fields with the priority on and off, and against the
    forward stage launches."""
    env = {"DFX_PERSIST_CHUNKS": "16"}
    on, off, ref = _solve("engaged", env), _solve("engaged", dict(env, DFX_PERSIST_PRIO="0")), _solve("engaged", {"DFX_PERSIST": "0"})
    assert on[3]["tile_kernels"] == 3 and off[3]["tile_kernels"] == 3 and ref[3]["tile_kernels"] != 3, (on[3], off[3], ref[3])
    assert np.array_equal(on[0], off[0])
    e_f = relerr(on[0], ref[0])
    print(f"[prio] forward loop against stage launches: fields {e_f:.2e}")
    assert e_f < 1e-13, e_f
    assert np.abs(ref[0][:, -1]).max() > 0


def test_kagome_packed_members_one_per_xcd(hip_lib):
    """24 designs of the 32 x 32-cell kagome lattice: five triangles per 16 lanes, 26 workgroups per member, every member on one XCD and
    three members deep on it."""
    on, off, ref = _solve("kagome", {}), _solve("kagome", {"DFX_PERSIST_PRIO": "0"}), _solve("kagome", {"DFX_PERSIST": "0"})
    _same_bits("kagome 32 x 24", on, off)
    _against_stage_launches("kagome 32 x 24", on, ref, nonzero=tuple(k for k in RAW if k != "void_angle0"))
    # the placement this case is here for: dense packing instead changes no bit either
    _same_bits("kagome 32 x 24, dense packing", _solve("kagome", {"DFX_PERSIST_XCD": "0"}), off)


def _culling_bound(c):
    """kappa_safe of dfx_plan.h: min(phi_lo - cutoff, pi - phi_hi) over the member's void angles, with its rounding margin."""
    phi = geo_mod.void_angles0(c.cnv, c.bonds)
    return min(phi.min() - c.contact_params[1], math.pi - phi.max()) * (1.0 - 1e-12) - 1e-12


def test_cull_premise_and_gradients_against_stage_launches_and_oracle(hip_lib):
    c = _case("mixed")
    out, ref = _solve("mixed", {}), _solve("mixed", {"DFX_PERSIST": "0"})
    _against_stage_launches("mixed, one launch", out, ref)
    _same_bits("mixed, one launch", out, _solve("mixed", {"DFX_PERSIST_PRIO": "0"}))
    assert _culling_bound(_case("engaged")) < 0 and _culling_bound(_case("culled")) > 0.5        # what the other two cases stand for
    # -- the premise, from the fields: relative rotation of every ligament at the last output, member by member
    safe = _culling_bound(c)
    assert safe > 0, safe
    npb = c.geo.n_npb
    a, b = c.bonds[:, 0] // npb, c.bonds[:, 1] // npb
    nb = c.geo.n_blocks
    theta = out[0].reshape(len(c.cps), len(TS), 2, nb, 3)[:, :, 0, :, 2]
    kap = np.abs(theta[:, :, b] - theta[:, :, a])                       # (member, time, ligament)
    far = (kap > safe).any(axis=1)
    per_block = np.zeros((len(c.cps), nb), dtype=int)
    for m in range(len(c.cps)):
        np.add.at(per_block[m], a, far[m]); np.add.at(per_block[m], b, far[m])
    ligaments = np.bincount(np.concatenate([a, b]), minlength=nb)
    print(f"[prio] culling bound {safe:.4f} rad: {int(far.sum())} of {far.size} member-ligaments beyond it at an output time, "
          f"{int(((per_block == 0) & (ligaments == 4)).sum())} member-blocks with all four inside")
    assert far.any(axis=1).all(), "no ligament beyond the culling bound: the case tests nothing"
    assert ((per_block == 0) & (ligaments == 4)).any(axis=1).all(), "no block with all four ligaments inside the bound"
    assert np.abs(out[2]["void_angle0"]).max() > 0                      # ... and the engaged contact reached the void-angle gradient
    # -- the member driven hardest against autograd through the oracle, every leaf
    m = len(c.cps) - 1
    leaves = dict(cnv=T64(c.cnv, True), inertia=T64(OG.compute_inertia(T64(c.cnv), DENSITY).numpy(), True), damping=T64(c.dval, True),
                  **{k: T64(v, True) for k, v in c.cps[m].constraint_params.items()})
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=SPI)
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(np.zeros((2, nb, 3))), TS, c.oracle_cp(leaves), SPI)
    free = list(osol.free_DOF_ids)
    obj = sum((leaves["inertia"][blk, d] * hist[:, 1, free.index(blk * 3 + d)] ** 2 / 2).sum() for blk in c.target for d in range(3))
    grads = dict(zip(leaves, torch.autograd.grad(obj, list(leaves.values()))))
    g = out[2]
    mine = dict(cnv=g["centroid_node_vectors"][m].reshape(c.cnv.shape) + geo_mod.void_angles0_vjp(c.cnv, c.bonds, g["void_angle0"][m].reshape(len(c.bonds), 2)),
                inertia=g["inertia"][m].reshape(nb, 3), damping=g["damping"][m].reshape(nb, 3)[c.damped])
    mine["amplitude"], mine["loading_rate"], mine["input_delay"] = g["fn_params"][m][0][:3]
    errs = {"objective": abs(out[1][m] - obj.item()) / abs(obj.item())}
    errs.update({k: relerr(mine[k], grads[k].numpy()) for k in mine})
    print(f"[prio] member {m} against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < RTOL_GRAD, (k, v)
