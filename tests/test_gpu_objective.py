"""-m gpu: weighted kinetic-energy and angular-momentum objectives evaluated and differentiated on the device
(include/dfx.h: dfx_objective_value, dfx_objective_value_and_grad; kernels in difflexmm_amd/csrc/dfx_objective.h) against the host
yardstick ``objective.host_value_and_cotangent`` + ``dfx_adjoint`` on the cotangent it builds + its explicit terms, on the same kept
solve.  Both sides run the SAME reverse sweep on cotangents that differ by rounding only (the device forms them from 1 / inv_m, the host
from the inertia), so the bar is the suite's bar for that situation, 1e-12 of the largest entry (jvp_multi's columns against jvp).
Shapes: the smallest at which the kernels can go wrong -- quads 6x6 with the angle contact engaged, kagome 4x4 (3 nodes per block, a padded
fourth slot), 3 members, 5 output times, 4 Dopri5 steps per interval, pulse drive.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r12_device_objectives.txt): 4.6e-14 in
case 1 (kagome, stages level, angular kind, fn_params), 0 against the kinetic entry, 1.7e-14 against the oracle."""
import math
import os

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P
from difflexmm_amd.geometry import compute_inertia

from .common import DENSITY, Case, relerr

pytestmark = pytest.mark.gpu

FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
TS = np.linspace(0.0, 4e-4, 5)
SPI = 4
BATCH = 3
WHICH = ("centroid_node_vectors", "void_angle0", "inertia", "block_centroids", "state0", "fn_params")
TAU = np.array([0.0, 1.0, 0.37, 2.0, 1.0])                              # tau[0] = 0, a non-integer entry
WEIGHTS = np.array([[1.0, -0.5], [0.25, 2.0], [-1.5, 0.75]])            # per member, one negative each way
TOL = 1e-12

PATHS = {
    "stage-launches": (dict(DFX_PERSIST="0", DFX_CHECKPOINT="records"), SPI),
    "persistent": (dict(DFX_PERSIST="1", DFX_CHECKPOINT="records"), SPI),
    "stages": (dict(DFX_CHECKPOINT="stages"), SPI),
    "segments": (dict(DFX_CHECKPOINT="segments"), SPI),
    "adaptive-kept-steps": (dict(), None),
}
PATH_ENV = ("DFX_PERSIST", "DFX_CHECKPOINT", "DFX_STAGE_CHECKPOINT", "DFX_ADAPTIVE_RECORDS", "DFX_EAGER_STEPS", "DFX_STREAMS")


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in PATH_ENV}
    for k in PATH_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Ensemble:
    """A Case of BATCH members with different designs (so node vectors, centroids and inertia differ between members), two overlapping
    targets away from the boundary blocks, and the arrays both sides need."""

    def __init__(self, lattice):
        n = 6 if lattice == "quads" else 4
        c = self.c = Case(lattice, n, True, True, seed=41, batch=BATCH, cutoff_deg=42.0 if lattice == "quads" else 125.0)
        rng = np.random.default_rng(7)
        amp = 0.15 if lattice == "quads" else 0.05
        self.cps, self.inertia, self.cen = [], [], []
        for m in range(BATCH):
            design = tuple(d + (rng.uniform(-amp, amp, d.shape) if m else 0.0) for d in c.design)
            cnv, cen = c.geo.centroid_node_vectors(*design), c.geo.block_centroids(*design)
            self.cps.append(c.cp._replace(geometrical_params=dm.GeometricalParams(cen, cnv), constraint_params=dict(FAST)))
            self.inertia.append(compute_inertia(cnv, DENSITY))
            self.cen.append(cen)
        self.inertia, self.cen = np.stack(self.inertia), np.stack(self.cen)
        self.nb = nb = c.geo.n_blocks
        if lattice == "quads":        # (row-major 6x6: 2x2 and 1x3 regions sharing block 15)
            self.targets = [np.array([14, 15, 20, 21]), np.array([15, 16, 17])]
        else:
            self.targets = [np.array([9, 10, 11, 12]), np.array([12, 13, 18])]
        self.w = O.block_weights_from_targets(nb, self.targets, WEIGHTS)
        centre = self.cen[0][self.targets[0]].mean(0)
        self.lever0 = self.cen - centre

    def spec(self, kind, tau=TAU):
        return O.ObjectiveSpec(kind, self.w, tau, self.lever0 if kind == O.ANGULAR_MOMENTUM else None)

    def solve(self, spi):
        c = self.c
        return c.solver(np.zeros((2, self.nb, 3)), TS, self.cps, keep_trajectory=True, steps_per_interval=spi)


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    return Ensemble(request.param)


def host_reference(eng, spec, fields, inertia, which=WHICH):
    """value, raw gradients: dfx_adjoint on the host-built cotangent + the explicit terms."""
    val, fb, m_bar, c_bar = O.host_value_and_cotangent(spec, fields, inertia)
    ref, _ = eng.adjoint(fb, which=which)
    ref = {k: np.array(v) for k, v in ref.items()}
    ref["inertia"] = ref["inertia"] + m_bar
    if spec.kind == O.ANGULAR_MOMENTUM:
        ref["block_centroids"] = ref.get("block_centroids", 0.0) + c_bar
    return np.atleast_1d(val), ref


def compare(tag, obj, out, val, ref, tol=TOL):
    worst = {"value": float(np.abs(obj - val).max() / np.abs(val).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[objective] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, (tag, bad)
    return worst


@pytest.mark.parametrize("path", list(PATHS))
def test_device_objective_equals_host_cotangent_through_the_same_sweep(ens, path):
    """Case 1: both kinds, per-member weights of both signs on two overlapping targets, tau with a zero and a non-integer entry; value and
    the raw gradients of every group a design or a drive reaches, on every form of the reverse sweep."""
    env, spi = PATHS[path]
    eng = ens.c.solver.engine

    def run():
        fields = np.array(ens.solve(spi))
        st_f = dict(ens.c.solver.stats)
        res = {}
        for kind in (O.KINETIC, O.ANGULAR_MOMENTUM):
            spec = ens.spec(kind)
            val, ref = host_reference(eng, spec, fields, ens.inertia)
            obj, out, st = eng.objective_value_and_grad(kind, spec.block_weights, spec.time_weights, spec.lever0, which=WHICH)
            out = {k: np.array(v) for k, v in out.items()}
            only = eng.objective_value(kind, spec.block_weights, spec.time_weights, spec.lever0)
            res[kind] = (val, ref, obj, out, st, only)
        return st_f, res
    st_f, res = _with_env(env, run)
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    for kind, (val, ref, obj, out, st, only) in res.items():
        tag = f"{ens.c.geo.__class__.__name__} {path} kind={kind}"
        if path == "stage-launches":
            assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
        elif path == "persistent":
            assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
        elif path == "stages":
            assert st["stage_checkpoint"] == 1, st
        elif path == "segments":
            assert st["checkpoint_records"] == 2, st
        assert np.array_equal(only, obj)                      # the value-only entry: the same reduction on the same history
        assert set(out) == set(WHICH) - ({"block_centroids"} if kind == O.KINETIC else set()), (tag, sorted(out))
        assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["state0"]).max() > 0 and np.abs(ref["fn_params"]).max() > 0
        assert all(np.abs(ref["inertia"][m]).max() > 0 for m in range(BATCH))
        compare(tag, obj, out, val, ref)
    if ens.c.geo.n_npb == 4:                                   # quads: the contact really is engaged
        assert np.abs(res[O.KINETIC][1]["void_angle0"]).max() > 0


def test_kinetic_kind_reproduces_the_kinetic_entry(ens):
    """Case 2: 0/1 weights on a 2x2 target, tau = NULL: dfx_kinetic_value_and_grad to 1e-13 (only the order of the value's sum differs);
    two consecutive calls return the same bits."""
    eng, tb = ens.c.solver.engine, ens.targets[0].astype(np.int32)
    which = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params")

    def run():
        ens.solve(SPI)
        v_k, g_k, _ = eng.kinetic_value_and_grad(tb, which=which)
        v_k, g_k = v_k.copy(), {k: np.array(v) for k, v in g_k.items()}
        w = O.block_weights_from_targets(ens.nb, [tb], [1.0])
        v1, g1, _ = eng.objective_value_and_grad(O.KINETIC, w, which=which)
        g1 = {k: np.array(v) for k, v in g1.items()}
        v2, g2, _ = eng.objective_value_and_grad(O.KINETIC, w, which=which)
        return v_k, g_k, v1, g1, v2, {k: np.array(v) for k, v in g2.items()}
    v_k, g_k, v1, g1, v2, g2 = _with_env({}, run)
    assert v_k.min() > 0
    compare("kinetic kind vs dfx_kinetic_value_and_grad", v1, g1, v_k, g_k, tol=1e-13)
    assert np.array_equal(v1, v2) and all(np.array_equal(g1[k], g2[k]) for k in g1)


SPIN_KW = dict(spacing=15.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19, k_rot=1.5, density=6.18e-9, amplitude=4.0, loading_rate=1500.0,
               input_delay=5e-5, n_excited_blocks=1, simulation_time=9e-4, n_timepoints=4, use_contact=True, k_contact=1.5,
               min_angle=5 * math.pi / 180, cutoff_angle=45 * math.pi / 180)


def _spin_damping(n):
    return 0.05 * np.array([2 * math.sqrt(0.36125 * 6.18e-9 * 225 * 1.19)] * 2 + [2 * math.sqrt(0.02175026 * 6.18e-9 * 15.0 ** 4 * 1.5)]) * np.ones((n, 1))


def _spin_forward(batch=1):
    fw = P.QuadsSpinForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=10,
                            batch=batch, **SPIN_KW)
    fw.setup()
    rng = np.random.default_rng(9)
    base = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    return fw, tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base)


def test_angular_momentum_on_the_device_against_the_oracle(hip_lib):
    """Case 3: 6x6 quads, one member, angular momentum about the target's mean centroid: the design gradient through
    TargetAngularMomentum([design]) on the device path against torch.autograd through the oracle's fixed-grid solve (1e-9, the suite's
    bar for discrete-adjoint gradients)."""
    from oracle import ref_problems as RP
    fw, x = _spin_forward()
    obj = P.TargetAngularMomentum(fw, (2, 2), (1, 0), spin_center="center", reference_design=x)
    v, g = obj.value_and_grad([x])
    assert v.shape == (1,) and len(g) == 1
    ofw = RP.ForwardProblem("quads", 6, 6, SPIN_KW["spacing"], SPIN_KW["bond_length"], SPIN_KW["k_stretch"], SPIN_KW["k_shear"], SPIN_KW["k_rot"],
                            SPIN_KW["density"], _spin_damping(36), SPIN_KW["amplitude"], SPIN_KW["loading_rate"], SPIN_KW["input_delay"], 1,
                            SPIN_KW["simulation_time"], SPIN_KW["n_timepoints"], "left", 0, use_contact=True, k_contact=1.5,
                            min_angle=SPIN_KW["min_angle"], cutoff_angle=SPIN_KW["cutoff_angle"], signal=RP.harmonic_signal)
    tb = RP.quads_target_blocks(6, 6, (2, 2), (1, 0))
    assert np.array_equal(tb, obj.target_blocks)
    xt = [torch.tensor(a, requires_grad=True) for a in x]
    ov = RP.target_angular_momentum(ofw, xt, tb, obj.spin_center, 10)
    og = torch.autograd.grad(ov, xt)
    e_v = abs(v[0] - ov.item()) / abs(ov.item())
    e_g = max(np.abs(a - r.numpy()).max() / np.abs(r.numpy()).max() for a, r in zip(g[0], og))
    print(f"[objective] angular momentum on the device vs the oracle: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert abs(ov.item()) > 0 and e_v < 1e-9 and e_g < 1e-9
    # a single design with on_device=True: the same numbers without the member axis
    v1, g1 = obj.value_and_grad(x, on_device=True)
    assert isinstance(v1, float) and v1 == v[0] and all(np.array_equal(a, r) for a, r in zip(g1, g[0]))


@pytest.mark.parametrize("kind", [O.KINETIC, O.ANGULAR_MOMENTUM])
def test_target_block_with_a_prescribed_dof(hip_lib, kind):
    """Case 4: the driven block (x prescribed, y and theta held) and its free neighbours as the target: what dfx_adjoint returns for the
    host-built cotangent, the gradient of the drive's parameters included."""
    c = Case("quads", 6, True, True, seed=43, cutoff_deg=42.0)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    driven = int(c.con[0, 0])
    tb = np.array([driven, driven + 1, driven + 6, driven + 7])
    fields = _with_env({}, lambda: np.array(c.solver(np.zeros((2, 36, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI)))
    assert np.abs(fields[:, 0, driven, 0]).max() > 0 and np.abs(fields[:, 1, driven, 0]).max() > 0
    spec = O.ObjectiveSpec(kind, O.block_weights_from_targets(36, [tb], [1.0]), TAU,
                           c.cen - c.cen[tb].mean(0) if kind == O.ANGULAR_MOMENTUM else None)
    eng = c.solver.engine
    val, ref = host_reference(eng, spec, fields[None], compute_inertia(c.cnv, DENSITY)[None])
    obj, out, _ = eng.objective_value_and_grad(kind, spec.block_weights, spec.time_weights, spec.lever0, which=WHICH)
    assert np.abs(ref["fn_params"]).max() > 0
    compare(f"prescribed DOF in the target, kind={kind}", obj, {k: np.array(v) for k, v in out.items()}, val, ref)


def test_device_views_equal_pinned_views(ens):
    """Case 5: device=True leaves the gradients in HBM: DeviceArray.to_host() equals the pinned views bit for bit; block_centroids is there
    for the angular kind on a lattice without distance contact."""
    eng = ens.c.solver.engine
    which = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "block_centroids")

    def run():
        ens.solve(SPI)
        out = {}
        for kind in (O.KINETIC, O.ANGULAR_MOMENTUM):
            s = ens.spec(kind)
            v_h, g_h, _ = eng.objective_value_and_grad(kind, s.block_weights, s.time_weights, s.lever0, which=which)
            v_h, g_h = v_h.copy(), {k: np.array(v) for k, v in g_h.items()}
            v_d, g_d, _ = eng.objective_value_and_grad(kind, s.block_weights, s.time_weights, s.lever0, which=which, device=True)
            out[kind] = (v_h, g_h, v_d, {k: a.to_host() for k, a in g_d.items()})
        return out
    out = _with_env({}, run)
    for kind, (v_h, g_h, v_d, g_d) in out.items():
        assert np.array_equal(v_h, v_d) and set(g_h) == set(g_d)
        assert ("block_centroids" in g_h) == (kind == O.ANGULAR_MOMENTUM)
        for k in g_h:
            assert g_d[k].shape == g_h[k].shape and np.array_equal(g_d[k], g_h[k]), (kind, k)
    assert np.abs(out[O.ANGULAR_MOMENTUM][1]["block_centroids"]).max() > 0
    with pytest.raises(RuntimeError, match="assembled on the host"):
        s = ens.spec(O.KINETIC)
        eng.objective_value_and_grad(O.KINETIC, s.block_weights, s.time_weights, None, which=("fn_params",), device=True)


def test_block_centroid_gradient_with_distance_contact_is_the_sum_of_both_parts(hip_lib):
    """Case 5, second half: with distance contact the sweep itself accumulates a block-centroid gradient; the angular kind adds its explicit
    term to it, for the pinned views and the device views alike."""
    from .test_distance_contact import DistCase
    c = DistCase("quads", None, n=4)
    ts = np.linspace(0.0, 4e-4, 5)
    fields = _with_env({}, lambda: np.array(c.solver(np.zeros((2, 16, 3)), ts, c.cp, keep_trajectory=True, steps_per_interval=SPI)))
    tb = np.array([5, 6, 9, 10])
    spec = O.ObjectiveSpec(O.ANGULAR_MOMENTUM, O.block_weights_from_targets(16, [tb], [1.0]), TAU, c.cen - c.cen[tb].mean(0))
    eng = c.solver.engine
    which = ("centroid_node_vectors", "inertia", "block_centroids", "state0")
    val, fb, m_bar, c_bar = O.host_value_and_cotangent(spec, fields[None], compute_inertia(c.cnv, DENSITY)[None])
    sweep, _ = eng.adjoint(fb, which=which)
    sweep = {k: np.array(v) for k, v in sweep.items()}
    assert np.abs(sweep["block_centroids"]).max() > 0 and np.abs(c_bar).max() > 0            # both parts are there
    ref = dict(sweep, inertia=sweep["inertia"] + m_bar, block_centroids=sweep["block_centroids"] + c_bar)
    obj, out, _ = eng.objective_value_and_grad(spec.kind, spec.block_weights, spec.time_weights, spec.lever0, which=which)
    out = {k: np.array(v) for k, v in out.items()}
    compare("distance contact, angular kind", obj, out, np.atleast_1d(val), ref)
    _, dev, _ = eng.objective_value_and_grad(spec.kind, spec.block_weights, spec.time_weights, spec.lever0, which=which, device=True)
    assert all(np.array_equal(dev[k].to_host(), out[k]) for k in out)


FOCUS_KW = dict(spacing=15.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19, k_rot=1.5, density=6.18e-9, amplitude=5.0, loading_rate=2500.0,
                input_delay=2e-5, n_excited_blocks=2, simulation_time=6e-4, n_timepoints=4, use_contact=True, k_contact=1.5,
                min_angle=5 * math.pi / 180, cutoff_angle=45 * math.pi / 180)


def _focus_forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=7, n2_blocks=6, damping=_spin_damping(42), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **FOCUS_KW)
    fw.setup()
    return fw


def _three_designs(fw, seed):
    rng = np.random.default_rng(seed)
    base = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    return [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]


def _check_list_against_singles(tag, many, single, designs):
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and len(set(np.round(v / np.abs(v).max(), 9))) == 3
    ind = getattr(many, "last_individual", None)
    for m, d in enumerate(designs):
        v1, g1 = single.value_and_grad(d)                     # the host path: history downloaded, cotangent built in NumPy
        e_v = abs(v[m] - v1) / abs(v1)
        e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g[m], g1))
        print(f"[objective] {tag}, design {m}: value {e_v:.2e}, design gradient {e_g:.2e}")
        assert e_v <= 1e-12 and e_g <= 1e-10
        if ind is not None:
            assert ind.shape == (3, len(single.last_individual)) and relerr(ind[m], single.last_individual) <= 1e-12


def test_problem_classes_take_a_list_of_designs(hip_lib):
    """Case 6: SplitTargetKineticEnergy and TargetAngularMomentum with a list of 3 different designs (one ensemble on the device) against
    three single-design calls on the host path; then two lock-step iterations of run_ensemble_optimization on the split objective."""
    sizes, shifts, weights = ((2, 2), (1, 2), (2, 1)), ((1, 1), (-1, 0), (1, 0)), (1.0, -0.5, 0.25)
    fw3, fw1 = _focus_forward(3), _focus_forward(1)
    designs = _three_designs(fw1, 19)
    many = P.SplitTargetKineticEnergy(fw3, sizes, shifts, weights)
    _check_list_against_singles("energy splitting", many, P.SplitTargetKineticEnergy(fw1, sizes, shifts, weights), designs)
    sp3, x = _spin_forward(3)
    sp1, _ = _spin_forward(1)
    sdesigns = _three_designs(sp1, 29)
    _check_list_against_singles("angular momentum", P.TargetAngularMomentum(sp3, (2, 2), (1, 0), spin_center="center", reference_design=x),
                                P.TargetAngularMomentum(sp1, (2, 2), (1, 0), spin_center="center", reference_design=x), sdesigns)
    best, logs = P.run_ensemble_optimization(many, designs, 2, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0,
                                             min_edge_length=1.0)
    assert len(best) == 3 and all(len(log["objective_values"]) == 2 for log in logs)
    v0, _ = many.value_and_grad(designs)
    assert np.allclose([log["objective_values"][0] for log in logs], v0, rtol=1e-12)
    assert all(np.isfinite(log["objective_values"]).all() for log in logs)


def test_refusals_leave_the_handle_usable(ens):
    """Case 7: wrong arguments only -- each raises RuntimeError with the library's text, and the same handle still answers afterwards."""
    eng = ens.c.solver.engine
    s = ens.spec(O.KINETIC)
    fresh = Case("quads", 4, True, False, seed=3)
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        fresh.solver.engine.objective_value_and_grad(O.KINETIC, np.ones(16))
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.objective_value(O.KINETIC, np.ones(16))
    _with_env({}, lambda: ens.solve(SPI))
    good = eng.objective_value(O.KINETIC, s.block_weights, s.time_weights)
    with pytest.raises(RuntimeError, match="unknown objective kind 7"):
        eng.objective_value_and_grad(7, s.block_weights, s.time_weights)
    with pytest.raises(RuntimeError, match="needs lever0"):
        eng.objective_value_and_grad(O.ANGULAR_MOMENTUM, s.block_weights, s.time_weights, None)
    with pytest.raises(RuntimeError, match="needs lever0"):
        eng.objective_value(O.ANGULAR_MOMENTUM, s.block_weights)
    bad = s.block_weights.copy()
    bad[1, 3] = np.nan
    with pytest.raises(RuntimeError, match="non-finite block weight"):
        eng.objective_value_and_grad(O.KINETIC, bad)
    with pytest.raises(RuntimeError, match="non-finite time weight"):
        eng.objective_value_and_grad(O.KINETIC, s.block_weights, np.array([1.0, np.inf, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError):
        eng.objective_value(O.KINETIC, np.ones(ens.nb + 1))
    obj, out, _ = eng.objective_value_and_grad(O.KINETIC, s.block_weights, s.time_weights, which=("inertia",))
    assert np.array_equal(obj, good) and np.abs(out["inertia"]).max() > 0
    # a shared checkpoint that another handle's forward pass has overwritten
    a, c2 = Case("quads", 4, True, False, seed=3), Case("quads", 4, True, False, seed=4)
    for c in (a, c2):
        c.cp = c.cp._replace(constraint_params=dict(FAST))
    c2.solver.engine.share_checkpoint(a.solver.engine)
    run = lambda c: c.solver(np.zeros((2, 16, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI)      # noqa: E731
    _with_env({}, lambda: (run(a), run(c2)))
    with pytest.raises(RuntimeError, match="shared trajectory checkpoint was overwritten"):
        a.solver.engine.objective_value_and_grad(O.KINETIC, np.ones(16))
    v, _, _ = c2.solver.engine.objective_value_and_grad(O.KINETIC, np.ones(16), which=("inertia",))
    _with_env({}, lambda: run(a))
    v_a, _, _ = a.solver.engine.objective_value_and_grad(O.KINETIC, np.ones(16), which=("inertia",))
    assert v[0] > 0 and v_a[0] > 0
