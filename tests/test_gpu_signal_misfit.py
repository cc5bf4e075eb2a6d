"""-m gpu: the signal misfit evaluated and differentiated on the device (include/dfx.h: dfx_signal_values, dfx_signal_misfit_value,
dfx_signal_misfit_value_and_grad; kernels k_signal_* in difflexmm_amd/csrc/dfx_objective.h, per-ligament arithmetic dfx_signal.h).

Yardstick (tests/signal_yardstick.py): signals and misfit written in torch with ``oracle.ref_energy``'s energies on the history downloaded
from the same kept solve; the force channels are ``autograd.grad(E, u, create_graph=True)``, a second pass of autograd gives the value,
``fields_bar`` and every explicit term, and ``dfx_adjoint(fields_bar)`` plus the explicit terms is the reference gradient.  Bars: those of
tests/test_gpu_strain_objective.py for this construction -- value 1e-12, every leaf 1e-11 of its largest entry -- and 1e-12 of the largest
signal for the signal values; 1e-9 end to end against the oracle alone and for the hinge fit (tests/hinge_common.py).
Shapes are those of test_gpu_objective.py: quads 6x6 with the angle contact engaged (cutoff 42 deg), kagome 4x4 (a padded fourth slot), 3
members with different designs AND different targets, 5 outputs, 4 Dopri5 steps per interval, pulse drive.  The specification holds force
terms on the driven block, on a clamped block and on a corner block, the moment component (8) as well as x and y, two signals that share a
block, one signal of several terms with coefficients of both signs, displacement and velocity terms; tau has a zero and a non-integer
entry.  T x listed blocks is no multiple of the 64 items of a workgroup, and exceeds one workgroup on the quads.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r17_signal_misfit.txt): signal values
2.7e-15; 2.1e-14 for a gradient through the same sweep (quads, adaptive kept steps, fn_params) and 1.6e-14 for the value over both lattices,
the five sweep forms and the four bond models with and without the angle contact; 1.2e-13 end to end against the oracle (quads, contact
constants); hinge 4.1e-15 against the second-handle forces and 1.9e-15 against the oracle's fit gradient; 2.7e-7 for the directional
derivatives of TargetSignalMisfit against central differences.  No leaf missed its bar."""
import math

import numpy as np
import pytest
import torch

from difflexmm_amd import geometry as G
from difflexmm_amd import hinge as H
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import hinge_common as HC
from .common import Case, relerr
from .model_matrix import ModelCase
from .signal_yardstick import signal_misfit
from .strain_yardstick import T64
from .test_gpu_objective import BATCH, FAST, FOCUS_KW, PATHS, SPI, TAU, TS, Ensemble, _spin_damping, _with_env
from .test_gpu_strain_objective import leaves_of

pytestmark = pytest.mark.gpu

ALL = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params", "reference_vector", "k_bond", "contact", "damping")
DESIGN = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params")      # no per-ligament gradients: the persistent loop stays eligible
TOL_SIGNAL, TOL_VALUE, TOL_GRAD = 1e-12, 1e-12, 1e-11
OMEGA = np.array([1.0, 0.5, 2.0, 0.25])
ITEMS_PER_WORKGROUP = 64                                                                # kObjQuads


def neighbours(c, block):
    b = np.asarray(c.bonds) // c.geo.n_npb
    return sorted(set(int(x) for x in b[(b == block).any(1)].ravel()) - {block})


def make_terms(c):
    """4 signals: force terms on the driven block (x and moment), the clamped block 0 (y), the last corner block (moment and x) and, on the
    quads, an interior block (moment); signals 0, 1 and 3 share the driven block; signal 1 has several terms with coefficients of both
    signs; signal 2 is a displacement and a velocity term, signal 3 mixes a rotation with a force."""
    nb = c.geo.n_blocks
    driven, clamped, corner = int(c.con[0, 0]), 0, nb - 1
    quads = c.geo.n_npb == 4
    i1, i2 = (14, 21) if quads else (9, 13)
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7),
             (1, clamped, 7, -1.3), (1, corner, 8, 0.9), (1, corner, 6, 0.5), (1, driven, 7, 0.4),
             (2, i1, 0, 2.0), (2, i1, 4, -1e-4),
             (3, i2, 2, 1.0), (3, driven, 6, 0.01)]
    if quads:
        terms.insert(5, (1, 15, 8, 0.3))
    force_blocks = sorted({b for _, b, comp, _ in terms if comp >= 6})
    listed = sorted(set(force_blocks) | {n for b in force_blocks for n in neighbours(c, b)})
    return terms, force_blocks, listed


def member_leaves(c, cps, m):
    lv = leaves_of(c, cps, m)
    if "am" not in lv:
        lv.pop("phi0")
    return lv


def yardstick(eng, c, leaves, fields, terms, ns, targets, omega, tau, which, model="nonlinear"):
    """value (B,), signals (B, T, ns), raw reference gradients: dfx_adjoint on the autograd cotangent + the autograd explicit terms."""
    fields = np.asarray(fields, dtype=float)
    if fields.ndim == 4:
        fields = fields[None]
    B = fields.shape[0]
    targets = np.broadcast_to(targets, (B,) + np.shape(targets)[-2:])
    val, S, fb, explicit = np.zeros(B), [], np.zeros_like(fields), []
    for m in range(B):
        val[m], s, fb[m], g = signal_misfit(fields[m], leaves[m], c.bonds, terms, ns, targets[m], omega, tau, model)
        S.append(s)
        explicit.append(g)
    ref, _ = eng.adjoint(fb, which=which)
    ref = {k: np.array(v) for k, v in ref.items()}
    for m, g in enumerate(explicit):
        ref["centroid_node_vectors"][m] += g["cnv"]
        if "void_angle0" in ref and "phi0" in g:
            ref["void_angle0"][m] += g["phi0"]
        if "reference_vector" in ref:
            ref["reference_vector"][m] += g["refv"]
        if "k_bond" in ref:
            ref["k_bond"][m] += np.stack([g["ks"], g["ksh"], g["kr"]], 1)
        if "contact" in ref and "am" in g:
            ref["contact"][m] += np.array([g["am"], g["ac"], g["kc"]])
    return val, np.stack(S), ref, fb, explicit


def compare(tag, obj, out, val, ref, tol=TOL_GRAD, tol_value=TOL_VALUE):
    worst = {"value": float(np.abs(obj - val).max() / np.abs(val).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[signal misfit] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= (tol_value if k == "value" else tol)}
    assert not bad, (tag, bad)
    return worst


def host(out):
    return {k: np.array(v) for k, v in out.items()}


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    """The ensemble of test_gpu_objective.py with the terms above and per-member targets: the yardstick's signals of a first solve, scaled
    by a different random factor per member, output and signal (fixed inputs from then on)."""
    e = Ensemble(request.param)
    e.terms, e.force_blocks, e.listed = make_terms(e.c)
    e.ns = 4
    e.leaves = [member_leaves(e.c, e.cps, m) for m in range(BATCH)]
    fields = np.array(_with_env({}, lambda: e.solve(SPI)))
    rng = np.random.default_rng(29)
    e.targets = np.stack([signal_misfit(fields[m], e.leaves[m], e.c.bonds, e.terms, e.ns, np.zeros((len(TS), e.ns)), None, None)[1]
                          for m in range(BATCH)]) * rng.uniform(0.5, 1.5, (BATCH, len(TS), e.ns))
    assert len(set(np.round(e.targets[:, -1, 0] / np.abs(e.targets[:, -1, 0]).max(), 9))) == BATCH
    return e


def test_the_specification_is_the_one_the_kernels_can_go_wrong_on(ens):
    c, T = ens.c, len(TS)
    driven, clamped, corner = int(c.con[0, 0]), 0, c.geo.n_blocks - 1
    comps = {(b, comp) for _, b, comp, _ in ens.terms}
    assert {driven, clamped, corner} <= set(ens.force_blocks) and {(driven, 8), (corner, 8), (driven, 6), (clamped, 7)} <= comps
    assert any(comp < 3 for _, comp in comps) and any(3 <= comp < 6 for _, comp in comps)
    coefs = [co for s, _, _, co in ens.terms if s == 1]
    assert len(coefs) >= 4 and min(coefs) < 0 < max(coefs)
    assert {s for s, b, _, _ in ens.terms if b == driven} == {0, 1, 3}
    assert TAU[0] == 0 and any(t != round(t) for t in TAU)
    for n in (len(ens.force_blocks), len(ens.listed)):
        assert (T * n) % ITEMS_PER_WORKGROUP != 0, n
    if c.geo.n_npb == 4:
        assert T * len(ens.listed) > ITEMS_PER_WORKGROUP


# ---- 1. signal values --------------------------------------------------------------------------------------------------------------------------
def test_signal_values(ens):
    """Field-only signals equal the fields bit for bit; the signals of the specification against the yardstick at 1e-12 of the largest."""
    c, eng = ens.c, ens.c.solver.engine
    bd = [(int(c.con[0, 0]), 0), (14, 2), (9, 1), (c.geo.n_blocks - 1, 0)]

    def run():
        fields = np.array(ens.solve(SPI))
        out = {kind: c.solver.signal_values(O.SignalSpec.fields_of(bd, kind)) for kind in ("displacement", "velocity")}
        return fields, out, c.solver.signal_values(O.SignalSpec(ens.terms, ens.ns))
    fields, out, S = _with_env({}, run)
    for kind, plane in (("displacement", 0), ("velocity", 1)):
        want = np.stack([fields[:, :, plane, b, d] for b, d in bd], -1)
        assert out[kind].shape == (BATCH, len(TS), len(bd)) and np.abs(want).max() > 0
        assert np.array_equal(out[kind], want), kind
        assert np.array_equal(out[kind], O.host_signal_values(O.SignalSpec.fields_of(bd, kind), fields))
    ref = np.stack([signal_misfit(fields[m], ens.leaves[m], c.bonds, ens.terms, ens.ns, np.zeros((len(TS), ens.ns)), None, None)[1]
                    for m in range(BATCH)])
    worst = float(np.abs(S - ref).max() / np.abs(ref).max())
    per = [float(np.abs(S[..., s] - ref[..., s]).max() / np.abs(ref[..., s]).max()) for s in range(ens.ns)]
    print(f"[signal misfit] {c.geo.__class__.__name__}: signal values against the yardstick {worst:.2e} of the largest signal; each signal of its own "
          f"largest entry: " + ", ".join(f"{v:.2e}" for v in per))
    assert all(np.abs(ref[..., s]).max() > 0 for s in range(ens.ns))
    assert worst <= TOL_SIGNAL and max(per) <= 1e-11


# ---- 2. value and raw gradients on every form of the sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(ens.solve(spi))
        st_f = dict(c.solver.stats)
        val, S, ref, fb, explicit = yardstick(eng, c, ens.leaves, fields, ens.terms, ens.ns, ens.targets, OMEGA, TAU, ALL)
        obj, out, _ = eng.signal_misfit_value_and_grad(ens.terms, ens.ns, ens.targets, OMEGA, TAU, which=ALL)
        obj, out = obj.copy(), host(out)
        obj_d, out_d, st = eng.signal_misfit_value_and_grad(ens.terms, ens.ns, ens.targets, OMEGA, TAU, which=DESIGN)
        obj_d, out_d = obj_d.copy(), host(out_d)
        only = eng.signal_misfit_value(ens.terms, ens.ns, ens.targets, OMEGA, TAU)
        return st_f, val, ref, fb, explicit, obj, out, obj_d, out_d, st, only
    st_f, val, ref, fb, explicit, obj, out, obj_d, out_d, st, only = _with_env(env, run)
    tag = f"{c.geo.__class__.__name__} {path}"
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    elif path == "stage-launches":
        assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
    elif path == "persistent":                     # without per-ligament gradients the persistent builds stay eligible
        assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
    elif path == "stages":
        assert st["stage_checkpoint"] == 1, st
    elif path == "segments":
        assert st["checkpoint_records"] == 2, st
    assert np.array_equal(only, obj) and np.array_equal(obj_d, obj)          # one reduction on one history
    assert set(out) == set(ALL) and set(out_d) == set(DESIGN), (tag, sorted(out))
    # the cotangent reaches position rows (force and displacement terms) and velocity rows; tau[0] = 0 silences the first output
    assert np.abs(fb[:, :, 0]).max() > 0 and np.abs(fb[:, :, 1]).max() > 0 and not fb[:, 0].any()
    engaged = c.geo.n_npb == 4                                                 # quads: the contact really is engaged
    assert all(np.abs(ref[k]).max() > 0 for k in ALL if engaged or k not in ("void_angle0", "contact")), tag
    # the moment terms reach the bending stiffness and, on the quads, the contact constants through the EXPLICIT terms
    assert all(np.abs(g["kr"]).max() > 0 for g in explicit) and (not engaged or all(np.abs(g["kc"]) > 0 for g in explicit))
    compare(tag, obj, out, val, ref)
    compare(tag + " (design leaves)", obj_d, out_d, val, {k: ref[k] for k in DESIGN})


MODEL_NAMES = {"nonlinear": "nonlinear", "linearized": "linearized", "simple": "simple_spring", "torsion": "stretch_torsion"}


@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_every_bond_model_with_and_without_the_angle_contact(hip_lib, model, contact):
    """Quads 4x4, one member, per-ligament stiffnesses: every leaf against the yardstick written with that model's energy."""
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    nbd, p = len(mc.bonds), mc.members[0]
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
    nb = mc.geo.n_blocks
    driven, corner = int(mc.con[0, 0]), nb - 1
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7), (1, 0, 7, -1.3), (1, corner, 8, 0.9), (1, 5, 8, 0.5), (1, 5, 6, -0.2), (2, 6, 1, 2.0), (2, 6, 3, 1e-4)]
    eng = mc.solver.engine

    def run():
        fields = np.array(mc.solver(np.zeros((2, nb, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
        zero = signal_misfit(fields, lv, mc.bonds, terms, 3, np.zeros((len(TS), 3)), None, None, MODEL_NAMES[model])[1]
        targets = zero * np.random.default_rng(3).uniform(0.5, 1.5, zero.shape)
        val, S, ref, fb, explicit = yardstick(eng, mc, [lv], fields, terms, 3, targets, OMEGA[:3], TAU, ALL, MODEL_NAMES[model])
        obj, out, _ = eng.signal_misfit_value_and_grad(terms, 3, targets, OMEGA[:3], TAU, which=ALL)
        return val, S, ref, obj.copy(), host(out), eng.signal_values(terms, 3)
    val, S, ref, obj, out, Sd = _with_env({}, run)
    tag = f"quads 4x4 {model} contact={contact}"
    e_s = float(np.abs(Sd - S).max() / np.abs(S).max())
    print(f"[signal misfit] {tag}: signal values {e_s:.2e}")
    assert e_s <= TOL_SIGNAL and np.abs(val).max() > 0 and np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
    if contact:
        assert np.abs(ref["contact"]).max() > 0 and np.abs(ref["void_angle0"]).max() > 0
    compare(tag, obj, out, val, ref)


# ---- 3. end to end against the oracle alone ----------------------------------------------------------------------------------------------------
def _oracle_misfit(c, lv, hist, osol, ts, terms, ns, targets, omega, tau, contact=True):
    """J with the oracle's energies on the oracle's history: bond energy, and the contact penalty on the void angles of the deformed nodes."""
    from oracle import ref_energy as OE
    nb, nbd = c.geo.n_blocks, len(c.bonds)
    free, con = torch.as_tensor(osol.free_DOF_ids), torch.as_tensor(osol.constrained_DOF_ids)
    drive = c.osolver_args["constrained_DOFs_fn"]
    bonds_t = torch.as_tensor(np.asarray(c.bonds), dtype=torch.long)
    J = torch.zeros((), dtype=torch.float64)
    for k, t in enumerate(ts):
        u = torch.zeros(nb * 3, dtype=torch.float64)
        u = u.index_put((free,), hist[k, 0]).index_put((con,), drive(float(t), lv["amplitude"], lv["loading_rate"], lv["input_delay"]))
        v = torch.zeros(nb * 3, dtype=torch.float64).index_put((free,), hist[k, 1]).reshape(nb, 3)
        # the force at this configuration: the gradient of E w.r.t. a copy of u that stays connected to the history
        u = u.reshape(nb, 3)
        nd = OE.block_to_node_kinematics(u, lv["cnv"])
        nodal = (nd.reshape(-1, 3)[bonds_t[:, 0]], nd.reshape(-1, 3)[bonds_t[:, 1]])
        E = torch.sum(OE.ligament_energy(nodal, lv["refv"], lv["ks"], lv["ksh"], lv["kr"]))
        if contact:
            nodes = T64(c.cen)[:, None] + lv["cnv"] + nd[:, :, :2]
            E = E + torch.sum(OE.contact_energy(OE.void_angles(nodes, c.bonds), lv["min_angle"], lv["cutoff_angle"], lv["k_contact"]))
        F, = torch.autograd.grad(E, u, create_graph=True)
        S = [None] * ns
        for s, b, comp, coef in terms:
            src = u[b, comp] if comp < 3 else v[b, comp - 3] if comp < 6 else F[b, comp - 6]
            S[s] = coef * src if S[s] is None else S[s] + coef * src
        for s in range(ns):
            J = J + 0.5 * tau[k] * omega[s] * (S[s] - targets[k, s]) ** 2
    return J


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_end_to_end_against_the_oracle(hip_lib, lattice):
    """Case 3: 4x4 with contact, 3 outputs, batch 1: autograd through the oracle's fixed-grid solve and ITS energies (twice, for the force
    terms) against the device entry mapped onto the ControlParams leaves.  No force term on the driven block or next to it and no field
    term on it (a prescribed output would add a direct drive term that the raw fn_params leave to the caller).  Bar 1e-9 (tests/parity.py)."""
    from oracle import ref_dynamics as OD
    quads = lattice == "quads"
    c = Case(lattice, 4, True, True, seed=47, cutoff_deg=42.0 if quads else 125.0, per_bond_k=True)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    # (the kagome with its engaged contact is stiffer: at the quads' step of 3.75e-5 the explicit integration is unstable and two solvers
    # drift apart by rounding alone)
    ts, spi = (np.linspace(0.0, 3e-4, 3), 4) if quads else (np.linspace(0.0, 1.5e-4, 3), 6)
    nb, nbd = c.geo.n_blocks, len(c.bonds)
    driven = int(c.con[0, 0])
    near = set(neighbours(c, driven)) | {driven}
    force_blocks = [b for b in ([0, nb - 1, 6] if quads else [0, nb - 1, 9]) if not (set(neighbours(c, b)) | {b}) & {driven}]
    assert len(force_blocks) >= 2 and not any(b in near for b in force_blocks)
    free_block = next(b for b in range(5, nb) if b not in near and b not in force_blocks)
    terms = [(0, force_blocks[0], 7, 1.0), (0, force_blocks[1], 8, -0.6), (0, force_blocks[-1], 6, 0.8), (1, force_blocks[-1], 8, 1.0),
             (1, free_block, 0, 3.0), (2, free_block, 2, 1.0), (2, free_block, 4, 1e-4)]
    tau, omega = np.array([0.0, 0.37, 1.0]), np.array([1.0, 0.5, 2.0])
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = np.array(_with_env({}, lambda: s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi)))
    print(f"[signal misfit] {lattice}: end to end: largest rotation of the solve {np.abs(fields[:, 0, :, 2]).max():.3f} rad")
    assert np.abs(fields[:, 0, :, 2]).max() < 1.0, "rotations beyond 1 rad: not a stable solve"
    targets = s.signal_values(O.SignalSpec(terms, 3))[0] * np.random.default_rng(5).uniform(0.5, 1.5, (3, 3))
    spec = O.SignalSpec(terms, 3, targets, omega, tau)
    obj, raw = s.signal_misfit_value_and_raw(spec, which=s.engine.ALL_GRADS)
    tree, _ = s._unflatten_grads(host(raw), None)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    refv = np.broadcast_to(c.refv, (nbd, 2)).copy()
    names = ["cnv", "refv", "ks", "ksh", "kr", "min_angle", "cutoff_angle", "k_contact", "amplitude", "loading_rate", "input_delay"]
    src = dict(cnv=c.cnv, refv=refv, ks=c.ks, ksh=c.ksh, kr=c.kr, min_angle=c.contact_params[0], cutoff_angle=c.contact_params[1],
               k_contact=c.contact_params[2], **FAST)
    lv = {k: T64(src[k], True) for k in names}
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(y0), ts, c.oracle_cp(lv), spi, "dopri5")
    J = _oracle_misfit(c, lv, hist, osol, ts, terms, 3, targets, omega, tau)
    og = dict(zip(names, torch.autograd.grad(J, [lv[k] for k in names])))
    bp, cpar = tree.mechanical_params.bond_params, tree.mechanical_params.contact_params
    errs = {"value": abs(obj[0] - J.item()) / abs(J.item()),
            "centroid_node_vectors": relerr(tree.geometrical_params.centroid_node_vectors, og["cnv"].numpy()),
            "k_bond": relerr(np.stack([bp.k_stretch, bp.k_shear, bp.k_rot], 1), np.stack([og[k].numpy() for k in ("ks", "ksh", "kr")], 1)),
            "reference_vector": relerr(bp.reference_vector, og["refv"].numpy()),
            "fn_params": relerr([tree.constraint_params[k] for k in FAST], [og[k].item() for k in FAST])}
    engaged = all(abs(og[k].item()) > 0 for k in ("min_angle", "cutoff_angle", "k_contact"))
    assert engaged or not quads
    if engaged:
        errs["contact"] = relerr([cpar.min_angle, cpar.cutoff_angle, cpar.k_contact], [og[k].item() for k in ("min_angle", "cutoff_angle", "k_contact")])
    print(f"[signal misfit] {lattice}: end to end against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert abs(J.item()) > 0 and all(np.abs(og[k].numpy()).max() > 0 for k in names if k not in ("min_angle", "cutoff_angle", "k_contact"))
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad


# ---- 4. the hinge characterisation ---------------------------------------------------------------------------------------------------------------
def _no_second_handle(fws, monkeypatch):
    def refuse(self, control_params):
        raise AssertionError("the device path loaded the second (reaction-force) handle")
    for fw in fws:
        monkeypatch.setattr(type(fw), "_load_force_engine", refuse)


def test_hinge_fit_on_the_kept_solves(hip_lib, monkeypatch):
    """The three rotated-square tests of tests/hinge_common.py: force_displacement_device against force_displacement (the second-handle
    path) at 1e-12 of the largest force; value_and_grad_device against value_and_grad and against autograd through the oracle's
    hinge_response_squared_error at 1e-9, with the second handle's loader made to fail."""
    from oracle import ref_problems as RP
    fws, ofs = HC.forwards(None)
    rng = np.random.default_rng(4)
    targets = {}
    for fw in fws:
        fw.setup()
        u = np.linspace(0, HC.KW["amplitude"], 9) * (-1.0 if fw.loading_type == "compression" else 1.0)
        targets[fw.loading_type] = np.array([u, 3.0 * np.abs(u) + rng.uniform(-0.2, 0.2, 9), 0.1 * np.ones(9)])
    opt = H.HingeResponseError(fws, targets)
    v, g = opt.value_and_grad(HC.K)
    worst = 0.0
    for fw in fws:
        sol, cp = fw.solve(HC.K)
        ref = fw.force_displacement(sol, cp)
        got = fw.force_displacement_device(cp)
        assert np.array_equal(got[0], ref[0]) and np.abs(ref[1]).max() > 1e-3
        worst = max(worst, float(np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max()))
    print(f"[signal misfit] hinge: force_displacement_device against the second-handle path {worst:.2e}")
    assert worst <= TOL_SIGNAL
    _no_second_handle(fws, monkeypatch)
    vd, gd = opt.value_and_grad_device(HC.K)
    kt = [torch.tensor(k, dtype=torch.float64, requires_grad=True) for k in HC.K]
    ov = RP.hinge_response_squared_error(ofs, opt.target_forces, kt, HC.SPI)
    og = [x.item() for x in torch.autograd.grad(ov, kt)]
    e_host = max(abs(vd - v) / abs(v), max(abs(a - b) for a, b in zip(gd, g)) / max(abs(b) for b in g))
    e_oracle = max(abs(vd - ov.item()) / abs(ov.item()), max(abs(a - b) for a, b in zip(gd, og)) / max(abs(b) for b in og))
    print(f"[signal misfit] hinge: value_and_grad_device against value_and_grad {e_host:.2e}, against the oracle {e_oracle:.2e}")
    assert e_host < 1e-9 and e_oracle < 1e-9
    # the loops take the switch
    gd_fit = H.HingeResponseError(fws, targets)
    gd_fit.run_optimization_GD(HC.K, 2, step_size=0.05 / np.abs(g).max(), lower_bound=0.5, upper_bound=200.0, on_device=True)
    assert len(gd_fit.objective_values) == 2 and abs(gd_fit.objective_values[0] - v) < 1e-9 * abs(v)


def test_hinge_quads_sample_on_the_kept_solve(hip_lib, monkeypatch):
    """The 4x4 quad sample of tests/hinge_common.py in shear: the device path against the host path and the oracle, 1e-9."""
    from difflexmm_amd.geometry import QuadGeometry
    from oracle import ref_problems as RP
    KW, n1, n2 = HC.KW, 4, 4
    g = QuadGeometry(n1, n2, KW["spacing"], KW["bond_length"])
    rng = np.random.default_rng(8)
    hs, vs = (b + rng.uniform(-0.3, 0.3, b.shape) for b in g.get_design_from_rotated_square(25 * math.pi / 180))
    fw = H.HingeQuadsForward(n1_blocks=n1, n2_blocks=n2, horizontal_shifts=hs, vertical_shifts=vs, loading_type="shear",
                             steps_per_interval=HC.SPI, **KW)
    of = RP.HingeForward("quads", n1, n2, KW["spacing"], KW["bond_length"], (hs, vs), KW["k_stretch"], KW["density"], KW["damping"], "shear",
                         KW["amplitude"], KW["loading_rate"], HC.NT, use_contact=True, k_contact=1.5, min_angle=KW["min_angle"],
                         cutoff_angle=KW["cutoff_angle"])
    u = np.linspace(0, KW["amplitude"], 7)
    opt = H.HingeResponseError([fw], {"shear": np.array([u, 2.0 * u, np.ones(7)])})
    v, grad = opt.value_and_grad(HC.K)
    _no_second_handle([fw], monkeypatch)
    vd, gd = opt.value_and_grad_device(HC.K)
    kt = [torch.tensor(k, dtype=torch.float64, requires_grad=True) for k in HC.K]
    ov = RP.hinge_response_squared_error([of], opt.target_forces, kt, HC.SPI)
    og = [x.item() for x in torch.autograd.grad(ov, kt)]
    e_host = max(abs(vd - v) / abs(v), max(abs(a - b) for a, b in zip(gd, grad)) / max(abs(b) for b in grad))
    e_oracle = max(abs(vd - ov.item()) / abs(ov.item()), max(abs(a - b) for a, b in zip(gd, og)) / max(abs(b) for b in og))
    print(f"[signal misfit] hinge, quad sample: value_and_grad_device against value_and_grad {e_host:.2e}, against the oracle {e_oracle:.2e}")
    assert e_host < 1e-9 and e_oracle < 1e-9


# ---- 5. shared and per-member targets, default weights, repeatability ---------------------------------------------------------------------------
def test_shared_targets_default_weights_repeatable_and_nothing_left_behind(ens):
    eng, c = ens.c.solver.engine, ens.c
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    T, ns = len(TS), ens.ns
    shared = ens.targets[1]

    def run():
        fields = np.array(ens.solve(SPI))
        fb = np.random.default_rng(2).normal(size=fields.shape)
        a = eng.signal_misfit_value_and_grad(ens.terms, ns, shared, OMEGA, TAU, which=which)
        a = (a[0].copy(), host(a[1]))
        b = eng.signal_misfit_value_and_grad(ens.terms, ns, np.broadcast_to(shared, (BATCH, T, ns)).copy(), OMEGA, TAU, which=which)
        b = (b[0].copy(), host(b[1]))
        d0 = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, None, None, which=which)
        d0 = (d0[0].copy(), host(d0[1]))
        d1 = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, np.ones(ns), np.ones(T), which=which)
        d1 = (d1[0].copy(), host(d1[1]))
        r1 = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, OMEGA, TAU, which=which)
        r1 = (r1[0].copy(), host(r1[1]))
        r2 = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, OMEGA, TAU, which=which)
        r2 = (r2[0].copy(), host(r2[1]))
        r3 = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, OMEGA, TAU, which=which, device=True)
        r3 = (r3[0].copy(), {k: x.to_host() for k, x in r3[1].items()})
        after = host(c.solver.vjp_raw(fb, which=which))
        fresh = np.array(ens.solve(SPI))
        before = host(c.solver.vjp_raw(fb, which=which))
        return fields, fresh, a, b, d0, d1, r1, r2, r3, after, before
    fields, fresh, a, b, d0, d1, r1, r2, r3, after, before = _with_env({}, run)
    same = lambda x, y: np.array_equal(x[0], y[0]) and set(x[1]) == set(y[1]) and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])     # noqa: E731
    assert np.abs(a[0]).min() > 0 and all(np.abs(a[1][k]).max() > 0 for k in which if k != "void_angle0" or c.geo.n_npb == 4)
    assert same(a, b), "shared targets against the same targets per member"
    assert same(d0, d1), "omega / tau of None against explicit ones"
    assert same(r1, r2) and same(r1, r3), "two identical calls, device views"
    assert not same(r1, d0)
    # a vjp after the calls serves the same kept solve as one on a fresh solve of the same problem
    assert np.array_equal(fields, fresh) and all(np.array_equal(after[k], before[k]) for k in which)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_the_handle_still_solves(ens):
    eng, c = ens.c.solver.engine, ens.c
    T, ns, nb = len(TS), ens.ns, c.geo.n_blocks
    fresh = Case("quads", 4, True, False, seed=3)
    one = [(0, 1, 6, 1.0)]
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        fresh.solver.engine.signal_misfit_value_and_grad(one, 1, np.zeros((T, 1)))
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.signal_misfit_value(one, 1, np.zeros((T, 1)))
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.signal_values(one, 1)
    _with_env({}, lambda: ens.solve(SPI))
    good = eng.signal_misfit_value(ens.terms, ns, ens.targets, OMEGA, TAU)
    tg1 = np.zeros((T, 1))
    for call in (lambda t, n: eng.signal_misfit_value_and_grad(t, n, np.zeros((T, n))), lambda t, n: eng.signal_misfit_value(t, n, np.zeros((T, n))),
                 lambda t, n: eng.signal_values(t, n)):
        with pytest.raises(RuntimeError, match=f"names block {nb} out of range"):
            call([(0, nb, 6, 1.0)], 1)
        with pytest.raises(RuntimeError, match="names component 9 out of range"):
            call([(0, 1, 9, 1.0)], 1)
        with pytest.raises(RuntimeError, match="names signal 2 out of range"):
            call([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 2)
        with pytest.raises(RuntimeError, match="signal 1 is empty"):
            call([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 3)
    with pytest.raises(RuntimeError, match="non-finite target"):
        eng.signal_misfit_value(one, 1, np.full((T, 1), np.nan))
    with pytest.raises(RuntimeError, match="non-finite time weight"):
        eng.signal_misfit_value_and_grad(one, 1, tg1, None, np.array([1.0, np.inf, 1.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="non-finite signal weight"):
        eng.signal_misfit_value_and_grad(one, 1, tg1, np.array([np.nan]))
    with pytest.raises(ValueError):
        eng.signal_misfit_value(one, 1, np.zeros((T + 1, 1)))
    with pytest.raises(ValueError):
        eng.signal_misfit_value(one, 1, tg1, np.ones(2))
    obj, out, _ = eng.signal_misfit_value_and_grad(ens.terms, ns, ens.targets, OMEGA, TAU, which=("inertia",))      # the handle still answers
    assert np.array_equal(obj, good) and np.abs(out["inertia"]).max() > 0
    fields = np.array(_with_env({}, lambda: ens.solve(SPI)))                                                         # ... and still solves
    assert np.isfinite(fields).all() and np.abs(fields[:, -1]).max() > 0
    run = lambda k: k.solver(np.zeros((2, 16, 3)), TS, k.cp, keep_trajectory=True, steps_per_interval=SPI)      # noqa: E731
    # force components with the distance-based contact; field components are served there
    mc = ModelCase("quads", "nonlinear", "distance", 4, "uniform", batch=1)
    _with_env({}, lambda: mc.solver(np.zeros((2, 16, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
    for call in (lambda: mc.solver.engine.signal_misfit_value_and_grad(one, 1, tg1), lambda: mc.solver.engine.signal_values(one, 1)):
        with pytest.raises(RuntimeError, match="distance-based contact energy is not part of the signal channels"):
            call()
    v, g, _ = mc.solver.engine.signal_misfit_value_and_grad([(0, 5, 0, 1.0), (0, 6, 4, 1e-4)], 1, tg1, which=("centroid_node_vectors", "block_centroids"))
    assert v[0] > 0 and np.abs(g["centroid_node_vectors"]).max() > 0
    f2 = mc.solver(np.zeros((2, 16, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI)
    assert np.isfinite(np.asarray(f2)).all()
    # a general bond list with extra ligaments
    ex = Case("quads", 4, True, False, seed=3, extra_bonds=[[1, 6], [9, 14]])
    ex.cp = ex.cp._replace(constraint_params=dict(FAST))
    _with_env({}, lambda: run(ex))
    for call in (lambda: ex.solver.engine.signal_misfit_value_and_grad(one, 1, tg1), lambda: ex.solver.engine.signal_misfit_value(one, 1, tg1)):
        with pytest.raises(RuntimeError, match="more than one ligament"):
            call()
    v, _, _ = ex.solver.engine.signal_misfit_value_and_grad([(0, 5, 1, 1.0)], 1, tg1 + 1.0, which=("inertia",))
    assert v[0] > 0 and np.isfinite(np.asarray(run(ex))).all()


# ---- 7. the problem class ----------------------------------------------------------------------------------------------------------------------
def _forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **FOCUS_KW)
    fw.setup()
    return fw


def test_target_signal_misfit_directional_derivatives(hip_lib):
    """TargetSignalMisfit on quads 6x6 for a list of 3 designs with per-member targets (one ensemble): directional derivatives along random
    design directions against central differences of ``value`` with the relative step 1e-6 and the 1e-6 bar of
    test_gpu_strain_objective.py's TargetStrainEnergy case; a one-design call with on_device=True equals member 0 of the list call to
    1e-13; a field-only specification on the host path equals its device path to 1e-12."""
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(19)
    base = fw1.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    terms = [(0, 14, 6, 1.0), (0, 15, 8, 0.5), (1, 21, 7, -1.0), (1, 20, 8, 1.0), (2, 16, 0, 1.0), (2, 16, 3, 1e-4)]
    fw3.solve(designs, keep_trajectory=False, want_fields=False)
    T = fw3.solve_dynamics.engine.n_timepoints
    S0 = fw3.solve_dynamics.signal_values(O.SignalSpec(terms, 3))
    targets = S0 * rng.uniform(0.5, 1.5, S0.shape)
    many = P.TargetSignalMisfit(fw3, O.SignalSpec(terms, 3, targets, [1.0, 2.0, 0.5]))
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and (v > 0).all()
    assert np.allclose(many.value(designs), v, rtol=1e-13, atol=0.0)
    scale = max(np.abs(a).max() for a in base)
    for trial in range(2):
        dirs = [tuple(rng.normal(size=a.shape) for a in base) for _ in range(3)]
        dirs = [tuple(a / max(np.abs(x).max() for x in d) for a in d) for d in dirs]
        h = 1e-6 * scale
        vp = many.value([tuple(a + h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        vm = many.value([tuple(a - h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        fd = (vp - vm) / (2 * h)
        mine = np.array([sum(float(np.sum(a * e)) for a, e in zip(gm, dd)) for gm, dd in zip(g, dirs)])
        err = np.abs(mine - fd) / np.abs(fd)
        print(f"[signal misfit] TargetSignalMisfit, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.TargetSignalMisfit(fw1, O.SignalSpec(terms, 3, targets[0], [1.0, 2.0, 0.5]))
    v1, g1 = single.value_and_grad(designs[0], on_device=True)
    e_v = abs(v1 - v[0]) / abs(v[0])
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[signal misfit] TargetSignalMisfit, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13
    with pytest.raises(ValueError, match="on_device=True"):
        single.value_and_grad(designs[0])
    fo = P.TargetSignalMisfit(fw1, O.SignalSpec.fields_of([(16, 0), (21, 2)], "displacement", targets[0][:, :2] * 0.0 + 0.01, tau=np.linspace(0.0, 1.0, T)))
    vh, gh = fo.value_and_grad(designs[0])
    vd, gdv = fo.value_and_grad(designs[0], on_device=True)
    e_v = abs(vh - vd) / abs(vd)
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(gh, gdv))
    print(f"[signal misfit] TargetSignalMisfit, field-only: host path against device path: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert vd > 0 and e_v <= 1e-12 and e_g <= 1e-12
