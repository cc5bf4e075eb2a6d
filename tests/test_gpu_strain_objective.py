"""-m gpu: the ligament strain-energy objective evaluated and differentiated on the device (include/dfx.h: dfx_strain_objective_value,
dfx_strain_objective_value_and_grad; kernels k_strain_objective / k_strain_objective_explicit in difflexmm_amd/csrc/dfx_objective.h).

Yardstick (tests/strain_yardstick.py): the objective written with ``oracle.ref_energy``'s bond and contact energies in torch on the history
downloaded from the same kept solve; autograd gives the value, ``fields_bar`` and every explicit parameter term, and ``dfx_adjoint(fields_bar)``
plus the explicit terms is the reference gradient.  Both sides run the same linear sweep on cotangents that differ only in how the ligament
force was formed (hand-derived against autograd): the suite holds that difference to 1e-12 (RHS and VJPs against autograd) and two routes
through one sweep to 1e-12 (test_gpu_objective.py), so the bar is 1e-11 of the largest entry of each leaf for the product of the two
effects, and 1e-12 for the value.  As for ``dfx_adjoint`` and the kinetic kinds, the raw ``fn_params`` hold what the sweep accumulates: the
direct dependence of a prescribed output DOF on its drive is on neither side of case 1 and is kept out of case 2 (no weighted bond on the
driven block there).
Shapes are those of test_gpu_objective.py: quads 6x6 with the angle contact engaged (cutoff 42 deg), kagome 4x4 (3 nodes per block, a padded
fourth slot), 3 members with different designs, 5 outputs, 4 Dopri5 steps per interval, pulse drive.  Bond weights are per member and of
both signs with most bonds at zero; the weighted set holds a bond on the driven block, one on a clamped block and one of a corner block
whose other slots carry no weighted ligament; tau has a zero and a non-integer entry.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r15_strain_objective.txt): case 1 1.4e-14
for a gradient (quads, adaptive kept steps, parts (1, 0, 0, 0), contact) and 1.4e-15 for the value over 60 configurations; 2.4e-14 end to end
against the oracle (k_bond); 5.4e-16 against response_data(); 1.1e-8 for the directional derivatives against central differences."""
import math

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from .common import Case, relerr
from .strain_yardstick import T64, strain_objective, void_angle_gap
from .test_gpu_objective import BATCH, FAST, FOCUS_KW, PATHS, SPI, TAU, TS, Ensemble, _spin_damping, _with_env

pytestmark = pytest.mark.gpu

ALL = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params", "reference_vector", "k_bond", "contact", "damping")
DESIGN = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params")      # no per-ligament gradients: the persistent loop stays eligible
PARTS = ((1.0, 1.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 0.5, 2.0, 1.5))
TOL_VALUE, TOL_GRAD = 1e-12, 1e-11


def bonds_of_block(bonds, npb, block):
    return np.nonzero((np.asarray(bonds) // npb == block).any(1))[0]


def weighted_bonds(c, seed, members=BATCH, interior=4):
    """(members, n_bonds) weights of both signs, most bonds at zero: one bond of the driven block, one of the clamped block 0, one of the
    last corner block (its other slots then carry no weighted ligament), a few more drawn at random; every member drops one of the random
    ones (so the members' sets differ) and keeps the three special ones."""
    rng = np.random.default_rng(seed)
    bonds, npb, nbd = c.bonds, c.geo.n_npb, len(c.bonds)
    driven, clamped, corner = int(c.con[0, 0]), 0, c.geo.n_blocks - 1
    special = [int(bonds_of_block(bonds, npb, b)[0]) for b in (driven, clamped, corner)]
    assert len(set(special)) == 3
    rest = [int(b) for b in rng.permutation(nbd) if b not in special][:interior]
    w = np.zeros((members, nbd))
    for m in range(members):
        for i, b in enumerate(special + rest):                         # signs alternate along the list, starting with the member's parity
            w[m, b] = (-1.0) ** (i + m) * rng.uniform(0.25, 2.0)
        w[m, rest[m % len(rest)]] = 0.0
    assert (w < 0).any() and (w > 0).any() and (w == 0).mean() > 0.7
    return w, special


def leaves_of(c, cps, m):
    """the parameter leaves of member m as the engine's raw gradients name them (NumPy)"""
    cp = cps[m] if isinstance(cps, (list, tuple)) and not hasattr(cps, "_fields") else cps
    nbd = len(c.bonds)
    cnv = np.asarray(cp.geometrical_params.centroid_node_vectors, dtype=float)
    bp = cp.mechanical_params.bond_params
    get = lambda name, default: np.broadcast_to(np.asarray(getattr(bp, name, default), dtype=float), (nbd,)).copy()     # noqa: E731
    lv = dict(cnv=cnv, ks=get("k_stretch", 0.0), ksh=get("k_shear", 0.0), kr=get("k_rot", 0.0),
              refv=np.broadcast_to(np.asarray(getattr(bp, "reference_vector", np.zeros(2)), dtype=float), (nbd, 2)).copy(),
              phi0=G.void_angles0(cnv, c.bonds))
    cpar = cp.mechanical_params.contact_params
    if cpar is not None:
        lv.update(am=float(cpar.min_angle), ac=float(cpar.cutoff_angle), kc=float(cpar.k_contact))
    return lv


def yardstick(eng, c, cps, fields, w, tau, parts, which, model="nonlinear"):
    """value (B,), raw reference gradients: dfx_adjoint on the autograd cotangent + the autograd explicit terms."""
    fields = np.asarray(fields, dtype=float)
    if fields.ndim == 4:
        fields = fields[None]
    B, T = fields.shape[:2]
    w = np.broadcast_to(w, (B, len(c.bonds)))
    tau = np.ones(T) if tau is None else np.asarray(tau, dtype=float)
    fb = np.zeros_like(fields)
    val = np.zeros(B)
    explicit = []
    for m in range(B):
        lv = leaves_of(c, cps, m)
        names = ["cnv", "refv", "ks", "ksh", "kr"] + (["phi0", "am", "ac", "kc"] if "am" in lv else [])
        t = {k: T64(lv[k], True) for k in names}
        u = T64(fields[m, :, 0], True)
        contact = (t["phi0"], t["am"], t["ac"], t["kc"]) if "am" in lv else None
        J = strain_objective(u, t["cnv"], c.bonds, t["refv"], t["ks"], t["ksh"], t["kr"], T64(w[m]), T64(tau), parts, model, contact)
        gr = torch.autograd.grad(J, [u] + [t[k] for k in names], allow_unused=True)
        g = {k: (np.zeros_like(lv[k]) if v is None else v.numpy()) for k, v in zip(names, gr[1:])}
        val[m], fb[m, :, 0] = J.item(), gr[0].numpy()
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
    return val, ref, fb


def compare(tag, obj, out, val, ref, tol=TOL_GRAD, tol_value=TOL_VALUE):
    worst = {"value": float(np.abs(obj - val).max() / np.abs(val).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[strain objective] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= (tol_value if k == "value" else tol)}
    assert not bad, (tag, bad)
    return worst


def host(out):
    return {k: np.array(v) for k, v in out.items()}


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    e = Ensemble(request.param)
    e.bw, e.special = weighted_bonds(e.c, seed=23)
    return e


# ---- 1. the device entry against the yardstick on every form of the sweep ------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    """Case 1: every leaf, three sets of part coefficients, five sweep forms; the call without per-ligament gradients runs the sweep builds
    of the kinetic kinds (the persistent loop where the path asks for it).  Worst case seen on an MI355X: 1.4e-14 (bar 1e-11), value 1.4e-15 (bar 1e-12)."""
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(ens.solve(spi))
        st_f = dict(c.solver.stats)
        res = []
        for parts in PARTS:
            val, ref, fb = yardstick(eng, c, ens.cps, fields, ens.bw, TAU, parts, ALL)
            obj, out, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=ALL)
            obj, out = obj.copy(), host(out)
            obj_d, out_d, st = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=DESIGN)
            obj_d, out_d = obj_d.copy(), host(out_d)
            only = eng.strain_objective_value(ens.bw, TAU, parts)
            res.append((parts, val, ref, fb, obj, out, obj_d, out_d, st, only))
        return fields, st_f, res
    fields, st_f, res = _with_env(env, run)
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    for parts, val, ref, fb, obj, out, obj_d, out_d, st, only in res:
        tag = f"{c.geo.__class__.__name__} {path} parts={parts}"
        if path == "stage-launches":
            assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
        elif path == "persistent":
            assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
        elif path == "stages":
            assert st["stage_checkpoint"] == 1, st
        elif path == "segments":
            assert st["checkpoint_records"] == 2, st
        assert np.array_equal(only, obj) and np.array_equal(obj_d, obj)          # one reduction on one history
        assert set(out) == set(ALL) and set(out_d) == set(DESIGN), (tag, sorted(out))
        # the weighted set reaches the driven block, the clamped block and the corner block; velocity rows stay zero
        npb = c.geo.n_npb
        for b in ens.special:
            blocks = np.asarray(c.bonds)[b] // npb
            assert np.abs(fb[:, :, 0, blocks]).max() > 0
        assert not fb[:, :, 1].any() and not fb[:, 0].any()                       # tau[0] = 0
        engaged = c.geo.n_npb == 4                                                 # quads: the contact really is engaged
        assert all(np.abs(ref[k]).max() > 0 for k in ALL if engaged or k not in ("void_angle0", "contact")), tag
        compare(tag, obj, out, val, ref)
        compare(tag + " (design leaves)", obj_d, out_d, val, {k: ref[k] for k in DESIGN})
    # the contact parametrisation of the yardstick is the oracle's void angle on the deformed nodes
    gap = max(void_angle_gap(fields[m, -1, 0], ens.cen[m], leaves_of(c, ens.cps, m)["cnv"], c.bonds, leaves_of(c, ens.cps, m)["phi0"])
              for m in range(BATCH))
    print(f"[strain objective] {c.geo.__class__.__name__} {path}: void angles phi0 -/+ kappa against the oracle's on the deformed nodes {gap:.2e}")
    assert gap <= 1e-12


# ---- 2. end to end against the oracle alone ------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_oracle(hip_lib):
    """Case 2: quads 4x4 with contact, 3 outputs, batch 1: autograd through the oracle's fixed-grid solve and ITS energies (bond energy, and the
    contact penalty on the void angles of the deformed nodes) against the device entry mapped onto the ControlParams leaves.  The engine's
    history is not shared with the yardstick.  Bar: the suite's 1e-9 for discrete-adjoint gradients (tests/parity.py).  No weighted bond on
    the driven block (its prescribed output would add a direct drive term that the raw fn_params leave to the caller)."""
    from oracle import ref_dynamics as OD
    from oracle import ref_energy as OE
    c = Case("quads", 4, True, True, seed=47, cutoff_deg=42.0, per_bond_k=True)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    ts, spi, parts = np.linspace(0.0, 3e-4, 3), 4, (1.0, 0.5, 2.0, 1.5)
    nb, nbd, npb = c.geo.n_blocks, len(c.bonds), c.geo.n_npb
    driven = int(c.con[0, 0])
    rng = np.random.default_rng(3)
    free_bonds = [b for b in range(nbd) if b not in set(bonds_of_block(c.bonds, npb, driven))]
    w = np.zeros(nbd)
    pick = [int(bonds_of_block(c.bonds, npb, 0)[0])] + [int(b) for b in rng.permutation(free_bonds)[:5]]
    w[pick] = rng.choice([-1.0, 1.0], len(pick)) * rng.uniform(0.25, 2.0, len(pick))
    tau = np.array([0.0, 0.37, 1.0])
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    _with_env({}, lambda: s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi))
    spec = O.StrainObjectiveSpec(w, tau, parts)
    obj, raw = s.strain_objective_value_and_raw(spec, which=s.engine.ALL_GRADS)
    tree, _ = s._unflatten_grads(host(raw), None)
    # the oracle
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    refv = np.broadcast_to(c.refv, (nbd, 2)).copy()
    names = ["cnv", "refv", "ks", "ksh", "kr", "min_angle", "cutoff_angle", "k_contact", "amplitude", "loading_rate", "input_delay"]
    src = dict(cnv=c.cnv, refv=refv, ks=c.ks, ksh=c.ksh, kr=c.kr, min_angle=c.contact_params[0], cutoff_angle=c.contact_params[1],
               k_contact=c.contact_params[2], **FAST)
    lv = {k: T64(src[k], True) for k in names}
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(y0), ts, c.oracle_cp(lv), spi, "dopri5")
    free, con = torch.as_tensor(osol.free_DOF_ids), torch.as_tensor(osol.constrained_DOF_ids)
    drive = c.osolver_args["constrained_DOFs_fn"]
    bonds_t = torch.as_tensor(np.asarray(c.bonds), dtype=torch.long)
    J = torch.zeros((), dtype=torch.float64)
    for k, t in enumerate(ts):
        u = torch.zeros(nb * 3, dtype=torch.float64)
        u = u.index_put((free,), hist[k, 0]).index_put((con,), drive(float(t), lv["amplitude"], lv["loading_rate"], lv["input_delay"]))
        u = u.reshape(nb, 3)
        nd = OE.block_to_node_kinematics(u, lv["cnv"])
        nodal = (nd.reshape(-1, 3)[bonds_t[:, 0]], nd.reshape(-1, 3)[bonds_t[:, 1]])
        e = OE.ligament_energy(nodal, lv["refv"], parts[0] * lv["ks"], parts[1] * lv["ksh"], parts[2] * lv["kr"])
        nodes = T64(c.cen)[:, None] + lv["cnv"] + nd[:, :, :2]
        ce = OE.contact_energy(OE.void_angles(nodes, c.bonds), lv["min_angle"], lv["cutoff_angle"], parts[3] * lv["k_contact"])
        e = e + ce[:nbd] + ce[nbd:]
        J = J + tau[k] * torch.sum(T64(w) * e)
    og = dict(zip(names, torch.autograd.grad(J, [lv[k] for k in names])))
    bp, cpar = tree.mechanical_params.bond_params, tree.mechanical_params.contact_params
    errs = {"value": abs(obj[0] - J.item()) / abs(J.item()),
            "centroid_node_vectors": relerr(tree.geometrical_params.centroid_node_vectors, og["cnv"].numpy()),
            "k_bond": relerr(np.stack([bp.k_stretch, bp.k_shear, bp.k_rot], 1), np.stack([og[k].numpy() for k in ("ks", "ksh", "kr")], 1)),
            "reference_vector": relerr(bp.reference_vector, og["refv"].numpy()),
            "contact": relerr([cpar.min_angle, cpar.cutoff_angle, cpar.k_contact], [og[k].item() for k in ("min_angle", "cutoff_angle", "k_contact")]),
            "fn_params": relerr([tree.constraint_params[k] for k in FAST], [og[k].item() for k in FAST])}
    print("[strain objective] end to end against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert abs(J.item()) > 0 and all(np.abs(og[k].numpy()).max() > 0 for k in names)
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad


# ---- 3. the value-only call against response_data() ------------------------------------------------------------------------------------------
def test_value_only_call_equals_response_data(ens):
    """Case 3: after a forward pass WITHOUT a kept trajectory, parts = e_i and tau = e_k pick one part at one output time:
    response_data()'s strain_energy_*[k] @ w to 1e-13 (the same per-ligament numbers, summed in another order)."""
    eng = ens.c.solver.engine

    def run():
        ens.c.solver(np.zeros((2, ens.nb, 3)), TS, ens.cps, keep_trajectory=False, steps_per_interval=SPI)
        resp = {k: v.copy() for k, v in eng.response_data(kinetic=False).items()}
        vals = {(i, k): eng.strain_objective_value(ens.bw, np.eye(len(TS))[k], np.eye(4)[i]) for i in range(3) for k in range(len(TS))}
        with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
            eng.strain_objective_value_and_grad(ens.bw, TAU, which=DESIGN)
        return resp, vals
    resp, vals = _with_env({}, run)
    worst = 0.0
    for i, name in enumerate(("strain_energy_stretch", "strain_energy_shear", "strain_energy_bending")):
        scale = np.abs(np.einsum("mkb,mb->mk", resp[name], ens.bw)).max()
        assert scale > 0
        for k in range(len(TS)):
            ref = np.einsum("mb,mb->m", resp[name][:, k], ens.bw)
            worst = max(worst, float(np.abs(vals[(i, k)] - ref).max() / scale))
    print(f"[strain objective] {ens.c.geo.__class__.__name__}: value-only call against response_data(): {worst:.2e}")
    assert worst <= 1e-13


# ---- 4. further cases --------------------------------------------------------------------------------------------------------------------------
def _single_case_check(tag, c, model, parts, which, seed):
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    w, _ = weighted_bonds(c, seed=seed, members=1)
    eng = c.solver.engine
    nb = c.geo.n_blocks

    def run():
        fields = np.array(c.solver(np.zeros((2, nb, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI))
        val, ref, _ = yardstick(eng, c, c.cp, fields, w[0], TAU, parts, which, model)
        obj, out, _ = eng.strain_objective_value_and_grad(w[0], TAU, parts, which=which)
        return val, ref, obj.copy(), host(out)
    val, ref, obj, out = _with_env({}, run)
    assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(val).max() > 0
    return compare(tag, obj, out, val, ref)


def test_linearised_ligaments(hip_lib):
    _single_case_check("linearised ligaments, quads 4x4 with contact", Case("quads", 4, False, True, seed=51, cutoff_deg=42.0), "linearized",
                       (0.0, 0.5, 2.0, 1.5), ALL, 31)


def test_per_bond_stiffnesses_and_a_dictionary_of_reference_vectors(hip_lib):
    """k_uniform off (every ligament its own stiffnesses) on the kagome lattice, whose reference vectors form a dictionary of several entries."""
    c = Case("kagome", 4, True, True, seed=52, cutoff_deg=125.0, per_bond_k=True)
    assert len(np.unique(np.round(np.broadcast_to(c.refv, (len(c.bonds), 2)), 12), axis=0)) > 1
    _single_case_check("per-bond stiffnesses, kagome 4x4", c, "nonlinear", (1.0, 1.0, 1.0, 0.0), ALL, 32)
    cu = Case("kagome", 4, True, True, seed=52, cutoff_deg=125.0, per_bond_k=False)
    _single_case_check("uniform stiffnesses, kagome 4x4", cu, "nonlinear", (1.0, 1.0, 1.0, 0.0), ALL, 32)


@pytest.mark.parametrize("model", ["simple", "torsion"])
def test_spring_models(hip_lib, model):
    """One case each of the two spring models: a part the model does not have contributes nothing (the shear part, and for the simple spring
    the bending part, carry arbitrary coefficients here)."""
    from .test_spring_models import SpringCase
    c = SpringCase(model, None)
    c.contact = False
    which = ("centroid_node_vectors", "inertia", "state0", "fn_params", "reference_vector", "k_bond")
    worst = _single_case_check(f"{model} spring, quads 4x4", c, {"simple": "simple_spring", "torsion": "stretch_torsion"}[model],
                               (1.5, 7.0, 0.5, 0.0), which, 33)
    assert set(worst) == set(which) | {"value"}
    with pytest.raises(RuntimeError, match="c_contact != 0 needs a lattice with the angle contact"):
        c.solver.engine.strain_objective_value(np.ones(len(c.bonds)), None, (1.0, 1.0, 1.0, 1.0))


def test_repeatable_device_views_and_nothing_left_behind(ens):
    """The same call twice returns the same bits; device=True views equal the pinned arrays bit for bit; a kinetic objective call after a strain
    call on the same handle returns what it returned before it (the scope guard leaves nothing on the handle)."""
    eng = ens.c.solver.engine
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    parts = PARTS[2]
    kspec = ens.spec(O.KINETIC)

    def run():
        ens.solve(SPI)
        k0, gk0, _ = eng.objective_value_and_grad(O.KINETIC, kspec.block_weights, kspec.time_weights, which=which)
        k0, gk0 = k0.copy(), host(gk0)
        v1, g1, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=which)
        v1, g1 = v1.copy(), host(g1)
        v2, g2, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=which)
        v2, g2 = v2.copy(), host(g2)
        v3, g3, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=which, device=True)
        g3 = {k: a.to_host() for k, a in g3.items()}
        with pytest.raises(RuntimeError, match="assembled on the host"):
            eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=("k_bond",), device=True)
        k1, gk1, _ = eng.objective_value_and_grad(O.KINETIC, kspec.block_weights, kspec.time_weights, which=which)
        return k0, gk0, v1, g1, v2, g2, v3.copy(), g3, k1.copy(), host(gk1)
    k0, gk0, v1, g1, v2, g2, v3, g3, k1, gk1 = _with_env({}, run)
    assert np.abs(v1).min() > 0 and all(np.abs(g1[k]).max() > 0 for k in g1)
    assert np.array_equal(v1, v2) and all(np.array_equal(g1[k], g2[k]) for k in which)
    assert np.array_equal(v1, v3) and set(g3) == set(which) and all(g3[k].shape == g1[k].shape and np.array_equal(g1[k], g3[k]) for k in which)
    assert np.array_equal(k0, k1) and all(np.array_equal(gk0[k], gk1[k]) for k in which)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(ens):
    eng = ens.c.solver.engine
    fresh = Case("quads", 4, True, False, seed=3)
    nbd4 = len(fresh.bonds)
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        fresh.solver.engine.strain_objective_value_and_grad(np.ones(nbd4))
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.strain_objective_value(np.ones(nbd4))
    _with_env({}, lambda: ens.solve(SPI))
    good = eng.strain_objective_value(ens.bw, TAU)
    bad = ens.bw.copy()
    bad[1, ens.special[0]] = np.nan
    with pytest.raises(RuntimeError, match="non-finite bond weight"):
        eng.strain_objective_value_and_grad(bad, TAU)
    with pytest.raises(RuntimeError, match="non-finite time weight"):
        eng.strain_objective_value_and_grad(ens.bw, np.array([1.0, np.inf, 1.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="non-finite part coefficient"):
        eng.strain_objective_value(ens.bw, TAU, (1.0, np.nan, 1.0, 0.0))
    with pytest.raises(ValueError):
        eng.strain_objective_value(np.ones(len(ens.c.bonds) + 1))
    with pytest.raises(ValueError):
        eng.strain_objective_value(ens.bw, TAU, (1.0, 1.0, 1.0))
    obj, out, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, which=("inertia",))          # the handle still answers
    assert np.array_equal(obj, good) and np.abs(out["inertia"]).max() > 0
    # c_contact != 0 without the angle contact
    nc = Case("quads", 4, True, False, seed=3)
    nc.cp = nc.cp._replace(constraint_params=dict(FAST))
    run = lambda c: c.solver(np.zeros((2, 16, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI)      # noqa: E731
    _with_env({}, lambda: run(nc))
    with pytest.raises(RuntimeError, match="c_contact != 0 needs a lattice with the angle contact"):
        nc.solver.engine.strain_objective_value_and_grad(np.ones(nbd4), None, (1.0, 1.0, 1.0, 0.5))
    assert nc.solver.engine.strain_objective_value(np.ones(nbd4))[0] > 0
    # a general bond list with extra ligaments
    ex = Case("quads", 4, True, False, seed=3, extra_bonds=[[1, 6], [9, 14]])
    ex.cp = ex.cp._replace(constraint_params=dict(FAST))
    _with_env({}, lambda: run(ex))
    with pytest.raises(RuntimeError, match="more than one ligament"):
        ex.solver.engine.strain_objective_value_and_grad(np.ones(len(ex.bonds)))
    with pytest.raises(RuntimeError, match="more than one ligament"):
        ex.solver.engine.strain_objective_value(np.ones(len(ex.bonds)))
    # a shared checkpoint that another handle's forward pass has overwritten
    a, c2 = Case("quads", 4, True, False, seed=3), Case("quads", 4, True, False, seed=4)
    for c in (a, c2):
        c.cp = c.cp._replace(constraint_params=dict(FAST))
    c2.solver.engine.share_checkpoint(a.solver.engine)
    _with_env({}, lambda: (run(a), run(c2)))
    with pytest.raises(RuntimeError, match="shared trajectory checkpoint was overwritten"):
        a.solver.engine.strain_objective_value_and_grad(np.ones(nbd4))
    v, _, _ = c2.solver.engine.strain_objective_value_and_grad(np.ones(nbd4), which=("inertia",))
    assert v[0] > 0


# ---- 6. the problem class ----------------------------------------------------------------------------------------------------------------------
def _forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **FOCUS_KW)
    fw.setup()
    return fw


def test_target_strain_energy_directional_derivatives(hip_lib):
    """Case 6: TargetStrainEnergy.value_and_grad on quads 6x6 for a list of 3 designs (one ensemble): directional derivatives along two random
    design directions against central differences of ``value`` with the relative step 1e-6 and the 1e-6 bar of the batch-1 jacfwd case of
    test_gpu_tangent_multi.py; a one-design call equals member 0 of the list call to 1e-13."""
    sizes, shifts, weights = ((2, 2), (1, 2)), ((1, 1), (-1, 0)), (1.0, -0.5)
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(19)
    base = fw1.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    many = P.TargetStrainEnergy(fw3, sizes, shifts, weights, parts=(1.0, 1.0, 1.0, 0.5), ends="any")
    assert (many.bond_weights > 0).any() and (many.bond_weights < 0).any() and (many.bond_weights == 0).any()
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and len(set(np.round(v / np.abs(v).max(), 9))) == 3
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
        print(f"[strain objective] TargetStrainEnergy, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.TargetStrainEnergy(fw1, sizes, shifts, weights, parts=(1.0, 1.0, 1.0, 0.5), ends="any")
    v1, g1 = single.value_and_grad(designs[0])
    e_v = abs(v1 - v[0]) / abs(v[0])
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[strain objective] TargetStrainEnergy, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13
    best, logs = P.run_ensemble_optimization(many, designs, 2, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0,
                                             min_edge_length=1.0)
    assert len(best) == 3 and np.allclose([log["objective_values"][0] for log in logs], v, rtol=1e-12)
