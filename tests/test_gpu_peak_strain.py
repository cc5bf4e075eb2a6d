"""-m gpu: the peak ligament strain -- a smooth maximum over (output time, ligament) pairs -- evaluated and differentiated on the device
(include/dfx.h: dfx_strain_peak_value, dfx_strain_peak_value_and_grad; kernels k_strain_peak_* in difflexmm_amd/csrc/dfx_objective.h).

Yardstick (tests/peak_strain_yardstick.py): q = 2 E_bond with the coefficient triple as stiffnesses, written with the oracle's bond energies
in torch on the history downloaded from the same kept solve, ``torch.logsumexp`` / the p-norm on top; autograd gives the value, ``fields_bar``
and the explicit node-vector and reference-vector terms, and ``dfx_adjoint(fields_bar)`` plus the explicit terms is the reference gradient.
Bars: those of tests/test_gpu_strain_objective.py (1e-12 for the value, 1e-11 of the largest entry of each leaf: both sides run the same
linear sweep on cotangents that differ in how the ligament force was formed).  The softmax amplifies the relative error of q (1e-15 in that
suite) by at most beta q_hat, so every case that uses these bars takes its sharpness from the data with 5 <= beta q_hat <= 40, or p = 6
(tests/peak_strain_cases.py; the premises are checked on the CPU port in tests/test_peak_strain_host.py).
Shapes: the small ensembles of tests/test_gpu_objective.py (quads 6x6 with the contact engaged, kagome 4x4 with its padded fourth slot, 3
members, 5 outputs) and, for the reductions, the large cases of tests/objective_shapes.py (257 outputs, 1 161 / 1 157 workgroups).
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r23_peak_strain.txt): 3.3e-14 for a gradient
leaf (quads, T x n = 8 x 32, p-norm, k_bond) and 1.7e-14 in case 1 (kagome, stage launches, p-norm, state0), with value 8.7e-16 and peak 8.2e-16
over the sweep forms; 1.3e-14 end to end against the oracle (k_bond; value 1.8e-15); 8.7e-16 against the host restatement; 0 for the gradients and
2.8e-16 for the value against 2 x the strain-energy entry; 8.1e-15 on the large cases (late tau, fn_params), 2.4e-15 for the one-hot values; 1.4e-15
for the sharp softmax; 1.2e-8 for the directional derivatives against central differences."""
import math

import numpy as np
import pytest
import torch

from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import objective_shapes as OS
from . import peak_strain_cases as PC
from .common import Case, relerr
from .peak_strain_yardstick import aggregate, hard_peak, measure
from .strain_yardstick import T64, bond_energies
from .test_gpu_objective import BATCH, FAST, FOCUS_KW, PATHS, SPI, TAU, TS, Ensemble, _spin_damping, _with_env
from .test_gpu_strain_objective import ALL, DESIGN, TOL_GRAD, TOL_VALUE, bonds_of_block, leaves_of

pytestmark = pytest.mark.gpu


def host(out):
    return {k: np.array(v) for k, v in out.items()}


def yardstick(eng, c, cps, fields, coef, bw, tau, cases, which, model="nonlinear", single_pair=False):
    """For every (aggregate, sharpness) of ``cases``: ((J, peak, peak_at), raw reference gradients): dfx_adjoint on the autograd cotangent
    + the autograd explicit terms.  The graph of q is built once per member.  ``single_pair``: J is q at the hard maximum alone."""
    fields = np.asarray(fields, dtype=float)
    if fields.ndim == 4:
        fields = fields[None]
    B, T = fields.shape[:2]
    nbd = len(c.bonds)
    coef = np.broadcast_to(coef, (B, nbd, 3))
    bw = np.broadcast_to(np.ones(nbd) if bw is None else bw, (B, nbd))
    tau = np.ones(T) if tau is None else np.asarray(tau, dtype=float)
    vals = [(np.zeros(B), np.zeros(B), np.zeros((B, 2), dtype=np.int32)) for _ in cases]
    fbs = [np.zeros_like(fields) for _ in cases]
    explicit = [[] for _ in cases]
    for m in range(B):
        lv = leaves_of(c, cps, m)
        u, cnv, refv = T64(fields[m, :, 0], True), T64(lv["cnv"], True), T64(lv["refv"], True)
        q = measure(u, cnv, c.bonds, refv, T64(coef[m]), model)
        qh, at = hard_peak(q.detach().numpy(), tau[:, None] * bw[m][None, :])
        for i, (agg, sharp) in enumerate(cases):
            J = q[at] if single_pair else aggregate(q, bw[m], tau, agg, sharp)
            gu, gc, gr = torch.autograd.grad(J, [u, cnv, refv], allow_unused=True, retain_graph=True)
            vals[i][0][m], vals[i][1][m], vals[i][2][m] = J.item(), qh, at
            fbs[i][m, :, 0] = gu.numpy()
            explicit[i].append((gc.numpy(), np.zeros_like(lv["refv"]) if gr is None else gr.numpy()))
    out = []
    for i in range(len(cases)):
        ref, _ = eng.adjoint(fbs[i], which=which)
        ref = {k: np.array(v) for k, v in ref.items()}
        for m, (gc, gr) in enumerate(explicit[i]):
            ref["centroid_node_vectors"][m] += gc
            if "reference_vector" in ref:
                ref["reference_vector"][m] += gr
        out.append((vals[i], ref, fbs[i]))
    return out


def compare(tag, res, out, val, ref, tol=TOL_GRAD, tol_value=TOL_VALUE):
    """res = (J, peak, peak_at) of the device, val the yardstick's"""
    assert np.array_equal(res[2], val[2]), (tag, res[2], val[2])
    worst = {"value": float(np.abs(res[0] - val[0]).max() / np.abs(val[0]).max()), "peak": float(np.abs(res[1] - val[1]).max() / np.abs(val[1]).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[peak strain] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= (tol_value if k in ("value", "peak") else tol)}
    assert not bad, (tag, bad)
    return worst


def sharpness_cases(c, cps, fields, coef, bw, tau, model="nonlinear"):
    """[("ks", beta from the data), ("pnorm", 6)] with the range of beta q_hat asserted"""
    tau = np.ones(np.asarray(fields).shape[-4]) if tau is None else tau
    pairs = PC.weighted_pairs(PC.measure(c, cps, fields, coef, model), np.ones(len(c.bonds)) if bw is None else bw, tau)
    qhat = np.array([p[0] for p in pairs])
    beta = PC.choose_beta(qhat)
    assert (qhat > 0).all() and PC.in_range(beta, qhat), (beta, qhat)
    return [("ks", beta), ("pnorm", PC.P_NORM)]


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib, cpu_lib):
    e = Ensemble(request.param)
    e.coef, e.bw, e.special = PC.small_inputs(e.c)
    # the premises of these cases are checked on the CPU port (tests/test_peak_strain_host.py) on PC.cpu_ensemble, which repeats the
    # constructor of Ensemble on another library: the two must describe the same members
    twin = PC.cpu_ensemble(request.param, cpu_lib)
    assert all(np.array_equal(PC.cnv_of(a), PC.cnv_of(b)) for a, b in zip(e.cps, twin.cps)) and np.array_equal(e.cen, twin.cen)
    assert np.array_equal(e.inertia, twin.inertia) and np.array_equal(e.c.bonds, twin.c.bonds) and np.array_equal(e.c.con, twin.c.con)
    assert all(a.constraint_params == b.constraint_params for a, b in zip(e.cps, twin.cps))
    assert e.c.contact_params == twin.c.contact_params
    return e


# ---- 1. the device entry against the yardstick on every form of the sweep ------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    """Case 1: every leaf, both aggregates, five sweep forms; per-member coefficients and bond weights (most bonds at zero; a bond on the
    driven block, one on a clamped block, one on a corner block), tau with a zero and a non-integer entry."""
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(ens.solve(spi))
        st_f = dict(c.solver.stats)
        cases = sharpness_cases(c, ens.cps, fields, ens.coef, ens.bw, TAU)
        refs = yardstick(eng, c, ens.cps, fields, ens.coef, ens.bw, TAU, cases, ALL)
        res = []
        for (agg, sharp), (val, ref, fb) in zip(cases, refs):
            r, out, _ = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, sharp, which=ALL)
            out = host(out)
            r_d, out_d, st = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, sharp, which=DESIGN)
            out_d = host(out_d)
            only = eng.strain_peak_value(ens.coef, ens.bw, TAU, agg, sharp)
            res.append((agg, sharp, val, ref, fb, r, out, r_d, out_d, st, only))
        return st_f, res
    st_f, res = _with_env(env, run)
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    for agg, sharp, val, ref, fb, r, out, r_d, out_d, st, only in res:
        tag = f"{c.geo.__class__.__name__} {path} {agg} sharpness={sharp:.4g}"
        if path == "stage-launches":
            assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
        elif path == "persistent":
            assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
        elif path == "stages":
            assert st["stage_checkpoint"] == 1, st
        elif path == "segments":
            assert st["checkpoint_records"] == 2, st
        assert all(np.array_equal(a, b) for a, b in zip(only, r)) and all(np.array_equal(a, b) for a, b in zip(r_d, r))     # one reduction on one history
        assert set(out) == set(ALL) and set(out_d) == set(DESIGN), (tag, sorted(out))
        npb = c.geo.n_npb
        for b in ens.special:                                                     # the weighted set reaches the driven, the clamped and the corner block
            assert np.abs(fb[:, :, 0, np.asarray(c.bonds)[b] // npb]).max() > 0
        assert not fb[:, :, 1].any() and not fb[:, 0].any()                       # no velocity cotangent; tau[0] = 0
        assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["reference_vector"]).max() > 0
        compare(tag, r, out, val, ref)
        compare(tag + " (design leaves)", r_d, out_d, val, {k: ref[k] for k in DESIGN})


# ---- 2. end to end against the oracle alone ------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_oracle(hip_lib):
    """Case 2: quads 4x4 with contact, 3 outputs, batch 1: autograd through the oracle's fixed-grid solve and ITS bond energies against the
    device entry mapped onto the ControlParams leaves; the engine's history is not shared with the yardstick.  Bar: the suite's 1e-9 for
    discrete-adjoint gradients.  No weighted bond on the driven block (its prescribed output would add a direct drive term that the raw
    fn_params leave to the caller)."""
    from oracle import ref_dynamics as OD
    from oracle import ref_energy as OE
    c = Case("quads", 4, True, True, seed=47, cutoff_deg=42.0, per_bond_k=True)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    ts, spi = np.linspace(0.0, 3e-4, 3), 4
    nb, nbd, npb = c.geo.n_blocks, len(c.bonds), c.geo.n_npb
    driven = int(c.con[0, 0])
    rng = np.random.default_rng(3)
    free_bonds = [b for b in range(nbd) if b not in set(bonds_of_block(c.bonds, npb, driven))]
    w = np.zeros(nbd)
    pick = [int(bonds_of_block(c.bonds, npb, 0)[0])] + [int(b) for b in rng.permutation(free_bonds)[:5]]
    w[pick] = rng.uniform(0.25, 2.0, len(pick))
    coef = PC.coefficients(5, 1, nbd)[0]
    tau = np.array([0.0, 0.37, 1.0])
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = np.array(_with_env({}, lambda: s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi)))
    (agg, beta), _ = sharpness_cases(c, c.cp, fields, coef, w, tau)
    spec = O.PeakStrainSpec(coef, w, tau, agg, beta)
    (obj, peak, at), raw = s.peak_strain_value_and_raw(spec, which=s.engine.ALL_GRADS)
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
    ct = T64(coef)
    rows = []
    for k, t in enumerate(ts):
        u = torch.zeros(nb * 3, dtype=torch.float64)
        u = u.index_put((free,), hist[k, 0]).index_put((con,), drive(float(t), lv["amplitude"], lv["loading_rate"], lv["input_delay"]))
        nd = OE.block_to_node_kinematics(u.reshape(nb, 3), lv["cnv"]).reshape(-1, 3)
        rows.append(2.0 * bond_energies("nonlinear", (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]]), lv["refv"], ct[:, 0], ct[:, 1], ct[:, 2], (1.0, 1.0, 1.0)))
    q = torch.stack(rows)
    J = aggregate(q, w, tau, agg, beta)
    qh, where = hard_peak(q.detach().numpy(), tau[:, None] * w[None, :])
    og = dict(zip(names, torch.autograd.grad(J, [lv[k] for k in names])))
    bp, cpar = tree.mechanical_params.bond_params, tree.mechanical_params.contact_params
    errs = {"value": abs(obj[0] - J.item()) / abs(J.item()), "peak": abs(peak[0] - qh) / qh,
            "centroid_node_vectors": relerr(tree.geometrical_params.centroid_node_vectors, og["cnv"].numpy()),
            "k_bond": relerr(np.stack([bp.k_stretch, bp.k_shear, bp.k_rot], 1), np.stack([og[k].numpy() for k in ("ks", "ksh", "kr")], 1)),
            "reference_vector": relerr(bp.reference_vector, og["refv"].numpy()),
            "contact": relerr([cpar.min_angle, cpar.cutoff_angle, cpar.k_contact], [og[k].item() for k in ("min_angle", "cutoff_angle", "k_contact")]),
            "fn_params": relerr([tree.constraint_params[k] for k in FAST], [og[k].item() for k in FAST])}
    print("[peak strain] end to end against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert tuple(at[0]) == where and abs(J.item()) > 0 and all(np.abs(og[k].numpy()).max() > 0 for k in names)
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad


# ---- 3. the value-only call against the host restatement ----------------------------------------------------------------------------------
def test_value_only_call_equals_the_host_restatement(ens):
    """Case 3: after a forward pass WITHOUT a kept trajectory: J, peak and peak_at of objective.host_peak_strain_value on the downloaded
    fields.  Members 0 and 1 get identical designs: they report the same bits.  A tie of the maximum: tau = e_0 picks the state at rest,
    where every q of the quads is 0 -- peak_at is (0, lowest watched bond); a tie over outputs as well: test_state_at_rest."""
    eng, c = ens.c.solver.engine, ens.c
    cps = [ens.cps[0], ens.cps[0], ens.cps[2]]
    coef, bw = ens.coef.copy(), ens.bw.copy()
    coef[1], bw[1] = coef[0], bw[0]
    refv = np.broadcast_to(c.refv, (len(c.bonds), 2))

    def run():
        fields = np.array(c.solver(np.zeros((2, ens.nb, 3)), TS, cps, keep_trajectory=False, steps_per_interval=SPI))
        cases = sharpness_cases(c, cps, fields, coef, bw, TAU)
        res = [eng.strain_peak_value(coef, bw, TAU, agg, sharp) for agg, sharp in cases]
        rest = [eng.strain_peak_value(coef, bw, np.eye(len(TS))[0], agg, sharp) for agg, sharp in cases]
        with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
            eng.strain_peak_value_and_grad(coef, bw, TAU, which=DESIGN)
        return fields, cases, res, rest
    fields, cases, res, rest = _with_env({}, run)
    for (agg, sharp), (J, peak, at), (J0, peak0, at0) in zip(cases, res, rest):
        Jh, ph, ath = O.host_peak_strain_value(O.PeakStrainSpec(coef, bw, TAU, agg, sharp), fields, PC.cnv_of(cps), c.bonds, refv)
        e_v, e_p = float(np.abs(J - Jh).max() / np.abs(Jh).max()), float(np.abs(peak - ph).max() / np.abs(ph).max())
        print(f"[peak strain] {c.geo.__class__.__name__} value-only call against the host, {agg}: value {e_v:.2e}, peak {e_p:.2e}, at {at.tolist()}")
        assert e_v <= TOL_VALUE and e_p <= TOL_VALUE and np.array_equal(at, ath) and at.dtype == np.int32
        assert J[0] == J[1] and peak[0] == peak[1] and np.array_equal(at[0], at[1])
        # output 0 holds the state at rest.  Where every q is exactly 0 there (quads: reference vectors and node positions cancel bit for
        # bit) the maximum is a tie over all watched bonds and the lowest one takes it; the kagome's q at rest is rounding noise (1e-35)
        assert (at0[:, 0] == 0).all() and peak0.max() < 1e-30 and np.array_equal(at0[0], at0[1])
        if not peak0.any():
            lowest = [int(np.nonzero(bw[m])[0][0]) for m in range(BATCH)]
            assert np.array_equal(at0, [[0, b] for b in lowest]), (at0, lowest)
        Jr = O.peak_of_measure(O.PeakStrainSpec(coef, bw, np.eye(len(TS))[0], agg, sharp), np.zeros((BATCH, len(TS), len(c.bonds))))[0]
        assert np.abs(J0 - Jr).max() <= 4 * np.spacing(np.abs(Jr).max()) + 1e-30


# ---- 4. p = 1 is twice the strain energy ------------------------------------------------------------------------------------------------------
def test_p_equal_one_is_twice_the_strain_energy_entry(ens):
    """Case 4: with coef_b = parts x k_b the p-norm with p = 1 is 2 x dfx_strain_objective_value_and_grad (parts with c_contact = 0) -- the
    parent's tested path as a second yardstick -- on the value and the DESIGN leaves, to 1e-12.  k_bond is excluded: the strain-energy
    objective depends on the stiffnesses explicitly, whereas the coefficients of the peak measure are constants of the call."""
    eng, c = ens.c.solver.engine, ens.c
    parts = (1.0, 0.5, 2.0, 0.0)
    nbd = len(c.bonds)
    k = np.stack([np.broadcast_to(np.asarray(x, dtype=float), (nbd,)) for x in (c.ks, c.ksh, c.kr)], 1)
    coef = k * np.array(parts[:3])

    def run():
        ens.solve(SPI)
        (J, peak, at), out, _ = eng.strain_peak_value_and_grad(coef, ens.bw, TAU, "pnorm", 1.0, which=DESIGN)
        out = host(out)
        obj, ref, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=DESIGN)
        return J, out, obj.copy(), host(ref)
    J, out, obj, ref = _with_env({}, run)
    worst = {"value": float(np.abs(J - 2 * obj).max() / np.abs(2 * obj).max())}
    worst.update({n: relerr(out[n], 2 * ref[n]) for n in DESIGN})
    print(f"[peak strain] {c.geo.__class__.__name__} p = 1 against 2 x the strain-energy entry: " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    assert np.abs(obj).min() > 0 and all(np.abs(ref[n]).max() > 0 for n in DESIGN if n != "void_angle0")
    assert all(v <= 1e-12 for v in worst.values()), worst


# ---- 5. models -------------------------------------------------------------------------------------------------------------------------------------
def _single_case_check(tag, c, model, which, seed):
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    coef, w, _ = PC.small_inputs(c, seed=seed, members=1)
    eng = c.solver.engine
    nb = c.geo.n_blocks

    def run():
        fields = np.array(c.solver(np.zeros((2, nb, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI))
        lv = leaves_of(c, c.cp, 0)
        u = T64(fields[:, 0])
        q = measure(u, T64(lv["cnv"]), c.bonds, T64(lv["refv"]), T64(coef[0]), model).numpy()
        qhat = hard_peak(q, TAU[:, None] * w[0][None, :])[0]
        cases = [("ks", PC.choose_beta([qhat])), ("pnorm", PC.P_NORM)]
        assert qhat > 0 and PC.in_range(cases[0][1], [qhat])
        refs = yardstick(eng, c, c.cp, fields, coef[0], w[0], TAU, cases, which, model)
        res = []
        for (agg, sharp), (val, ref, _) in zip(cases, refs):
            r, out, _ = eng.strain_peak_value_and_grad(coef[0], w[0], TAU, agg, sharp, which=which)
            res.append((agg, val, ref, r, host(out)))
        return res
    worst = {}
    for agg, val, ref, r, out in _with_env({}, run):
        assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(val[0]).max() > 0
        worst[agg] = compare(f"{tag} {agg}", r, out, val, ref)
    return worst


def test_linearised_ligaments(hip_lib):
    _single_case_check("linearised ligaments, quads 4x4 with contact", Case("quads", 4, False, True, seed=51, cutoff_deg=42.0), "linearized", ALL, 31)


def test_per_bond_stiffnesses_and_a_dictionary_of_reference_vectors(hip_lib):
    c = Case("kagome", 4, True, True, seed=52, cutoff_deg=125.0, per_bond_k=True)
    assert len(np.unique(np.round(np.broadcast_to(c.refv, (len(c.bonds), 2)), 12), axis=0)) > 1
    _single_case_check("per-bond stiffnesses, kagome 4x4", c, "nonlinear", ALL, 32)


@pytest.mark.parametrize("model", ["simple", "torsion"])
def test_spring_models(hip_lib, model):
    """a part the model does not have contributes nothing (the shear coefficient, and for the simple spring the bending one, are arbitrary)"""
    from .test_spring_models import SpringCase
    c = SpringCase(model, None)
    c.contact = False
    which = ("centroid_node_vectors", "inertia", "state0", "fn_params", "reference_vector", "k_bond")
    worst = _single_case_check(f"{model} spring, quads 4x4", c, {"simple": "simple_spring", "torsion": "stretch_torsion"}[model], which, 33)
    assert all(set(w) == set(which) | {"value", "peak"} for w in worst.values())


# ---- 6. edges of the reduction -------------------------------------------------------------------------------------------------------------------
def test_state_at_rest(hip_lib):
    """q = 0 everywhere (no drive, no contact, zero initial state): KS gives log(sum W) / beta (dyadic weights: the sum is exact in any
    order; its logarithm is the one inexact step, and the device's math library is specified to 1 ulp, not to libm's bits: 4 ulp of slack --
    and EXACTLY with weights that add up to 1, where S = 1 and log(1) = 0 in every library), the p-norm gives 0, every gradient is zero and
    nothing is NaN.
    The maximum is a tie over every watched bond at every weighted output: peak_at is (lowest output with tau > 0, lowest watched bond)."""
    c = Case("quads", 4, True, False, seed=5)
    c.cp = c.cp._replace(constraint_params=dict(FAST, amplitude=0.0))
    nbd = len(c.bonds)
    w = np.zeros(nbd)
    w[[1, 4, 9, 17]] = [0.5, 1.0, 2.0, 0.25]
    tau = np.array([0.0, 1.0, 0.5, 2.0, 1.0])
    coef = PC.coefficients(2, 1, nbd)[0]
    eng = c.solver.engine

    def run():
        fields = np.array(c.solver(np.zeros((2, 16, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI))
        res = {}
        for agg, sharp in (("ks", 3.0), ("pnorm", 4.0)):
            r, out, _ = eng.strain_peak_value_and_grad(coef, w, tau, agg, sharp, which=ALL)
            res[agg] = (r, host(out))
        wx = np.zeros(nbd)
        wx[[1, 4, 9, 17]] = [0.125, 0.125, 0.25, 0.5]
        exact = eng.strain_peak_value(coef, wx, np.array([0.0, 0.0, 0.5, 0.0, 0.5]), "ks", 3.0)          # sum W = 1, every product dyadic
        return fields, res, exact
    fields, res, exact = _with_env({}, run)
    assert not fields.any()
    (J, peak, at), out = res["ks"]
    ref = math.log(3.75 * 4.5) / 3.0
    print(f"[peak strain] at rest: KS {J[0]!r} against log(sum W) / beta {ref!r}")
    assert abs(J[0] - ref) <= 4 * np.spacing(ref) and peak[0] == 0.0 and tuple(at[0]) == (1, 1)
    assert all(np.isfinite(a).all() and not a.any() for a in out.values())
    (J, peak, at), out = res["pnorm"]
    assert J[0] == 0.0 and peak[0] == 0.0 and tuple(at[0]) == (1, 1)
    assert all(np.isfinite(a).all() and not a.any() for a in out.values())
    # weights that add up to 1: S = 1 and log(1) = 0 in every math library, so here the KS value is EXACTLY log(sum W) / beta = 0
    assert exact[0][0] == 0.0 and exact[1][0] == 0.0 and tuple(exact[2][0]) == (2, 1)


def test_rest_state_tie_goes_through_many_workgroups(hip_lib):
    """The lowest-key tie rule across workgroups and through k_strain_peak_finish: quads 17x17 without contact and without a drive, zero
    initial state, 257 outputs -- 74 273 items in 1 161 workgroups, every q exactly 0.  With tau = 0 on the first 100 outputs and the first 7
    bonds unwatched every workgroup from output 100 on reports the same maximum; peak_at must be (100, 7)."""
    c = Case("quads", OS.SIZES["quads"], True, False, seed=5)
    c.cp = c.cp._replace(constraint_params=dict(OS.GENTLE, amplitude=0.0))
    nbd = len(c.bonds)
    bw, tau = np.ones(nbd), np.ones(OS.N_OUT)
    bw[:7], tau[:100] = 0.0, 0.0
    assert OS.chunks(OS.N_OUT * len(OS.strain_blocks(c.bonds, c.geo.n_npb, bw)), OS.ITEMS_QUAD) > 1000
    coef = PC.coefficients(2, 1, nbd)[0]
    eng = c.solver.engine

    def run():
        fields = np.array(c.solver(np.zeros((2, c.geo.n_blocks, 3)), OS.TS, c.cp, keep_trajectory=False, steps_per_interval=OS.SPI))
        return fields, [eng.strain_peak_value(coef, bw, tau, agg, sharp) for agg, sharp in (("ks", 2.0), ("pnorm", 3.0))]
    fields, res = _with_env({}, run)
    assert not fields.any()
    for J, peak, at in res:
        assert peak[0] == 0.0 and tuple(at[0]) == (100, 7), at
    assert abs(res[0][0][0] - math.log(157.0 * (nbd - 7)) / 2.0) <= 4 * np.spacing(math.log(157.0 * (nbd - 7)) / 2.0) and res[1][0][0] == 0.0


def test_sharp_softmax_is_the_single_pair(hip_lib):
    """beta = 800 / (q_hat - second largest q): every pi but one underflows to 0 and the gradient is that of q at (k_hat, b_hat) alone,
    formed by the yardstick, to the bar of the other cases; J = q_hat + log(W_hat) / beta."""
    ens = Ensemble("quads")
    coef, bw, _ = PC.small_inputs(ens.c)
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(ens.solve(SPI))
        pairs = PC.weighted_pairs(PC.measure(c, ens.cps, fields, coef), bw, TAU)
        beta = PC.sharp_beta(pairs)
        (val, ref, _), = yardstick(eng, c, ens.cps, fields, coef, bw, TAU, [("ks", beta)], ALL, single_pair=True)
        r, out, _ = eng.strain_peak_value_and_grad(coef, bw, TAU, "ks", beta, which=ALL)
        return pairs, beta, val, ref, r, host(out)
    pairs, beta, val, ref, r, out = _with_env({}, run)
    assert min((p[0] - p[1]) / p[0] for p in pairs) > 1e-3
    W = np.array([TAU[k] * bw[m, b] for m, (k, b) in enumerate(val[2])])
    val = (val[1] + np.log(W) / beta, val[1], val[2])
    compare(f"sharp softmax, beta {beta:.4g}", r, out, val, ref)


def test_one_pair_is_its_own_peak(ens):
    """one weighted bond at one output time with W = 1: J = q exactly, for both aggregates"""
    eng, c = ens.c.solver.engine, ens.c
    b = ens.special[2]
    w, tau = np.zeros(len(c.bonds)), np.zeros(len(TS))
    w[b], tau[3] = 1.0, 1.0

    def run():
        fields = np.array(ens.solve(SPI))
        return fields, [eng.strain_peak_value(ens.coef, w, tau, agg, sharp) for agg, sharp in (("ks", 0.3), ("pnorm", 5.0))]
    fields, res = _with_env({}, run)
    q = PC.measure(c, ens.cps, fields, ens.coef)[:, 3, b]
    for J, peak, at in res:
        assert np.array_equal(J, peak) and np.array_equal(at, [[3, b]] * BATCH) and (peak > 0).all()
        assert np.abs(peak - q).max() <= TOL_VALUE * np.abs(q).max()


# ---- 7. many workgroups ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["quads", "kagome"])
def big(request, hip_lib):
    L = OS.LargeCase(request.param)
    cnt, wg, _ = L.counts()
    assert wg["k_strain_objective"] > 1000 and (OS.N_OUT * cnt["n_act_strain"]) % OS.ITEMS_QUAD != 0      # the peak kernels share that grid
    L.coef, L.pw, L.ptau = PC.large_inputs(L)
    return L


def test_peak_across_many_workgroups(big):
    """257 outputs, more than 1 000 workgroups and more than 256 partials (the finish loops make a second trip): both aggregates with the
    case's tau, KS with the late tau (the argmax in the last third of the items), against the yardstick; then tau = e_k at the outputs
    of OS.ONE_HOT, which moves the argmax across workgroup boundaries, against the host's reduction of the yardstick's q."""
    L, eng, c = big, big.c.solver.engine, big.c
    env, spi = dict(DFX_CHECKPOINT="records"), OS.SPI
    late = PC.late_tau(L.ptau)

    def run():
        fields = L.solve(spi)
        assert np.isfinite(fields).all()
        cases = sharpness_cases(c, L.cps, fields, L.coef, L.pw, L.ptau)
        refs = yardstick(eng, c, L.cps, fields, L.coef, L.pw, L.ptau, cases, ALL)
        res = []
        for (agg, sharp), (val, ref, _) in zip(cases, refs):
            r, out, _ = eng.strain_peak_value_and_grad(L.coef, L.pw, L.ptau, agg, sharp, which=ALL)
            res.append((f"{agg} sharpness={sharp:.4g}", val, ref, r, host(out)))
        (lagg, lbeta), _ = sharpness_cases(c, L.cps, fields, L.coef, L.pw, late)
        (val, ref, _), = yardstick(eng, c, L.cps, fields, L.coef, L.pw, late, [(lagg, lbeta)], DESIGN)
        r, out, _ = eng.strain_peak_value_and_grad(L.coef, L.pw, late, lagg, lbeta, which=DESIGN)
        res.append((f"late tau, ks sharpness={lbeta:.4g}", val, ref, r, host(out)))
        hot = {k: eng.strain_peak_value(L.coef, L.pw, np.eye(OS.N_OUT)[k], "ks", cases[0][1]) for k in OS.ONE_HOT}
        return fields, cases, res, hot
    fields, cases, res, hot = _with_env(env, run)
    for tag, val, ref, r, out in res:
        compare(f"{L.lattice} large {tag}", r, out, val, ref)
        if tag.startswith("late"):
            assert all(3 * item >= 2 * total for item, total in (PC.item_of(L, int(k), int(b)) for k, b in r[2]))
    q = np.stack([measure(T64(fields[m, :, 0]), T64(leaves_of(c, L.cps, m)["cnv"]), c.bonds, T64(leaves_of(c, L.cps, m)["refv"]),
                          T64(L.coef[m])).numpy() for m in range(OS.BATCH)])
    worst = 0.0
    for k, (J, peak, at) in hot.items():
        Jh, ph, ath = O.peak_of_measure(O.PeakStrainSpec(L.coef, L.pw, np.eye(OS.N_OUT)[k], "ks", cases[0][1]), q)
        assert np.array_equal(at, ath) and (at[:, 0] == k).all()
        worst = max(worst, float(np.abs(J - Jh).max() / np.abs(Jh).max()), float(np.abs(peak - ph).max() / np.abs(ph).max()))
    print(f"[peak strain] {L.lattice} large, one-hot tau at {OS.ONE_HOT}: worst value / peak error {worst:.2e}")
    assert worst <= TOL_VALUE


@pytest.mark.parametrize("name", list(OS.SMALL))
def test_items_that_fill_their_workgroups_exactly(ens, name):
    """T x n_act = 256 (four full workgroups of the 64-item kernels, no padded lane), 64 and 65, on the small ensemble."""
    T, n = OS.SMALL[name]
    c, eng = ens.c, ens.c.solver.engine
    lattice = "quads" if c.geo.n_npb == 4 else "kagome"
    blocks, inside = OS.small_blocks(c.bonds, c.geo.n_npb, ens.nb, n, OS.SMALL_CENTRE[lattice])
    rng = np.random.default_rng(13)
    ts = np.linspace(0.0, 1e-4 * (T - 1), T)
    tau = rng.uniform(0.25, 2.0, T)
    tau[0] = 0.0
    bw = np.zeros((BATCH, len(c.bonds)))
    bw[:, inside] = rng.uniform(0.25, 2.0, (BATCH, len(inside)))
    assert len(OS.strain_blocks(c.bonds, c.geo.n_npb, bw)) == n and T * n == {"exactly-256": 256, "exactly-64": 64, "65": 65}[name]
    env, spi = PATHS["stage-launches"]

    def run():
        fields = np.array(c.solver(np.zeros((2, ens.nb, 3)), ts, ens.cps, keep_trajectory=True, steps_per_interval=spi))
        cases = sharpness_cases(c, ens.cps, fields, ens.coef, bw, tau)
        refs = yardstick(eng, c, ens.cps, fields, ens.coef, bw, tau, cases, ALL)
        res = []
        for (agg, sharp), (val, ref, _) in zip(cases, refs):
            r, out, _ = eng.strain_peak_value_and_grad(ens.coef, bw, tau, agg, sharp, which=ALL)
            res.append((agg, val, ref, r, host(out)))                  # (the views are valid until the next call: copied here)
        return res
    for agg, val, ref, r, out in _with_env(env, run):
        compare(f"{lattice} T x n = {T} x {n} {agg}", r, out, val, ref)


# ---- 8. repeatability and hygiene ---------------------------------------------------------------------------------------------------------------
def test_repeatable_device_views_and_nothing_left_behind(ens):
    """The same call twice returns the same bits (J, peak, peak_at and every view); device=True views equal the pinned arrays bit for bit and
    stay valid until the next call; a strain-energy call and a plain vjp on the same solve return what they returned before the peak call."""
    eng, c = ens.c.solver.engine, ens.c
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    parts = (0.0, 0.5, 2.0, 1.5)
    rng = np.random.default_rng(2)

    def run():
        fields = np.array(ens.solve(SPI))
        fb = rng.normal(size=fields.shape)
        (agg, beta), _ = sharpness_cases(c, ens.cps, fields, ens.coef, ens.bw, TAU)
        s0, gs0, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=which)
        s0, gs0 = s0.copy(), host(gs0)
        a0 = host(eng.adjoint(fb, which=which)[0])
        r1, g1, _ = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, beta, which=which)
        g1 = host(g1)
        r2, g2, _ = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, beta, which=which)
        g2 = host(g2)
        r3, g3, _ = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, beta, which=which, device=True)
        only = eng.strain_peak_value(ens.coef, ens.bw, TAU, "pnorm", PC.P_NORM)                 # another entry, not a gradient call: the views stay
        g3 = {k: a.to_host() for k, a in g3.items()}
        with pytest.raises(RuntimeError, match="assembled on the host"):
            eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, agg, beta, which=("reference_vector",), device=True)
        s1, gs1, _ = eng.strain_objective_value_and_grad(ens.bw, TAU, parts, which=which)
        s1, gs1 = s1.copy(), host(gs1)
        a1 = host(eng.adjoint(fb, which=which)[0])
        return s0, gs0, a0, r1, g1, r2, g2, r3, g3, only, s1, gs1, a1
    s0, gs0, a0, r1, g1, r2, g2, r3, g3, only, s1, gs1, a1 = _with_env({}, run)
    assert np.abs(r1[0]).min() > 0 and all(np.abs(g1[k]).max() > 0 for k in ("centroid_node_vectors", "inertia"))
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2)) and all(np.array_equal(g1[k], g2[k]) for k in which)
    assert all(np.array_equal(a, b) for a, b in zip(r1, r3)) and set(g3) == set(which) and all(np.array_equal(g1[k], g3[k]) for k in which)
    assert np.array_equal(only[1], r1[1]) and np.array_equal(only[2], r1[2])
    assert np.array_equal(s0, s1) and all(np.array_equal(gs0[k], gs1[k]) for k in which) and all(np.array_equal(a0[k], a1[k]) for k in which)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(ens):
    eng, c = ens.c.solver.engine, ens.c
    fresh = Case("quads", 4, True, False, seed=3)
    nbd4 = len(fresh.bonds)
    one = np.ones((nbd4, 3))
    with pytest.raises(RuntimeError, match="run forward with keep_trajectory=1 first"):
        fresh.solver.engine.strain_peak_value_and_grad(one)
    with pytest.raises(RuntimeError, match="run forward first"):
        fresh.solver.engine.strain_peak_value(one)
    _with_env({}, lambda: ens.solve(SPI))
    good = eng.strain_peak_value(ens.coef, ens.bw, TAU, "ks", 0.2)

    def bad(arr, at, v):
        a = arr.copy()
        a[at] = v
        return a
    for args, match in [
        ((bad(ens.coef, (1, 3, 2), np.nan), ens.bw, TAU), "non-finite or negative bond coefficient"),
        ((bad(ens.coef, (0, 0, 0), -1.0), ens.bw, TAU), "non-finite or negative bond coefficient"),
        ((ens.coef, bad(ens.bw, (1, ens.special[0]), np.inf), TAU), "non-finite or negative bond weight"),
        ((ens.coef, bad(ens.bw, (2, ens.special[1]), -0.5), TAU), "non-finite or negative bond weight"),
        ((ens.coef, ens.bw, bad(TAU, 1, np.nan)), "non-finite or negative time weight"),
        ((ens.coef, ens.bw, bad(TAU, 2, -1.0)), "non-finite or negative time weight"),
        ((ens.coef, bad(ens.bw, 1, 0.0), TAU), "all weights are zero for member 1"),
        ((ens.coef, ens.bw, np.zeros(len(TS))), "all weights are zero"),
        ((ens.coef, ens.bw, TAU, 2, 1.0), "unknown aggregate 2"),
        ((ens.coef, ens.bw, TAU, "ks", np.nan), "sharpness is not finite"),
        ((ens.coef, ens.bw, TAU, "ks", 0.0), "beta must be positive"),
        ((ens.coef, ens.bw, TAU, "pnorm", 0.5), "p must be at least 1"),
    ]:
        with pytest.raises(RuntimeError, match=match):
            eng.strain_peak_value_and_grad(*args)
        with pytest.raises(RuntimeError, match=match):
            eng.strain_peak_value(*args)
    with pytest.raises(ValueError):
        eng.strain_peak_value(np.ones((len(c.bonds) + 1, 3)))
    with pytest.raises(ValueError):
        eng.strain_peak_value(ens.coef, np.ones(len(c.bonds) + 1))
    # the NULL arguments of the C entries
    import ctypes as C
    lib, h = eng.lib, eng._h
    obj = np.zeros(BATCH)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                         # noqa: E731
    assert lib.dfx_strain_peak_value(h, None, 0, None, 0, None, 0, 1.0, dp(obj), None, None) == 1
    assert b"bond_coef is NULL" in lib.dfx_last_error(h)
    shared = np.ascontiguousarray(ens.coef[0])
    assert lib.dfx_strain_peak_value(h, dp(shared), 0, None, 0, None, 0, 1.0, None, None, None) == 1
    assert b"objective is NULL" in lib.dfx_last_error(h)
    r, out, _ = eng.strain_peak_value_and_grad(ens.coef, ens.bw, TAU, "ks", 0.2, which=("inertia",))      # the handle still answers
    assert all(np.array_equal(a, b) for a, b in zip(r, good)) and np.abs(out["inertia"]).max() > 0
    # a general bond list with extra ligaments
    run = lambda c: c.solver(np.zeros((2, 16, 3)), TS, c.cp, keep_trajectory=True, steps_per_interval=SPI)      # noqa: E731
    ex = Case("quads", 4, True, False, seed=3, extra_bonds=[[1, 6], [9, 14]])
    ex.cp = ex.cp._replace(constraint_params=dict(FAST))
    _with_env({}, lambda: run(ex))
    for call in (ex.solver.engine.strain_peak_value_and_grad, ex.solver.engine.strain_peak_value):
        with pytest.raises(RuntimeError, match="more than one ligament"):
            call(np.ones((len(ex.bonds), 3)))
    # a shared checkpoint that another handle's forward pass has overwritten
    a, c2 = Case("quads", 4, True, False, seed=3), Case("quads", 4, True, False, seed=4)
    for x in (a, c2):
        x.cp = x.cp._replace(constraint_params=dict(FAST))
    c2.solver.engine.share_checkpoint(a.solver.engine)
    _with_env({}, lambda: (run(a), run(c2)))
    with pytest.raises(RuntimeError, match="shared trajectory checkpoint was overwritten"):
        a.solver.engine.strain_peak_value_and_grad(one)
    (v, _, _), _, _ = c2.solver.engine.strain_peak_value_and_grad(one, which=("inertia",))
    assert v[0] > 0


# ---- 10. the problem class -------------------------------------------------------------------------------------------------------------------
def _forward(batch):
    fw = P.QuadsFocusingForward(n1_blocks=6, n2_blocks=6, damping=_spin_damping(36), loaded_side="left", input_shift=0, steps_per_interval=8,
                                batch=batch, **FOCUS_KW)
    fw.setup()
    return fw


LIMITS = (0.02, 0.2, 0.2)          # eps_lim, gamma_lim, kappa_lim: the focusing pulse takes the 6x6 lattice beyond them


def test_peak_ligament_strain_directional_derivatives(hip_lib):
    """Case 10: PeakLigamentStrain.value_and_grad on quads 6x6 for a list of 3 designs (one ensemble): directional derivatives along two
    random design directions against central differences of ``value`` with the relative step 1e-6 and the 1e-6 bar of
    test_target_strain_energy_directional_derivatives; a one-design call equals member 0 of the list call to 1e-13."""
    fw3, fw1 = _forward(3), _forward(1)
    rng = np.random.default_rng(19)
    base = fw1.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    many = P.PeakLigamentStrain(fw3, LIMITS, beta=1.0, target_sizes=((3, 3),), target_shifts=((1, 0),), ends="any")
    assert (many.bond_weights > 0).any() and (many.bond_weights == 0).any() and set(np.unique(many.bond_weights)) == {0.0, 1.0}
    v, g = many.value_and_grad(designs)
    peak, at = np.array(many.last_peak), np.array(many.last_peak_at)
    beta = PC.choose_beta(peak)
    many = P.PeakLigamentStrain(fw3, LIMITS, beta=beta, target_sizes=((3, 3),), target_shifts=((1, 0),), ends="any")
    assert PC.in_range(beta, peak)
    v, g = many.value_and_grad(designs)
    assert v.shape == (3,) and len(g) == 3 and np.array_equal(many.last_peak, peak) and np.array_equal(many.last_peak_at, at)
    assert (v + 1.0 >= peak * (1 - 1e-14)).all() and at.shape == (3, 2)          # J >= q_hat + log(W at the argmax) / beta, W = 1
    assert np.allclose(many.value(designs), v, rtol=1e-13, atol=1e-13 * np.abs(v + 1).max())
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
        print(f"[peak strain] PeakLigamentStrain, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    single = P.PeakLigamentStrain(fw1, LIMITS, beta=beta, target_sizes=((3, 3),), target_shifts=((1, 0),), ends="any")
    v1, g1 = single.value_and_grad(designs[0])
    e_v = abs(v1 - v[0]) / abs(v[0] + 1.0)
    e_g = max(np.abs(a - r).max() / np.abs(r).max() for a, r in zip(g1, g[0]))
    print(f"[peak strain] PeakLigamentStrain, one design against member 0 of the list: value {e_v:.2e}, design gradient {e_g:.2e}")
    assert isinstance(v1, float) and e_v <= 1e-13 and e_g <= 1e-13 and single.last_peak == peak[0] and tuple(single.last_peak_at) == tuple(at[0])
    everywhere = P.PeakLigamentStrain(fw1, LIMITS, beta=beta)                     # no target regions: every ligament is watched
    assert everywhere.bond_weights is None and everywhere.value(designs[0]) >= v1 - 1e-12
    best, logs = P.run_ensemble_optimization(many, designs, 2, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0,
                                             min_edge_length=1.0)
    assert len(best) == 3 and np.allclose([log["objective_values"][0] for log in logs], v, rtol=1e-12)


def test_state_constraint_in_the_nlopt_loop(hip_lib):
    """run_optimization_nlopt(state_constraints=[limit]) for 4 evaluations from a design whose peak utilisation exceeds 1 (the stretch limit
    is 0.95 of the initial design's peak stretch strain): constraints_violation["state"] has one entry per optimisation point -- the
    constraint is evaluated once per distinct point, the points of the objective among them --, and the accepted result satisfies
    J - 1 <= 1e-8 or MMA reports infeasibility (the bookkeeping, not a convergence rate)."""
    fw, fwc = _forward(1), _forward(1)
    x0 = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    probe = P.PeakLigamentStrain(fwc, (1.0, None, None), beta=1.0)
    probe.value(x0)
    limit = P.PeakLigamentStrain(fwc, (0.95 * math.sqrt(probe.last_peak), None, None), beta=20.0)
    c0 = limit.value(x0)
    assert c0 > 0.0 and 1.0 < limit.last_peak < 1.2
    points = []
    inner = limit.value_and_grad
    limit.value_and_grad = lambda d: (points.append(P._flatten_design(d).tobytes()), inner(d))[1]
    objective = P.TargetKineticEnergy(fw, (2, 2), (2, 0))
    asked = []                                                                  # every point at which MMA evaluates the objective
    inner_obj = objective.value_and_grad
    objective.value_and_grad = lambda d: (asked.append(P._flatten_design(d).tobytes()), inner_obj(d))[1]
    prob = P.OptimizationProblem(objective, name="strain-limited")
    best = prob.run_optimization_nlopt(x0, 4, lower_bound=-4.5, upper_bound=4.5, min_void_angle=0.0, min_block_angle=0.0, min_edge_length=1.0,
                                       verbose=False, state_constraints=[limit])
    state = prob.constraints_violation["state"]
    print(f"[peak strain] strain-limited focusing, 4 evaluations: objective {prob.objective_values}, J - 1 {state}, feasible {prob.mma_result.feasible}")
    assert len(prob.objective_values) == len(asked) == 4 and np.isfinite(state).all()
    # one entry per optimisation point: the runs of equal consecutive points that MMA asked the objective at, counted independently of
    # the constraint, are the points of the constraint (MMA evaluates the constraints wherever it evaluates the objective)
    distinct = [a for i, a in enumerate(asked) if i == 0 or a != asked[i - 1]]
    assert points == distinct and len(state) == len(distinct), (len(points), len(distinct), len(state))
    assert len(prob.constraints_violation["angles"]) == len(prob.constraints_violation["edge_lengths"]) >= len(state)
    assert abs(state[0] - c0) <= 1e-12 * (1.0 + c0)                              # the first point is the initial guess
    final = limit.value(best)
    assert final <= 1e-8 or not prob.mma_result.feasible
