"""-m gpu: the hinge-force signal channels (components 9 + 3 node + dof of the dfx_signal_* term lists: include/dfx.h; kernels
k_signal_hinge_channels and the hinge seeds of k_signal_cotangent / k_signal_explicit in difflexmm_amd/csrc/dfx_objective.h) through the
misfit, the projections and the cross-correlation, and the two problem classes on them (TargetCutEnergy, TargetTransmittedForce).

Yardstick (tests/hinge_signal_yardstick.py): tests/signal_yardstick.py's construction with ``autograd.grad(E_h, u, create_graph=True)`` per
listed hinge on the history downloaded from the same kept solve; a second pass of autograd gives the value, ``fields_bar`` and the explicit
terms, and ``dfx_adjoint(fields_bar)`` plus the explicit terms is the reference gradient.  Bars: those of tests/test_gpu_signal_misfit.py
for this construction -- 1e-12 of the largest signal for signal values, value 1e-12, every leaf 1e-11 of its largest entry -- 1e-12 of the
largest entry for the two identities on device values, 1e-9 end to end against the oracle alone, 1e-12 for TargetCutEnergy against the
NumPy sum, 1e-6 with the relative step 1e-6 for its directional derivatives (test_gpu_signal_misfit.py's TargetSignalMisfit case).
Shapes: the Ensemble of test_gpu_objective.py -- quads 6x6 with the angle contact engaged (cutoff 42 deg), kagome 4x4 (a padded fourth
slot), 3 members with different designs, 5 outputs, 4 Dopri5 steps per interval.  The listed hinges are all hinges of the driven block, the
clamped block 0, the corner block that starts the last row and two bonded interior blocks: both hinges of the bond between those two, two hinges of one block
in different signals, the moment component, one signal that mixes a hinge term with a block-force term on the same block and a velocity
term, coefficients of both signs.  T x listed hinges is no multiple of the 64 items of a workgroup of k_signal_hinge_channels and exceeds
one workgroup on the quads.
The hinge components are opt-in (``SignalSpec(..., hinge_channels=True)``, ``engine.hinge_channels``: dfx_signal_hinge_channels); the refusal test
holds a handle that was not asked to the parent's "component 9 out of range".
Every comparison prints its worst case before it asserts; the worst cases seen on an MI355X are in profiles/r24_hinge_signal.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P

from . import objective_shapes as OS
from . import xcorr_yardstick as XY
from .common import Case, relerr
from .hinge_signal_yardstick import HingeGraph, add_explicit, bond_of_hinge, partner_of_hinge
from .model_matrix import ModelCase
from .strain_yardstick import T64
from .test_gpu_objective import BATCH, FAST, PATHS, SPI, TAU, TS, Ensemble, _with_env
from .test_gpu_signal_misfit import ALL, MODEL_NAMES, TOL_GRAD, TOL_SIGNAL, TOL_VALUE, _forward, host, member_leaves

pytestmark = pytest.mark.gpu

ITEMS_PER_WORKGROUP = 64                                  # kHingeThreads
TOL_IDENTITY = 1e-12
NS = 8
OMEGA = np.array([1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 1.0, 1.0])
HS = functools.partial(O.SignalSpec, hinge_channels=True)      # the hinge components are off unless a spec (or the engine) asks for them
PAIRS = [(2, 6), (3, 7), (0, 6)]                          # hinge-carrying signals against velocity signals: the form of TargetCutEnergy


def hinges_of(c, block):
    npb = c.geo.n_npb
    return [(block, n) for n in range(npb) if (np.asarray(c.bonds) == block * npb + n).any()]


def make_terms(c):
    """8 signals over ALL hinges of five blocks -- the driven block, the clamped block 0, the corner block of the last row and two bonded interior
    blocks i1, i2.  0: x and moment of a hinge of the driven block; 1: hinges of the clamped and the corner block, coefficients of both
    signs; 2: a hinge of i1, the block force on i1 and its velocity; 3 and 4: the two hinges of the bond i1 - i2 (y) -- 2 and 3 are two hinges
    of one block in different signals; 5: every other hinge of the five blocks, components in rotation, signs alternating; 6, 7: velocities."""
    nb, npb = c.geo.n_blocks, c.geo.n_npb
    rows = int(round(math.sqrt(nb / (1 if npb == 4 else 2))))
    # (the corner at the start of the last row, on the driven side: within the 5 outputs the pulse does not reach the far corners, whose
    # hinges stay below 1e-3 of the largest force channel)
    driven, clamped, corner = int(c.con[0, 0]), 0, nb - nb // rows
    i1 = 14 if npb == 4 else 11
    hb = {b: hinges_of(c, b) for b in (driven, clamped, corner, i1)}
    interior = lambda b: b not in (driven, clamped, corner) and len(hinges_of(c, b)) == npb                # noqa: E731
    link = next((b, n) for b, n in hb[i1] if interior(partner_of_hinge(c.bonds, npb, b, n)[0]))
    i2, n2 = partner_of_hinge(c.bonds, npb, *link)
    hb[i2] = hinges_of(c, i2)
    other = next(h for h in hb[i1] if h != link)
    hc = lambda h, d: 9 + 3 * h[1] + d                                                      # noqa: E731
    terms = [(0, driven, hc(hb[driven][0], 0), 1.0), (0, driven, hc(hb[driven][0], 2), 0.7),
             (1, clamped, hc(hb[clamped][0], 1), -1.3), (1, corner, hc(hb[corner][0], 2), 0.9), (1, corner, hc(hb[corner][-1], 0), 0.5),
             (2, i1, hc(other, 0), 1.0), (2, i1, 6, -0.4), (2, i1, 3, 1e-3),
             (3, i1, hc(link, 1), 1.0), (4, i2, hc((i2, n2), 1), 0.8),
             (6, i1, 3, 1.0), (7, i1, 4, 1.0)]
    used = {(b, (comp - 9) // 3) for _, b, comp, _ in terms if comp >= 9}
    rest = [h for b in hb for h in hb[b] if h not in used]
    terms[10:10] = [(5, b, hc((b, n), i % 3), (-1.0) ** i * (0.3 + 0.1 * i)) for i, (b, n) in enumerate(rest)]
    listed = sorted({(b, (comp - 9) // 3) for _, b, comp, _ in terms if comp >= 9})
    assert listed == sorted(h for b in hb for h in hb[b])
    return terms, listed, dict(driven=driven, clamped=clamped, corner=corner, i1=i1, i2=i2, link=link, back=(i2, n2), other=other)


def graphs_of(c, leaves, fields, terms, ns, model="nonlinear", by_node=False):
    return [HingeGraph(fields[m], leaves[m], c.bonds, c.geo.n_npb, terms, ns, model, by_node) for m in range(len(leaves))]


def reference(eng, graphs, fn, which=ALL):
    """value (B,), raw reference gradients: dfx_adjoint on the autograd cotangent + the autograd explicit terms.  fn(graph, m) ->
    (J, fields_bar, explicit)."""
    res = [fn(g, m) for m, g in enumerate(graphs)]
    ref, _ = eng.adjoint(np.stack([r[1] for r in res]), which=which)
    return np.array([r[0] for r in res]), add_explicit({k: np.array(v) for k, v in ref.items()}, [r[2] for r in res])


def compare(tag, obj, out, val, ref, tol=TOL_GRAD, tol_value=TOL_VALUE):
    worst = {"value": float(np.abs(obj - val).max() / np.abs(val).max())}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[hinge signal] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= (tol_value if k == "value" else tol)}
    assert not bad, (tag, bad)
    return worst


def xcorr_specs(sig):
    return {"none, lag 0": O.CorrelationSpec(sig, PAIRS, 0, None, "none", "at", 0, None, -2.5e-5),
            "softmax": O.CorrelationSpec(sig, PAIRS, 2, None, "coefficient", "softmax", None, 4.0, -1.0, 0.1, 0.5)}


def families(eng, graphs, terms, ns, targets, omega, tau, basis, W, Ptg, which=ALL):
    """name -> (device value (B,), device gradients, yardstick value, reference gradients) for the misfit, the projection and the two
    cross-correlations, on the kept solve the graphs were built from"""
    eng.hinge_channels = True
    out = {}
    val, ref = reference(eng, graphs, lambda g, m: g.misfit(targets[m], omega, tau), which)
    obj, gr, _ = eng.signal_misfit_value_and_grad(terms, ns, targets, omega, tau, which=which)
    out["misfit"] = (obj.copy(), host(gr), val, ref)
    val, ref = reference(eng, graphs, lambda g, m: g.value_and_grads(basis, W, Ptg[m]), which)
    obj, gr, _ = eng.signal_projection_value_and_grad(terms, ns, basis, W, Ptg, which=which)
    out["projection"] = (obj.copy(), host(gr), val, ref)
    for name, sp in xcorr_specs(HS(terms, ns)).items():
        def one(g, m, sp=sp):
            r = XY.evaluate(g, sp, None)
            return r.J, r.fb, r.explicit
        val, ref = reference(eng, graphs, one, which)
        obj, _, _, gr, _ = eng.signal_xcorr_value_and_grad(terms, ns, sp.pairs, sp.max_lag, None, sp.normalisation, sp.reduce, sp.lag, sp.beta, sp.w_peak,
                                                           sp.w_delay, sp.delay_target, which=which)
        out["xcorr " + name] = (obj.copy(), host(gr), val, ref)
    return out


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    """The ensemble of test_gpu_objective.py with the terms above; per-member targets of every family from the yardstick's signals of a
    first solve, scaled by a random factor per entry (fixed inputs from then on)."""
    e = Ensemble(request.param)
    e.terms, e.listed, e.names = make_terms(e.c)
    e.leaves = [member_leaves(e.c, e.cps, m) for m in range(BATCH)]
    e.fields0 = np.array(_with_env({}, lambda: e.solve(SPI)))
    e.S0 = np.stack([g.signal_values() for g in graphs_of(e.c, e.leaves, e.fields0, e.terms, NS)])
    rng = np.random.default_rng(29)
    e.targets = e.S0 * rng.uniform(0.5, 1.5, e.S0.shape)
    e.basis = O.fourier_basis(TS, [1500.0, 4000.0])[[0, 1, 3]]
    e.W = rng.uniform(0.5, 2.0, (NS, 3)) * np.where(np.arange(NS)[:, None] == 1, -1.0, 1.0)
    e.Ptg = np.einsum("jk,mks->msj", e.basis, e.S0) * rng.uniform(0.5, 1.5, (BATCH, NS, 3))
    return e


def test_the_specification_is_the_one_the_kernels_can_go_wrong_on(ens):
    c, T, nm = ens.c, len(TS), ens.names
    npb = c.geo.n_npb
    blocks = {b for b, _ in ens.listed}
    assert {nm["driven"], nm["clamped"], nm["corner"], nm["i1"], nm["i2"]} == blocks and len(blocks) == 5
    assert nm["driven"] == int(c.con[0, 0]) and nm["clamped"] in set(c.con[:, 0]) and len(hinges_of(c, nm["corner"])) < npb
    assert all(len(hinges_of(c, b)) == (4 if npb == 4 else 3) for b in (nm["i1"], nm["i2"]))                      # interior: every node carries a ligament
    assert partner_of_hinge(c.bonds, npb, *nm["link"]) == nm["back"] and {nm["link"], nm["back"]} <= set(ens.listed)
    sig_of = lambda h: {s for s, b, comp, _ in ens.terms if comp >= 9 and (b, (comp - 9) // 3) == h}              # noqa: E731
    assert sig_of(nm["other"]) == {2} and sig_of(nm["link"]) == {3} and nm["other"][0] == nm["link"][0]           # two hinges of one block, two signals
    assert any(comp >= 9 and (comp - 9) % 3 == 2 for _, _, comp, _ in ens.terms)                                  # the moment
    mixed = [(b, comp) for s, b, comp, _ in ens.terms if s == 2]
    assert [comp >= 9 for _, comp in mixed] == [True, False, False] and {comp for _, comp in mixed[1:]} == {6, 3} and len({b for b, _ in mixed}) == 1
    coefs = [co for *_, comp, co in ens.terms if comp >= 9]
    assert min(coefs) < 0 < max(coefs)
    assert TAU[0] == 0 and any(t != round(t) for t in TAU)
    n_items = len(ens.listed)
    assert (T * n_items) % ITEMS_PER_WORKGROUP != 0, n_items
    if npb == 4:
        assert T * n_items > ITEMS_PER_WORKGROUP


# ---- 1, 2. signal values and the two identities ------------------------------------------------------------------------------------------------
def test_signal_values_and_identities(ens):
    c, eng, npb = ens.c, ens.c.solver.engine, ens.c.geo.n_npb
    blocks = sorted({b for b, _ in ens.listed})
    every = O.SignalSpec.hinge_force([(b, n, d) for b, n in ens.listed for d in range(3)])
    block_force = HS([(3 * i + d, b, 6 + d, 1.0) for i, b in enumerate(blocks) for d in range(3)])
    # one call holds hinge terms and block-force terms on the same blocks: the channel space behind the block channels
    both = HS(every.terms + [(every.n_signals + s, b, comp, co) for s, b, comp, co in block_force.terms])

    def run():
        fields = np.array(ens.solve(SPI))
        return fields, c.solver.signal_values(HS(ens.terms, NS)), c.solver.signal_values(every), c.solver.signal_values(block_force), \
            c.solver.signal_values(both)
    fields, S, H, F, HF = _with_env({}, run)
    assert np.array_equal(fields, ens.fields0)
    assert np.array_equal(HF[..., :every.n_signals], H) and np.array_equal(HF[..., every.n_signals:], F)
    ref = ens.S0
    worst = float(np.abs(S - ref).max() / np.abs(ref).max())
    per = [float(np.abs(S[..., s] - ref[..., s]).max() / np.abs(ref[..., s]).max()) for s in range(NS)]
    print(f"[hinge signal] {c.geo.__class__.__name__}: signal values against the yardstick {worst:.2e} of the largest signal; each signal of its own "
          f"largest entry: " + ", ".join(f"{v:.2e}" for v in per))
    assert all(np.abs(ref[..., s]).max() > 0 for s in range(NS))
    assert worst <= TOL_SIGNAL and max(per) <= 1e-11
    H = H.reshape(BATCH, len(TS), len(ens.listed), 3)
    F = F.reshape(BATCH, len(TS), len(blocks), 3)
    scale = max(np.abs(H).max(), np.abs(F).max())
    share = np.abs(H).max(axis=(0, 1, 3)) / scale
    print(f"[hinge signal] {c.geo.__class__.__name__}: smallest share of a listed hinge in the largest force channel {share.min():.2e}")
    assert share.min() >= 1e-3, dict(zip(ens.listed, share))
    e_sum = max(float(np.abs(sum(H[:, :, i] for i, h in enumerate(ens.listed) if h[0] == b) - F[:, :, j]).max()) for j, b in enumerate(blocks)) / scale
    pairs = [(i, ens.listed.index(partner_of_hinge(c.bonds, npb, *h))) for i, h in enumerate(ens.listed) if partner_of_hinge(c.bonds, npb, *h) in ens.listed]
    e_third = max(float(np.abs(H[:, :, i, :2] + H[:, :, j, :2]).max()) for i, j in pairs) / scale
    print(f"[hinge signal] {c.geo.__class__.__name__}: hinge channels of a block against its block force {e_sum:.2e}, x and y of the two ends of "
          f"{len(pairs) // 2} bonds {e_third:.2e} (of the largest entry)")
    assert len(pairs) >= 2 and e_sum <= TOL_IDENTITY and e_third <= TOL_IDENTITY
    if npb == 4:       # the contact of a listed hinge is active: without k_contact the yardstick's moment channel of some listed hinge changes
        off = [dict(lv, kc=0.0) for lv in ens.leaves]
        S_off = np.stack([g.signal_values() for g in graphs_of(c, off, fields, every.terms, every.n_signals)]).reshape(H.shape)
        active = np.abs(S_off[..., 2] - H[..., 2]).max(axis=(0, 1)) / scale
        print(f"[hinge signal] quads: {int((active > 1e-6).sum())} of {len(ens.listed)} listed hinges with the contact active")
        assert (active > 1e-6).any()


# ---- 3. value and raw gradients of the three families on every form of the sweep ----------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_three_families_equal_autograd_cotangent_through_the_same_sweep(ens, path):
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c

    def run():
        fields = np.array(ens.solve(spi))
        st_f = dict(c.solver.stats)
        graphs = graphs_of(c, ens.leaves, fields, ens.terms, NS)
        return st_f, families(eng, graphs, ens.terms, NS, ens.targets, OMEGA, TAU, ens.basis, ens.W, ens.Ptg)
    st_f, fam = _with_env(env, run)
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    engaged = c.geo.n_npb == 4
    for name, (obj, out, val, ref) in fam.items():
        assert set(out) == set(ALL)
        assert all(np.abs(ref[k]).max() > 0 for k in ALL if engaged or k not in ("void_angle0", "contact")), (name, path)
        compare(f"{c.geo.__class__.__name__} {path} {name}", obj, out, val, ref)


@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_every_bond_model_with_and_without_the_angle_contact(hip_lib, model, contact):
    """Quads 4x4, one member, per-ligament stiffnesses: the three families against the yardstick written with that model's energy."""
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    nbd, p = len(mc.bonds), mc.members[0]
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
    nb = mc.geo.n_blocks
    driven, corner = int(mc.con[0, 0]), nb - 1
    a, b_ = hinges_of(mc, 5)[0], hinges_of(mc, 5)[-1]
    back = partner_of_hinge(mc.bonds, 4, *b_)
    terms = [(0, driven, 9 + 3 * hinges_of(mc, driven)[0][1], 1.0), (0, driven, 9 + 3 * hinges_of(mc, driven)[-1][1] + 2, 0.7),
             (1, 0, 9 + 3 * hinges_of(mc, 0)[0][1] + 1, -1.3), (1, corner, 9 + 3 * hinges_of(mc, corner)[0][1] + 2, 0.9),
             (2, 5, 9 + 3 * a[1], 1.0), (2, 5, 6, -0.4), (2, 5, 3, 1e-3), (3, 5, 9 + 3 * b_[1] + 1, 1.0), (4, back[0], 9 + 3 * back[1] + 1, 0.8),
             (5, 5, 9 + 3 * b_[1] + 2, 0.6), (6, 5, 3, 1.0), (7, 5, 4, 1.0)]
    eng = mc.solver.engine

    def run():
        fields = np.array(mc.solver(np.zeros((2, nb, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))[None]
        graphs = graphs_of(mc, [lv], fields, terms, NS, MODEL_NAMES[model])
        S0 = graphs[0].signal_values()[None]
        rng = np.random.default_rng(3)
        targets = S0 * rng.uniform(0.5, 1.5, S0.shape)
        basis = O.fourier_basis(TS, [1500.0, 4000.0])[[0, 1, 3]]
        Ptg = np.einsum("jk,mks->msj", basis, S0) * rng.uniform(0.5, 1.5, (1, NS, 3))
        eng.hinge_channels = True
        return S0, eng.signal_values(terms, NS), families(eng, graphs, terms, NS, targets, OMEGA, TAU, basis, rng.uniform(0.5, 2.0, (NS, 3)), Ptg)
    S0, Sd, fam = _with_env({}, run)
    tag = f"quads 4x4 {model} contact={contact}"
    e_s = float(np.abs(Sd - S0).max() / np.abs(S0).max())
    print(f"[hinge signal] {tag}: signal values {e_s:.2e}")
    assert e_s <= TOL_SIGNAL
    for name, (obj, out, val, ref) in fam.items():
        assert np.abs(val).max() > 0 and np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
        if contact:
            assert np.abs(ref["contact"]).max() > 0 and np.abs(ref["void_angle0"]).max() > 0
        compare(f"{tag} {name}", obj, out, val, ref)


# ---- 4. end to end against the oracle alone ------------------------------------------------------------------------------------------------------------
def _oracle_misfit(c, lv, hist, osol, ts, terms, ns, targets, omega, tau):
    """J with the oracle's energies on the oracle's history: per-bond energy and the contact penalty on the two void angles of the bond,
    measured on the deformed nodes; a hinge channel is the gradient of that one bond's energy w.r.t. its own block."""
    from oracle import ref_energy as OE
    nb, nbd, npb = c.geo.n_blocks, len(c.bonds), c.geo.n_npb
    free, con = torch.as_tensor(osol.free_DOF_ids), torch.as_tensor(osol.constrained_DOF_ids)
    drive = c.osolver_args["constrained_DOFs_fn"]
    bonds_t = torch.as_tensor(np.asarray(c.bonds), dtype=torch.long)
    J = torch.zeros((), dtype=torch.float64)
    for k, t in enumerate(ts):
        u = torch.zeros(nb * 3, dtype=torch.float64)
        u = u.index_put((free,), hist[k, 0]).index_put((con,), drive(float(t), lv["amplitude"], lv["loading_rate"], lv["input_delay"]))
        v = torch.zeros(nb * 3, dtype=torch.float64).index_put((free,), hist[k, 1]).reshape(nb, 3)
        u = u.reshape(nb, 3)
        nd = OE.block_to_node_kinematics(u, lv["cnv"])
        nodal = (nd.reshape(-1, 3)[bonds_t[:, 0]], nd.reshape(-1, 3)[bonds_t[:, 1]])
        nodes = T64(c.cen)[:, None] + lv["cnv"] + nd[:, :, :2]
        ce = OE.contact_energy(OE.void_angles(nodes, c.bonds), lv["min_angle"], lv["cutoff_angle"], lv["k_contact"])
        e = OE.ligament_energy(nodal, lv["refv"], lv["ks"], lv["ksh"], lv["kr"]) + ce[:nbd] + ce[nbd:]
        F = {}
        S = [None] * ns
        for s, b, comp, coef in terms:
            if comp >= 9 and (b, (comp - 9) // 3) not in F:
                F[(b, (comp - 9) // 3)] = torch.autograd.grad(e[bond_of_hinge(c.bonds, npb, b, (comp - 9) // 3)], u, create_graph=True)[0][b]
            if 6 <= comp < 9 and b not in F:
                F[b] = torch.autograd.grad(e.sum(), u, create_graph=True)[0][b]
            src = u[b, comp] if comp < 3 else v[b, comp - 3] if comp < 6 else F[b][comp - 6] if comp < 9 else F[(b, (comp - 9) // 3)][(comp - 9) % 3]
            S[s] = coef * src if S[s] is None else S[s] + coef * src
        for s in range(ns):
            J = J + 0.5 * tau[k] * omega[s] * (S[s] - targets[k, s]) ** 2
    return J


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_end_to_end_against_the_oracle(hip_lib, lattice):
    """The end-to-end case of test_gpu_signal_misfit.py (4x4 with contact, 3 outputs, batch 1) with hinge terms: autograd through the
    oracle's fixed-grid solve and ITS energies (twice) against the device entry mapped onto the ControlParams leaves.  No hinge on the driven
    block or next to it (the direct drive term of a prescribed output is left to the caller).  Bar 1e-9 (tests/parity.py)."""
    from oracle import ref_dynamics as OD
    from .test_gpu_signal_misfit import neighbours
    quads = lattice == "quads"
    c = Case(lattice, 4, True, True, seed=47, cutoff_deg=42.0 if quads else 125.0, per_bond_k=True)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    ts, spi = (np.linspace(0.0, 3e-4, 3), 4) if quads else (np.linspace(0.0, 1.5e-4, 3), 6)
    nb, nbd, npb = c.geo.n_blocks, len(c.bonds), c.geo.n_npb
    driven = int(c.con[0, 0])
    near = set(neighbours(c, driven)) | {driven}
    blocks = [b for b in ([0, nb - 1, 6] if quads else [0, nb - 1, 9]) if not (set(neighbours(c, b)) | {b}) & {driven}]
    assert len(blocks) >= 2 and not any(b in near for b in blocks)
    h0, h1, h2 = hinges_of(c, blocks[0])[0], hinges_of(c, blocks[1])[-1], hinges_of(c, blocks[-1])[0]
    back = partner_of_hinge(c.bonds, npb, *h2)
    assert back[0] not in near
    free_block = next(b for b in range(5, nb) if b not in near and b not in blocks)
    terms = [(0, h0[0], 9 + 3 * h0[1] + 1, 1.0), (0, h1[0], 9 + 3 * h1[1] + 2, -0.6), (0, h2[0], 9 + 3 * h2[1], 0.8), (1, h2[0], 9 + 3 * h2[1] + 2, 1.0),
             (1, back[0], 9 + 3 * back[1] + 1, 0.5), (1, h2[0], 6, 0.3), (1, free_block, 0, 3.0), (2, free_block, 2, 1.0), (2, free_block, 4, 1e-4)]
    tau, omega = np.array([0.0, 0.37, 1.0]), np.array([1.0, 0.5, 2.0])
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = np.array(_with_env({}, lambda: s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi)))
    assert np.abs(fields[:, 0, :, 2]).max() < 1.0, "rotations beyond 1 rad: not a stable solve"
    targets = s.signal_values(HS(terms, 3))[0] * np.random.default_rng(5).uniform(0.5, 1.5, (3, 3))
    obj, raw = s.signal_misfit_value_and_raw(HS(terms, 3, targets, omega, tau), which=s.engine.ALL_GRADS)
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
    print(f"[hinge signal] {lattice}: end to end against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert abs(J.item()) > 0 and all(np.abs(og[k].numpy()).max() > 0 for k in names if k not in ("min_angle", "cutoff_angle", "k_contact"))
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits(ens):
    eng = ens.c.solver.engine
    eng.hinge_channels = True
    sp = xcorr_specs(HS(ens.terms, NS))["softmax"]

    def run():
        ens.solve(SPI)
        out = []
        for _ in range(2):
            a = eng.signal_misfit_value_and_grad(ens.terms, NS, ens.targets, OMEGA, TAU, which=ALL)
            b = eng.signal_xcorr_value_and_grad(ens.terms, NS, sp.pairs, sp.max_lag, None, sp.normalisation, sp.reduce, sp.lag, sp.beta, sp.w_peak, sp.w_delay,
                                                sp.delay_target, which=ALL)
            out.append((a[0].copy(), host(a[1]), b[0].copy(), host(b[3])))
        return out
    first, second = _with_env({}, run)
    for x, y in zip(first, second):
        if isinstance(x, dict):
            assert set(x) == set(y) == set(ALL) and all(np.array_equal(x[k], y[k]) for k in x) and all(np.abs(x[k]).max() > 0 for k in ("centroid_node_vectors", "k_bond"))
        else:
            assert np.array_equal(x, y) and np.isfinite(x).all()


# ---- 6, 7. the problem classes -----------------------------------------------------------------------------------------------------------------------------
def test_target_cut_energy_value_and_directional_derivatives(hip_lib):
    """TargetCutEnergy on quads 6x6 around the 2x2 region (14, 15, 20, 21) for a list of 3 designs: the value against the NumPy sum
    -dt sum f v over the downloaded hinge signals and velocities (1e-12); directional derivatives along two random design directions against
    central differences of ``value``, relative step 1e-6 and bar 1e-6 (test_gpu_signal_misfit.py's TargetSignalMisfit case);
    TargetTransmittedForce against the NumPy value 1/2 sum tau |resultant|^2 of the downloaded resultants."""
    fw3 = _forward(3)
    rng = np.random.default_rng(19)
    base = fw3.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    designs = [tuple(a + rng.uniform(-0.2, 0.2, a.shape) for a in base) for _ in range(3)]
    inside = [14, 15, 20, 21]
    cut = P.TargetCutEnergy(fw3, inside)
    v, g = cut.value_and_grad(designs)
    sd = fw3.solve_dynamics
    hd = [(b, n, d) for b, n in cut.hinges for d in range(3)]
    assert len(cut.hinges) == 8 and all(b in inside for b, _ in cut.hinges)
    f = sd.signal_values(O.SignalSpec.hinge_force(hd))
    vel = sd.signal_values(O.SignalSpec.fields_of([(b, d) for b, _, d in hd], "velocity"))
    dt = fw3.timepoints[1] - fw3.timepoints[0]
    W = -dt * np.sum(f * vel, axis=(1, 2))
    e_v = float(np.abs(v - W).max() / np.abs(W).max())
    print(f"[hinge signal] TargetCutEnergy: value against -dt sum f v of the downloaded signals {e_v:.2e} (W = {W})")
    assert v.shape == (3,) and len(g) == 3 and np.abs(W).min() > 0 and e_v <= 1e-12
    assert np.array_equal(cut.value(designs), v) and np.array_equal(P.TargetCutEnergy(fw3, inside, sign=-1).value(designs), -v)
    scale = max(np.abs(a).max() for a in base)
    for trial in range(2):
        dirs = [tuple(rng.normal(size=a.shape) for a in base) for _ in range(3)]
        dirs = [tuple(a / max(np.abs(x).max() for x in d) for a in d) for d in dirs]
        h = 1e-6 * scale
        vp = cut.value([tuple(a + h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        vm = cut.value([tuple(a - h * e for a, e in zip(d, dd)) for d, dd in zip(designs, dirs)])
        fd = (vp - vm) / (2 * h)
        mine = np.array([sum(float(np.sum(a * e)) for a, e in zip(gm, dd)) for gm, dd in zip(g, dirs)])
        err = np.abs(mine - fd) / np.abs(fd)
        print(f"[hinge signal] TargetCutEnergy, direction {trial}: directional derivative against central differences {err.max():.2e}")
        assert np.abs(fd).min() > 0 and err.max() < 1e-6
    tau = np.linspace(0.5, 1.5, len(fw3.timepoints))
    tf = P.TargetTransmittedForce(fw3, inside, dofs=(0, 1), tau=tau)
    vt, gt = tf.value_and_grad(designs)
    R = sd.signal_values(O.SignalSpec.cut_force(cut.hinges, (0, 1)))
    want = 0.5 * np.sum(tau[None, :, None] * R ** 2, axis=(1, 2))
    e_t = float(np.abs(vt - want).max() / np.abs(want).max())
    print(f"[hinge signal] TargetTransmittedForce: value against 1/2 sum tau |resultant|^2 of the downloaded resultants {e_t:.2e}")
    assert (want > 0).all() and e_t <= 1e-12 and len(gt) == 3 and all(max(np.abs(a).max() for a in gm) > 0 for gm in gt)
    with pytest.raises(ValueError, match="on_device=True"):
        P.TargetCutEnergy(_forward(1), inside).value(designs[0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_device_side_refusals_name_the_term_and_the_handle_still_answers(ens):
    eng, c = ens.c.solver.engine, ens.c
    T, npb, nb = len(TS), c.geo.n_npb, c.geo.n_blocks
    _with_env({}, lambda: ens.solve(SPI))
    # off (the default of a handle), component 9 is what it was before the channels existed: out of range
    eng.hinge_channels = False
    with pytest.raises(RuntimeError, match="term 0 names component 9 out of range.*dfx_signal_hinge_channels"):
        eng.signal_values([(0, 1, 9, 1.0)], 1)
    assert np.isfinite(eng.signal_values([(0, 1, 8, 1.0)], 1)).all()
    eng.hinge_channels = True
    assert np.abs(eng.signal_values([(0, 1, 9, 1.0)], 1)).max() > 0
    good = eng.signal_misfit_value(ens.terms, NS, ens.targets, OMEGA, TAU)
    bare = next(n for n in range(npb) if (0, n) not in hinges_of(c, 0))                      # the clamped corner block has a node without a ligament
    sp = O.CorrelationSpec(HS([(0, 1, 9, 1.0)]), [(0, 0)], 0)
    calls = (lambda t: eng.signal_values(t, 1), lambda t: eng.signal_misfit_value(t, 1, np.zeros((T, 1))),
             lambda t: eng.signal_misfit_value_and_grad(t, 1, np.zeros((T, 1))), lambda t: eng.signal_projections(t, 1, np.ones((1, T))),
             lambda t: eng.signal_projection_value_and_grad(t, 1, np.ones((1, T)), np.ones((1, 1))),
             lambda t: eng.signal_xcorr(t, 1, sp.pairs, 0), lambda t: eng.signal_xcorr_value_and_grad(t, 1, sp.pairs, 0))
    for call in calls:
        with pytest.raises(RuntimeError, match=f"term 1 names the hinge on node {bare} of block 0, which carries no ligament"):
            call([(0, 1, 0, 1.0), (0, 0, 9 + 3 * bare, 1.0)])
        with pytest.raises(RuntimeError, match="term 0 names component 21 out of range"):
            call([(0, 1, 21, 1.0)])
        if npb == 3:
            with pytest.raises(RuntimeError, match="term 0 names the hinge on node 3 but a block of this lattice has 3 nodes"):
                call([(0, 9, 18, 1.0)])
    with pytest.raises(RuntimeError, match="forward_tangent_signals_multi.*which carries no ligament"):
        eng.forward_tangent_signals_multi(np.zeros((2, nb, 3)), None, None, 1, TS, SPI, [(0, 0, 9 + 3 * bare + 1, 1.0)], 1)
    obj, out, _ = eng.signal_misfit_value_and_grad(ens.terms, NS, ens.targets, OMEGA, TAU, which=("inertia",))      # the handle still answers
    assert np.array_equal(obj, good) and np.abs(out["inertia"]).max() > 0
    one, tg1 = [(0, 5, 9, 1.0)], np.zeros((T, 1))
    # hinge components with the distance-based contact, and on a general bond list with extra ligaments: refused as 6..8 are
    mc = ModelCase("quads", "nonlinear", "distance", 4, "uniform", batch=1)
    mc.solver.engine.hinge_channels = True
    _with_env({}, lambda: mc.solver(np.zeros((2, 16, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
    for call in (lambda: mc.solver.engine.signal_misfit_value_and_grad(one, 1, tg1), lambda: mc.solver.engine.signal_values(one, 1)):
        with pytest.raises(RuntimeError, match="distance-based contact energy is not part of the signal channels"):
            call()
    ex = Case("quads", 4, True, False, seed=3, extra_bonds=[[1, 6], [9, 14]])
    ex.cp = ex.cp._replace(constraint_params=dict(FAST))
    ex.solver.engine.hinge_channels = True
    _with_env({}, lambda: ex.solver(np.zeros((2, 16, 3)), TS, ex.cp, keep_trajectory=True, steps_per_interval=SPI))
    for call in (lambda: ex.solver.engine.signal_misfit_value_and_grad(one, 1, tg1), lambda: ex.solver.engine.signal_values(one, 1)):
        with pytest.raises(RuntimeError, match="more than one ligament"):
            call()


# ---- 9. many workgroups -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_many_workgroups(hip_lib, lattice):
    """The large case of tests/objective_shapes.py (quads 17x17 / kagome 12x12, 2 members, 257 outputs) with ALL hinges of one row of blocks
    listed: the two identities on device values, and the gradient of a misfit on three resultants with a different coefficient per hinge
    against the yardstick in its per-node form (one autograd pass per hinge would take minutes here)."""
    case = OS.LargeCase(lattice)
    c, npb, n = case.c, case.npb, OS.SIZES[lattice]
    per_row = case.nb // n
    row = list(range((n // 2) * per_row, (n // 2 + 1) * per_row))
    listed = [h for b in row for h in hinges_of(c, b)]
    T = OS.N_OUT
    assert T * len(listed) > 100 * ITEMS_PER_WORKGROUP and (T * len(listed)) % ITEMS_PER_WORKGROUP != 0
    rng = np.random.default_rng(13)
    coef = OS.signed(rng, len(listed))
    terms = [(d, b, 9 + 3 * nd + d, float(co * OS.TERM_SCALE[6 + d])) for d in range(3) for (b, nd), co in zip(listed, coef)]
    every = O.SignalSpec.hinge_force([(b, nd, d) for b, nd in listed for d in range(3)])
    block_force = HS([(3 * i + d, b, 6 + d, 1.0) for i, b in enumerate(row) for d in range(3)])
    eng = c.solver.engine
    which = ("centroid_node_vectors", "void_angle0", "inertia", "k_bond", "contact", "fn_params")

    def run():
        fields = case.solve()
        H, F = c.solver.signal_values(every), c.solver.signal_values(block_force)
        graphs = graphs_of(c, case.leaves(), fields, terms, 3, by_node=True)
        eng.hinge_channels = True
        S0 = np.stack([g.signal_values() for g in graphs])
        targets = OS.signal_targets(S0, rng.uniform(0.5, 1.5, S0.shape), rng.choice([-1.0, 1.0], (OS.BATCH, 3)))
        val, ref = reference(eng, graphs, lambda g, m: g.misfit(targets[m], None, case.tau), which)
        obj, out, _ = eng.signal_misfit_value_and_grad(terms, 3, targets, None, case.tau, which=which)
        return H, F, S0, c.solver.signal_values(HS(terms, 3)), val, ref, obj.copy(), host(out)
    H, F, S0, S, val, ref, obj, out = _with_env({}, run)
    H, F = H.reshape(OS.BATCH, T, len(listed), 3), F.reshape(OS.BATCH, T, len(row), 3)
    scale = max(np.abs(H).max(), np.abs(F).max())
    e_sum = max(float(np.abs(sum(H[:, :, i] for i, h in enumerate(listed) if h[0] == b) - F[:, :, j]).max()) for j, b in enumerate(row)) / scale
    pairs = [(i, listed.index(partner_of_hinge(c.bonds, npb, *h))) for i, h in enumerate(listed) if partner_of_hinge(c.bonds, npb, *h) in listed]
    e_third = max(float(np.abs(H[:, :, i, :2] + H[:, :, j, :2]).max()) for i, j in pairs) / scale
    e_s = float(np.abs(S - S0).max() / np.abs(S0).max())
    print(f"[hinge signal] {lattice} large, {len(listed)} hinges x {T} outputs = {-(-T * len(listed) // ITEMS_PER_WORKGROUP)} workgroups: hinge channels of a "
          f"block against its block force {e_sum:.2e}, x and y of the two ends of {len(pairs) // 2} bonds {e_third:.2e}, resultants against the yardstick {e_s:.2e}")
    assert len(pairs) >= 2 * (per_row // 2 - 1) and e_sum <= TOL_IDENTITY and e_third <= TOL_IDENTITY and e_s <= TOL_SIGNAL
    compare(f"{lattice} large", obj, out, val, ref)
