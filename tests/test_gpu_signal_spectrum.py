"""-m gpu: ratios of band powers of the signal projections, evaluated and differentiated on the device (include/dfx.h: dfx_signal_spectrum,
dfx_signal_spectrum_value, dfx_signal_spectrum_value_and_grad; kernels k_signal_spectrum_forms / _reduce / _weights / _residual in
difflexmm_amd/csrc/dfx_objective.h).

Yardstick (tests/spectrum_yardstick.py): the differentiable signals of projection_yardstick.MemberGraph on the history downloaded from the
same kept solve, P, N, D, l and J in torch fp64 (torch.logsumexp for KS); autograd gives ``fields_bar`` and every explicit term, and
``dfx_adjoint(fields_bar)`` plus the explicit terms is the reference gradient, as tests/test_gpu_signal_projection.py builds it.  Bars (same
history, same fp64 arithmetic, another summation order): N and D 1e-12 of their value, J 1e-12 of the sum of the absolute terms entering it
(sum_g |a_g| (|ln N_g| + |ln D_g|) for "log", sum_g |a_g l_g| for "ratio"), every gradient leaf 1e-11 of its largest reference entry.

Every comparison first asserts conditions on its INPUTS, on the yardstick's numbers alone: kappa = sum_k |B_jk S_ks| / |P_sj| <= 50 on every
(member, signal, row) that carries weight; every (signal, row) pair carries weight in at most one (group, side) (one case shares pairs and
asserts sum_g |term| / |Weff_sj| <= 50 instead); for KS beta = sqrt(200 / (smallest spread * largest spread)) of z = a l over the members of
the yardstick, and 5 <= beta * spread <= 40 for every member.  A case whose inputs miss a condition fails: none is skipped.

Shapes: the ensembles of test_gpu_objective.py (quads 6x6 with the angle contact engaged, kagome 4x4, 3 members with different designs), the
4-signal terms of test_gpu_signal_misfit.make_terms (force terms among them), the two time grids and the frequency tables of
test_gpu_signal_projection.py; G = 3 on the 6-row bases (24 pairs; 6 (group, side) waves: no multiple of the 4 of a workgroup), a per-member
d0, a group normalised by d0 alone; on the 70-output grid synthetic bases of 16 and 17 rows of distinct frequencies (SYNTHETIC_ROWS, chosen
on the CPU port's histories: tests/test_signal_spectrum_host.py) for 64 and 65 pairs -- a lane's second term in k_signal_spectrum_forms --
with G = 64 and 65 -- a lane's second group in k_signal_spectrum_reduce -- and G = 1 over all pairs and over one pair.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/spectrum_worst_cases.txt): N 1.2e-14
(quads 4x4, torsion, no contact), D 6.0e-15 (kagome, 5 outputs), J 7.4e-16 of the absolute terms (quads, 70 outputs, 68 pairs, G = 1), l
7.8e-16, gradient leaves 3.9e-14 (kagome, 70 outputs, 68 pairs, G = 65, log / ks, fn_params); the largest kappa of any input 7.2; beta *
spread between 7.6 and 26.3; cancellation in Weff of the shared-pairs case 1.0.  No bar was missed.
A departure from "beta = 10 / spread": one scalar beta serves the three members of an ensemble, whose spreads differ, so beta is the value
that centres the members' beta * spread in the window geometrically (sqrt(200 / (min spread * max spread))); the window 5 .. 40 itself is
asserted per member.  The single-member cases (end to end) use 10 / spread.
The hinge case runs on tests/hinge_signal_yardstick.HingeGraph at the same bars.  End to end against the oracle's own solve (4x4, 3 outputs,
batch 1, bar 1e-9; the case of test_gpu_signal_misfit.py): the figures are in profiles/spectrum_worst_cases.txt.  The problem classes and
DriveWaveformDesign: tests/test_gpu_spectrum_problems.py."""
import numpy as np
import pytest

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O

from . import projection_yardstick as PY
from . import spectrum_yardstick as SY
from .common import relerr
from .model_matrix import ModelCase
from .test_gpu_objective import BATCH, PATHS, SPI, TS, Ensemble, _with_env
from .test_gpu_signal_misfit import ALL, DESIGN, MODEL_NAMES, host, make_terms, member_leaves
from .test_gpu_signal_projection import FREQUENCIES, GRIDS, MODEL_FREQUENCIES, NS, PATH_FREQUENCIES, graphs_of, solve

pytestmark = pytest.mark.gpu

TOL_FORMS, TOL_VALUE, TOL_GRAD = 1e-12, 1e-12, 1e-11
GRID70 = GRIDS["70 outputs"]
# (frequency in Hz, 0: cos row / 1: sin row) of the synthetic 16- and 17-row bases on the 70-output grid: distinct frequencies whose row has
# kappa <= 4.1 (quads) / 4.7 (kagome) for every member and signal on the CPU port's history
SYNTHETIC_ROWS = {
    "quads": [(724.0, 0), (861.0, 0), (1546.0, 1), (1683.0, 1), (2231.0, 0), (2368.0, 1), (2505.0, 1), (2642.0, 1), (2779.0, 1), (2916.0, 1),
              (3053.0, 0), (3190.0, 0), (3327.0, 0), (3464.0, 0), (3601.0, 0), (3738.0, 0), (3875.0, 0)],
    "kagome": [(587.0, 0), (724.0, 0), (1135.0, 0), (1272.0, 0), (1409.0, 0), (1546.0, 0), (1683.0, 0), (2094.0, 1), (2231.0, 1), (2368.0, 1),
               (2505.0, 1), (2642.0, 1), (2779.0, 1), (2916.0, 1), (3053.0, 1), (3190.0, 0), (3327.0, 0)]}


def synthetic_basis(lattice, n_rows):
    return np.stack([O.fourier_basis(GRID70[0], [f])[j] for f, j in SYNTHETIC_ROWS[lattice][:n_rows]])


def three_groups(ns, seed=5):
    """G = 3 on a 6-row basis: group g weighs rows 2g, 2g + 1 of the last two signals in its numerator and of the first signal(s) in its
    denominator; group 2 has no denominator weights (d0 alone).  Non-integer weights; no pair in two (group, side)."""
    rng = np.random.default_rng(seed)
    Wn, Wd = np.zeros((3, ns, 6)), np.zeros((3, ns, 6))
    for g in range(3):
        Wn[g, ns - 2:, 2 * g:2 * g + 2] = rng.uniform(0.5, 2.0, (2, 2))
        if g < 2:
            Wd[g, :ns - 2, 2 * g:2 * g + 2] = rng.uniform(0.5, 2.0, (ns - 2, 2))
    return Wn, Wd


def offsets_for(graphs, B, Wn, Wd, seed=9):
    """per-member offsets on the scale of the yardstick's forms: n0 on group 1, d0 on groups 0 and 2 (group 2: the whole denominator)"""
    rng = np.random.default_rng(seed)
    Gn = len(Wn)
    n0, d0 = np.zeros((len(graphs), Gn)), np.zeros((len(graphs), Gn))
    for m, g in enumerate(graphs):
        P2 = g.projections(B) ** 2
        N, D = np.einsum("gsj,sj->g", Wn, P2), np.einsum("gsj,sj->g", Wd, P2)
        n0[m, 1] = N[1] * rng.uniform(0.1, 0.5)
        d0[m, 0] = D[0] * rng.uniform(0.1, 0.5)
        d0[m, 2] = N[2] * rng.uniform(0.5, 2.0)
    return n0, d0


def check_inputs(tag, graphs, B, Wn, Wd, shared=False):
    S = np.stack([g.signal_values() for g in graphs])
    Pr = np.stack([g.projections(B) for g in graphs])
    k = SY.kappa(B, S, Pr, (Wn.sum(0) + Wd.sum(0)) > 0)
    print(f"[signal spectrum] {tag}: kappa of the inputs {k.max():.1f} (bound {PY.KAPPA_MAX:.0f})")
    assert np.isfinite(k).all() and 0 < k.max() <= PY.KAPPA_MAX, (tag, float(k.max()))
    if not shared:
        assert ((Wn > 0).sum(0) + (Wd > 0).sum(0)).max() == 1, tag
    return float(k.max())


def yardstick(eng, graphs, B, Wn, Wd, n0, d0, a, measure, aggregate, which, tag, shared=False):
    """the yardstick's results per member, beta for KS from its own spread, the reference gradients"""
    n0, d0 = np.broadcast_to(n0, (len(graphs), len(Wn))), np.broadcast_to(d0, (len(graphs), len(Wn)))
    beta = None
    if aggregate == "ks":
        first = [SY.value_and_grads(g, B, Wn, Wd, n0[m], d0[m], a, measure, "sum") for m, g in enumerate(graphs)]
        spread = np.array([np.ptp(np.asarray(a) * r["l"]) for r in first])
        beta = float(np.sqrt(200.0 / (spread.min() * spread.max())))
        print(f"[signal spectrum] {tag}: beta * spread {np.round(beta * spread, 1)}")
        assert (5.0 <= beta * spread).all() and (beta * spread <= 40.0).all(), (tag, beta * spread)
    res = [SY.value_and_grads(g, B, Wn, Wd, n0[m], d0[m], a, measure, aggregate, beta) for m, g in enumerate(graphs)]
    if shared:
        c = max(SY.weff_cancellation(r, Wn, Wd, a, measure, aggregate, beta).max() for r in res)
        print(f"[signal spectrum] {tag}: cancellation in Weff {c:.1f} (bound 50)")
        assert c <= 50.0, (tag, c)
    ref, _ = eng.adjoint(np.stack([r["fb"] for r in res]), which=which)
    ref = {k: np.array(v) for k, v in ref.items()}
    for m, r in enumerate(res):
        g = r["explicit"]
        ref["centroid_node_vectors"][m] += g["cnv"]
        if "void_angle0" in ref and "phi0" in g:
            ref["void_angle0"][m] += g["phi0"]
        if "reference_vector" in ref:
            ref["reference_vector"][m] += g["refv"]
        if "k_bond" in ref:
            ref["k_bond"][m] += np.stack([g["ks"], g["ksh"], g["kr"]], 1)
        if "contact" in ref and "am" in g:
            ref["contact"][m] += np.array([g["am"], g["ac"], g["kc"]])
    return res, beta, ref


def compare(tag, res, ref, forms, J, l, out, kap=None):
    N, D = np.stack([r["N"] for r in res]), np.stack([r["D"] for r in res])
    worst = {"N": float(np.abs(forms[..., 0] / N - 1).max()), "D": float(np.abs(forms[..., 1] / D - 1).max()),
             "J": float(max(abs(J[m] - r["J"]) / r["terms"] for m, r in enumerate(res))),
             "l": float(max(np.abs(l[m] - r["l"]).max() / r["terms"] for m, r in enumerate(res)))}
    for k, a in out.items():
        assert k in ref and a.shape == ref[k].shape, (tag, k, a.shape)
        worst[k] = relerr(a, ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(a).max())
    print(f"[signal spectrum] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + ("" if kap is None else f" (kappa {kap:.1f})"))
    bad = {k: v for k, v in worst.items() if not v <= (TOL_FORMS if k in ("N", "D") else TOL_VALUE if k in ("J", "l") else TOL_GRAD)}
    assert not bad, (tag, bad, kap)
    return worst


def device(eng, terms, ns, B, Wn, Wd, n0, d0, a, measure, aggregate, beta, which):
    forms = eng.signal_spectrum(terms, ns, B, Wn, Wd, n0, d0, measure).copy()
    J, l, out, st = eng.signal_spectrum_value_and_grad(terms, ns, B, Wn, Wd, n0, d0, a, measure, aggregate, beta, which=which)
    J, l, out = J.copy(), l.copy(), host(out)
    Jv, lv = eng.signal_spectrum_value(terms, ns, B, Wn, Wd, n0, d0, a, measure, aggregate, beta)
    assert np.array_equal(Jv, J) and np.array_equal(lv, l, equal_nan=True)              # one reduction on one history
    assert np.array_equal(forms[..., 2], l, equal_nan=True)                              # the measure of the forms entry is the value entry's
    return forms, J, l, out, st


@pytest.fixture(scope="module", params=["quads", "kagome"])
def ens(request, hip_lib):
    e = Ensemble(request.param)
    e.lattice = request.param
    e.terms, e.force_blocks, e.listed = make_terms(e.c)
    e.leaves = [member_leaves(e.c, e.cps, m) for m in range(BATCH)]
    return e


A3 = np.array([1.0, -0.6, 0.8])


# ---- 1. both measures x both aggregates on both lattices and grids ------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_measures_and_aggregates_on_both_grids(ens, grid):
    eng = ens.c.solver.engine
    B = PY.make_bases(GRIDS[grid][0], FREQUENCIES[ens.lattice, grid], NS)["6 rows"][0]
    Wn, Wd = three_groups(NS)
    assert (2 * len(Wn)) % 4 != 0

    def run():
        graphs = graphs_of(ens, np.array(solve(ens, grid)))
        n0, d0 = offsets_for(graphs, B, Wn, Wd)
        out = {}
        for measure in O.MEASURES:
            for aggregate in O.AGGREGATES:
                tag = f"{ens.lattice} {grid} {measure} {aggregate}"
                res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, n0, d0, A3, measure, aggregate, ALL, tag)
                out[tag] = (res, ref, device(eng, ens.terms, NS, B, Wn, Wd, n0, d0, A3, measure, aggregate, beta, ALL))
        return graphs, n0, d0, out
    graphs, n0, d0, out = _with_env({}, run)
    kap = check_inputs(f"{ens.lattice} {grid}", graphs, B, Wn, Wd)
    assert len(set(np.round(d0[:, 0] / d0[:, 0].max(), 9))) == BATCH and not Wd[2].any() and (d0[:, 2] > 0).all()
    for tag, (res, ref, (forms, J, l, grads, _)) in out.items():
        assert set(grads) == set(ALL) and np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
        compare(tag, res, ref, forms, J, l, grads, kap)


# ---- 2. every form of the sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_device_entry_equals_autograd_cotangent_through_the_same_sweep(ens, path):
    env, spi = PATHS[path]
    eng, c = ens.c.solver.engine, ens.c
    B = PY.make_bases(TS, PATH_FREQUENCIES.get((ens.lattice, path), FREQUENCIES[ens.lattice, "5 outputs"]), NS)["6 rows"][0]
    Wn, Wd = three_groups(NS)
    tag = f"{ens.lattice} {path}"

    def run():
        fields = np.array(solve(ens, (TS, spi)))
        st_f = dict(c.solver.stats)
        graphs = graphs_of(ens, fields)
        n0, d0 = offsets_for(graphs, B, Wn, Wd)
        res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, n0, d0, A3, "log", "ks", ALL, tag)
        dev = device(eng, ens.terms, NS, B, Wn, Wd, n0, d0, A3, "log", "ks", beta, ALL)
        dev_d = device(eng, ens.terms, NS, B, Wn, Wd, n0, d0, A3, "log", "ks", beta, DESIGN)
        return st_f, graphs, res, ref, dev, dev_d
    st_f, graphs, res, ref, dev, dev_d = _with_env(env, run)
    st = dev_d[4]
    if path == "adaptive-kept-steps":
        assert st_f["step_control"] == "adaptive-records", st_f
    elif path == "stage-launches":
        assert st["tile_kernels"] != 3 and st["checkpoint_records"] == 1, st
    elif path == "persistent":
        assert st["tile_kernels"] == 3 and st["checkpoint_records"] == 1, st
    elif path == "stages":
        assert st["stage_checkpoint"] == 1, st
    elif path == "segments":
        assert st["checkpoint_records"] == 2, st
    kap = check_inputs(tag, graphs, B, Wn, Wd)
    assert np.array_equal(dev_d[1], dev[1]) and set(dev[3]) == set(ALL) and set(dev_d[3]) == set(DESIGN)
    compare(tag, res, ref, *dev[:4], kap)
    compare(tag + " (design leaves)", res, {k: ref[k] for k in DESIGN}, *dev_d[:4], kap)


# ---- 3. the four bond models with and without the angle contact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_every_bond_model_with_and_without_the_angle_contact(hip_lib, model, contact):
    """Quads 4x4, one member, per-ligament stiffnesses, 3 signals x 6 rows = 18 pairs, G = 3, "log" and "sum"."""
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    nbd, p = len(mc.bonds), mc.members[0]
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
    nb = mc.geo.n_blocks
    driven, corner = int(mc.con[0, 0]), nb - 1
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7), (1, 0, 7, -1.3), (1, corner, 8, 0.9), (1, 5, 8, 0.5), (1, 5, 6, -0.2), (2, 6, 1, 2.0), (2, 6, 3, 1e-4)]
    eng = mc.solver.engine
    B = PY.make_bases(TS, MODEL_FREQUENCIES[model], 3)["6 rows"][0]
    Wn, Wd = three_groups(3)
    tag = f"quads 4x4 {model} contact={contact}"

    def run():
        fields = np.array(mc.solver(np.zeros((2, nb, 3)), TS, mc.cps[0], keep_trajectory=True, steps_per_interval=SPI))
        graphs = [PY.MemberGraph(fields, lv, mc.bonds, terms, 3, MODEL_NAMES[model])]
        n0, d0 = offsets_for(graphs, B, Wn, Wd)
        res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, n0, d0, A3, "log", "sum", ALL, tag)
        return graphs, res, ref, device(eng, terms, 3, B, Wn, Wd, n0, d0, A3, "log", "sum", None, ALL)
    graphs, res, ref, dev = _with_env({}, run)
    kap = check_inputs(tag, graphs, B, Wn, Wd)
    assert np.abs(ref["centroid_node_vectors"]).max() > 0 and np.abs(ref["k_bond"]).max() > 0
    if contact:
        assert np.abs(ref["contact"]).max() > 0 and np.abs(ref["void_angle0"]).max() > 0
    compare(tag, res, ref, *dev[:4], kap)


# ---- 4. 64 and 65 pairs, 1, 64 and 65 groups ------------------------------------------------------------------------------------------------------
def test_a_lanes_second_pair_and_second_group(ens):
    eng = ens.c.solver.engine
    rng = np.random.default_rng(13)
    cases = {}
    for n_rows in (16, 17):
        B = synthetic_basis(ens.lattice, n_rows)
        np_ = NS * n_rows
        assert np_ in (64, 68)
        n_g = 64 if n_rows == 16 else 65
        # one pair per group, the denominator an offset: G = 64 and 65 (pairs 0 .. 63 / 0 .. 64, the 65th a lane's second term)
        Wn = np.zeros((n_g, np_))
        Wn[np.arange(n_g), np.arange(n_g)] = rng.uniform(0.5, 2.0, n_g)
        cases[f"{np_} pairs, G = {n_g}"] = (B, Wn.reshape(n_g, NS, n_rows), np.zeros((n_g, NS, n_rows)), rng.uniform(-1.0, 1.0, n_g))
        # one group over all pairs: the first 32 in the numerator, the others (index 64 among them for 17 rows) in the denominator
        Wn, Wd = np.zeros((1, np_)), np.zeros((1, np_))
        Wn[0, :32], Wd[0, 32:] = rng.uniform(0.5, 2.0, 32), rng.uniform(0.5, 2.0, np_ - 32)
        cases[f"{np_} pairs, G = 1"] = (B, Wn.reshape(1, NS, n_rows), Wd.reshape(1, NS, n_rows), np.array([-1.5]))
    B1 = synthetic_basis(ens.lattice, 1)
    W1 = np.zeros((1, NS, 1))
    W1[0, 2, 0] = 1.3
    cases["1 pair, G = 1"] = (B1, W1, np.zeros_like(W1), np.array([1.0]))

    def run():
        graphs = graphs_of(ens, np.array(solve(ens, "70 outputs")))
        out = {}
        for name, (B, Wn, Wd, a) in cases.items():
            P2 = np.stack([g.projections(B) ** 2 for g in graphs])
            scale = np.einsum("gsj,msj->mg", Wn, P2)
            d0 = np.where(Wd.any((1, 2))[None, :], 0.0, scale * np.random.default_rng(3).uniform(0.5, 2.0, scale.shape))       # per member
            for measure, aggregate in (("log", "ks"), ("ratio", "sum")) if len(a) > 1 else (("log", "sum"),):
                tag = f"{ens.lattice} 70 outputs, {name}, {measure} {aggregate}"
                res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, 0.0, d0, a, measure, aggregate, DESIGN, tag)
                out[tag] = (name, res, ref, device(eng, ens.terms, NS, B, Wn, Wd, None, d0, a, measure, aggregate, beta, DESIGN))
        return graphs, out
    graphs, out = _with_env({}, run)
    for tag, (name, res, ref, dev) in out.items():
        B, Wn, Wd, a = cases[name]
        kap = check_inputs(tag, graphs, B, Wn, Wd)
        compare(tag, res, ref, *dev[:4], kap)


# ---- 5. pairs shared between the groups -----------------------------------------------------------------------------------------------------------
def test_groups_that_share_pairs(ens):
    eng = ens.c.solver.engine
    B = PY.make_bases(TS, FREQUENCIES[ens.lattice, "5 outputs"], NS)["6 rows"][0]
    rng = np.random.default_rng(17)
    Wn, Wd = rng.uniform(0.5, 2.0, (3, NS, 6)), rng.uniform(0.5, 2.0, (3, NS, 6))
    Wn[:, :2], Wd[:, 2:] = 0.0, 0.0                                   # every numerator pair in all three numerators, likewise the denominators
    a = np.array([1.0, 0.5, 0.8])                                     # one sign: the shared terms add up
    tag = f"{ens.lattice} 5 outputs, shared pairs"

    def run():
        graphs = graphs_of(ens, np.array(solve(ens, "5 outputs")))
        res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, 0.0, 0.0, a, "log", "sum", ALL, tag, shared=True)
        return graphs, res, ref, device(eng, ens.terms, NS, B, Wn, Wd, None, None, a, "log", "sum", None, ALL)
    graphs, res, ref, dev = _with_env({}, run)
    kap = check_inputs(tag, graphs, B, Wn, Wd, shared=True)
    compare(tag, res, ref, *dev[:4], kap)


# ---- 6. device values alone: the quadratic special case, scale invariance, repeatability, the NaN rule -------------------------------------------------
def test_special_cases_on_device_values_alone(ens):
    eng = ens.c.solver.engine
    which = ("centroid_node_vectors", "void_angle0", "inertia")
    B = PY.make_bases(TS, FREQUENCIES[ens.lattice, "5 outputs"], NS)["6 rows"][0]
    Wn, Wd = three_groups(NS)
    # a fifth signal on the clamped block 0: its projections are exact zeros, a denominator built on it is d0 alone
    terms5 = ens.terms + [(4, 0, 0, 1.0)]
    Wn5, Wd5 = np.concatenate([Wn, np.zeros((3, 1, 6))], 1), np.zeros((3, 5, 6))
    Wd5[:, 4, :] = 1.0
    W1 = np.zeros((1, NS, 6))
    W1[0, 2, 1] = 1.7

    def call(terms, ns, *a, **kw):
        J, l, out, _ = eng.signal_spectrum_value_and_grad(terms, ns, *a, which=which, **kw)
        return J.copy(), l.copy(), host(out)

    def run():
        solve(ens, "5 outputs")
        r = {}
        forms = eng.signal_spectrum(ens.terms, NS, B, Wn, Wd, None, [0.0, 0.0, 1.0])
        d0 = np.array([0.0, 0.0, 1.0]) * forms[:, :, 0]
        r["a"] = call(ens.terms, NS, B, Wn, Wd, None, d0, A3, "log", "ks", 3.0)
        r["b"] = call(ens.terms, NS, B, Wn, Wd, None, d0, A3, "log", "ks", 3.0)
        # every term coefficient times 3: P times 3, the forms times 9 (so is the offset here), l, J and the gradients unchanged
        t3 = [(s, b, c, 3.0 * v) for s, b, c, v in ens.terms]
        for measure in O.MEASURES:
            r[measure] = call(ens.terms, NS, B, Wn, Wd, None, d0, A3, measure, "sum")
            r[measure + " x3"] = call(t3, NS, B, Wn, Wd, None, 9.0 * d0, A3, measure, "sum")
        # one group, one row, "ratio", d0 = 1, Wd = 0: twice the projection objective with W = Wn
        r["quad"] = call(ens.terms, NS, B, W1, np.zeros_like(W1), None, [1.0], None, "ratio", "sum")
        Jp, outp, _ = eng.signal_projection_value_and_grad(ens.terms, NS, B, W1[0], which=which)
        r["proj"] = (Jp.copy(), None, host(outp))
        # the clamped denominator: D = d0 per member, member 1 without one
        f5 = eng.signal_spectrum(terms5, 5, B, Wn5, Wd5)
        assert np.array_equal(f5[:, :, 1], np.zeros((BATCH, 3)))
        dm = f5[:, :, 0] * np.array([0.5, 1.0, 2.0])
        dz = dm.copy()
        dz[1, 1] = 0.0
        for measure, aggregate, beta in (("ratio", "sum", None), ("log", "ks", 3.0)):
            r[f"dead {measure}"] = call(terms5, 5, B, Wn5, Wd5, None, dz, A3, measure, aggregate, beta)
            r[f"alive {measure}"] = call(terms5, 5, B, Wn5, Wd5, None, dm, A3, measure, aggregate, beta)
        return r
    r = _with_env({}, run)
    same = lambda x, y, rows=slice(None): np.array_equal(x[0][rows], y[0][rows]) and all(np.array_equal(x[2][k][rows], y[2][k][rows]) for k in x[2])   # noqa: E731
    assert np.isfinite(r["a"][0]).all() and all(np.abs(r["a"][2][k]).max() > 0 for k in which if k != "void_angle0" or ens.c.geo.n_npb == 4)
    assert same(r["a"], r["b"]) and np.array_equal(r["a"][1], r["b"][1]), "two identical calls"
    for measure in O.MEASURES:
        x, y = r[measure], r[measure + " x3"]
        e_v = float(np.abs(x[0] - y[0]).max() / np.abs(x[1]).sum(1).max())
        e_g = relerr(y[2]["centroid_node_vectors"], x[2]["centroid_node_vectors"])       # a scale-free value: the same function of the design
        print(f"[signal spectrum] {ens.lattice} coefficients times 3, {measure}: value {e_v:.2e}, node-vector gradient {e_g:.2e}")
        assert e_v <= 1e-13 and e_g <= 1e-12
    e_v = float(np.abs(r["quad"][0] - 2 * r["proj"][0]).max() / np.abs(r["quad"][0]).max())
    e_g = max(relerr(r["quad"][2][k], 2 * r["proj"][2][k]) for k in which if np.abs(r["proj"][2][k]).max() > 0)
    print(f"[signal spectrum] {ens.lattice} one group, one row, ratio against twice the projection objective: value {e_v:.2e}, gradients {e_g:.2e}")
    assert np.abs(r["proj"][0]).min() > 0 and e_v <= 1e-15 and e_g <= 1e-13
    for measure in O.MEASURES:
        dead, alive = r[f"dead {measure}"], r[f"alive {measure}"]
        assert np.isnan(dead[0][1]) and np.isnan(dead[1][1, 1]) and np.isfinite(dead[1][1, [0, 2]]).all() and np.isfinite(alive[0]).all()
        assert all(not dead[2][k][1].any() for k in which) and alive[2]["centroid_node_vectors"][1].any()
        assert same(dead, alive, [0, 2]) and np.array_equal(dead[1][[0, 2]], alive[1][[0, 2]]), "the other members keep their bits"


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(ens):
    eng = ens.c.solver.engine
    T = len(TS)
    one = [(0, 1, 0, 1.0)]
    B1, W1, Z1 = np.ones((2, T)), np.ones((1, 1, 2)), np.zeros((1, 1, 2))
    _with_env({}, lambda: solve(ens, "5 outputs"))
    good = eng.signal_spectrum_value(ens.terms, NS, np.ones((2, T)), np.ones((1, NS, 2)), np.ones((1, NS, 2)))[0].copy()
    calls = (lambda t, n, *a, **kw: eng.signal_spectrum_value_and_grad(t, n, *a, **kw), lambda t, n, *a, **kw: eng.signal_spectrum_value(t, n, *a, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="n_rows must be at least 1"):
            call(one, 1, np.zeros((0, T)), np.zeros((1, 1, 0)), np.zeros((1, 1, 0)))
        with pytest.raises(RuntimeError, match="n_groups must be at least 1"):
            call(one, 1, B1, np.zeros((0, 1, 2)), np.zeros((0, 1, 2)))
        with pytest.raises(RuntimeError, match="non-finite basis entry"):
            call(one, 1, np.where(np.arange(T) == T - 1, np.nan, B1), W1, W1)
        for bad in (np.array([[[1.0, -1.0]]]), np.array([[[1.0, np.inf]]])):
            with pytest.raises(RuntimeError, match="non-finite or negative group weight"):
                call(one, 1, B1, bad, W1)
            with pytest.raises(RuntimeError, match="non-finite or negative group weight"):
                call(one, 1, B1, W1, bad)
        for bad in ([-1.0], [np.nan], np.where(np.arange(BATCH)[:, None] == BATCH - 1, -1.0, np.ones((BATCH, 1)))):
            with pytest.raises(RuntimeError, match="non-finite or negative offset"):
                call(one, 1, B1, W1, W1, bad, None)
            with pytest.raises(RuntimeError, match="non-finite or negative offset"):
                call(one, 1, B1, W1, W1, None, bad)
        with pytest.raises(RuntimeError, match="numerator of group 0 is empty"):
            call(one, 1, B1, Z1, W1)
        with pytest.raises(RuntimeError, match="numerator of group 0 is empty"):
            call(one, 1, B1, Z1, W1, np.where(np.arange(BATCH)[:, None] == 1, 0.0, np.ones((BATCH, 1))))
        with pytest.raises(RuntimeError, match="unknown measure 2"):
            call(one, 1, B1, W1, W1, measure=2)
        with pytest.raises(RuntimeError, match="unknown aggregate 7"):
            call(one, 1, B1, W1, W1, aggregate=7)
        for beta in (0.0, -1.0, np.inf):
            with pytest.raises(RuntimeError, match="beta must be positive and finite with the KS aggregate"):
                call(one, 1, B1, W1, W1, aggregate="ks", beta=beta)
        with pytest.raises(RuntimeError, match="non-finite group coefficient"):
            call(one, 1, B1, W1, W1, group_coef=[np.nan])
        # everything the projection entries refuse
        with pytest.raises(RuntimeError, match="names component 9 out of range"):
            call([(0, 1, 9, 1.0)], 1, B1, W1, W1)
        with pytest.raises(RuntimeError, match="signal 1 is empty"):
            call([(0, 1, 6, 1.0), (2, 1, 0, 1.0)], 3, B1, np.ones((1, 3, 2)), np.ones((1, 3, 2)))
    with pytest.raises(RuntimeError, match="unknown measure 2"):
        eng.signal_spectrum(one, 1, B1, W1, W1, measure=2)
    # NULL arrays: through the C entries themselves (the binding converts its arrays before it calls)
    from difflexmm_amd._binding import _ptr
    args, keep = eng._signal_terms(one, 1)
    J, a1 =np.zeros(BATCH), np.ones(1)
    lib, h = eng.lib, eng._h
    for call, what in ((lambda: lib.dfx_signal_spectrum_value(h, *args, None, 2, 1, _ptr(W1), _ptr(W1), None, None, 0, 1, 0, 1.0, _ptr(a1), _ptr(J), None), "basis is NULL"),
                       (lambda: lib.dfx_signal_spectrum_value(h, *args, _ptr(B1), 2, 1, None, _ptr(W1), None, None, 0, 1, 0, 1.0, _ptr(a1), _ptr(J), None), "den_weights is NULL"),
                       (lambda: lib.dfx_signal_spectrum_value(h, *args, _ptr(B1), 2, 1, _ptr(W1), None, None, None, 0, 1, 0, 1.0, _ptr(a1), _ptr(J), None), "den_weights is NULL"),
                       (lambda: lib.dfx_signal_spectrum_value(h, *args, _ptr(B1), 2, 1, _ptr(W1), _ptr(W1), None, None, 0, 1, 0, 1.0, None, _ptr(J), None), "group_coef is NULL"),
                       (lambda: lib.dfx_signal_spectrum_value_and_grad(h, *args, _ptr(B1), 2, 1, _ptr(W1), _ptr(W1), None, None, 0, 1, 0, 1.0, None, _ptr(J), None,
                                                                        None, None, 0, None), "group_coef is NULL"),
                       (lambda: lib.dfx_signal_spectrum(h, *args, _ptr(B1), 2, 0, _ptr(W1), _ptr(W1), None, None, 0, 1, _ptr(np.zeros((BATCH, 1, 3)))), "n_groups must be at least 1")):
        rc = call()
        assert rc == 1 and what in lib.dfx_last_error(h).decode(), (rc, what, lib.dfx_last_error(h))
    with pytest.raises(ValueError):
        eng.signal_spectrum_value(one, 1, B1, W1, np.ones((2, 1, 2)))
    with pytest.raises(ValueError):
        eng.signal_spectrum_value(one, 1, B1, W1, W1, np.ones(2))
    assert np.array_equal(eng.signal_spectrum_value(ens.terms, NS, np.ones((2, T)), np.ones((1, NS, 2)), np.ones((1, NS, 2)))[0], good)


# ---- 8. a hinge component ------------------------------------------------------------------------------------------------------------------------
def test_a_hinge_component(ens):
    """the 4 signals with the moment term of signal 0 replaced by the hinge force on one node of the driven block (hinge_channels=True):
    forms, value and every gradient leaf against the yardstick on tests/hinge_signal_yardstick.HingeGraph, at the bars of the other cases"""
    from .hinge_signal_yardstick import HingeGraph
    eng, c = ens.c.solver.engine, ens.c
    driven = int(c.con[0, 0])
    node = next(n for n in range(c.geo.n_npb) if any(b // c.geo.n_npb == driven and b % c.geo.n_npb == n for b in np.asarray(c.bonds).ravel()))
    comp = O.hinge_component(node, 0)
    terms = [t for t in ens.terms if t[:3] != (0, driven, 8)] + [(0, driven, comp, 0.7)]
    B = PY.make_bases(TS, FREQUENCIES[ens.lattice, "5 outputs"], NS)["6 rows"][0]
    Wn, Wd = three_groups(NS)
    tag = f"{ens.lattice} 5 outputs, hinge component {comp} on block {driven}"

    def run():
        fields = np.array(solve(ens, "5 outputs"))
        with pytest.raises(RuntimeError, match="out of range"):
            eng.signal_spectrum(terms, NS, B, Wn, Wd)
        graphs = [HingeGraph(fields[m], ens.leaves[m], c.bonds, c.geo.n_npb, terms, NS) for m in range(BATCH)]
        n0, d0 = offsets_for(graphs, B, Wn, Wd)
        eng.hinge_channels = True
        try:
            res, beta, ref = yardstick(eng, graphs, B, Wn, Wd, n0, d0, A3, "log", "ks", ALL, tag)
            return graphs, res, ref, device(eng, terms, NS, B, Wn, Wd, n0, d0, A3, "log", "ks", beta, ALL)
        finally:
            eng.hinge_channels = False
    graphs, res, ref, dev = _with_env({}, run)
    kap = check_inputs(tag, graphs, B, Wn, Wd)
    # signal 0, which holds the hinge term, carries weight (in the denominators of groups 0 and 1)
    assert Wd[:, 0].any() and all(np.abs(ref[k]).max() > 0 for k in ("centroid_node_vectors", "k_bond"))
    compare(tag, res, ref, *dev[:4], kap)


# ---- 9. end to end against the oracle alone ------------------------------------------------------------------------------------------------------------
def _oracle_signals(c, lv, hist, osol, ts, terms, ns, contact=True):
    """(T, n_signals) with the oracle's energies on the oracle's history, differentiable: bond energy, and the contact penalty on the void
    angles of the deformed nodes (the construction of test_gpu_signal_misfit._oracle_misfit)"""
    import torch
    from oracle import ref_energy as OE
    from .strain_yardstick import T64
    nb = c.geo.n_blocks
    free, con = torch.as_tensor(osol.free_DOF_ids), torch.as_tensor(osol.constrained_DOF_ids)
    drive = c.osolver_args["constrained_DOFs_fn"]
    bonds_t = torch.as_tensor(np.asarray(c.bonds), dtype=torch.long)
    rows = []
    for k, t in enumerate(ts):
        u = torch.zeros(nb * 3, dtype=torch.float64)
        u = u.index_put((free,), hist[k, 0]).index_put((con,), drive(float(t), lv["amplitude"], lv["loading_rate"], lv["input_delay"]))
        v = torch.zeros(nb * 3, dtype=torch.float64).index_put((free,), hist[k, 1]).reshape(nb, 3)
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
        rows.append(torch.stack(S))
    return torch.stack(rows)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_end_to_end_against_the_oracle(hip_lib, lattice):
    """The 4x4, 3-output, batch-1 case of test_gpu_signal_misfit.py's section 3 for a SpectrumSpec: autograd through the oracle's
    fixed-grid solve and ITS energies (twice, for the force terms) and the yardstick's formulas on the oracle's signals, against the device
    entry mapped onto the ControlParams leaves.  Two groups, "log" and KS (beta = 10 / spread of the device's z, a single member): the power
    of signal 0 over that of signal 1, and the power of signal 2 over an offset.  Two rows with non-negative entries (the trapezoid weights and
    a ramp times them).  Bar 1e-9 (tests/parity.py); the value against the sum of the absolute terms."""
    import torch
    from oracle import ref_dynamics as OD
    from .common import Case
    from .strain_yardstick import T64
    from .test_gpu_objective import FAST
    from .test_gpu_signal_misfit import neighbours
    quads = lattice == "quads"
    c = Case(lattice, 4, True, True, seed=47, cutoff_deg=42.0 if quads else 125.0, per_bond_k=True)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    ts, spi = (np.linspace(0.0, 3e-4, 3), 4) if quads else (np.linspace(0.0, 1.5e-4, 3), 6)
    nb, nbd = c.geo.n_blocks, len(c.bonds)
    driven = int(c.con[0, 0])
    near = set(neighbours(c, driven)) | {driven}
    force_blocks = [b for b in ([0, nb - 1, 6] if quads else [0, nb - 1, 9]) if not (set(neighbours(c, b)) | {b}) & {driven}]
    assert len(force_blocks) >= 2 and not any(b in near for b in force_blocks)
    free_block = next(b for b in range(5, nb) if b not in near and b not in force_blocks)
    terms = [(0, force_blocks[0], 7, 1.0), (0, force_blocks[1], 8, -0.6), (0, force_blocks[-1], 6, 0.8), (1, force_blocks[-1], 8, 1.0),
             (1, free_block, 0, 3.0), (2, free_block, 2, 1.0), (2, free_block, 4, 1e-4)]
    q = O.fourier_basis(ts, [0.0])[0]
    B = np.stack([q, q * np.linspace(0.0, 1.0, 3)])
    Wn, Wd = np.zeros((2, 3, 2)), np.zeros((2, 3, 2))
    Wn[0, 0], Wd[0, 1], Wn[1, 2] = (1.0, 0.7), (1.3, 0.5), (0.8, 1.9)
    a = np.array([1.0, -0.7])
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = np.array(_with_env({}, lambda: s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi)))
    assert np.abs(fields[:, 0, :, 2]).max() < 1.0, "rotations beyond 1 rad: not a stable solve"
    sig = O.SignalSpec(terms, 3)
    N0 = s.signal_spectrum(O.SpectrumSpec(sig, B, Wn, Wd, None, [0.0, 1.0]))[0][0]
    d0 = np.array([0.0, 0.6 * N0[1]])
    first = s.signal_spectrum_value(O.SpectrumSpec(sig, B, Wn, Wd, None, d0, a))[1][0]
    beta = 10.0 / float(np.ptp(a * first))
    spec = O.SpectrumSpec(sig, B, Wn, Wd, None, d0, a, "log", "ks", beta)
    (obj, l), raw = s.signal_spectrum_value_and_raw(spec, which=s.engine.ALL_GRADS)
    tree, _ = s._unflatten_grads(host(raw), None)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    refv = np.broadcast_to(c.refv, (nbd, 2)).copy()
    names = ["cnv", "refv", "ks", "ksh", "kr", "min_angle", "cutoff_angle", "k_contact", "amplitude", "loading_rate", "input_delay"]
    src = dict(cnv=c.cnv, refv=refv, ks=c.ks, ksh=c.ksh, kr=c.kr, min_angle=c.contact_params[0], cutoff_angle=c.contact_params[1],
               k_contact=c.contact_params[2], **FAST)
    lv = {k: T64(src[k], True) for k in names}
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(y0), ts, c.oracle_cp(lv), spi, "dopri5")
    S = _oracle_signals(c, lv, hist, osol, ts, terms, 3)
    _, N, D = SY.forms(S, B, Wn, Wd, np.zeros(2), d0)
    lo, J = SY.measure_and_value(N, D, a, "log", "ks", beta)
    Sn = S.detach().numpy()[None]
    kap = SY.kappa(B, Sn, np.einsum("jk,mks->msj", B, Sn), (Wn.sum(0) + Wd.sum(0)) > 0).max()
    spread = beta * float(np.ptp(a * lo.detach().numpy()))
    print(f"[signal spectrum] {lattice}: end to end: kappa of the oracle's signals {kap:.1f}, beta * spread {spread:.2f}")
    assert kap <= PY.KAPPA_MAX and 5.0 <= spread <= 40.0
    og = dict(zip(names, torch.autograd.grad(J, [lv[k] for k in names])))
    bp, cpar = tree.mechanical_params.bond_params, tree.mechanical_params.contact_params
    scale = float(np.sum(np.abs(a) * (np.abs(np.log(N.detach().numpy())) + np.abs(np.log(D.detach().numpy())))))
    errs = {"value": abs(obj[0] - J.item()) / scale, "l": float(np.abs(l[0] - lo.detach().numpy()).max() / scale),
            "centroid_node_vectors": relerr(tree.geometrical_params.centroid_node_vectors, og["cnv"].numpy()),
            "k_bond": relerr(np.stack([bp.k_stretch, bp.k_shear, bp.k_rot], 1), np.stack([og[k].numpy() for k in ("ks", "ksh", "kr")], 1)),
            "reference_vector": relerr(bp.reference_vector, og["refv"].numpy()),
            "fn_params": relerr([tree.constraint_params[k] for k in FAST], [og[k].item() for k in FAST])}
    engaged = all(abs(og[k].item()) > 0 for k in ("min_angle", "cutoff_angle", "k_contact"))
    assert engaged or not quads
    if engaged:
        errs["contact"] = relerr([cpar.min_angle, cpar.cutoff_angle, cpar.k_contact], [og[k].item() for k in ("min_angle", "cutoff_angle", "k_contact")])
    print(f"[signal spectrum] {lattice}: end to end against the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(np.abs(og[k].numpy()).max() > 0 for k in names if k not in ("min_angle", "cutoff_angle", "k_contact"))
    bad = {k: v for k, v in errs.items() if not v < 1e-9}
    assert not bad, bad
