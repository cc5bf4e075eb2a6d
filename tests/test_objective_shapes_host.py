"""The premises of tests/test_gpu_objective_shapes.py, checked without a GPU on the CPU port: the cases of tests/objective_shapes.py concern
the INPUTS of the device objectives, not their kernels.
  * the large solves are finite and in regime (largest |theta| < 0.5 rad); output 0 holds the initial state;
  * per family, at most 2 % of the weighted items (tau_k * weight != 0) have an absolute term below 1e-3 of the median weighted item -- a
    misrouted or lost item then shows in the value (measured: kinetic 1.3e-4, angular 1.0e-3, strain 3.0e-4, signal residuals 0);
  * the item and workgroup counts recomputed from the specification by the restated host rules are the ones the module states, and they
    span what the GPU file is there for (more than 256 partials, partial last workgroups, two or more workgroups of the explicit kernels);
  * math.fsum and np.sum of the items agree to 1e-15 of the sum of their absolute values (measured: 1.2e-16)."""
import numpy as np
import pytest

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O

from . import objective_shapes as OS
from .signal_yardstick import signal_misfit


class Premises:
    def __init__(self, lattice, lib):
        L = self.L = OS.LargeCase(lattice, lib)
        self.fields = L.solve()
        lv = L.leaves()
        self.unit = {}
        for kind, name in ((O.KINETIC, "kinetic"), (O.ANGULAR_MOMENTUM, "angular")):
            u = OS.weighted_unit_terms(kind, L.w, L.lever0, self.fields, L.inertia)
            self.unit[name] = [(u[m], L.w[m]) for m in range(OS.BATCH)]
        self.unit["strain"], self.contact = [], []
        for m in range(OS.BATCH):
            u, ce = OS.strain_unit_terms(self.fields[m, :, 0], lv[m], L.c.bonds, L.bw[m], OS.STRAIN_PARTS)
            self.unit["strain"].append((u, L.bw[m]))
            self.contact.append(ce)
        S = np.stack([signal_misfit(self.fields[m], lv[m], L.c.bonds, L.terms, L.ns, np.zeros((OS.N_OUT, L.ns)), None, None)[1]
                      for m in range(OS.BATCH)])
        tg = L.targets(S)
        self.unit["signal"] = [(OS.signal_unit_terms(S[m], tg[m], L.omega), L.omega) for m in range(OS.BATCH)]


@pytest.fixture(scope="module", params=["quads", "kagome"])
def prem(request, cpu_lib):
    return Premises(request.param, cpu_lib)


def test_large_solves_are_finite_and_in_regime(prem):
    L, f = prem.L, prem.fields
    assert f.shape == (OS.BATCH, OS.N_OUT, 2, L.nb, 3) and np.isfinite(f).all()
    worst = float(np.abs(f[:, :, 0, :, 2]).max())
    print(f"[objective shapes] {L.lattice}: largest |theta| {worst:.3f} rad")
    assert 0.02 < worst < 0.5
    assert not np.array_equal(f[0], f[1])                                          # the members differ
    assert np.abs(f[:, :, 0, int(L.c.con[0, 0]), 0]).max() == OS.GENTLE["amplitude"] > 0    # the pulse acts inside the horizon
    assert all(np.array_equal(f[m, 0], L.state0_as_output()) for m in range(OS.BATCH))
    if L.lattice == "quads":
        assert all(ce.sum() > 0 for ce in prem.contact)                            # the angle contact is engaged


def test_the_specification_holds_what_the_kernels_can_go_wrong_on(prem):
    L = prem.L
    assert len(L.listed) == 257 and not set(L.listed) & set(L.constrained)
    assert np.array_equal(OS.objective_blocks(L.w), L.listed) and (np.diff(L.listed) > 1).sum() >= 20          # no arange
    assert (L.w[0, L.listed] != 0).all() and (L.w[1, L.listed] == 0).sum() == 20 and (L.w < 0).any() and (L.w > 0).any()
    assert 0.25 <= np.abs(L.w[L.w != 0]).min() and np.abs(L.w).max() <= 2.0
    assert L.tau.shape == (257,) and L.tau[0] == 0 and L.tau[1:].min() >= 0.25
    assert (L.bw[0] != 0).sum() - (L.bw[1] != 0).sum() == 20 and (L.bw < 0).any() and (L.bw > 0).any()
    ends = np.isin(np.asarray(L.c.bonds) // L.npb, L.listed).any(1)
    assert np.array_equal(L.bw[0] != 0, ends)
    comps = {}
    for s, b, c, coef in L.terms:
        comps.setdefault(s, []).append((b, c, coef))
    assert len(comps) == 257 and all(len(v) == 3 for v in comps.values())
    assert all(v[0] == (int(L.listed[s]), 6 + s % 3) + v[0][2:] and v[1][1] < 3 and 3 <= v[2][1] < 6 for s, v in comps.items())
    coefs = np.array([t[3] for t in L.terms])
    assert (coefs < 0).any() and (coefs > 0).any() and len(set(np.round(L.omega, 12))) == 257


def test_item_and_workgroup_counts(prem):
    L = prem.L
    cnt, wg, sig = L.counts()
    print(f"[objective shapes] {L.lattice}: {cnt}, workgroups {wg}")
    assert cnt == OS.COUNTS[L.lattice] and wg == OS.WORKGROUPS[L.lattice]
    assert OS.N_OUT * cnt["n_act"] == 66049
    assert wg["k_objective"] == 259 and wg["k_objective_explicit"] == 5 and wg["k_signal_channels"] == 1033 and wg["k_signal_residual"] == 259
    OS.check_spans_many_workgroups(OS.N_OUT, cnt, wg)
    assert sig["n_distinct"] < sig["n_terms"] and sig["longest_uc"] == 2
    assert sum(len(v) == 2 for v in sig["by_dof"].values()) == sig["n_terms"] - sig["n_distinct"] >= 257 // 5


@pytest.mark.parametrize("family", ["kinetic", "angular", "strain", "signal"])
def test_few_negligible_items_and_an_exact_sum(prem, family):
    L = prem.L
    for m, (unit, weight) in enumerate(prem.unit[family]):
        share, n = OS.small_share(unit, L.tau, weight)
        value, total = OS.fsum_value(unit, L.tau)
        gap = abs(float((L.tau.reshape((-1,) + (1,) * (unit.ndim - 1)) * unit).sum()) - value) / total
        print(f"[objective shapes] {L.lattice} {family} member {m}: {n} weighted items, {share:.2e} of them below 1e-3 of the median; "
              f"|value| / sum |term| {abs(value) / total:.2e}; np.sum against fsum {gap:.2e}")
        assert n >= 0.9 * 256 * 237 and share <= OS.SMALL_SHARE
        assert total > 0 and gap <= 1e-15


def test_small_cases_fill_their_workgroups_exactly():
    assert {k: t * n for k, (t, n) in OS.SMALL.items()} == {"exactly-256": 256, "exactly-64": 64, "65": 65}
    for lattice, nb, npb in (("quads", 36, 4), ("kagome", 32, 3)):
        geo = G.QuadGeometry(6, 6, 15.0, 2.25) if lattice == "quads" else \
            G.KagomeGeometry(4, 4, 20.0 * np.array([[1.0, 0.0], [np.cos(np.pi / 3), np.sin(np.pi / 3)]]), 2.25)
        bonds = geo.bond_connectivity()
        assert geo.n_blocks == nb and geo.n_npb == npb
        for name, (T, n) in OS.SMALL.items():
            blocks, inside = OS.small_blocks(bonds, npb, nb, n, OS.SMALL_CENTRE[lattice])
            bw = np.zeros(len(bonds))
            bw[inside] = 1.0
            assert len(blocks) == n and np.array_equal(OS.strain_blocks(bonds, npb, bw), blocks)
            terms = OS.small_terms(blocks)
            sig = OS.signal_tables(bonds, npb, terms)
            assert sig["n_fb"] == n and sig["n_sig"] == n
            assert OS.chunks(T * n, OS.ITEMS_WIDE) == 1
            assert OS.chunks(T * n, OS.ITEMS_QUAD) == {"exactly-256": 4, "exactly-64": 1, "65": 2}[name]
