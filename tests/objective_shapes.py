"""Cases at which a launch of the device objectives (difflexmm_amd/csrc/dfx_objective.h, engine_objective.hip) spans many workgroups, built
without a GPU: lattices, members, weights, terms, and the item and workgroup counts that follow from them by the rules of
``prepare_objective`` / ``prepare_strain`` / ``prepare_signal`` restated here.  tests/test_objective_shapes_host.py checks the premises on the
CPU port, tests/test_gpu_objective_shapes.py runs the kernels on them.

The large case, one per lattice: quads 17x17 (289 blocks) and kagome 12x12 (288 blocks), angle contact, nonlinear ligaments, damping, 2 members
with different designs, 257 outputs one Dopri5 step apart, a random initial state (every (output, block) item then carries a term of
comparable size from the first output on).  257 blocks are weighted: all but the constrained ones and 29 more spread over the index range, so
that the compaction list is no arange; 257 is prime, so of the 258 workgroup boundaries inside the 257 x 257 = 66 049 items all but one
(item 256 x 257) fall inside an output time.
  k_objective          259 workgroups, the last one partial: more than 256 partials, k_objective_finish makes a second trip of its loop
  k_objective_explicit 5 workgroups
  k_signal_channels    1 033 workgroups (257 force blocks), k_signal_residual 259 (257 signals)
The bond weights sit on every ligament with an end on the 257 blocks and the signals have a force term on each of them, so the blocks that
``prepare_strain`` lists (the owners of a weighted end) and the set of ``prepare_signal`` (force blocks and the blocks bonded to them) are
LARGER than 257: they reach the neighbours, the constrained blocks included (289 / 288 blocks: 1 161 / 1 157 workgroups of
k_strain_objective and k_signal_cotangent, 19 / 18 of the two per-slot explicit kernels; WORKGROUPS below).  What the tests need of them holds
all the same: more than 256 partials, a last workgroup that is partial, at least 2 workgroups of every explicit kernel.  ``prepare_signal``
lists all three force components of a force block, so n_uc (1 233) exceeds the number of terms (771); the repeated (block, component) pairs
show as fewer distinct pairs (719) than terms and as uc ranges that hold two terms.
The drive is a gentle pulse inside the horizon (the default pulse of tests.common starts after it and would leave the gradient of the drive's
parameters at zero; the fast pulse of tests/test_gpu_objective.py takes these lattices to rotations of 1 rad).  The signal targets are the
signals times U(0.5, 1.5) moved by twice each signal's RMS (``signal_targets`` says why)."""
import math

import numpy as np

import difflexmm_amd as dm
from difflexmm_amd import objective as O
from difflexmm_amd.geometry import compute_inertia

from .common import DENSITY, Case

N_OUT = 257
TS = np.linspace(0.0, 2.56e-3, N_OUT)
SPI = 1
BATCH = 2
N_WEIGHTED = 257
STATE_SCALES = (0.05, 0.02, 5.0)
GENTLE = dict(amplitude=0.5, loading_rate=1000.0, input_delay=1e-4)           # the pulse: inside the horizon, rotations stay below 0.15 rad
STRAIN_PARTS = (0.0, 0.5, 2.0, 1.5)
ONE_HOT = (0, 1, 128, 255, 256)
SIZES = {"quads": 17, "kagome": 12}
N_BLOCKS = {"quads": 289, "kagome": 288}
ITEMS_WIDE, ITEMS_QUAD, LANES_EXPLICIT = 256, 64, 64          # kObjThreads, kObjQuads, the block size of the explicit kernels
SMALL_FAR_LOW = 1e-3                                           # an item is negligible below this share of the median weighted item ...
SMALL_SHARE = 0.02                                             # ... and at most this share of the weighted items may be


def chunks(items, per):
    return max(1, -(-int(items) // per))


# ---- the rules of the host side, restated ---------------------------------------------------------------------------------------------------
def objective_blocks(w):
    """prepare_objective: the blocks whose weight is non-zero in any member, ascending."""
    return np.nonzero((np.atleast_2d(w) != 0).any(0))[0]


def strain_blocks(bonds, npb, bw):
    """prepare_strain: both end slots of a ligament carry its weight; listed are the blocks that own a weighted end."""
    on = (np.atleast_2d(bw) != 0).any(0)
    return np.unique(np.asarray(bonds)[on] // npb)


def signal_tables(bonds, npb, terms):
    """prepare_signal: force blocks, the set (force blocks and the blocks bonded to them), and the terms grouped by distinct
    (block, component) with all three force components of every force block listed.  Returns a dict."""
    blocks = np.asarray(bonds) // npb
    fb = sorted({b for _, b, c, _ in terms if c >= 6})
    in_f = np.isin(blocks, fb)
    st = sorted(set(fb) | set(int(x) for x in blocks[in_f.any(1)].ravel()))
    by_dof = {(b, c): [] for b in fb for c in (6, 7, 8)}
    for i, (_, b, c, _) in enumerate(terms):
        by_dof.setdefault((b, c), []).append(i)
    return dict(fblocks=fb, set=st, by_dof=by_dof, n_fb=len(fb), n_set=len(st), n_sig=len({s for s, _, _, _ in terms}), n_uc=len(by_dof),
                n_terms=len(terms), n_distinct=len({(b, c) for _, b, c, _ in terms}), longest_uc=max(len(v) for v in by_dof.values()))


def workgroups(T, n_act, n_act_strain, sig):
    """grid.x of every kernel of the three families (engine_objective.hip: launch_objective, launch_strain, launch_signal,
    launch_objective_explicit); the partials k_objective_finish adds are the grid.x of the kernel in front of it."""
    return {"k_objective": chunks(T * n_act, ITEMS_WIDE), "k_objective_explicit": chunks(n_act, LANES_EXPLICIT),
            "k_strain_objective": chunks(T * n_act_strain, ITEMS_QUAD), "k_strain_objective_explicit": chunks(n_act_strain * 4, LANES_EXPLICIT),
            "k_signal_channels": chunks(T * sig["n_fb"], ITEMS_QUAD), "k_signal_residual": chunks(T * sig["n_sig"], ITEMS_WIDE),
            "k_signal_direction": chunks(T * sig["n_uc"], ITEMS_WIDE), "k_signal_cotangent": chunks(T * sig["n_set"], ITEMS_QUAD),
            "k_signal_explicit": chunks(sig["n_set"] * 4, LANES_EXPLICIT)}


# the counts of the large case: from the 257 x 257 items where the list holds the 257 blocks, from the neighbour rule elsewhere
COUNTS = {"quads": dict(n_act=257, n_act_strain=289, n_fb=257, n_set=289, n_sig=257, n_uc=1233),
          "kagome": dict(n_act=257, n_act_strain=288, n_fb=257, n_set=288, n_sig=257, n_uc=1233)}
WORKGROUPS = {"quads": {"k_objective": 259, "k_objective_explicit": 5, "k_strain_objective": 1161, "k_strain_objective_explicit": 19,
                        "k_signal_channels": 1033, "k_signal_residual": 259, "k_signal_direction": 1238, "k_signal_cotangent": 1161,
                        "k_signal_explicit": 19},
              "kagome": {"k_objective": 259, "k_objective_explicit": 5, "k_strain_objective": 1157, "k_strain_objective_explicit": 18,
                         "k_signal_channels": 1033, "k_signal_residual": 259, "k_signal_direction": 1238, "k_signal_cotangent": 1157,
                         "k_signal_explicit": 18}}


def check_spans_many_workgroups(T, counts, wg):
    """What the large case is for; a later edit cannot quietly shrink it back into one workgroup."""
    for k in ("k_objective", "k_strain_objective", "k_signal_residual"):
        assert wg[k] > ITEMS_WIDE, (k, wg[k])                                  # a second trip of the loop of k_objective_finish
    for n, per in ((counts["n_act"], ITEMS_WIDE), (counts["n_act_strain"], ITEMS_QUAD), (counts["n_fb"], ITEMS_QUAD), (counts["n_set"], ITEMS_QUAD),
                   (counts["n_sig"], ITEMS_WIDE), (counts["n_uc"], ITEMS_WIDE)):
        assert (T * n) % per != 0, (n, per)                                    # a partial last workgroup
    for n in (counts["n_act"], counts["n_sig"], counts["n_fb"]):
        for per in (ITEMS_WIDE, ITEMS_QUAD):                                   # n odd: a boundary meets the start of an output only where per | k
            assert sum((k * n) % per == 0 for k in range(1, T)) == (T - 1) // per, (n, per)
    for k in ("k_objective_explicit", "k_strain_objective_explicit", "k_signal_explicit"):
        assert wg[k] >= 2, (k, wg[k])


# ---- the large case -------------------------------------------------------------------------------------------------------------------------
def weighted_set(nb, constrained, n=N_WEIGHTED):
    """n blocks: all but the constrained ones, minus blocks spread evenly over the index range."""
    free = np.array([b for b in range(nb) if b not in set(int(x) for x in constrained)])
    drop = len(free) - n
    assert drop > 0
    out = free[np.round(np.linspace(0, len(free) - 1, drop + 2)[1:-1]).astype(int)]
    assert len(set(out)) == drop
    keep = np.array(sorted(set(free) - set(out)))
    assert len(keep) == n and not np.array_equal(keep, np.arange(keep[0], keep[0] + n))
    return keep


def signed(rng, shape):
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 2.0, shape)


TERM_SCALE = (10.0, 10.0, 40.0, 1.2e-3, 1.2e-3, 4e-3, 0.1, 0.1, 0.03)      # per component: mm, rad, mm/s, rad/s, N, N mm -> terms of the order of 1


def make_terms(listed, rng):
    """len(listed) signals: signal s = a force term on block b_s (components 6, 7, 8 in rotation), a displacement and a velocity term on
    block b_(s+1); every fifth signal repeats, alternately with its displacement and its velocity term, the (block, component) of the
    next signal's.  Coefficients of both signs, scaled per component so that the three terms of a signal are of one order."""
    n = len(listed)
    B = lambda s: int(listed[s % n])                                                    # noqa: E731
    terms = []
    for s in range(n):
        force, disp, vel = (B(s), 6 + s % 3), (B(s + 1), s % 3), (B(s + 1), 3 + (s + 1) % 3)
        if s % 10 == 0:
            disp = (B(s + 2), (s + 1) % 3)
        elif s % 10 == 5:
            vel = (B(s + 2), 3 + (s + 2) % 3)
        terms += [(s, b, c, float(cf * TERM_SCALE[c])) for (b, c), cf in zip((force, disp, vel), signed(rng, 3))]
    return terms


def signal_targets(S, factor, sign):
    """Per-member targets (B, T, n_signals): the yardstick's signals times U(0.5, 1.5), as the fixture of tests/test_gpu_signal_misfit.py
    builds them, moved by twice the signal's RMS over the outputs.  Without the shift a residual S (1 - U) vanishes wherever the signal
    crosses zero or U comes close to 1: 4.5 % of the items were below 1e-3 of the median one, and 2.1 % with any factor at all (the zero
    crossings of S alone); with it none is."""
    S = np.asarray(S)
    return S * factor + sign[:, None, :] * 2.0 * np.sqrt((S ** 2).mean(1, keepdims=True))


class LargeCase:
    """The Ensemble pattern of tests/test_gpu_objective.py at the large shape.  ``lib``: the CPU port, or None for the HIP library."""

    def __init__(self, lattice, lib=None):
        self.lattice = lattice
        n = SIZES[lattice]
        c = self.c = Case(lattice, n, True, True, seed=41, batch=BATCH, cutoff_deg=42.0 if lattice == "quads" else 125.0, lib=lib)
        self.nb, self.npb, self.nbd = c.geo.n_blocks, c.geo.n_npb, len(c.bonds)
        assert self.nb == N_BLOCKS[lattice]
        rng = np.random.default_rng(7)
        amp = 0.15 if lattice == "quads" else 0.05
        self.cps, self.inertia, self.cen = [], [], []
        for m in range(BATCH):
            design = tuple(d + (rng.uniform(-amp, amp, d.shape) if m else 0.0) for d in c.design)
            cnv, cen = c.geo.centroid_node_vectors(*design), c.geo.block_centroids(*design)
            self.cps.append(c.cp._replace(geometrical_params=dm.GeometricalParams(cen, cnv), constraint_params=dict(GENTLE)))
            self.inertia.append(compute_inertia(cnv, DENSITY))
            self.cen.append(cen)
        self.inertia, self.cen = np.stack(self.inertia), np.stack(self.cen)
        self.y0 = c.random_state(*STATE_SCALES)
        self.constrained = sorted(set(int(b) for b in c.con[:, 0]))
        # weighted blocks, weights, output-time weights
        rng = np.random.default_rng(11)
        self.listed = weighted_set(self.nb, self.constrained)
        self.w = np.zeros((BATCH, self.nb))
        self.w[:, self.listed] = signed(rng, (BATCH, N_WEIGHTED))
        self.zeroed = rng.permutation(self.listed)[:20]
        self.w[1, self.zeroed] = 0.0                                   # still listed (member 0 weights them): the tw != 0 skip inside a full launch
        self.tau = rng.uniform(0.25, 2.0, N_OUT)
        self.tau[0] = 0.0
        self.lever0 = self.cen - self.cen[0][self.listed].mean(0)
        # bond weights: every ligament with an end on the weighted blocks, same sign rule, 20 of them at zero in member 1
        on = np.nonzero(np.isin(np.asarray(c.bonds) // self.npb, self.listed).any(1))[0]
        self.bw = np.zeros((BATCH, self.nbd))
        self.bw[:, on] = signed(rng, (BATCH, len(on)))
        self.bw[1, rng.permutation(on)[:20]] = 0.0
        # signals
        self.terms = make_terms(self.listed, rng)
        self.ns = N_WEIGHTED
        self.omega = rng.uniform(0.25, 2.0, self.ns)
        self.target_factor = rng.uniform(0.5, 1.5, (BATCH, N_OUT, self.ns))
        self.target_sign = rng.choice([-1.0, 1.0], (BATCH, self.ns))

    def targets(self, S):
        return signal_targets(S, self.target_factor, self.target_sign)

    def spec(self, kind, tau=None):
        return O.ObjectiveSpec(kind, self.w, self.tau if tau is None else tau, self.lever0 if kind == O.ANGULAR_MOMENTUM else None)

    def solve(self, spi=SPI):
        return np.array(self.c.solver(self.y0, TS, self.cps, keep_trajectory=True, steps_per_interval=spi))

    def state0_as_output(self):
        """the initial state as output 0 holds it: the constrained DOFs at what the drive prescribes at t = 0, that is at rest"""
        y = self.y0.copy()
        y[:, self.c.con[:, 0], self.c.con[:, 1]] = 0.0
        return y

    def counts(self):
        sig = signal_tables(self.c.bonds, self.npb, self.terms)
        cnt = dict(n_act=len(objective_blocks(self.w)), n_act_strain=len(strain_blocks(self.c.bonds, self.npb, self.bw)),
                   n_fb=sig["n_fb"], n_set=sig["n_set"], n_sig=sig["n_sig"], n_uc=sig["n_uc"])
        return cnt, workgroups(N_OUT, cnt["n_act"], cnt["n_act_strain"], sig), sig

    def leaves(self):
        from .test_gpu_signal_misfit import member_leaves
        return [member_leaves(self.c, self.cps, m) for m in range(BATCH)]


# ---- per-item terms of the host yardsticks: unit terms carry the weight of the block / ligament / signal but not tau ----------------------------
def weighted_unit_terms(kind, w, lever0, fields, inertia):
    """(B, T, n_blocks): w_mb [ sum_d p v^2 / 2 ]  or  w_mb [ (a_x + u_x) m_y v_y - (a_y + u_y) m_x v_x + J omega ]"""
    f = np.asarray(fields, dtype=float)
    u, v, p = f[:, :, 0], f[:, :, 1], np.asarray(inertia, dtype=float)[:, None]
    if kind == O.KINETIC:
        t = (p * v ** 2 / 2).sum(-1)
    else:
        a = np.asarray(lever0, dtype=float)[:, None]
        t = (a[..., 0] + u[..., 0]) * p[..., 1] * v[..., 1] - (a[..., 1] + u[..., 1]) * p[..., 0] * v[..., 0] + p[..., 2] * v[..., 2]
    return np.asarray(w, dtype=float)[:, None, :] * t


def strain_unit_terms(u_hist, lv, bonds, w, parts, model="nonlinear"):
    """One member: (T, n_bonds) w_b [weighted ligament energy] and (T, n_bonds) the contact part of it, with the energies of
    tests/strain_yardstick.py (``strain_objective`` adds exactly these)."""
    import torch
    from oracle import ref_energy as OE
    from .strain_yardstick import T64, _wrap, bond_energies
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    t = {k: T64(v) for k, v in lv.items()}
    e_all, e_con = [], []
    with torch.no_grad():
        for k in range(len(u_hist)):
            nd = OE.block_to_node_kinematics(T64(u_hist[k]), t["cnv"]).reshape(-1, 3)
            nodal = (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]])
            e = bond_energies(model, nodal, t["refv"], t["ks"], t["ksh"], t["kr"], parts)
            ce = torch.zeros_like(e)
            if "am" in t and parts[3] != 0.0:
                kap = nodal[1][:, 2] - nodal[0][:, 2]
                ce = OE.contact_energy(_wrap(t["phi0"][:, 0] - kap), t["am"], t["ac"], parts[3] * t["kc"]) \
                    + OE.contact_energy(_wrap(t["phi0"][:, 1] + kap), t["am"], t["ac"], parts[3] * t["kc"])
            e_all.append((e + ce).numpy())
            e_con.append(ce.numpy())
    return np.asarray(w, dtype=float)[None, :] * np.stack(e_all), np.stack(e_con)


def signal_unit_terms(S, targets, omega):
    """(.., T, n_signals): omega_s (S - Starget)^2 / 2"""
    return 0.5 * np.asarray(omega, dtype=float) * (np.asarray(S) - np.asarray(targets)) ** 2


def fsum_value(unit, tau):
    """(value, sum of |term|) of one member: math.fsum over the items tau_k * unit[k, ...]"""
    t = (np.asarray(tau, dtype=float).reshape((-1,) + (1,) * (unit.ndim - 1)) * unit).ravel()
    return math.fsum(t), math.fsum(np.abs(t))


def small_share(unit, tau, weight):
    """(share, count) of the weighted items (tau_k * weight != 0, ``weight`` broadcast against ``unit`` without its output axis) whose |term|
    is below SMALL_FAR_LOW of the median weighted item"""
    tk = np.asarray(tau, dtype=float).reshape((-1,) + (1,) * (unit.ndim - 1))
    on = np.abs(tk * unit)[np.broadcast_to((tk != 0) & (np.asarray(weight) != 0), unit.shape)]
    return float((on < SMALL_FAR_LOW * np.median(on)).mean()), len(on)


# ---- the exact-boundary small cases on the ensemble of tests/test_gpu_objective.py ------------------------------------------------------------
SMALL = {"exactly-256": (8, 32), "exactly-64": (8, 8), "65": (5, 13)}          # name: (outputs, weighted blocks)


SMALL_CENTRE = {"quads": 18, "kagome": 16}                                     # the driven block of tests.common.Case on 6x6 / 4x4


def small_blocks(bonds, npb, nb, n, centre):
    """n blocks of consecutive index around the driven block (the pulse reaches them within the few outputs of these cases), every one with
    a ligament to another of them, and the ligaments INSIDE the set: weights on those make ``prepare_strain`` list exactly these n blocks"""
    lo = min(max(centre - n // 2, 0), nb - n)
    blocks = np.arange(lo, lo + n)
    inside = np.isin(np.asarray(bonds) // npb, blocks).all(1)
    assert centre in blocks and np.array_equal(np.unique((np.asarray(bonds) // npb)[inside]), blocks)
    return blocks, np.nonzero(inside)[0]


def small_terms(blocks):
    """one signal per block: a force term on it (components 6, 7, 8 in rotation) and a displacement term on the next block of the list"""
    n = len(blocks)
    terms = []
    for s in range(n):
        terms += [(s, int(blocks[s]), 6 + s % 3, (-1.0) ** s * TERM_SCALE[6 + s % 3]), (s, int(blocks[(s + 1) % n]), s % 3, TERM_SCALE[s % 3])]
    return terms
