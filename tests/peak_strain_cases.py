"""The inputs of the peak-strain cases (include/dfx.h: dfx_strain_peak_value[_and_grad]), built without a GPU so that
tests/test_peak_strain_host.py can check their premises on the CPU port and tests/test_gpu_peak_strain.py runs the kernels on them.

The bars of the GPU file (1e-12 for the value, 1e-11 of the largest entry of a leaf) carry over from the strain-energy suite when the
softmax does not amplify the 1e-15 relative error of q by more than 40: the sharpness of every case that uses them is chosen FROM THE DATA,
beta = 15 / (geometric mean of the members' q_hat) so that 5 <= beta q_hat <= 40 for every member, and p = 6.
  small     the ensembles of tests/test_gpu_objective.py (quads 6x6 with the contact engaged, kagome 4x4, 3 members, 5 outputs): per-member
            coefficients U(0.5, 2), per-member bond weights with most bonds at zero (the weighted set of the strain-energy suite, made
            non-negative), tau with a zero and a non-integer entry
  sharp     the small quads case with beta = 800 / (q_hat - second largest q): every pi but one underflows to 0
  large     the large cases of tests/objective_shapes.py (257 outputs, 1 161 / 1 157 workgroups): |its bond weights|, its tau; "late": tau
            zero on the first 172 outputs, so that the argmax sits in the last third of the items"""
import numpy as np

import difflexmm_amd as dm
from difflexmm_amd import objective as O
from difflexmm_amd.geometry import compute_inertia

from . import objective_shapes as OS
from .common import DENSITY, Case

BETA_TARGET, BETA_RANGE = 15.0, (5.0, 40.0)
P_NORM, P_RANGE = 6.0, (2.0, 16.0)
SHARP_EXPONENT = 800.0                  # exp(-800) = 0 in float64 (the smallest subnormal is exp(-745))
LATE_FROM = 172                         # 172 / 257 > 2/3


def cpu_ensemble(lattice, lib):
    """tests/test_gpu_objective.Ensemble on another library: the same seeds, hence the same members (that class builds its Case on the HIP
    library, which needs a GPU).  The ``ens`` fixture of tests/test_gpu_peak_strain.py asserts that the two hold the same members, bonds,
    constraints, drive and contact constants, so a change of that constructor cannot go unnoticed here."""
    from . import test_gpu_objective as TO
    e = TO.Ensemble.__new__(TO.Ensemble)
    n = 6 if lattice == "quads" else 4
    c = e.c = Case(lattice, n, True, True, seed=41, batch=TO.BATCH, cutoff_deg=42.0 if lattice == "quads" else 125.0, lib=lib)
    rng = np.random.default_rng(7)
    amp = 0.15 if lattice == "quads" else 0.05
    e.cps, e.inertia, e.cen = [], [], []
    for m in range(TO.BATCH):
        design = tuple(d + (rng.uniform(-amp, amp, d.shape) if m else 0.0) for d in c.design)
        cnv, cen = c.geo.centroid_node_vectors(*design), c.geo.block_centroids(*design)
        e.cps.append(c.cp._replace(geometrical_params=dm.GeometricalParams(cen, cnv), constraint_params=dict(TO.FAST)))
        e.inertia.append(compute_inertia(cnv, DENSITY))
        e.cen.append(cen)
    e.inertia, e.cen = np.stack(e.inertia), np.stack(e.cen)
    e.nb = c.geo.n_blocks
    return e


def coefficients(seed, members, nbd):
    """(members, n_bonds, 3) coefficient triples U(0.5, 2)"""
    return np.random.default_rng(seed).uniform(0.5, 2.0, (members, nbd, 3))


def small_inputs(c, seed=23, members=3):
    """(coef (members, n_bonds, 3), bond weights (members, n_bonds) >= 0 with most at zero, the three special bonds): the weighted set of
    tests/test_gpu_strain_objective.weighted_bonds -- a bond on the driven block, one on a clamped block, one on a corner block whose other
    slots carry no weighted ligament, a few more, every member dropping one -- with the signs removed."""
    from .test_gpu_strain_objective import weighted_bonds
    w, special = weighted_bonds(c, seed=seed, members=members)
    return coefficients(seed + 1, members, len(c.bonds)), np.abs(w), special


def cnv_of(cps):
    cps = cps if isinstance(cps, (list, tuple)) and not hasattr(cps, "_fields") else [cps]
    return np.stack([np.asarray(cp.geometrical_params.centroid_node_vectors, dtype=float) for cp in cps])


def measure(c, cps, fields, coef, model="nonlinear"):
    """(B, T, n_bonds) q on the host (objective.host_strain_measure) for a Case and its members' parameters"""
    f = np.asarray(fields, dtype=float)
    f = f[None] if f.ndim == 4 else f
    return O.host_strain_measure(coef, f, cnv_of(cps), c.bonds, np.broadcast_to(c.refv, (len(c.bonds), 2)), model)


def weighted_pairs(q, bw, tau):
    """per member: the q of the pairs with W > 0, descending"""
    B = q.shape[0]
    bw = np.broadcast_to(bw, (B, q.shape[2]))
    out = []
    for m in range(B):
        on = (np.asarray(tau)[:, None] * bw[m][None, :]) > 0
        out.append(np.sort(q[m][on])[::-1])
    return out


def choose_beta(qhat):
    """beta = 15 / geometric mean of the members' q_hat"""
    return float(BETA_TARGET / np.exp(np.mean(np.log(np.asarray(qhat, dtype=float)))))


def in_range(beta, qhat):
    x = beta * np.asarray(qhat, dtype=float)
    return bool((x >= BETA_RANGE[0]).all() and (x <= BETA_RANGE[1]).all())


def sharp_beta(pairs):
    """the beta at which every pair but the largest of every member has beta (q - q_hat) <= -800"""
    return float(SHARP_EXPONENT / min(p[0] - p[1] for p in pairs))


def late_tau(tau):
    t = np.array(tau, dtype=float)
    t[:LATE_FROM] = 0.0
    return t


def large_inputs(L):
    """(coef (B, n_bonds, 3), bond weights (B, n_bonds) >= 0, tau) of an objective_shapes.LargeCase"""
    return coefficients(31, OS.BATCH, L.nbd), np.abs(L.bw), L.tau


def item_of(L, k, bond):
    """the item (output k, listed block of the bond's end 0) of the 64-item kernels, and the number of items: the listed blocks are the
    owners of a weighted end, ascending (prepare_peak lists them as prepare_strain does)"""
    listed = OS.strain_blocks(L.c.bonds, L.npb, L.bw)
    j = int(np.searchsorted(listed, int(np.asarray(L.c.bonds)[bond, 0]) // L.npb))
    return k * len(listed) + j, OS.N_OUT * len(listed)
