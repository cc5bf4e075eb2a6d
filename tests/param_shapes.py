"""Parameter images that steer the engine's data-dependent code paths (dfx_plan.h, pack_params): stiffnesses per ligament (k_uniform),
damping per block and DOF (damping_uniform), and the number of distinct reference vectors per member, which decides between the
dictionary in LDS (<= kDictLds = 16), the dictionary in global memory (17..256) and no dictionary at all (> 256).

``ShapeCase(shape, ...)`` builds a :class:`tests.common.Case` plus one ControlParams per member with that image, and asserts on the host
that the image really has the property the shape is named after (a test whose premise silently stops holding must fail, not pass)."""
import numpy as np

import difflexmm_amd as dm
from difflexmm_amd.geometry import compute_inertia

from .common import DENSITY, K_ROT, K_SHEAR, K_STRETCH, Case, paper_damping

SHAPES = ("uniform", "k_per_bond", "damping_per_block", "refv_16", "refv_17", "refv_256", "refv_257", "mixed_batch", "mixed_batch_17")
K_DICT_LDS, K_DICT_MAX = 16, 256       # dfx_kernels.h kDictLds; dfx_plan.h: a member with more distinct reference vectors has no dictionary


def n_distinct(refv):
    """Distinct reference vectors by exact equality (as pack_params compares them)."""
    return len(np.unique(np.asarray(refv, dtype=float).reshape(-1, 2), axis=0))


def refv_pool(lattice_refv, n_pool, rng):
    """Per-ligament reference vectors drawn from a pool of exactly ``n_pool`` distinct vectors: every lattice vector times small distinct
    factors, each ligament keeping (a scaled copy of) its own lattice vector, every pool entry used at least once."""
    base = np.asarray(lattice_refv, dtype=float)
    uniq, inv = np.unique(base, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = base.copy()
    for i in range(len(uniq)):
        n_i = n_pool // len(uniq) + (i < n_pool % len(uniq))
        idx = rng.permutation(np.flatnonzero(inv == i))
        assert len(idx) >= n_i, ("lattice too small for a pool of", n_pool)
        pick = np.concatenate([np.arange(n_i), rng.integers(0, n_i, len(idx) - n_i)])
        factors = 1.0 + 0.04 * (np.arange(n_i) / max(n_i - 1, 1) - 0.5)
        out[idx] = uniq[i] * factors[pick][:, None]
    assert n_distinct(out) == n_pool, (n_distinct(out), n_pool)
    return out


class ShapeCase:
    """``c``: the Case (solver for ``len(members)`` members, oracle builders); ``members``: per member the parameter leaves
    (ks, ksh, kr, refv, damping, inertia: NumPy, as passed to the engine); ``cps``: their ControlParams; ``expect``: the host-side
    flags pack_params must compute for the batch (k_uniform, damping_uniform, n_dict per member)."""

    def __init__(self, shape, lattice="quads", n=5, lib=None, contact=True, nonlinear=True, seed=0, batch=None, integrator="dopri5",
                 explicit_inertia=True):
        assert shape in SHAPES, shape
        self.shape = shape
        rng = np.random.default_rng(1000 + seed)
        n_members = batch or (3 if shape.startswith("mixed_batch") else 2 if shape in ("k_per_bond", "damping_per_block") else 1)
        damped = None
        if shape == "damping_per_block":
            n_blocks = n * n if lattice == "quads" else 2 * n * n
            damped = np.sort(rng.choice(n_blocks, (2 * n_blocks) // 3, replace=False))
        cut = 42.0 if lattice == "quads" else 125.0
        self.c = c = Case(lattice, n, nonlinear, contact, seed=seed, lib=lib, cutoff_deg=cut, batch=n_members, integrator=integrator,
                          damped_blocks=damped)
        nbd = len(c.bonds)
        lattice_refv = np.broadcast_to(c.refv, (nbd, 2)).copy()
        n_lattice = n_distinct(lattice_refv)
        self.members = []
        for m in range(n_members):
            p = dict(ks=K_STRETCH, ksh=K_SHEAR, kr=K_ROT, refv=lattice_refv.copy(), damping=np.array(c.dval, dtype=float))
            if shape == "k_per_bond":
                p.update(ks=K_STRETCH * (1 + 0.1 * rng.uniform(-1, 1, nbd)), ksh=K_SHEAR * (1 + 0.1 * rng.uniform(-1, 1, nbd)),
                         kr=K_ROT * (1 + 0.1 * rng.uniform(-1, 1, nbd)))
            elif shape == "damping_per_block":
                p["damping"] = paper_damping() * rng.uniform(0.5, 1.5, (len(c.damped), 3))
            elif shape.startswith("refv_"):
                p["refv"] = refv_pool(lattice_refv, int(shape[5:]), rng)
            elif shape.startswith("mixed_batch"):
                # member 0: the common values; 1: other (uniform) stiffnesses; 2: other (uniform) damping and its own dictionary
                if m % 3 == 1:
                    p.update(ks=1.1 * K_STRETCH, ksh=0.9 * K_SHEAR, kr=1.2 * K_ROT)
                elif m % 3 == 2:
                    p["damping"] = 1.5 * paper_damping()
                    p["refv"] = refv_pool(lattice_refv, 17 if shape == "mixed_batch_17" else 16, rng)
            if explicit_inertia:      # inertia as a leaf of its own: the geometric one, perturbed per block and DOF
                p["inertia"] = compute_inertia(c.cnv, DENSITY) * rng.uniform(0.9, 1.1, (c.geo.n_blocks, 3))
            else:
                p["inertia"] = None
            self.members.append(p)
        self.cps = [self.control_params(p) for p in self.members]
        # -- the premise of the shape, on the host
        full_k = [np.stack([np.broadcast_to(p[k], (nbd,)) for k in ("ks", "ksh", "kr")], 1) for p in self.members]
        full_d = [self.damping_image(p) for p in self.members]
        k_uni = [bool(np.all(k == k[0])) for k in full_k]
        d_uni = [bool(np.all(d == d[0])) for d in full_d]
        self.n_dict = [n_distinct(p["refv"]) for p in self.members]
        self.expect = dict(k_uniform=all(k_uni), damping_uniform=all(d_uni), n_dict=self.n_dict)
        if shape == "k_per_bond":
            assert not any(k_uni) and all(np.all(k.max(0) > k.min(0)) for k in full_k), "stiffnesses do not vary per ligament"
        else:
            assert all(k_uni), "stiffnesses are not uniform"
        if shape == "damping_per_block":
            assert not any(d_uni) and all(np.all(d.max(0) > d.min(0)) for d in full_d), "damping does not vary per block"
            assert all((d[np.setdiff1d(np.arange(c.geo.n_blocks), c.damped)] == 0).all() for d in full_d)
            assert len(c.damped) < c.geo.n_blocks
        else:
            assert all(d_uni), "damping is not uniform"
        want = {"refv_16": [16], "refv_17": [17], "refv_256": [256], "refv_257": [257], "mixed_batch": [n_lattice, n_lattice, 16],
                "mixed_batch_17": [n_lattice, n_lattice, 17]}.get(shape, [n_lattice])
        assert self.n_dict == [want[m % len(want)] for m in range(n_members)], (shape, self.n_dict)
        if shape.startswith("mixed_batch"):
            assert len({(p["ks"], p["ksh"], p["kr"]) for p in self.members}) == 2, "members do not differ in their stiffnesses"
            assert len({tuple(np.ravel(d)[:3]) for d in full_d}) == 2, "members do not differ in their damping"

    @property
    def dict_layout(self):
        """What the host-side counts make pack_params choose: 'lds', 'global' or 'none'."""
        mx = max(self.n_dict)
        return "none" if mx > K_DICT_MAX else ("global" if mx > K_DICT_LDS else "lds")

    def damping_image(self, p):
        d = np.zeros((self.c.geo.n_blocks, 3))
        d[self.c.damped] = np.broadcast_to(p["damping"], (len(self.c.damped), 3))
        return d

    def control_params(self, p):
        c = self.c
        return dm.ControlParams(
            dm.GeometricalParams(c.cen, c.cnv),
            dm.MechanicalParams(dm.LigamentParams(p["ks"], p["ksh"], p["kr"], p["refv"]), DENSITY, p["inertia"], p["damping"],
                                dm.ContactParams(*c.contact_params) if c.contact else None),
            constraint_params=dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5))

    def engine_params(self):
        """The members' ControlParams as the solver takes them (one object for a single member)."""
        return self.cps if len(self.cps) > 1 else self.cps[0]
