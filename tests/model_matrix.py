"""Every bond model with every contact model: the shared builder of tests/test_model_matrix.py (CPU port) and
tests/test_gpu_model_matrix.py (-m gpu).  The kernels are compiled once per (MODEL, CONTACT) pair -- four bond models (nonlinear and
linearised ligaments, the simple spring, the zero-length stretching + torsional spring) times three contact settings (none, angle,
distance) -- and the rest of the suite takes one corner of that space everywhere (nonlinear ligaments + angle contact).

``ModelCase(lattice, model, contact, n, image)`` is modelled on tests/common.Case, test_spring_models.SpringCase and
test_distance_contact.DistCase: the engine solver and its oracle twin on one seeded problem, damping on every block, a fast pulse, inertia
as a leaf of its own.  Two parameter images: ``uniform`` (a batch of 2, each member its own uniform stiffnesses and damping, the lattice's
reference vectors: the shape the per-stage builds compile for) and ``per_bond`` (one member, per-ligament values of the stiffnesses the
model owns).  ``run_engine`` / ``oracle`` are the twins of parity.run_engine_param_leaves / parity.oracle_param_leaves for these cases:
the same runs (forward, vjp_raw, forward, vjp), per-member dicts of every leaf the MODEL has, and -- under ``unowned`` -- the gradients
of what the model does not read, which must be exact zeros.  Premises are asserted (a test whose premise stops holding must fail)."""
import math

import numpy as np
import torch

import difflexmm_amd as dm
from difflexmm_amd import energy as en_mod
from difflexmm_amd import geometry as geo_mod
from difflexmm_amd import loading as ld
from difflexmm_amd.dynamics import setup_dynamic_solver
from difflexmm_amd.geometry import compute_inertia
from oracle import ref_dynamics as OD
from oracle import ref_energy as OE
from oracle import ref_geometry as OG

from .common import BOND_LENGTH, DENSITY, K_ROT, K_SHEAR, K_STRETCH, SPACING, paper_damping, relerr, torch_pulse
from .parity import RAW_WHICH, RTOL_GRAD, RTOL_TRAJ, T64, _fields_bar, _y0, compare_param_leaves

MODELS = ("nonlinear", "linearized", "simple", "torsion")
CONTACTS = (None, "angle", "distance")
SIZES = {"quads": 13, "kagome": 11}                 # a partial last wave: 676 slots = 10.6 waves, 242 triangles = 12.1 packed waves
OWNED = {"nonlinear": ("ks", "ksh", "kr", "refv"), "linearized": ("ks", "ksh", "kr", "refv"), "simple": ("ks", "refv"), "torsion": ("ks", "kr")}
UNOWNED = {"nonlinear": (), "linearized": (), "simple": ("ksh", "kr"), "torsion": ("ksh", "refv")}
FIELD = {"ks": "k_stretch", "ksh": "k_shear", "kr": "k_rot", "refv": "reference_vector"}
K0 = {"ks": K_STRETCH, "ksh": K_SHEAR, "kr": K_ROT}
CONTACT_NAMES = ("min_angle", "cutoff_angle", "k_contact")
PULSE_NAMES = ("amplitude", "loading_rate", "input_delay")
_EN = {"nonlinear": (en_mod.ligament_energy, OE.ligament_energy), "linearized": (en_mod.ligament_energy_linearized, OE.ligament_energy_linearized),
       "simple": (en_mod.simple_spring_energy, OE.simple_spring_energy),
       "torsion": (en_mod.stretching_torsional_spring_energy, OE.stretching_torsional_spring_energy)}


def loop_serves(model, contact):
    """The physics the persistent loops and the kept adaptive steps serve (engine_launch.hip persist_shape_ok, engine_adaptive.hip): the
    two ligament models, without contact or with angle contact.  Also what the per-stage builds exist for (dfx_builds.h, stage_build_ok)."""
    return model in ("nonlinear", "linearized") and contact != "distance"


def case_id(lattice, model, contact):
    return f"{lattice}-{model}-{contact or 'none'}"


def rotating_contacts(models=MODELS, start=0):
    """One contact per model, rotating through none / angle / distance."""
    return [(m, CONTACTS[(start + i) % 3]) for i, m in enumerate(models)]


class ModelCase:
    def __init__(self, lattice, model, contact, n, image, lib=None, batch=None, seed=0):
        assert model in MODELS and contact in CONTACTS and image in ("uniform", "per_bond"), (model, contact, image)
        self.lattice, self.model, self.contact, self.image = lattice, model, contact, image
        self.c = self                     # (parity._y0 / parity._fields_bar read a ShapeCase: sc.c.geo, sc.c.solver, sc.members)
        rng = self.rng = np.random.default_rng(2000 + seed)
        if lattice == "quads":
            self.geo, self.ogeo = geo_mod.QuadGeometry(n, n, SPACING, BOND_LENGTH), OG.QuadGeometry(n, n, SPACING, BOND_LENGTH)
            base = self.geo.get_design_from_rotated_square(25 * math.pi / 180)
            self.design = tuple(b + rng.uniform(-0.02 * SPACING, 0.02 * SPACING, b.shape) for b in base)
            mid = (n // 2) * n
            con = [[mid, 0], [mid, 1], [mid, 2], [0, 0], [0, 1], [0, 2], [n * n - 1, 1]]
            cutoff_deg = 42.0
        else:
            basis = 20.0 * np.array([[1.0, 0.0], [math.cos(math.pi / 3), math.sin(math.pi / 3)]])
            self.geo, self.ogeo = geo_mod.KagomeGeometry(n, n, basis, BOND_LENGTH), OG.KagomeGeometry(n, n, basis, BOND_LENGTH)
            self.design = tuple(rng.uniform(-0.3, 0.3, s) for s in self.geo.design_shapes())
            mid = 2 * n * (n // 2)
            con = [[mid, 0], [mid, 1], [mid, 2], [0, 0], [0, 1], [0, 2]]
            cutoff_deg = 125.0
        self.con = np.array(con)
        self.vec = np.array([1.0] + [0.0] * (len(con) - 1))
        self.bonds = self.geo.bond_connectivity()
        self.cnv, self.cen = self.geo.centroid_node_vectors(*self.design), self.geo.block_centroids(*self.design)
        nb, nbd = self.geo.n_blocks, len(self.bonds)
        # the premise of the lattice sizes: the last wave is partial (quad mapping: 4 lanes per block, packed triangles: 20 blocks per wave)
        self.n_slots = 4 * nb
        self.lattice_refv = np.broadcast_to(self.geo.reference_bond_vectors(), (nbd, 2)).copy()
        self.damped = np.arange(nb)
        # A = 1.5 with distance contact: the hinges must stay off the penalty's asymptote (test_distance_contact.DistCase)
        self.pulse = dict(amplitude=1.5 if contact == "distance" else 7.5, loading_rate=3000.0, input_delay=1e-5)
        self.contact_params = {None: None, "angle": (-15.0 * math.pi / 180, cutoff_deg * math.pi / 180, 1.5), "distance": (1.0, 2.6, 0.5)}[contact]
        efn, ofn = _EN[model]
        energy, oenergy = en_mod.build_strain_energy(self.bonds, efn), OE.build_strain_energy(self.bonds, ofn)
        self.ostrain = oenergy
        if contact:
            energy = en_mod.combine_block_energies(energy, en_mod.build_contact_energy(self.bonds, angle_based=contact == "angle"))
            oenergy = OE.combine_block_energies(oenergy, OE.build_contact_energy(self.bonds, angle_based=contact == "angle"))
        self.oenergy = oenergy
        n_members = batch or (2 if image == "uniform" else 1)
        self.solver = setup_dynamic_solver(self.geo, energy, constrained_block_DOF_pairs=self.con, constrained_DOFs_fn=ld.Pulse(self.vec),
                                           damped_blocks=self.damped, batch=n_members, _lib=lib)
        self.members = []
        for m in range(n_members):
            p = {}
            for k in OWNED[model]:
                if k == "refv":
                    p[k] = self.lattice_refv.copy()
                elif image == "uniform":          # each member its own uniform values
                    p[k] = K0[k] * (1.0 + 0.1 * (m + 1) * {"ks": 1.0, "ksh": -1.0, "kr": 2.0}[k])
                else:
                    p[k] = K0[k] * (1 + 0.1 * rng.uniform(-1, 1, nbd))
            p["damping"] = paper_damping() * (1.0 + 0.5 * m)
            p["inertia"] = compute_inertia(self.cnv, DENSITY) * rng.uniform(0.9, 1.1, (nb, 3))
            self.members.append(p)
        self.cps = [self.control_params(p) for p in self.members]
        # -- the premises of the image, on the host
        stiff = [k for k in OWNED[model] if k != "refv"]
        if image == "uniform":
            assert all(np.ndim(p[k]) == 0 for p in self.members for k in stiff) and all(np.shape(p["damping"]) == (3,) for p in self.members)
            if n_members > 1:
                assert all(len({float(p[k]) for p in self.members}) == n_members for k in stiff), "members do not differ in their stiffnesses"
                assert len({tuple(p["damping"]) for p in self.members}) == n_members, "members do not differ in their damping"
        else:
            assert all(np.shape(p[k]) == (nbd,) and p[k].max() > p[k].min() for p in self.members for k in stiff), "stiffnesses do not vary per ligament"

    def assert_partial_last_wave(self):
        nb = self.geo.n_blocks
        assert self.n_slots % 64 != 0 and self.n_slots > 64, self.n_slots
        if self.lattice == "kagome":
            assert nb % 20 != 0 and nb > 20 and (3 * nb) % 64 != 0, nb

    # -- parameters ------------------------------------------------------------------------------------------------------------------------
    def control_params(self, p):
        if self.model == "torsion":
            bp = dm.StretchingTorsionalSpringParams(p["ks"], p["kr"])
        elif self.model == "simple":              # k_shear / k_rot are not parameters of this model: whatever they hold is not read
            bp = dm.LigamentParams(p["ks"], 123.0, 456.0, p["refv"])
        else:
            bp = dm.LigamentParams(p["ks"], p["ksh"], p["kr"], p["refv"])
        return dm.ControlParams(dm.GeometricalParams(self.cen, self.cnv),
                                dm.MechanicalParams(bp, DENSITY, p["inertia"], p["damping"],
                                                    dm.ContactParams(*self.contact_params) if self.contact else None),
                                constraint_params=dict(self.pulse))

    def engine_params(self):
        return self.cps if len(self.cps) > 1 else self.cps[0]

    def leaf_names(self):
        return list(OWNED[self.model]) + ["inertia", "damping"] + list(PULSE_NAMES) + (list(CONTACT_NAMES) if self.contact else [])

    def oracle_cp(self, m, leaves=None):
        """Oracle ControlParams of member m; ``leaves`` (name -> tensor) replaces entries so that autograd tracks them."""
        p = self.members[m]
        lv = {k: T64(p[k]) for k in OWNED[self.model]}
        lv.update(cnv=T64(self.cnv), cen=T64(self.cen), inertia=T64(p["inertia"]), damping=T64(p["damping"]))
        lv.update({k: T64(v) for k, v in self.pulse.items()})
        if self.contact:
            lv.update({k: T64(v) for k, v in zip(CONTACT_NAMES, self.contact_params)})
        lv.update(leaves or {})
        if self.model == "torsion":
            bp = OE.StretchingTorsionalSpringParams(lv["ks"], lv["kr"])
        elif self.model == "simple":
            bp = OE.SimpleSpringParams(lv["ks"], lv["refv"])
        else:
            bp = OE.LigamentParams(lv["ks"], lv["ksh"], lv["kr"], lv["refv"])
        return OE.ControlParams(OE.GeometricalParams(lv["cen"], lv["cnv"]),
                                OE.MechanicalParams(bp, T64(DENSITY), lv["inertia"], lv["damping"],
                                                    OE.ContactParams(*[lv[k] for k in CONTACT_NAMES]) if self.contact else None),
                                constraint_params={k: lv[k] for k in PULSE_NAMES})

    def oracle_solver(self, **kw):
        return OD.setup_dynamic_solver(self.ogeo, self.oenergy, constrained_block_DOF_pairs=self.con, constrained_DOFs_fn=torch_pulse(self.vec),
                                       damped_blocks=self.damped, **kw)

    # -- the engine --------------------------------------------------------------------------------------------------------------------------
    def run_engine(self, ts, spi=None, adaptive=False, rtol=1e-5, atol=1e-5):
        """Forward, ``vjp_raw(which=RAW_WHICH)``, forward again, ``vjp``: per-member dicts in the oracle's layout (parity.run_engine_param_leaves
        for these cases).  ``unowned``: the gradients of the leaves the model does not own, out of the tree and out of the engine's raw arrays."""
        s = self.solver
        B, y0, nb = len(self.members), _y0(self), self.geo.n_blocks
        fb = _fields_bar(self, len(ts))
        free = s.free_DOF_ids
        if adaptive:
            s.rtol, s.atol = rtol, atol

        def solve():
            out = s(y0, ts, self.engine_params(), keep_trajectory=True, steps_per_interval=None if adaptive else spi)
            return np.array(out).reshape(B, len(ts), 2, nb, 3), dict(s.stats)

        fields, st_fwd = solve()
        step_times = None
        if adaptive and st_fwd["step_control"] == "adaptive-records":
            step_times = [np.concatenate([ts[:1], s.engine.adaptive_step_times(m)]) for m in range(B)]
        adaptive_stats = dict(getattr(s, "adaptive_stats", {})) if adaptive and st_fwd["step_control"] == "adaptive-grid" else None
        raw = {k: np.array(v) for k, v in s.vjp_raw(fb if B > 1 else fb[0], which=RAW_WHICH).items()}
        st_raw = dict(s.adjoint_stats)
        fields2, st_fwd2 = solve()
        seen, engine_adjoint = [], s.engine.adjoint

        def recording_adjoint(*a, **kw):          # the raw arrays of the whole-tree sweep: what the tree does not show of an unowned leaf
            out = engine_adjoint(*a, **kw)
            seen.append({k: np.array(v) for k, v in out[0].items()})
            return out
        s.engine.adjoint = recording_adjoint
        try:
            trees, s0 = s.vjp(fb if B > 1 else fb[0])
        finally:
            del s.engine.adjoint
        st_tree = dict(s.adjoint_stats)
        trees, s0 = (trees, s0) if B > 1 else ([trees], s0[None])
        assert len(seen) == 1
        out = []
        for m, (p, tree) in enumerate(zip(self.members, trees)):
            d = {"fields": fields[m].reshape(len(ts), 2, -1)[:, :, free]}
            gp, mp = tree.geometrical_params, tree.mechanical_params
            if self.contact == "distance":
                assert np.abs(gp.block_centroids).max() > 0, "the block_centroids cotangent is zero with distance contact"
            else:
                assert np.all(np.asarray(gp.block_centroids) == 0.0)
            for i, g in enumerate(self.geo.vjp(self.design, gp.centroid_node_vectors, gp.block_centroids)):
                d[f"design{i}"] = g
            bp = mp.bond_params
            assert type(bp) is type(self.cps[m].mechanical_params.bond_params)
            for k in OWNED[self.model]:
                d[k] = getattr(bp, FIELD[k])
            d.update(inertia=mp.inertia, damping=mp.damping)
            if self.contact:
                d.update({k: getattr(mp.contact_params, k) for k in CONTACT_NAMES})
            for k in PULSE_NAMES:
                d[k] = tree.constraint_params[k]
            d["state0"] = s0[m].reshape(2, -1)[:, free]
            un = {}
            for k in UNOWNED[self.model]:
                un["raw:" + k] = seen[0]["reference_vector"][m] if k == "refv" else seen[0]["k_bond"][m][:, {"ksh": 1, "kr": 2}[k]]
                if hasattr(bp, FIELD[k]):
                    un["tree:" + k] = np.asarray(getattr(bp, FIELD[k]))
            d["unowned"] = un
            r = {}
            cnv_bar = raw["centroid_node_vectors"][m]
            if self.contact == "angle":
                cnv_bar = cnv_bar + geo_mod.void_angles0_vjp(self.cnv, self.bonds, raw["void_angle0"][m])
            cen_bar = raw["block_centroids"][m].reshape(self.cen.shape) if self.contact == "distance" else np.zeros_like(self.cen)
            for i, g in enumerate(self.geo.vjp(self.design, cnv_bar, cen_bar)):
                r[f"design{i}"] = g
            r["inertia"] = raw["inertia"][m].reshape(np.shape(p["inertia"]))
            r["damping"] = raw["damping"][m][self.damped].sum(0)
            r["amplitude"], r["loading_rate"], r["input_delay"] = raw["fn_params"][m][0][:3]
            d["raw"] = r
            d["fields_again"] = fields2[m].reshape(len(ts), 2, -1)[:, :, free]
            out.append(d)
        return dict(members=out, fwd_stats=st_fwd, fwd_stats_again=st_fwd2, raw_stats=st_raw, tree_stats=st_tree, step_times=step_times,
                    adaptive_stats=adaptive_stats)

    def run_plain_adaptive(self, ts, rtol=1e-5, atol=1e-5):
        """The reference's call as it stands (no ``keep_trajectory``): fields on the free DOFs and accepted steps per member, and the stats."""
        s = self.solver
        s.rtol, s.atol = rtol, atol
        B = len(self.members)
        out = np.array(s(_y0(self), ts, self.engine_params())).reshape(B, len(ts), 2, -1)
        assert s.stats["step_control"] == "adaptive", s.stats["step_control"]
        return [out[m][:, :, s.free_DOF_ids] for m in range(B)], [len(s.engine.adaptive_step_times(m)) for m in range(B)], dict(s.stats)

    # -- the oracle --------------------------------------------------------------------------------------------------------------------------
    def oracle_plain_adaptive(self, ts, rtol=1e-5, atol=1e-5):
        """The oracle's ``odeint`` on the same inputs: per member the fields on the free DOFs and the number of accepted steps."""
        fields, steps = [], []
        for m in range(len(self.members)):
            osol = self.oracle_solver(integrator="adaptive", rtol=rtol, atol=atol)
            of = osol(_y0(self), ts, self.oracle_cp(m)).numpy().reshape(len(ts), 2, -1)
            fields.append(of[:, :, osol.free_DOF_ids])
            steps.append(len(osol.stats["step_times"]) - 1)
        return fields, steps

    def oracle(self, ts, spi=None, step_times=None, grid=None):
        """torch.autograd through the oracle's unrolled solve with every leaf of the model on the tape, member by member: on ``spi`` equal
        steps per interval, on the replay of the accepted adaptive steps ``step_times[m]`` (dense output), or on the frozen grid
        ``grid = (steps per interval, step boundaries)``."""
        y0 = _y0(self)
        fb = _fields_bar(self, len(ts))
        names = self.leaf_names()
        out = []
        for m, p in enumerate(self.members):
            design = [T64(d, True) for d in self.design]
            cnv, cen = self.ogeo.centroid_node_vectors(*design), self.ogeo.block_centroids(*design)
            src = dict(p, **self.pulse)
            if self.contact:
                src.update(zip(CONTACT_NAMES, self.contact_params))
            leaves = {k: T64(src[k], True) for k in names}
            y0t = T64(y0, True)
            cp = self.oracle_cp(m, dict(cnv=cnv, cen=cen, **leaves))
            if step_times is not None:
                osol = self.oracle_solver(integrator="adaptive")
                hist, _ = OD.solve_adaptive_replay_differentiable(osol, self.ogeo, y0t, ts, cp, step_times[m])
            elif grid is not None:
                osol = self.oracle_solver(integrator="fixed", steps_per_interval=grid[0], step_times=grid[1])
                hist, _ = OD.solve_fixed_differentiable(osol, self.ogeo, y0t, ts, cp, grid[0], "dopri5", step_times=grid[1])
            else:
                osol = self.oracle_solver(integrator="fixed", steps_per_interval=spi)
                hist, _ = OD.solve_fixed_differentiable(osol, self.ogeo, y0t, ts, cp, spi, "dopri5")
            free = osol.free_DOF_ids
            L = (hist * T64(fb[m].reshape(len(ts), 2, -1)[:, :, free])).sum()
            gr = torch.autograd.grad(L, design + [leaves[k] for k in names] + [y0t])
            d = {"fields": hist.detach().numpy()}
            for i, g in enumerate(gr[:len(design)]):
                d[f"design{i}"] = g.numpy()
            for k, g in zip(names, gr[len(design):-1]):
                d[k] = g.numpy()
            d["state0"] = gr[-1].numpy().reshape(2, -1)[:, free]
            if self.contact:
                assert np.abs([d[k] for k in CONTACT_NAMES]).max() > 0, "contact inactive: the test would be vacuous"
            out.append(d)
        return out

    # -- energy ------------------------------------------------------------------------------------------------------------------------------
    def check_energy(self, rtol=1e-11):
        """``engine.energy`` (k_energy<MODEL, CONTACT>) of a random configuration against the oracle's energy, member by member; with contact
        the contact share must be above 1e-6 of the total (test_distance_contact.check_rhs_and_vjp)."""
        s = self.solver
        s.prepare(self.engine_params())
        scale = np.array([0.15, 0.15, 0.05]) if self.contact == "distance" else np.array([0.3, 0.3, 0.1])
        u = np.random.default_rng(91).normal(size=(self.geo.n_blocks, 3)) * scale
        mine = s.engine.energy(np.stack([u] * len(self.members)))
        errs = []
        for m in range(len(self.members)):
            e = float(self.oenergy(T64(u), self.oracle_cp(m)))
            if self.contact:
                share = e - float(self.ostrain(T64(u), self.oracle_cp(m)))
                assert share > 1e-6 * e, ("contact inactive: the test would be vacuous", share, e)
            errs.append(abs(mine[m] - e) / abs(e))
            assert errs[-1] < rtol, (self.model, self.contact, m, mine[m], e, errs[-1])
        assert len(self.members) == 1 or mine[0] != mine[1]
        return max(errs)


def compare(mc, eng, ref, rtol_fwd=None, rtol_grad=RTOL_GRAD):
    """parity.compare_param_leaves for a ModelCase (fields: RTOL_TRAJ, 1e-9 with distance contact -- the bar of test_distance_contact.py: the
    penalty is stiff near its asymptote and the reference's sqrt(|a|^2 - t^2 |e|^2) loses digits the closest-point form keeps), and the exact
    zeros of the leaves the model does not own.  Returns the errors."""
    if rtol_fwd is None:
        rtol_fwd = 1e-9 if mc.contact == "distance" else RTOL_TRAJ
    for m, d in enumerate(eng["members"]):
        assert set(k.split(":")[1] for k in d["unowned"]) == set(UNOWNED[mc.model])
        for k, v in d["unowned"].items():
            assert np.all(np.asarray(v) == 0.0), (mc.model, m, k, np.abs(v).max())
    stripped = dict(eng, members=[{k: v for k, v in d.items() if k != "unowned"} for d in eng["members"]])
    return compare_param_leaves(stripped, ref, rtol_fwd=rtol_fwd, rtol_grad=rtol_grad)


def worst(errs):
    """(worst fields error, worst gradient error) out of compare's result."""
    f = max(v for k, v in errs.items() if k[1].endswith("fields"))
    g = max(v for k, v in errs.items() if not k[1].endswith("fields"))
    return f, g


def same_as(eng, ref_eng, exact):
    """An arm against the stage arm at the bars of test_gpu_persistent.py: fields 1e-13, gradients 1e-11; ``exact``: equality (the same
    kernels ran, or a build without contraction).  Returns (worst fields, worst gradient) difference."""
    wf = wg = 0.0
    for a, b in zip(eng["members"], ref_eng["members"]):
        for k in b:
            items = [(kk, a[k][kk], bv) for kk, bv in b[k].items()] if k in ("raw", "unowned") else [(k, a[k], b[k])]
            for kk, av, bv in items:
                if exact or k == "unowned":
                    assert np.array_equal(av, bv), (k, kk, relerr(av, bv))
                else:
                    e = relerr(av, bv) if np.abs(bv).max() > 0 else float(np.abs(av).max())
                    assert e < (1e-13 if "fields" in k else 1e-11), (k, kk, e)
                    wf, wg = (max(wf, e), wg) if "fields" in k else (wf, max(wg, e))
    return wf, wg


# -- the adaptive call ---------------------------------------------------------------------------------------------------------------------
def check_plain_adaptive(mc, ts, rtol=1e-5, atol=1e-5, oracle=None):
    """The reference's call (no ``keep_trajectory``) against the oracle's ``odeint``: fields at 1e-8 (parity.check_adaptive_records_adjoint:
    two controllers, rounding in the error estimate moves the step sizes by ~1e-8) and the same number of accepted steps.  ``oracle``:
    what ``mc.oracle_plain_adaptive`` returned for the same case (computed once per test).  Returns (worst fields error, steps of member 0)."""
    fields, steps, _ = mc.run_plain_adaptive(ts, rtol, atol)
    ofields, osteps = oracle if oracle is not None else mc.oracle_plain_adaptive(ts, rtol, atol)
    assert steps == osteps, (steps, osteps)
    errs = [relerr(a, b) for a, b in zip(fields, ofields)]
    assert max(errs) < 1e-8, ("adaptive forward", errs)
    return max(errs), steps[0]


def check_kept_adaptive(mc, ts, expect_control, rtol=1e-5, atol=1e-5, ref_cache=None):
    """``keep_trajectory=True`` without a grid, then the reverse sweeps.  ``"adaptive-records"``: every leaf against autograd through the
    oracle's replay of the steps the engine accepted; ``"adaptive-grid"``: fields and every leaf against autograd through the oracle's
    fixed-grid solve on the frozen grid ``solver.stats`` reports, at RTOL_TRAJ / RTOL_GRAD.  ``ref_cache`` (dict): the oracle's result is
    kept under the step boundaries it belongs to (two arms that froze the same grid share it).  Returns (engine result, errors)."""
    eng = mc.run_engine(ts, adaptive=True, rtol=rtol, atol=atol)
    st = eng["fwd_stats"]
    assert st["step_control"] == expect_control and eng["fwd_stats_again"]["step_control"] == expect_control, (st["step_control"], expect_control)
    if expect_control == "adaptive-records":
        key = tuple(np.concatenate(eng["step_times"]).tolist())
        make = lambda: mc.oracle(ts, step_times=eng["step_times"])        # noqa: E731
        rtol_fwd = None
    else:
        spis, grid = np.asarray(st["steps_per_interval"]), np.asarray(st["step_times"])
        assert len(spis) == len(ts) - 1 and spis.sum() == len(grid) - 1 == st["steps"] and spis.min() >= 1, (spis, len(grid), st["steps"])
        assert grid[0] == ts[0] and np.all(np.isin(ts, grid)) and np.all(np.diff(grid) > 0)
        key = tuple(grid.tolist())
        make = lambda: mc.oracle(ts, grid=(spis, grid))                   # noqa: E731
        rtol_fwd = RTOL_TRAJ
    if ref_cache is None:
        ref = make()
    else:
        if key not in ref_cache:
            ref_cache[key] = make()
        ref = ref_cache[key]
    return eng, compare(mc, eng, ref, rtol_fwd=rtol_fwd)
