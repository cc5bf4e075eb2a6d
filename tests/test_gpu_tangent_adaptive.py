"""-m gpu: forward mode through the adaptive solve (DynamicSolver.jvp(adaptive=True) -> jvp_multi along one direction ->
dfx_forward_tangent_dense_multi; the single-direction entry dfx_forward_tangent_dense is that one at n_dirs = 1): its fields are the
fields of the default call, its tangent is torch.autograd through the oracle's replay of the engine's own accepted steps with the dense
output, it is the transpose of vjp on the SAME solve, and its contract.  Host side: tests/test_tangent_adaptive_host.py."""
import math

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import _binding as b
from difflexmm_amd import energy as en_mod
from difflexmm_amd import geometry as geo
from difflexmm_amd import loading as ld
from difflexmm_amd.dynamics import setup_dynamic_solver
from oracle import ref_dynamics as OD

from .common import DENSITY, K_ROT, K_SHEAR, K_STRETCH, Case, paper_damping, relerr
from .parity import RTOL_GRAD, T64
from .test_gpu_tangent import FAST, _case, _explicit_inertia, _per_bond, _tangent_tree, _tree_dot

pytestmark = pytest.mark.gpu

ZERO = dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None))


def _scaled(cp, f):
    bp = cp.mechanical_params.bond_params
    return cp._replace(mechanical_params=cp.mechanical_params._replace(
        bond_params=bp._replace(k_stretch=bp.k_stretch * f, k_shear=bp.k_shear * f, k_rot=bp.k_rot * f)))


def _batch3(lattice):
    """The inputs of parity.check_adaptive_records_adjoint, three members with stiffnesses x 1 / 2.5 / 0.4."""
    c = Case(lattice, 4, True, True, seed=9, cutoff_deg=125.0 if lattice == "kagome" else 42.0, batch=3)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    ts = np.linspace(0, 3e-4, 61)
    c.solver.rtol = c.solver.atol = 1e-5
    y0 = c.random_state(0.05, 0.02, 5.0)
    return c, [_scaled(c.cp, f) for f in (1.0, 2.5, 0.4)], ts, y0


def _steps_of(s, ts):
    """(step boundaries t_0 .. t_N, outputs per step) of every member of the last adaptive-dense jvp."""
    grid, ns = s.stats["step_times"], s.stats["steps_per_member"]
    op, _ = b.dense_output_map(grid, ns, ts)
    return [grid[m, :n + 1] for m, n in enumerate(ns)], [np.diff(op[m, :n + 1]) for m, n in enumerate(ns)]


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_the_fields_are_the_fields_of_the_default_call(lattice):
    c, cps, ts, y0 = _batch3(lattice)
    s = c.solver
    ref = s(y0, ts, cps)
    assert s.stats["step_control"] == "adaptive"
    cd = ZERO._replace(constraint_params=dict(amplitude=1.0))
    fields, fdot = s.jvp(y0, ts, cps, None, cd, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and s.stats["kept_trajectory"]
    times, per_step = _steps_of(s, ts)
    ns = s.stats["steps_per_member"]
    print(lattice, "steps", ns, "max outputs per step", [int(p.max()) for p in per_step], "steps without output",
          [int((p == 0).sum()) for p in per_step], "last step beyond ts[-1] by", [float(t[-1] - ts[-1]) for t in times])
    assert len(set(ns)) == 3, ns                                                            # every member on its own clock
    for t, p in zip(times, per_step):
        assert p.max() >= 2 and (p == 0).any() and (p == 1).any(), p                        # steps with no, one and several outputs
        assert t[-1] > ts[-1]                                                               # the zero-size step is exercised
    e = relerr(fields, ref)
    print(lattice, "relerr(jvp(adaptive=True)[0], solve_dynamics(state0, ts, cps)) =", e)
    assert e < 1e-10, e
    assert np.abs(fdot).max() > 0.0
    # the default (no flag, no grid) is what it was: the frozen grid of the slowest member, whose fields are a re-integration
    f_grid, _ = s.jvp(y0, ts, cps, None, cd)
    assert s.stats["step_control"] == "adaptive-grid"
    print(lattice, "the frozen-grid re-integration is", relerr(f_grid, ref), "from the call's fields")


NAMES = ["cnv", "refv", "ks", "ksh", "kr", "inertia", "damping", "amplitude", "loading_rate", "input_delay", "state0"]
CASES = [(lat, nl, ct) for lat in ("quads", "kagome") for nl in (True, False) for ct in (True, False)]


@pytest.mark.parametrize("lattice,nonlinear,contact", CASES)
def test_tangent_matches_autograd_through_the_replay_of_the_accepted_steps(lattice, nonlinear, contact):
    c = _case(lattice, 4, nonlinear, contact, seed=9)
    rng = np.random.default_rng(3)
    c.cp = _per_bond(c)
    cp, inertia = _explicit_inertia(c)
    ts = np.linspace(0, 3e-4, 61)
    s = c.solver
    s.rtol = s.atol = 1e-5
    y0 = c.random_state(0.05, 0.02, 5.0)
    y0d = c.random_state(0.05, 0.02, 5.0)
    cd = _tangent_tree(c, rng, inertia)
    fields, fdot = s.jvp(y0, ts, cp, y0d, cd, adaptive=True)
    times, per_step = _steps_of(s, ts)
    assert per_step[0].max() >= 2 and (per_step[0] == 0).any(), per_step[0]
    # the oracle: the replay of the ENGINE's accepted steps on the autograd tape, every leaf seeded at once
    osol = c.oracle_solver(integrator="adaptive", rtol=1e-5, atol=1e-5)
    free = osol.free_DOF_ids
    mp, md = cp.mechanical_params, cd.mechanical_params
    names = list(NAMES)
    prim = dict(cnv=c.cnv, refv=np.broadcast_to(c.refv, (len(c.bonds), 2)), ks=mp.bond_params.k_stretch, ksh=mp.bond_params.k_shear,
                kr=mp.bond_params.k_rot, inertia=inertia, damping=mp.damping, state0=y0, **FAST)
    tan = dict(cnv=cd.geometrical_params.centroid_node_vectors, refv=md.bond_params.reference_vector, ks=md.bond_params.k_stretch,
               ksh=md.bond_params.k_shear, kr=md.bond_params.k_rot, inertia=md.inertia, damping=md.damping, state0=y0d,
               **cd.constraint_params)
    if contact:
        names += ["min_angle", "cutoff_angle", "k_contact"]
        prim.update(min_angle=mp.contact_params.min_angle, cutoff_angle=mp.contact_params.cutoff_angle, k_contact=mp.contact_params.k_contact)
        tan.update(min_angle=md.contact_params.min_angle, cutoff_angle=md.contact_params.cutoff_angle, k_contact=md.contact_params.k_contact)

    def f(*xs):
        lv = dict(zip(names, xs))
        y0t = lv.pop("state0")
        hist, _ = OD.solve_adaptive_replay_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(lv), times[0])
        return hist
    of, ojv = torch.autograd.functional.jvp(f, tuple(T64(prim[k]) for k in names), tuple(T64(tan[k]) for k in names))
    n = len(ts)
    e0 = relerr(fields.reshape(n, 2, -1)[:, :, free], of.detach().numpy())
    e = relerr(fdot.reshape(n, 2, -1)[:, :, free], ojv.numpy())
    print(lattice, nonlinear, contact, "steps", len(times[0]) - 1, "primal", e0, "tangent", e)
    assert e0 < 1e-10, e0
    assert e < RTOL_GRAD, (lattice, nonlinear, contact, e)
    if contact:
        # the contact constants must matter, or the check above says nothing about them
        cd0 = cd._replace(mechanical_params=md._replace(contact_params=dm.ContactParams(0.0, 0.0, 0.0)))
        _, fdot0 = s.jvp(y0, ts, cp, y0d, cd0, adaptive=True)
        assert np.abs(fdot0 - fdot).max() > 1e-6 * np.abs(fdot).max()


def _replay_jvp(c, osol, ts, times, names, prim, tan, make_cp):
    def f(*xs):
        lv = dict(zip(names, xs))
        hist, _ = OD.solve_adaptive_replay_differentiable(osol, c.ogeo, lv.pop("state0"), ts, make_cp(lv), times)
        return hist
    return torch.autograd.functional.jvp(f, tuple(T64(prim[k]) for k in names), tuple(T64(tan[k]) for k in names))


def test_distance_contact_tangent_matches_autograd():
    """Physics the kept-steps reverse path does not serve: the adaptive pass keeps nothing, the tangent pass needs only its clocks."""
    from .test_distance_contact import DistCase
    c = DistCase("quads", None, n=4, seed=5)
    rng = np.random.default_rng(13)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 31)
    y0 = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02]) * np.array([[1.0], [5.0]])[:, :, None]
    y0d = rng.normal(size=y0.shape) * np.abs(y0).max()
    cd = dm.ControlParams(dm.GeometricalParams(0.05 * rng.normal(size=np.shape(c.cen)), 0.02 * rng.normal(size=np.shape(c.cnv))),
                          dm.MechanicalParams(None, None, None, None, dm.ContactParams(0.02, -0.03, 0.05)),
                          constraint_params=dict(amplitude=0.2))
    fields, fdot = s.jvp(y0, ts, c.cp, y0d, cd, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and not s.stats["kept_trajectory"]
    with pytest.raises(RuntimeError, match="keep_trajectory"):
        s.vjp(np.zeros_like(fields))
    times, per_step = _steps_of(s, ts)
    osol = c.oracle_solver(integrator="adaptive", rtol=1e-5, atol=1e-5)
    free = osol.free_DOF_ids
    names = ["cnv", "cen", "min", "cutoff", "k", "amplitude", "state0"]
    prim = dict(cnv=c.cnv, cen=c.cen, min=c.contact_params[0], cutoff=c.contact_params[1], k=c.contact_params[2], amplitude=c.pulse["amplitude"],
                state0=y0)
    tan = dict(cnv=cd.geometrical_params.centroid_node_vectors, cen=cd.geometrical_params.block_centroids, min=0.02, cutoff=-0.03, k=0.05,
               amplitude=0.2, state0=y0d)
    of, ojv = _replay_jvp(c, osol, ts, times[0], names, prim, tan,
                          lambda lv: c.oracle_cp(cnv=lv["cnv"], cen=lv["cen"], contact=[lv["min"], lv["cutoff"], lv["k"]], amplitude=lv["amplitude"]))
    n = len(ts)
    e0 = relerr(fields.reshape(n, 2, -1)[:, :, free], of.detach().numpy())
    e = relerr(fdot.reshape(n, 2, -1)[:, :, free], ojv.numpy())
    print("distance contact: steps", len(times[0]) - 1, "outputs per step", per_step[0], "primal", e0, "tangent", e)
    assert e0 < 1e-10 and e < RTOL_GRAD, (e0, e)
    _, fdot0 = s.jvp(y0, ts, c.cp, y0d, cd._replace(mechanical_params=dm.MechanicalParams(None, None)), adaptive=True)
    assert np.abs(fdot0 - fdot).max() > 1e-6 * np.abs(fdot).max()


def test_spring_model_tangent_matches_autograd():
    from .test_spring_models import SpringCase
    c = SpringCase("torsion", None, seed=5)
    rng = np.random.default_rng(17)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 31)
    y0 = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02]) * np.array([[1.0], [5.0]])[:, :, None]
    y0d = rng.normal(size=y0.shape) * np.abs(y0).max()
    ksd, krd = 0.1 * rng.normal(size=c.ks.shape) * c.ks, 0.1 * rng.normal(size=c.kr.shape) * c.kr
    cd = dm.ControlParams(dm.GeometricalParams(None, 0.02 * rng.normal(size=np.shape(c.cnv))),
                          dm.MechanicalParams(dm.StretchingTorsionalSpringParams(ksd, krd), None),
                          constraint_params=dict(amplitude=0.2))
    fields, fdot = s.jvp(y0, ts, c.cp, y0d, cd, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and not s.stats["kept_trajectory"]
    times, per_step = _steps_of(s, ts)
    osol = c.oracle_solver(integrator="adaptive", rtol=1e-5, atol=1e-5)
    free = osol.free_DOF_ids
    names = ["cnv", "ks", "kr", "amplitude", "state0"]
    prim = dict(cnv=c.cnv, ks=c.ks, kr=c.kr, amplitude=c.pulse["amplitude"], state0=y0)
    tan = dict(cnv=cd.geometrical_params.centroid_node_vectors, ks=ksd, kr=krd, amplitude=0.2, state0=y0d)
    of, ojv = _replay_jvp(c, osol, ts, times[0], names, prim, tan,
                          lambda lv: c.oracle_cp(cnv=lv["cnv"], ks=lv["ks"], kr=lv["kr"], amplitude=lv["amplitude"]))
    n = len(ts)
    e0 = relerr(fields.reshape(n, 2, -1)[:, :, free], of.detach().numpy())
    e = relerr(fdot.reshape(n, 2, -1)[:, :, free], ojv.numpy())
    print("stretching + torsional springs: steps", len(times[0]) - 1, "outputs per step", per_step[0], "primal", e0, "tangent", e)
    assert e0 < 1e-10 and e < RTOL_GRAD, (e0, e)


def _transpose_gap(s, B, ts, y0, cps, trees, seed=11, scale_state0=None):
    """|<fb, fields_dot> - (<tree_bar, tangent> + <state0_bar, state0_dot>)| / max(|lhs|, |rhs|): jvp(adaptive=True), then vjp WITHOUT another solve."""
    rng = np.random.default_rng(seed)
    nb = s.n_blocks
    y0d = rng.normal(size=(B, 2, nb, 3)) * (np.abs(y0).max() if scale_state0 is None else scale_state0)
    y0d.reshape(B, 2, -1)[:, :, s.constrained_DOF_ids] = 0.0          # (state0 of prescribed DOFs is not read)
    solves = s.solve_count
    fields, fdot = s.jvp(y0, ts, cps, y0d, trees, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and s.stats["kept_trajectory"]
    fb = rng.normal(size=fields.shape)
    fb.reshape(B, len(ts), 2, -1)[:, :, :, s.constrained_DOF_ids] = 0.0
    bars, s0b = s.vjp(fb)
    assert s.solve_count == solves
    if B == 1:
        bars, s0b = [bars], np.asarray(s0b)[None]
    lhs = float(np.sum(fb * fdot))
    rhs = sum(_tree_dot(bars[m], trees[m]) for m in range(B)) + float(np.sum(np.asarray(s0b) * y0d))
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs)), lhs, rhs


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_it_is_the_transpose_of_vjp_on_the_same_solve(lattice):
    c, cps, ts, y0 = _batch3(lattice)
    rng = np.random.default_rng(7)
    c.cp = _per_bond(c)
    cps = [_scaled(c.cp, f) for f in (1.0, 2.5, 0.4)]
    y0 = np.stack([y0] * 3)
    gap, lhs, rhs = _transpose_gap(c.solver, 3, ts, y0, cps, [_tangent_tree(c, rng, scale=1.0 + m) for m in range(3)])
    print(lattice, "steps", c.solver.stats["steps_per_member"], "transposition gap", gap, lhs, rhs)
    assert gap <= 1e-11, (gap, lhs, rhs)


def test_it_is_the_transpose_of_vjp_128x128_contact():
    """At size: 128 x 128 quads with contact, tolerances chosen for a few hundred accepted steps (the fixed-grid identity holds 1e-11 at 500
    steps on this lattice, tests/test_gpu_tangent.py)."""
    c = _case("quads", 128, True, True, batch=1, seed=2)
    c.cp = _per_bond(c)
    rng = np.random.default_rng(4)
    s = c.solver
    s.rtol, s.atol = 1e-10, 1e-10         # (186 accepted steps at 1e-9 on the CPU port; steps ~ tol^-1/5)
    ts = np.linspace(0, 3e-4, 13)
    y0 = c.random_state(0.05, 0.02, 5.0)[None]
    gap, lhs, rhs = _transpose_gap(s, 1, ts, y0, [c.cp], [_tangent_tree(c, rng)])
    n = s.stats["steps_per_member"][0]
    print("128 x 128: accepted steps", n, "transposition gap", gap, lhs, rhs)
    assert 200 <= n <= 600, n
    assert gap <= 1e-11, (gap, lhs, rhs)


def test_it_is_the_transpose_of_vjp_on_the_paper_lattice():
    """24 x 16 quads with contact and damping, rtol 1e-8 / atol 1e-4, 200 outputs over 2 / 30 s: ~1 600 accepted steps, a horizon no
    transposition test of the suite reaches.  The bound is therefore not fixed in advance: the same identity is measured on the frozen grid
    of this solve (jvp(step_times=grid) against vjp on the "adaptive-grid" path, both fixed-grid code that the identity at 1e-11 / 500 steps
    vouches for), and the adaptive pair is allowed 10 x that value -- two linearisation points that differ by rounding, amplified over the
    same horizon.  Measured on the MI355X (profiles/r08_tangent_adaptive.txt): PAPER_GAPS below."""
    n1, n2 = 24, 16
    g = geo.QuadGeometry(n1, n2, 15.0, 2.25)
    rng = np.random.default_rng(0)
    design = tuple(x + rng.uniform(-0.3, 0.3, x.shape) for x in g.get_design_from_rotated_square(25 * math.pi / 180))
    bonds = g.bond_connectivity()
    energy = en_mod.combine_block_energies(en_mod.build_strain_energy(bonds, en_mod.ligament_energy), en_mod.build_contact_energy(bonds))
    left = np.arange(0, n1 * n2, n1)[n2 // 2 - 1:n2 // 2 + 1]             # two excited blocks on the left edge
    con = np.array([[blk, d] for blk in left for d in range(3)])
    vec = np.array([1.0 if d == 0 else 0.0 for blk in left for d in range(3)])
    s = setup_dynamic_solver(g, energy, constrained_block_DOF_pairs=con, constrained_DOFs_fn=ld.Pulse(vec), damped_blocks=np.arange(n1 * n2))
    s.rtol, s.atol = 1e-8, 1e-4
    nbd = len(bonds)
    cp = dm.ControlParams(dm.GeometricalParams(g.block_centroids(*design), g.centroid_node_vectors(*design)),
                          dm.MechanicalParams(dm.LigamentParams(np.full(nbd, K_STRETCH), np.full(nbd, K_SHEAR), np.full(nbd, K_ROT),
                                                                g.reference_bond_vectors()), DENSITY, None,
                                              paper_damping() * np.ones((n1 * n2, 1)), dm.ContactParams(-15 * math.pi / 180, -10 * math.pi / 180, K_ROT)),
                          constraint_params=dict(amplitude=7.5, loading_rate=30.0, input_delay=0.1 / 30.0))
    cd = dm.ControlParams(dm.GeometricalParams(None, 0.02 * rng.normal(size=np.shape(cp.geometrical_params.centroid_node_vectors))),
                          dm.MechanicalParams(dm.LigamentParams(rng.normal(size=nbd) * K_STRETCH, rng.normal(size=nbd) * K_SHEAR,
                                                                rng.normal(size=nbd) * K_ROT, None), 0.1 * DENSITY, None,
                                              0.1 * paper_damping() * np.ones((n1 * n2, 1)), dm.ContactParams(0.01, -0.02, 0.05)),
                          constraint_params=dict(amplitude=0.5, loading_rate=1.0, input_delay=1e-4))
    ts = np.linspace(0.0, 2.0 / 30.0, 200)
    y0 = np.zeros((1, 2, n1 * n2, 3))
    gap, lhs, rhs = _transpose_gap(s, 1, ts, y0, [cp], [cd], scale_state0=1e-3)
    n_acc = s.stats["steps_per_member"][0]
    # the yardstick: the fixed-grid pair on the frozen grid of the same solve
    _, flats = s.prepare(cp)
    spi, grid = s.adaptive_grid(y0, ts, flats)
    rng2 = np.random.default_rng(11)
    y0d = rng2.normal(size=y0.shape) * 1e-3
    y0d.reshape(1, 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    _, fdot = s.jvp(y0[0], ts, cp, y0d[0], cd, steps_per_interval=spi, step_times=grid)
    fields = s(y0[0], ts, cp, keep_trajectory=True, steps_per_interval=spi, step_times=grid)
    fb = rng2.normal(size=fields.shape)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    bars, s0b = s.vjp(fb)
    lhs_g = float(np.sum(fb * fdot))
    rhs_g = _tree_dot(bars, cd) + float(np.sum(np.asarray(s0b) * y0d[0]))
    gap_g = abs(lhs_g - rhs_g) / max(abs(lhs_g), abs(rhs_g))
    print("paper lattice: accepted steps", n_acc, "frozen-grid steps", int(np.sum(spi)), "transposition gap adaptive-dense", gap,
          "frozen grid", gap_g, "bound", 10 * gap_g)
    assert n_acc >= 1000, n_acc
    assert gap <= 10.0 * gap_g, (gap, gap_g)


# (accepted steps, steps of the frozen grid, gap of the adaptive pair, gap of the frozen-grid pair) as measured on the MI355X
PAPER_GAPS = (2421, 2616, 5.0e-12, 6.7e-12)


def test_grids_are_refused_with_the_flag_and_the_default_is_unchanged():
    c = _case("quads", 4, True, True, seed=10)
    s = c.solver
    ts = np.linspace(0, 1e-4, 5)
    y0 = c.random_state(0.05, 0.02, 5.0)
    cd = ZERO._replace(constraint_params=dict(amplitude=1.0))
    with pytest.raises(ValueError, match="adaptive=True"):
        s.jvp(y0, ts, c.cp, None, cd, adaptive=True, steps_per_interval=4)
    with pytest.raises(ValueError, match="adaptive=True"):
        s.jvp(y0, ts, c.cp, None, cd, adaptive=True, steps_per_interval=1, step_times=ts)
    with pytest.raises(ValueError, match="per-member timepoints"):
        s.jvp(y0, ts[None], c.cp, None, cd, adaptive=True)
    s.grid_refine = 2
    with pytest.raises(ValueError, match="grid_refine"):
        s.jvp(y0, ts, c.cp, None, cd, adaptive=True)
    s.grid_refine = 1
    s.rtol = s.atol = 1e-6
    # a zero tangent gives exactly zero
    fields, fdot = s.jvp(y0, ts, c.cp, None, ZERO, adaptive=True)
    assert s.stats["step_control"] == "adaptive-dense" and np.all(fdot == 0.0)
    assert relerr(fields, s(y0, ts, c.cp)) < 1e-10
    # one timepoint: the initial state and its tangent
    y0d = c.random_state(0.05, 0.02, 5.0)
    f1, d1 = s.jvp(y0, ts[:1], c.cp, y0d, ZERO, adaptive=True)
    free = s.free_DOF_ids
    assert np.array_equal(f1.reshape(1, 2, -1)[:, :, free], y0.reshape(1, 2, -1)[:, :, free])
    assert np.array_equal(d1.reshape(1, 2, -1)[:, :, free], y0d.reshape(1, 2, -1)[:, :, free])
    # no flag, no grid: the frozen grid, as before
    s.jvp(y0, ts, c.cp, None, cd)
    assert s.stats["step_control"] == "adaptive-grid"


def test_extra_ligaments_are_refused_and_the_handle_still_works():
    c = _case("quads", 4, True, False, seed=12, extra_bonds=[[1, 6], [9, 14]])
    ts = np.linspace(0, 1e-4, 3)
    y0 = c.random_state(0.05, 0.02, 5.0)
    cd = ZERO._replace(constraint_params=dict(amplitude=1.0))
    with pytest.raises(RuntimeError, match="more than one ligament"):
        c.solver.jvp(y0, ts, c.cp, None, cd, adaptive=True)
    fields = c.solver(y0, ts, c.cp, steps_per_interval=4)
    assert np.all(np.isfinite(fields)) and np.abs(fields).max() > 0
    # and a lattice without them on the same process still runs the adaptive tangent
    c2 = _case("quads", 4, True, False, seed=12)
    c2.solver.rtol = c2.solver.atol = 1e-5
    _, fdot = c2.solver.jvp(y0, ts, c2.cp, None, cd, adaptive=True)
    assert c2.solver.stats["step_control"] == "adaptive-dense" and np.abs(fdot).max() > 0


def test_the_entry_point_refuses_bad_step_times_and_leaves_the_kept_solve_alone():
    c = _case("quads", 4, True, True, seed=14)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 16)
    y0 = c.random_state(0.05, 0.02, 5.0)
    rng = np.random.default_rng(1)

    def solve_and_vjp(between):
        fields = s(y0, ts, c.cp, keep_trajectory=True)
        assert s.stats["step_control"] == "adaptive-records"
        fb = np.random.default_rng(2).normal(size=fields.shape)
        between()
        tree, s0b = s.vjp(fb)
        return tree, s0b

    seen = {}

    def tangent_in_between():
        e = s.engine
        grid, ns = b.padded_step_times([e.adaptive_step_times(0)], ts[0])
        dots = {"fn_params": np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]]), "k_bond": rng.normal(size=(1, len(c.bonds), 3))}
        f, fd, _ = e.forward_tangent_dense(y0[None], None, dots, ts, grid, ns)
        seen["fields"], seen["fdot"] = f, fd
        # refusals: the handle says why, and goes on working
        for bad, msg in ((np.concatenate([grid[:, :3], grid[:, 2:-1]], 1), "strictly increasing"), (grid + 1e-7, "t_0"),
                         (grid[:, :ns[0] - 1], "last step")):
            n_bad = np.array([bad.shape[1] - 1])
            with pytest.raises(RuntimeError, match=msg):
                e.forward_tangent_dense(y0[None], None, dots, ts, bad, n_bad)
    t1, s1 = solve_and_vjp(tangent_in_between)
    t0, s0 = solve_and_vjp(lambda: None)
    assert np.abs(seen["fdot"]).max() > 0 and relerr(seen["fields"][0], s._last_fields[0]) < 1e-10
    assert np.array_equal(np.asarray(s1), np.asarray(s0))
    for a, bb in zip(_leaves(t1), _leaves(t0)):
        assert np.array_equal(a, bb)
    # a tableau other than dopri5 has no dense output
    c4 = _case("quads", 4, True, True, integrator="rk4", seed=14)
    c4.solver.prepare(c4.cp)
    grid, ns = b.padded_step_times([np.array([2e-4])], 0.0)
    with pytest.raises(RuntimeError, match="dopri5"):
        c4.solver.engine.forward_tangent_dense(y0[None], None, {}, ts, grid, ns)


def _leaves(tree):
    if tree is None:
        return []
    if isinstance(tree, dict):
        return [np.asarray(v, dtype=float) for _, v in sorted(tree.items())]
    if isinstance(tree, tuple) and hasattr(tree, "_fields"):
        return [x for f in tree._fields for x in _leaves(getattr(tree, f))]
    return [np.asarray(tree, dtype=float)]


def test_a_flagged_member_fails_the_call():
    """A member the adaptive pass flagged (here: out of its step budget, failure policy = isolate) has no solve to differentiate."""
    c = _case("quads", 4, True, True, seed=14, batch=2)
    s = c.solver
    s.rtol = s.atol = 1e-5
    ts = np.linspace(0, 1.5e-4, 16)
    y0 = c.random_state(0.05, 0.02, 5.0)
    s(y0, ts, c.cp)
    grid, ns = b.padded_step_times([s.engine.adaptive_step_times(m) for m in range(2)], ts[0])
    s.engine.set_failure_policy(True)
    s.max_attempts = 3
    s(y0, ts, c.cp)
    assert list(s.engine.member_status()) == [3, 3]
    with pytest.raises(RuntimeError, match="flagged"):
        s.engine.forward_tangent_dense(np.stack([y0] * 2), None, None, ts, grid, ns)
    s.engine.set_failure_policy(False)
    s.max_attempts = 10_000_000
    fields, fdot = s.jvp(y0, ts, c.cp, None, ZERO._replace(constraint_params=dict(amplitude=1.0)), adaptive=True)
    assert np.all(np.isfinite(fdot)) and np.abs(fdot).max() > 0 and list(s.stats["steps_per_member"]) == [int(n) for n in ns]
