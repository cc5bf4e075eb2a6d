"""Forward mode, host side (no GPU): the JVPs of the derived ControlParams leaves, the tangent of the flattening, and the CPU port's
refusal.  The kernel side is tests/test_gpu_tangent.py."""
import math

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import energy as en_mod
from difflexmm_amd import geometry as geo
from difflexmm_amd import loading as ld
from difflexmm_amd.dynamics import setup_dynamic_solver
from oracle import ref_geometry as OG

from .common import DENSITY, Case, relerr


def _design(lattice="quads", seed=3):
    return Case(lattice, 4, True, True, seed=seed, lib=_cpu(), cutoff_deg=42.0)


def _cpu():
    from oracle.cpu import load
    return load()


def _central(f, x, dx, eps):
    return (np.asarray(f(x + eps * dx)) - np.asarray(f(x - eps * dx))) / (2 * eps)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_inertia_and_void_angle_jvps(lattice):
    c = _design(lattice)
    rng = np.random.default_rng(1)
    cnv = np.asarray(c.cnv, dtype=float)
    cnv_dot = rng.normal(size=cnv.shape)
    rho_dot = 0.3 * DENSITY
    mine_m = geo.compute_inertia_jvp(cnv, DENSITY, cnv_dot, rho_dot)
    mine_phi = geo.void_angles0_jvp(cnv, c.bonds, cnv_dot)
    # central differences (step relative to the node vectors)
    eps = 1e-6 * np.abs(cnv).max()
    fd_m = _central(lambda x: geo.compute_inertia(x, DENSITY), cnv, cnv_dot, eps) + \
        _central(lambda r: geo.compute_inertia(cnv, r), DENSITY, rho_dot, 1e-6)
    fd_phi = _central(lambda x: geo.void_angles0(x, c.bonds), cnv, cnv_dot, eps)
    assert relerr(mine_m, fd_m) < 1e-7
    assert relerr(mine_phi, fd_phi) < 1e-7
    # torch.autograd through the oracle's restatements
    T = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))       # noqa: E731
    _, ref_m = torch.autograd.functional.jvp(lambda x, r: OG.compute_inertia(x, r), (T(cnv), T(DENSITY)), (T(cnv_dot), T(rho_dot)))
    _, ref_phi = torch.autograd.functional.jvp(lambda x: torch.stack(OG.compute_edge_angles(x, c.bonds)[:2], 1), T(cnv), T(cnv_dot))
    assert relerr(mine_m, ref_m.numpy()) < 1e-12
    assert relerr(mine_phi, ref_phi.numpy()) < 1e-12


def _terms():
    drive = ld.static_tuning_drive(np.array([1.0, 0.0]), np.array([0.0, 1.0]), length=60.0)
    table = ld.Table([0.0, 1e-3, 2e-3, 5e-3], [0.0, 1.0, -0.5, 0.25], amplitude="amplitude", delay="input_delay")
    return {"pulse": [ld.Pulse()], "ramp_cap_pulse": drive.terms, "table": [table]}


PARAMS = dict(amplitude=7.5, loading_rate=30.0, input_delay=3e-3, compressive_strain=0.07, compressive_strain_rate=2.5)


def _torch_resolve(term, p):
    """Restatement of resolve in torch (the delayed pulse's chain: delay = strain / rate + input_delay)."""
    vals = [p[term.params[n]] if isinstance(term.params[n], str) else torch.tensor(float(term.params[n]), dtype=torch.float64) for n in term.param_names]
    if isinstance(term, ld.DelayedPulse):
        vals[2] = vals[2] + p[term.strain] / p[term.strain_rate]
    return torch.stack(vals + [torch.zeros((), dtype=torch.float64)] * (5 - len(vals)))


@pytest.mark.parametrize("which", ["pulse", "ramp_cap_pulse", "table"])
def test_fn_params_resolution_jvp(which):
    rng = np.random.default_rng(5)
    dot = {k: float(rng.normal()) * v for k, v in PARAMS.items()}
    dot["loading_rate"] = None                      # None: zero tangent
    del dot["amplitude"]                            # missing key: zero tangent
    for term in _terms()[which]:
        mine = term.resolve_jvp(PARAMS, dot)
        d = {k: (v or 0.0) for k, v in dot.items()}
        eps = 1e-6
        fd = (term.resolve({k: v + eps * d.get(k, 0.0) for k, v in PARAMS.items()})
              - term.resolve({k: v - eps * d.get(k, 0.0) for k, v in PARAMS.items()})) / (2 * eps)
        assert relerr(mine, fd) < 1e-7, (which, mine, fd)
        keys = sorted(PARAMS)
        _, ref = torch.autograd.functional.jvp(lambda *xs: _torch_resolve(term, dict(zip(keys, xs))),
                                               tuple(torch.tensor(PARAMS[k], dtype=torch.float64) for k in keys),
                                               tuple(torch.tensor(d.get(k, 0.0), dtype=torch.float64) for k in keys))
        assert relerr(mine, ref.numpy()) < 1e-12, (which, mine, ref)
        if which != "pulse":
            assert np.any(mine != 0.0)


def _solver_and_tree(model, contact, scalar_k=True):
    """A quads lattice with every kind of leaf: scalar or per-bond stiffnesses, density-derived inertia, damping on some blocks,
    contact constants, a pulse on the driven block and a ramp load."""
    g = geo.QuadGeometry(4, 4, 15.0, 2.25)
    rng = np.random.default_rng(2)
    design = tuple(b + rng.uniform(-0.3, 0.3, b.shape) for b in g.get_design_from_rotated_square(25 * math.pi / 180))
    cnv, cen = g.centroid_node_vectors(*design), g.block_centroids(*design)
    bonds = g.bond_connectivity()
    nbd = len(bonds)
    efn = {"nonlinear": en_mod.ligament_energy, "linearized": en_mod.ligament_energy_linearized,
           "simple_spring": en_mod.simple_spring_energy, "stretch_torsion": en_mod.stretching_torsional_spring_energy}[model]
    energy = en_mod.build_strain_energy(bonds, efn)
    if contact:
        energy = en_mod.combine_block_energies(energy, en_mod.build_contact_energy(bonds))
    s = setup_dynamic_solver(g, energy, loaded_block_DOF_pairs=np.array([[5, 0], [6, 1]]), loading_fn=ld.Ramp(amplitude="load", rate=30.0),
                             constrained_block_DOF_pairs=np.array([[8, 0], [0, 1]]), constrained_DOFs_fn=ld.Pulse(np.array([1.0, 0.0])),
                             damped_blocks=np.array([1, 2, 7]), _lib=_cpu())
    k = (120.0, 1.19, 1.5) if scalar_k else tuple(v * (1 + 0.1 * rng.uniform(-1, 1, nbd)) for v in (120.0, 1.19, 1.5))
    bp = dm.StretchingTorsionalSpringParams(k[0], k[2]) if model == "stretch_torsion" else dm.LigamentParams(*k, g.reference_bond_vectors())
    cp = dm.ControlParams(dm.GeometricalParams(cen, cnv),
                          dm.MechanicalParams(bp, DENSITY, None, np.array([1e-4, 2e-4, 3e-6]),
                                              dm.ContactParams(-0.2, 0.7, 1.5) if contact else None),
                          loading_params=dict(load=0.5), constraint_params=dict(PARAMS))

    def leafdot(x):
        return rng.normal(size=np.shape(x)) * (np.abs(x) + 1e-3 if np.ndim(x) else abs(x) + 1e-3)
    bd = type(bp)(*[leafdot(v) for v in bp])
    cd = dm.ControlParams(dm.GeometricalParams(leafdot(cen), leafdot(cnv)),
                          dm.MechanicalParams(bd, 0.2 * DENSITY, None, leafdot(cp.mechanical_params.damping),
                                              dm.ContactParams(0.01, 0.02, 0.3) if contact else None),
                          loading_params=dict(load=0.3), constraint_params=dict(amplitude=0.7, input_delay=1e-4))
    return s, cp, cd


def _axpy(cp, cd, eps):
    """cp + eps cd over the leaves cd holds (None / missing: 0)."""
    def add(x, d):
        if d is None:
            return x
        if isinstance(x, tuple) and hasattr(x, "_fields"):
            return type(x)(*[add(a, getattr(d, f, None)) for f, a in zip(x._fields, x)])
        if isinstance(x, dict):
            return {k: v + eps * (d.get(k) or 0.0) for k, v in x.items()}
        if x is None:
            return None
        return np.asarray(x, dtype=float) + eps * np.asarray(d, dtype=float)
    return add(cp, cd)


@pytest.mark.parametrize("model,contact,scalar_k", [("nonlinear", True, True), ("nonlinear", False, False), ("linearized", True, False),
                                                    ("simple_spring", False, True), ("stretch_torsion", True, False)])
def test_flatten_tangent_is_the_derivative_of_flatten(model, contact, scalar_k):
    s, cp, cd = _solver_and_tree(model, contact, scalar_k)
    mine = s._flatten_tangent(cp, cd)
    eps = 1e-6
    plus, minus = s._flatten(_axpy(cp, cd, eps)), s._flatten(_axpy(cp, cd, -eps))
    assert sorted(mine) == sorted(plus)
    for k in mine:
        fd = (np.asarray(plus[k]) - np.asarray(minus[k])) / (2 * eps)
        assert mine[k].shape == np.shape(plus[k]), k
        assert np.abs(mine[k] - fd).max() <= 1e-7 * max(np.abs(fd).max(), 1e-300) + 1e-12, (k, relerr(mine[k], fd))
    # linear in the tangent: 2 cd -> twice the arrays; an all-None tangent -> zeros
    twice = s._flatten_tangent(cp, _axpy(cd, cd, 1.0))
    for k in mine:
        assert np.allclose(twice[k], 2 * mine[k], rtol=1e-14, atol=0.0), k
    empty = dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None))
    for k, v in s._flatten_tangent(cp, empty).items():
        assert not np.any(v), k
    if model == "simple_spring":
        assert not np.any(mine["k_bond"][:, 1:])        # what the model does not read has no tangent
    if model == "stretch_torsion":
        assert not np.any(mine["k_bond"][:, 1])


def test_jvp_on_the_cpu_port_is_not_implemented():
    c = _design()
    ts = np.linspace(0.0, 1e-4, 3)
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent"):
        c.solver.jvp(np.zeros((2, 16, 3)), ts, c.cp, None, c.cp, steps_per_interval=2)
