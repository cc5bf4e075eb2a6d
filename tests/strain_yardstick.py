"""The yardstick of the ligament strain-energy objective (include/dfx.h: dfx_strain_objective_value[_and_grad]) shared by the host and the
GPU tests: the objective written with ``oracle.ref_energy``'s own bond and contact energies in torch, so that autograd gives the value, the
cotangent on the displacement history and every explicit parameter term.

    J = sum_k tau_k sum_bonds w_b [ c_stretch E_stretch + c_shear E_shear + c_bend E_bend + c_contact E_contact ]

The bond energies are linear in the stiffnesses, so the weighted parts are the oracle's energy called with (c_stretch k_stretch,
c_shear k_shear, c_bend k_rot); the contact part is the oracle's penalty (``contact_energy``, linear in k_contact) on the two void angles
of the bond written as the engine parametrises them -- wrap(phi1 - kappa), wrap(phi2 + kappa) with phi the undeformed void angles (a leaf:
the raw ``void_angle0`` gradient) and kappa = theta_2 - theta_1 (rigid blocks: geometry.void_angles0).  ``void_angle_gap`` measures that
identity against the oracle's ``void_angles`` on the deformed nodes."""
import math

import numpy as np
import torch

from oracle import ref_energy as OE

MODELS = ("linearized", "nonlinear", "simple_spring", "stretch_torsion")


def T64(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=grad)


def _wrap(a):
    return a - 2 * math.pi * torch.round(a / (2 * math.pi))


def bond_energies(model, nodal, refv, ks, ksh, kr, parts):
    """(n_bonds,) weighted bond energy of the oracle's bond model."""
    c0, c1, c2 = parts[0], parts[1], parts[2]
    if model == "nonlinear":
        return OE.ligament_energy(nodal, refv, c0 * ks, c1 * ksh, c2 * kr)
    if model == "linearized":
        return OE.ligament_energy_linearized(nodal, refv, c0 * ks, c1 * ksh, c2 * kr)
    if model == "simple_spring":
        return OE.simple_spring_energy(nodal, refv, c0 * ks)
    if model == "stretch_torsion":
        return OE.stretching_torsional_spring_energy(nodal, c0 * ks, c2 * kr)
    raise ValueError(model)


def strain_objective(u_hist, cnv, bonds, refv, ks, ksh, kr, w, tau, parts, model="nonlinear", contact=None):
    """Scalar J of one member.  ``u_hist`` (T, n_blocks, 3) displacements, ``w`` (n_bonds,), ``tau`` (T,), ``contact`` = None or
    (phi0 (n_bonds, 2), min_angle, cutoff_angle, k_contact).  Every argument may be a torch leaf."""
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    total = torch.zeros((), dtype=torch.float64)
    for k in range(u_hist.shape[0]):
        nd = OE.block_to_node_kinematics(u_hist[k], cnv).reshape(-1, 3)
        nodal = (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]])
        e = bond_energies(model, nodal, refv, ks, ksh, kr, parts)
        if contact is not None and parts[3] != 0.0:
            phi0, am, ac, kc = contact
            kap = nodal[1][:, 2] - nodal[0][:, 2]
            e = e + OE.contact_energy(_wrap(phi0[:, 0] - kap), am, ac, parts[3] * kc) \
                  + OE.contact_energy(_wrap(phi0[:, 1] + kap), am, ac, parts[3] * kc)
        total = total + tau[k] * torch.sum(w * e)
    return total


def void_angle_gap(u, cen, cnv, bonds, phi0):
    """max |wrap(phi0 -/+ kappa) - oracle void angles of the deformed nodes| (mod 2 pi) for one configuration (NumPy in, float out)."""
    u, cnv_t = T64(u), T64(cnv)
    nd = OE.block_to_node_kinematics(u, cnv_t)
    nodes = T64(cen)[:, None] + cnv_t + nd[:, :, :2]
    a = OE.void_angles(nodes, bonds).numpy()
    th = np.asarray(u)[:, 2]
    b = np.asarray(bonds)
    npb = cnv_t.shape[1]
    kap = th[b[:, 1] // npb] - th[b[:, 0] // npb]
    mine = np.concatenate([phi0[:, 0] - kap, phi0[:, 1] + kap])
    d = mine - a
    return float(np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi))).max())
