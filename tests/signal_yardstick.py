"""The yardstick of the signal misfit (include/dfx.h: dfx_signal_values, dfx_signal_misfit_value[_and_grad]) for the GPU tests: signals and
misfit written in torch with ``oracle.ref_energy``'s own bond and contact energies,

    S_ks = sum over the terms of signal s: coef * channel(block, component; u_k, v_k, params)
    J    = 1/2 sum_k tau_k sum_s omega_s (S_ks - Starget_ks)^2

component 0..2 the displacement, 3..5 the velocity, 6..8 the elastic force: ``autograd.grad(E, u, create_graph=True)`` of the ligament plus
angle-contact energy, so that a second pass of autograd gives the cotangent on the history (a Hessian-vector product for the force terms)
and every explicit parameter term (mixed second derivatives).  Bond energies and the contact parametrisation -- wrap(phi1 - kappa),
wrap(phi2 + kappa) on the undeformed void angles, a leaf -- are those of tests/strain_yardstick.py."""
import numpy as np
import torch

from oracle import ref_energy as OE

from .strain_yardstick import T64, _wrap, bond_energies

LEAVES = ("cnv", "refv", "ks", "ksh", "kr", "phi0", "am", "ac", "kc")


def elastic_energy(u_hist, cnv, bonds, refv, ks, ksh, kr, model="nonlinear", contact=None):
    """Total ligament (+ angle-contact) energy of every output configuration, summed: the configurations do not interact, so its gradient
    w.r.t. ``u_hist`` (T, n_blocks, 3) is the elastic force at every output time."""
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    total = torch.zeros((), dtype=torch.float64)
    for k in range(u_hist.shape[0]):
        nd = OE.block_to_node_kinematics(u_hist[k], cnv).reshape(-1, 3)
        nodal = (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]])
        e = bond_energies(model, nodal, refv, ks, ksh, kr, (1.0, 1.0, 1.0))
        if contact is not None:
            phi0, am, ac, kc = contact
            kap = nodal[1][:, 2] - nodal[0][:, 2]
            e = e + OE.contact_energy(_wrap(phi0[:, 0] - kap), am, ac, kc) + OE.contact_energy(_wrap(phi0[:, 1] + kap), am, ac, kc)
        total = total + torch.sum(e)
    return total


def signals(terms, n_signals, u_hist, v_hist, force):
    """(T, n_signals): every signal adds its terms in list order.  ``force`` (T, n_blocks, 3) or None when no term needs it."""
    cols = [None] * n_signals
    for s, b, c, coef in terms:
        src = u_hist[:, b, c] if c < 3 else v_hist[:, b, c - 3] if c < 6 else force[:, b, c - 6]
        cols[s] = coef * src if cols[s] is None else cols[s] + coef * src
    return torch.stack(cols, dim=1)


def signal_misfit(fields, leaves, bonds, terms, n_signals, targets, omega, tau, model="nonlinear"):
    """One member.  ``fields`` (T, 2, n_blocks, 3) NumPy, ``leaves``: dict of NumPy arrays by the names of LEAVES (contact leaves present:
    the angle contact is part of E).  Returns (J float, S (T, n_signals), fields_bar (T, 2, n_blocks, 3), explicit: dict name -> gradient)."""
    T = fields.shape[0]
    u, v = T64(fields[:, 0], True), T64(fields[:, 1], True)
    t = {k: T64(leaves[k], True) for k in LEAVES if k in leaves}
    contact = (t["phi0"], t["am"], t["ac"], t["kc"]) if "am" in t else None
    force = None
    if any(c >= 6 for _, _, c, _ in terms):
        E = elastic_energy(u, t["cnv"], bonds, t["refv"], t["ks"], t["ksh"], t["kr"], model, contact)
        force, = torch.autograd.grad(E, u, create_graph=True)
    S = signals(terms, n_signals, u, v, force)
    om = torch.ones(n_signals, dtype=torch.float64) if omega is None else T64(omega)
    ta = torch.ones(T, dtype=torch.float64) if tau is None else T64(tau)
    J = 0.5 * torch.sum(ta[:, None] * om[None, :] * (S - T64(targets)) ** 2)
    names = list(t)
    gr = torch.autograd.grad(J, [u, v] + [t[k] for k in names], allow_unused=True)
    fb = np.zeros_like(fields)
    fb[:, 0] = 0.0 if gr[0] is None else gr[0].numpy()
    fb[:, 1] = 0.0 if gr[1] is None else gr[1].numpy()
    explicit = {k: (np.zeros_like(np.asarray(leaves[k], dtype=float)) if g is None else g.numpy()) for k, g in zip(names, gr[2:])}
    return J.item(), S.detach().numpy(), fb, explicit
