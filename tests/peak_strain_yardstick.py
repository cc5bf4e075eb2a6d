"""The yardstick of the peak ligament-strain objective (include/dfx.h: dfx_strain_peak_value[_and_grad]) shared by the host and the GPU
tests: the measure written with the oracle's own bond energies in torch (``tests/strain_yardstick.bond_energies`` with the coefficient triple
as stiffnesses: q = 2 E), ``torch.logsumexp`` / the p-norm on top, so that autograd gives the value, the cotangent on the displacement
history and the explicit terms.

    q_kb = 2 E_bond(b; u_k) with (a_b, s_b, r_b) in place of (k_stretch, k_shear, k_rot)          W_kb = tau_k omega_b
    "ks"     J = logsumexp over W > 0 of (beta q + log W) / beta
    "pnorm"  J = c (sum over W > 0 of W (q / c)^p)^(1/p)     with c the hard maximum held constant (J does not depend on c)

The hard maximum and its place are NumPy's: argmax over the row-major (output, bond) image with -inf where W = 0 -- on ties the lowest
output, then the lowest bond."""
import numpy as np
import torch

from oracle import ref_energy as OE

from .strain_yardstick import T64, bond_energies


def measure(u_hist, cnv, bonds, refv, coef, model="nonlinear"):
    """(T, n_bonds) q of one member.  ``u_hist`` (T, n_blocks, 3), ``coef`` (n_bonds, 3); every argument may be a torch leaf."""
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    rows = []
    for k in range(u_hist.shape[0]):
        nd = OE.block_to_node_kinematics(u_hist[k], cnv).reshape(-1, 3)
        nodal = (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]])
        rows.append(2.0 * bond_energies(model, nodal, refv, coef[:, 0], coef[:, 1], coef[:, 2], (1.0, 1.0, 1.0)))
    return torch.stack(rows)


def hard_peak(q, W):
    """(q_hat, (output, bond)) of the NumPy image q over the pairs with W > 0"""
    q, W = np.asarray(q), np.asarray(W)
    flat = int(np.argmax(np.where(W > 0, q, -np.inf)))
    return float(q.reshape(-1)[flat]), (flat // q.shape[1], flat % q.shape[1])


def aggregate(q, w, tau, kind, sharp):
    """Scalar J (torch) of the image q (T, n_bonds) with bond weights w (n_bonds,) and output weights tau (T,), both NumPy."""
    W = T64(np.asarray(tau, dtype=float)[:, None] * np.asarray(w, dtype=float)[None, :])
    on = W > 0
    qs, Ws = q[on], W[on]
    if kind == "ks":
        return torch.logsumexp(sharp * qs + torch.log(Ws), 0) / sharp
    if kind != "pnorm":
        raise ValueError(kind)
    c = float(qs.max())
    if c == 0.0:
        return qs.sum() * 0.0
    return c * torch.sum(Ws * (qs / c) ** sharp) ** (1.0 / sharp)


def peak_objective(u_hist, cnv, bonds, refv, coef, w, tau, kind, sharp, model="nonlinear"):
    """(J (torch scalar), q_hat, (output, bond)) of one member"""
    q = measure(u_hist, cnv, bonds, refv, coef, model)
    W = np.asarray(tau, dtype=float)[:, None] * np.asarray(w, dtype=float)[None, :]
    qh, at = hard_peak(q.detach().numpy(), W)
    return aggregate(q, w, tau, kind, sharp), qh, at
