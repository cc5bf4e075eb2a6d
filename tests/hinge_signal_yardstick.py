"""The yardstick of the hinge-force signal channels (include/dfx.h: components 9 + 3 node + dof of the dfx_signal_* term lists) for the host
and the GPU tests: tests/signal_yardstick.py's construction with one more source.  A block-force channel is
``autograd.grad(E, u, create_graph=True)`` of the whole ligament plus angle-contact energy; a hinge channel is

    channel(b, 9 + 3 n + d) = autograd.grad(E_h, u, create_graph=True)[:, b, d]

with E_h the energy of the ONE ligament on node n of block b: its bond energy (tests/strain_yardstick.bond_energies, the oracle's own) plus
the two angle-contact terms of that bond, in the parametrisation of tests/signal_yardstick.elastic_energy -- which is the sum of these E_h
over the bonds.  ``HingeGraph`` is a tests/projection_yardstick.MemberGraph whose signals may hold hinge terms, so the misfit below, its
``value_and_grads`` (projections) and tests/xcorr_yardstick.evaluate run on it unchanged: a second pass of autograd gives the value, the
cotangent on the history and every explicit parameter term."""
import numpy as np
import torch

from oracle import ref_energy as OE

from .projection_yardstick import MemberGraph
from .signal_yardstick import LEAVES
from .strain_yardstick import T64, _wrap, bond_energies

HINGE = 9


def bond_energy_history(u_hist, cnv, bonds, refv, ks, ksh, kr, model="nonlinear", contact=None):
    """(T, n_bonds): bond energy plus the two angle-contact terms of every bond at every output configuration; its sum is
    signal_yardstick.elastic_energy."""
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    rows = []
    for k in range(u_hist.shape[0]):
        nd = OE.block_to_node_kinematics(u_hist[k], cnv).reshape(-1, 3)
        nodal = (nd[bonds_t[:, 0]], nd[bonds_t[:, 1]])
        e = bond_energies(model, nodal, refv, ks, ksh, kr, (1.0, 1.0, 1.0))
        if contact is not None:
            phi0, am, ac, kc = contact
            kap = nodal[1][:, 2] - nodal[0][:, 2]
            e = e + OE.contact_energy(_wrap(phi0[:, 0] - kap), am, ac, kc) + OE.contact_energy(_wrap(phi0[:, 1] + kap), am, ac, kc)
        rows.append(e)
    return torch.stack(rows)


def hinge_channels_by_node(u_hist, cnv, bonds, refv, ks, ksh, kr, nodes, model="nonlinear", contact=None):
    """{n: (T, n_blocks, 3)} the hinge channels of node n of EVERY block at once, differentiable -- for the cases with many listed hinges,
    where one ``autograd.grad`` per hinge is too slow.  A block reaches the ligament on its node n through that node alone, so
    dE_h/du_b = (d node displacement(b, n) / du_b)^T dE/d(node displacement(b, n)): one vector-Jacobian product of the oracle's
    block_to_node_kinematics per node index, with dE/d(node displacements) from the same energies.  tests/test_hinge_signal_host.py holds
    it against the per-hinge construction of HingeGraph."""
    bonds_t = torch.as_tensor(np.asarray(bonds), dtype=torch.long)
    out = {n: [] for n in nodes}
    for k in range(u_hist.shape[0]):
        uk = u_hist[k]
        nd = OE.block_to_node_kinematics(uk, cnv)
        flat = nd.reshape(-1, 3)
        nodal = (flat[bonds_t[:, 0]], flat[bonds_t[:, 1]])
        e = bond_energies(model, nodal, refv, ks, ksh, kr, (1.0, 1.0, 1.0))
        if contact is not None:
            phi0, am, ac, kc = contact
            kap = nodal[1][:, 2] - nodal[0][:, 2]
            e = e + OE.contact_energy(_wrap(phi0[:, 0] - kap), am, ac, kc) + OE.contact_energy(_wrap(phi0[:, 1] + kap), am, ac, kc)
        g, = torch.autograd.grad(e.sum(), nd, create_graph=True)
        for n in nodes:
            pick = torch.zeros_like(nd)
            pick[:, n] = 1.0
            r, = torch.autograd.grad(nd, uk, grad_outputs=pick * g, create_graph=True)
            out[n].append(r)
    return {n: torch.stack(v) for n, v in out.items()}


def bond_of_hinge(bonds, n_npb, block, node):
    """the index of the one bond with an end on node ``node`` of ``block``"""
    at = np.flatnonzero((np.asarray(bonds) == block * n_npb + node).any(1))
    assert len(at) == 1, (block, node, at)
    return int(at[0])


def partner_of_hinge(bonds, n_npb, block, node):
    """(block, node) of the other end of that bond"""
    row = np.asarray(bonds)[bond_of_hinge(bonds, n_npb, block, node)]
    other = int(row[1] if row[0] == block * n_npb + node else row[0])
    return other // n_npb, other % n_npb


class HingeGraph(MemberGraph):
    """One member on one history: ``fields`` (T, 2, n_blocks, 3), ``leaves`` by the names of signal_yardstick.LEAVES; terms with
    components 0..8 as there, 9 + 3 node + dof the hinge channels.  ``by_node``: the channels from hinge_channels_by_node (a block force
    is then the sum of the block's hinge channels) instead of one autograd pass per listed hinge."""

    def __init__(self, fields, leaves, bonds, n_npb, terms, n_signals, model="nonlinear", by_node=False):
        self.fields = np.asarray(fields, dtype=float)
        self.leaves = leaves
        self.u, self.v = T64(self.fields[:, 0], True), T64(self.fields[:, 1], True)
        self.t = t = {k: T64(leaves[k], True) for k in LEAVES if k in leaves}
        contact = (t["phi0"], t["am"], t["ac"], t["kc"]) if "am" in t else None
        force, hinge = None, {}
        if by_node and any(c >= 6 for _, _, c, _ in terms):
            ch = hinge_channels_by_node(self.u, t["cnv"], bonds, t["refv"], t["ks"], t["ksh"], t["kr"], range(n_npb), model, contact)
            force = sum(ch.values())
            hinge = {(b, (c - HINGE) // 3): ch[(c - HINGE) // 3][:, b, :] for _, b, c, _ in terms if c >= HINGE}
        elif any(c >= 6 for _, _, c, _ in terms):
            e = bond_energy_history(self.u, t["cnv"], bonds, t["refv"], t["ks"], t["ksh"], t["kr"], model, contact)
            if any(6 <= c < HINGE for _, _, c, _ in terms):
                force, = torch.autograd.grad(e.sum(), self.u, create_graph=True)
            for b, n in sorted({(b, (c - HINGE) // 3) for _, b, c, _ in terms if c >= HINGE}):
                g, = torch.autograd.grad(e[:, bond_of_hinge(bonds, n_npb, b, n)].sum(), self.u, create_graph=True)
                hinge[(b, n)] = g[:, b, :]
        cols = [None] * n_signals
        for s, b, c, coef in terms:
            src = (self.u[:, b, c] if c < 3 else self.v[:, b, c - 3] if c < 6 else force[:, b, c - 6] if c < HINGE
                   else hinge[(b, (c - HINGE) // 3)][:, (c - HINGE) % 3])
            cols[s] = coef * src if cols[s] is None else cols[s] + coef * src
        self.S = torch.stack(cols, dim=1)                                           # (T, n_signals), differentiable

    def grads_of(self, J):
        """fields_bar (T, 2, n_blocks, 3) and explicit: dict leaf name -> gradient of the torch scalar J"""
        names = list(self.t)
        gr = torch.autograd.grad(J, [self.u, self.v] + [self.t[k] for k in names], allow_unused=True, retain_graph=True)
        fb = np.zeros_like(self.fields)
        fb[:, 0] = 0.0 if gr[0] is None else gr[0].numpy()
        fb[:, 1] = 0.0 if gr[1] is None else gr[1].numpy()
        return fb, {k: (np.zeros_like(np.asarray(self.leaves[k], dtype=float)) if g is None else g.numpy()) for k, g in zip(names, gr[2:])}

    def misfit(self, targets, omega, tau):
        """J float, fields_bar, explicit of 1/2 sum_k tau_k sum_s omega_s (S_ks - Starget_ks)^2"""
        T, ns = self.S.shape
        om = torch.ones(ns, dtype=torch.float64) if omega is None else T64(omega)
        ta = torch.ones(T, dtype=torch.float64) if tau is None else T64(tau)
        J = 0.5 * torch.sum(ta[:, None] * om[None, :] * (self.S - T64(targets)) ** 2)
        return (J.item(),) + self.grads_of(J)


def add_explicit(ref, explicit):
    """the autograd explicit terms of every member added to the raw gradients of ``eng.adjoint(fields_bar)``, as
    tests/test_gpu_signal_misfit.py::yardstick adds them"""
    for m, g in enumerate(explicit):
        ref["centroid_node_vectors"][m] += g["cnv"]
        if "void_angle0" in ref and "phi0" in g:
            ref["void_angle0"][m] += g["phi0"]
        if "reference_vector" in ref:
            ref["reference_vector"][m] += g["refv"]
        if "k_bond" in ref:
            ref["k_bond"][m] += np.stack([g["ks"], g["ksh"], g["kr"]], 1)
        if "contact" in ref and "am" in g:
            ref["contact"][m] += np.array([g["am"], g["ac"], g["kc"]])
    return ref
