"""The yardstick of the signal spectral ratios (include/dfx.h: dfx_signal_spectrum, dfx_signal_spectrum_value[_and_grad]) for the GPU and
host tests: on the differentiable signals of projection_yardstick.MemberGraph, in torch fp64,

    P_sj = sum_k B_jk S_ks      N_g = n0_g + sum W^n_gsj P_sj^2      D_g = d0_g + sum W^d_gsj P_sj^2
    l_g = N_g / D_g or ln N_g - ln D_g      J = sum_g a_g l_g or logsumexp(beta a_g l_g) / beta

with autograd for the cotangent on the history and every explicit parameter term."""
import numpy as np
import torch

from .strain_yardstick import T64


def forms(S, basis, Wn, Wd, n0, d0):
    """P (n_signals, n_rows), N, D (G,) as differentiable tensors from signals ``S`` (T, n_signals)"""
    P = (T64(basis) @ S).T
    P2 = P * P
    N = T64(n0) + torch.einsum("gsj,sj->g", T64(Wn), P2)
    D = T64(d0) + torch.einsum("gsj,sj->g", T64(Wd), P2)
    return P, N, D


def measure_and_value(N, D, a, measure, aggregate, beta):
    l = torch.log(N) - torch.log(D) if measure == "log" else N / D
    z = T64(a) * l
    J = torch.logsumexp(beta * z, 0) / beta if aggregate == "ks" else z.sum()
    return l, J


def value_and_grads(graph, basis, Wn, Wd, n0, d0, a, measure, aggregate, beta=None):
    """For a projection_yardstick.MemberGraph: dict with J (float), N, D, l (G,), P (n_signals, n_rows), fb = fields_bar (T, 2, n_blocks, 3),
    explicit = {leaf name: gradient}, terms = the sum of the absolute terms entering J (the scale of its bar)."""
    P, N, D = forms(graph.S, basis, Wn, Wd, n0, d0)
    l, J = measure_and_value(N, D, a, measure, aggregate, beta)
    names = list(graph.t)
    gr = torch.autograd.grad(J, [graph.u, graph.v] + [graph.t[k] for k in names], allow_unused=True, retain_graph=True)
    fb = np.zeros_like(graph.fields)
    fb[:, 0] = 0.0 if gr[0] is None else gr[0].numpy()
    fb[:, 1] = 0.0 if gr[1] is None else gr[1].numpy()
    explicit = {k: (np.zeros_like(np.asarray(graph.leaves[k], dtype=float)) if g is None else g.numpy()) for k, g in zip(names, gr[2:])}
    Nn, Dn, ln = N.detach().numpy(), D.detach().numpy(), l.detach().numpy()
    aa = np.abs(np.asarray(a, dtype=float))
    terms = float(np.sum(aa * (np.abs(np.log(Nn)) + np.abs(np.log(Dn))))) if measure == "log" else float(np.sum(aa * np.abs(ln)))
    return dict(J=J.item(), N=Nn, D=Dn, l=ln, P=P.detach().numpy(), fb=fb, explicit=explicit, terms=terms)


def kappa(basis, S, P, weighted):
    """projection_yardstick.kappa with zero targets: sum_k |B_jk S_ks| / |P_sj| on the (signal, row) pairs of ``weighted`` (n_signals,
    n_rows, bool), zero elsewhere.  ``S`` (batch, T, n_signals), ``P`` (batch, n_signals, n_rows)."""
    from .projection_yardstick import kappa as k
    return k(basis, S, P, np.zeros_like(P), weighted.astype(float))


def weff_cancellation(r, Wn, Wd, a, measure, aggregate, beta=None):
    """sum_g |term| / |Weff_sj| of the effective row weights, on the yardstick's N, D, l of one member (``r`` of value_and_grads): 1 where a
    pair carries weight in one (group, side) only; zero on pairs without weight."""
    N, D, l = r["N"], r["D"], r["l"]
    a = np.asarray(a, dtype=float)
    lam = a.copy()
    if aggregate == "ks":
        z = beta * a * l
        e = np.exp(z - z.max())
        lam = a * e / e.sum()
    dN, dD = (1.0 / N, -1.0 / D) if measure == "log" else (1.0 / D, -N / D ** 2)
    tn, td = (lam * dN)[:, None, None] * Wn, (lam * dD)[:, None, None] * Wd
    mass = np.abs(tn).sum(0) + np.abs(td).sum(0)
    net = np.abs((tn + td).sum(0))
    return np.where(mass > 0, mass / np.where(net > 0, net, 1e-300), 0.0)
