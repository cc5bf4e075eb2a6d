"""The yardstick of the signal cross-correlation (include/dfx.h: dfx_signal_xcorr, dfx_signal_xcorr_value[_and_grad]) for the GPU tests,
and the inputs they share: the differentiable signals S of tests/projection_yardstick.MemberGraph and, in torch fp64,

    R[d] = sum_p sum_k A_p[k] B_p[k + d]     rho = R / N     J = w_peak M + 1/2 w_delay (delta - delta_target)^2

with autograd for the cotangent on the history and every explicit parameter term.  The parameters of a call travel in an
``objective.CorrelationSpec`` (its templates are ignored here: a member's templates (T, n_templates) are passed beside it)."""
import numpy as np
import torch

from .projection_yardstick import KAPPA_MAX, MemberGraph      # noqa: F401
from .strain_yardstick import T64

GAP_MIN = 1e-3                          # "max": the gap between the largest and the second-largest rho, relative to the peak
BETA_SPREAD_MAX = 30.0                  # "softmax": beta (max rho - min rho)


def sides(S, G, pairs):
    """A, B (n_pairs, T) torch"""
    A = torch.stack([S[:, a] for a, _ in pairs])
    B = torch.stack([S[:, b] if b >= 0 else G[:, -1 - b] for _, b in pairs])
    return A, B


def correlation(S, G, spec):
    """rho (2 D + 1,), N, mass (2 D + 1,) = sum_p sum_k |A_p[k] B_p[k + d]|, all torch"""
    A, B = sides(S, G, spec.pairs)
    T, D = A.shape[1], spec.max_lag
    R, mass = [], []
    for d in range(-D, D + 1):
        prod = A[:, max(0, -d):T - max(0, d)] * B[:, max(0, d):T - max(0, -d)]
        R.append(prod.sum())
        mass.append(prod.abs().sum())
    EA, EB = (A * A).sum(), (B * B).sum()
    N = EA if spec.normalisation == "reference" else torch.sqrt(EA * EB) if spec.normalisation == "coefficient" else torch.ones((), dtype=torch.float64)
    return torch.stack(R) / N, N, torch.stack(mass)


def reduction(rho, spec):
    """J, M, delta (torch scalars)"""
    D = spec.max_lag
    lags = torch.arange(-D, D + 1, dtype=torch.float64)
    if spec.reduce == "at":
        M, delta = rho[spec.lag + D], torch.tensor(float(spec.lag), dtype=torch.float64)
    elif spec.reduce == "max":
        M, at = torch.max(rho, 0)
        delta = lags[at]
    else:
        M = torch.logsumexp(spec.beta * rho, 0) / spec.beta
        delta = (torch.softmax(spec.beta * rho, 0) * lags).sum()
    return spec.w_peak * M + 0.5 * spec.w_delay * (delta - spec.delay_target) ** 2, M, delta


class Result:
    """One member, one spec: the yardstick's numbers and the measures of the conditions on the inputs."""


def evaluate(graph, spec, templates, grads=True):
    """``graph``: a MemberGraph; ``templates`` (T, n_templates) or None.  Returns a Result with J, M, delta (floats), rho, mass (arrays),
    N, and -- with ``grads`` -- fields_bar (T, 2, n_blocks, 3) and explicit: dict leaf name -> gradient."""
    G = None if templates is None else T64(templates)
    rho, N, mass = correlation(graph.S, G, spec)
    J, M, delta = reduction(rho, spec)
    r = Result()
    r.J, r.M, r.delta, r.N = J.item(), M.item(), delta.item(), N.item()
    r.rho, r.mass = rho.detach().numpy(), mass.detach().numpy()
    r.g, = (x.numpy() for x in torch.autograd.grad(J, rho, retain_graph=True))
    if grads:
        names = list(graph.t)
        gr = torch.autograd.grad(J, [graph.u, graph.v] + [graph.t[k] for k in names], allow_unused=True, retain_graph=True)
        r.fb = np.zeros_like(graph.fields)
        r.fb[:, 0] = 0.0 if gr[0] is None else gr[0].numpy()
        r.fb[:, 1] = 0.0 if gr[1] is None else gr[1].numpy()
        r.explicit = {k: (np.zeros_like(np.asarray(graph.leaves[k], dtype=float)) if g is None else g.numpy()) for k, g in zip(names, gr[2:])}
    return r


def conditions(r, spec):
    """The measures of the conditions on the inputs of one member, on the yardstick's numbers alone: dict with
    kappa       max over the lags with g_d != 0 of sum |A B| / |R[d]|                                   (<= KAPPA_MAX)
    gap         "max": (largest - second largest rho) / |peak| (inf with one lag)                       (>= GAP_MIN)
    spread      "softmax": beta (max rho - min rho)                                                     (<= BETA_SPREAD_MAX)
    amplify     "softmax": (|w_peak| + 2 |w_delay| |delta - delta_target| beta D) max_d sum |A B| / N / |J|    (<= KAPPA_MAX)"""
    live = r.g != 0
    R = r.rho * r.N
    out = dict(kappa=float((r.mass[live] / np.abs(R[live])).max()) if live.any() else 0.0)
    if spec.reduce == "max":
        srt = np.sort(r.rho)
        out["gap"] = float((srt[-1] - srt[-2]) / abs(srt[-1])) if len(srt) > 1 else np.inf
    if spec.reduce == "softmax":
        out["spread"] = float(spec.beta * (r.rho.max() - r.rho.min()))
        out["amplify"] = float((abs(spec.w_peak) + 2 * abs(spec.w_delay) * abs(r.delta - spec.delay_target) * spec.beta * spec.max_lag)
                               * r.mass.max() / abs(r.N) / abs(r.J))
    return out


def conditions_hold(c):
    return (c["kappa"] <= KAPPA_MAX and c.get("gap", np.inf) >= GAP_MIN and c.get("spread", 0.0) <= BETA_SPREAD_MAX
            and c.get("amplify", 0.0) <= KAPPA_MAX)


def rho_scale(r):
    """max_d sum |A B| / N: the scale of the bar on rho"""
    return float(r.mass.max() / abs(r.N))


def make_templates(S, rng, sources=(2, 1), shift=2):
    """Templates from a member's own signals S (T, n_signals): column j is signal sources[j] shifted by ``shift`` outputs (B lags A: a
    clear off-centre peak), scaled by a factor from U(0.5, 1.5), plus a smooth bump of a tenth of the signal's size."""
    S = np.asarray(S, dtype=float)
    T = S.shape[0]
    k = np.arange(T)
    out = np.zeros((T, len(sources)))
    for j, src in enumerate(sources):
        s = S[:, src]
        shifted = np.zeros(T)
        shifted[shift:] = s[:T - shift] if shift else s
        bump = np.exp(-0.5 * ((k - 0.6 * (T - 1)) / max(0.15 * T, 1.0)) ** 2)
        out[:, j] = rng.uniform(0.5, 1.5) * shifted + 0.1 * np.abs(s).max() * bump
    return out
