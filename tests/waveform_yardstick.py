"""The yardstick of the differentiable drive waveform (loading.Table with named values; include/dfx.h: dfx_fn_table_values,
dfx_fn_table_grads, dfx_fn_table_grad, dfx_drive_cotangent, dfx_fn_table_tangents) shared by tests/test_gpu_waveform.py: one table whose
samples are a leaf of the params dict, on the lattice, horizon and grid of tests/time_functions.py, against the torch oracle driven by
the same piecewise-linear formula with the samples as a tensor that requires grad.

The twin is time_functions.g_table (parity.torch_table states the same formula but freezes its values into NumPy, so autograd cannot reach
them).  As in time_functions, kinks are a condition and not a tolerance: ``check_premises`` asserts, before any comparison, how the drive's
evaluation times fall on the supports of the samples -- in particular that sample 6 has none, so its gradient is an exact zero on both
sides -- and that no evaluation time lies near a breakpoint."""
import numpy as np
import torch

from difflexmm_amd import loading as ld
from oracle import ref_dynamics as OD

from .parity import RTOL_GRAD, RTOL_TRAJ, T64          # noqa: F401  (the bars of the comparisons, re-exported for the tests)
from .time_functions import (HORIZON, LOAD_VEC, N_OUT, SPI, Problem, Term, fields_bar, fixed_step_bounds, g_table, rel,    # noqa: F401
                             stage_times)

NAME = "waveform"                        # the key of the samples in constraint_params / loading_params
DELAY, AMPLITUDE = 2e-5, 2.5
BREAKS = np.array([0, .21, .46, .71, .91, 1.10, 1.12, 1.14, 1.51, 1.91, 2.31]) * 1e-4
VALUES = np.random.default_rng(23).normal(size=len(BREAKS))
FORCE_AMPLITUDE = 4.0                    # as a force load: a few N on these blocks (time_functions.VALUES)
TS = np.linspace(0.0, HORIZON, N_OUT)

# the premises of this table on the 4 x 6 Dormand-Prince grid: evaluation times inside the support (T[j-1], T[j+1]) of every sample (the
# end samples: everything before T[1] / after T[-2]), at or before T[0], at or beyond T[-1]
SUPPORT_COUNTS = [20, 23, 24, 20, 19, 11, 0, 18, 37, 40, 45]
N_BEFORE, N_BEYOND = 9, 24
STAGE_GAP, OUTPUT_GAP = 1.4e-3, 0.1      # of an output interval


class WaveTerm(Term):
    """time_functions.Term for a Table whose samples are the entry NAME of the params dict."""

    def __init__(self, vector, amplitude=AMPLITUDE, values=VALUES):
        super().__init__("Table", (amplitude, DELAY), vector, table=(BREAKS, np.zeros(len(BREAKS))))
        self.samples = np.array(values, dtype=float)

    def lib(self):
        return ld.Table(BREAKS, NAME, self.vector, amplitude=self.names[0], delay=self.names[1])

    def params(self):
        return dict(super().params(), **{NAME: self.samples.copy()})

    def value(self, t, d):
        return g_table(t, d[self.names[0]], d[self.names[1]], (BREAKS, d[NAME])) * torch.as_tensor(self.vector)


def problem(lib, role="disp", lattice="quads", n=4, batch=1, seed=7):
    """The shared case: the waveform as the prescribed displacement of the Case's driven DOF, or as a force on a free block."""
    n_con = 7 if lattice == "quads" else 6
    if role == "disp":
        return Problem(lib, con_terms=[WaveTerm(np.array([1.0] + [0.0] * (n_con - 1)))], lattice=lattice, n=n, batch=batch, seed=seed)
    return Problem(lib, load_terms=[WaveTerm(LOAD_VEC, amplitude=FORCE_AMPLITUDE)], lattice=lattice, n=n, batch=batch, seed=seed)


def member(p, values=None, **over):
    """(constraint_params, loading_params) of one member with its own samples (and scalar overrides by name)."""
    pm = p.params(**over)
    if values is not None:
        for d in pm:
            if NAME in d:
                d[NAME] = np.array(values, dtype=float)
    return pm


def slot_of(p):
    return 0 if p.con_terms else 1


def evaluation_times(bounds):
    """Every time the solve evaluates the drive at: the stage times of every step and the end of the grid (the last record)."""
    bounds = np.asarray(bounds, dtype=float)
    return np.concatenate([stage_times(bounds), bounds[-1:]])


def support_counts(times, delay=DELAY):
    tau = np.asarray(times) - delay
    n = len(BREAKS)
    lo = [-np.inf if j == 0 else BREAKS[j - 1] for j in range(n)]
    hi = [np.inf if j == n - 1 else BREAKS[j + 1] for j in range(n)]
    return [int(np.sum((tau > a) & (tau < b))) for a, b in zip(lo, hi)], int(np.sum(tau <= BREAKS[0])), int(np.sum(tau >= BREAKS[-1]))


def check_premises(ts=TS, spi=SPI):
    times = evaluation_times(fixed_step_bounds(ts, spi))
    counts, before, beyond = support_counts(times)
    assert counts == SUPPORT_COUNTS, counts
    assert before == N_BEFORE and beyond == N_BEYOND, (before, beyond)
    dt = float(np.diff(ts).min())
    kinks = DELAY + BREAKS
    assert np.abs(times[:, None] - kinks[None, :]).min() > STAGE_GAP * dt
    assert np.abs(np.asarray(ts)[:, None] - kinks[None, :]).min() > OUTPUT_GAP * dt
    return times


def check_step_premises(bounds, ts, delay=DELAY):
    """Caller-chosen or accepted steps: no evaluation time near a breakpoint (the counts above belong to the uniform grid)."""
    times = evaluation_times(bounds)
    gap = 1e-9 * float(np.diff(ts).min())
    assert np.abs(times[:, None] - (delay + BREAKS)[None, :]).min() > gap
    return times


_ORACLE = {}        # the oracle's results by content of the case: computed once per process, shared, never written to


def _key(*xs):
    return tuple(None if x is None else (x if isinstance(x, (str, int, float, tuple)) else np.ascontiguousarray(x, dtype=float).tobytes()) for x in xs)


def _leaf_names(pm):
    return [(s, k) for s in (0, 1) for k in pm[s]]


def oracle(p, pm, ts, fb, spi=SPI, adaptive_steps=None, tangents=None):
    """The oracle on one member.  ``fb`` (T, 2, n_dof): the cotangent of the full fields.  Returns the differentiable history on the free
    DOFs, the gradient of sum(fb * fields) with respect to every leaf of the params dicts (the samples: an (n_tab,) array) -- free DOFs
    through autograd of the unrolled solve, prescribed rows through the drive's own value and rate -- and the tangent of the history along
    every entry of ``tangents`` (each a dict {(slot, name): tangent})."""
    key = _key(p.signature(), *[v for d in pm for kv in sorted(d.items()) for v in kv], ts, fb, int(spi), adaptive_steps,
               None if tangents is None else np.concatenate([np.ravel(t[k]) for t in tangents for k in sorted(t)]))
    if key in _ORACLE:
        return _ORACLE[key]
    c = p.c
    osol = p.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5") if adaptive_steps is None \
        else p.oracle_solver(integrator="adaptive")
    names = _leaf_names(pm)
    free = np.asarray(osol.free_DOF_ids)

    def dicts(xs):
        d = ({}, {})
        for (s, k), x in zip(names, xs):
            d[s][k] = x
        return d

    def hist_of(*xs):
        cp = p.oracle_cp(*dicts(xs))
        if adaptive_steps is None:
            return OD.solve_fixed_differentiable(osol, c.ogeo, T64(p.y0), ts, cp, spi, "dopri5")[0]
        return OD.solve_adaptive_replay_differentiable(osol, c.ogeo, T64(p.y0), ts, cp, adaptive_steps)[0]
    leaves = [T64(pm[s][k], True) for s, k in names]
    hist = hist_of(*leaves)
    fb = np.asarray(fb, dtype=float).reshape(len(ts), 2, -1)
    L = (hist * T64(fb[:, :, free])).sum()
    con = np.asarray(p.solver.constrained_DOF_ids)
    if len(con) and p.con_terms and np.any(fb[:, :, con]):
        # rows of prescribed DOFs: fields[k, 0, dof] = c_dof(t_k), fields[k, 1, dof] = dc_dof/dt(t_k)
        d = dicts(leaves)[0]
        dofs = p.con[:, 0] * 3 + p.con[:, 1]
        for k, t in enumerate(ts):
            tt = T64(float(t), True)
            val = sum(x.value(tt, d) for x in p.con_terms)
            rates = [torch.autograd.grad(v, tt, create_graph=True, allow_unused=True)[0] if v.requires_grad else None for v in val]
            rate = torch.stack([torch.zeros((), dtype=torch.float64) if r is None else r for r in rates])
            L = L + (val * T64(fb[k, 0, dofs])).sum() + (rate * T64(fb[k, 1, dofs])).sum()
    gr = torch.autograd.grad(L, leaves, allow_unused=True)
    out = dict(hist=hist.detach().numpy(),
               grad={nk: (np.zeros(np.shape(pm[nk[0]][nk[1]])) if g is None else g.numpy()) for nk, g in zip(names, gr)})
    if tangents is not None:
        prim = tuple(T64(pm[s][k]) for s, k in names)
        out["dots"] = []
        for tan in tangents:
            v = tuple(T64(tan.get(nk, np.zeros(np.shape(pm[nk[0]][nk[1]])))) for nk in names)
            out["dots"].append(torch.autograd.functional.jvp(hist_of, prim, v)[1].numpy())
    _ORACLE[key] = out
    return out


def engine_grads(p, tree):
    """{(slot, name): gradient} out of one member's vjp tree."""
    return {**{(0, k): np.asarray(v) for k, v in tree.constraint_params.items()}, **{(1, k): np.asarray(v) for k, v in tree.loading_params.items()}}


def grad_errors(mine, ref):
    """Relative error of every leaf of the params dicts (arrays: max-norm relative)."""
    return {nk: rel(np.atleast_1d(mine[nk]), np.atleast_1d(g)) for nk, g in ref.items()}


def sample_directions(K, seed=31):
    """K directions on the samples alone."""
    rng = np.random.default_rng(seed)
    return [rng.normal(size=len(BREAKS)) for _ in range(K)]


def sample_tangent_tree(p, dY):
    """A ControlParams-shaped tangent that moves the samples only."""
    d = ({NAME: np.asarray(dY, dtype=float)}, {}) if p.con_terms else ({}, {NAME: np.asarray(dY, dtype=float)})
    return p.c.cp._replace(geometrical_params=None, mechanical_params=None, constraint_params=d[0], loading_params=d[1])
