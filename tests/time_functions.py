"""Shared cases and checkers of tests/test_time_functions.py (CPU port) and tests/test_gpu_time_functions.py (HIP engine): the closed
library of time functions (difflexmm_amd/loading.py, eval_time_fn of csrc/dfx_physics.h) in both roles -- prescribed displacement and force
load --, in either slot, against the torch oracle driven by a torch twin of each function.  Every twin is a plain restatement of the
function's docstring formula in loading.py; the oracle takes any callable.

Kinks are a condition, not a tolerance: Ramp, CappedRamp and Table jump in d/dt and d/dp at their kinks, the engine and a twin round the
comparison that picks the side differently, so every checker first computes all stage times on the host and asserts that none lies
within KINK_GAP of the output interval of a kink (and that, between them, the stage times visit every branch of the function)."""
import math
import os

import numpy as np
import torch

from difflexmm_amd import loading as ld
from difflexmm_amd.dynamics import setup_dynamic_solver
from oracle import ref_dynamics as OD
from oracle import ref_ode

from .common import Case
from .parity import RAW_WHICH, RTOL_GRAD, RTOL_TRAJ, T64

HORIZON, N_OUT, SPI = 3e-4, 5, 6
KINK_GAP = 1e-9                                             # of the output interval
STAGE_C = np.concatenate([[0.0], ref_ode.ALPHA[:5]])        # Dormand-Prince stage times inside a step, the step end (c = 1) included
ZERO = torch.zeros((), dtype=torch.float64)


def _tt(t):
    return torch.as_tensor(t, dtype=torch.float64)


# -- torch twins: g(t, *params) -------------------------------------------------------------------------------------------------------------
def g_pulse(t, amplitude, loading_rate, input_delay):
    """amplitude/2 (1 - cos 2 pi f tau) on 0 < tau < 1/f, tau = t - input_delay"""
    tau = _tt(t) - input_delay
    return torch.where((tau > 0) & (tau < 1 / loading_rate), amplitude / 2 * (1 - torch.cos(2 * math.pi * loading_rate * tau)), ZERO)


def g_harmonic(t, amplitude, loading_rate, input_delay):
    """the same wave switched on at tau > 0 and never off"""
    tau = _tt(t) - input_delay
    return torch.where(tau > 0, amplitude / 2 * (1 - torch.cos(2 * math.pi * loading_rate * tau)), ZERO)


def g_ramp(t, amplitude, rate):
    """amplitude * min(t * rate, 1)"""
    x = _tt(t) * rate
    return amplitude * torch.where(x < 1, x, torch.ones_like(x))


def g_sech2tanh(t, amplitude, width):
    """2A/s^2 sech^2(t/s - 3) tanh(3 - t/s)"""
    z = _tt(t) / width
    return 2 * amplitude / width ** 2 / torch.cosh(z - 3) ** 2 * torch.tanh(3 - z)


def g_constant(t, amplitude):
    return amplitude + 0.0 * _tt(t)


def g_capped_ramp(t, length, rate, cap):
    """length * min(t * rate, cap), the reference's where(t < cap / rate, t * rate, cap)"""
    t = _tt(t)
    return length * torch.where(t < cap / rate, t * rate, cap + 0.0 * t)


def g_delayed_pulse(t, amplitude, loading_rate, input_delay, strain, strain_rate):
    """the pulse with tau = t - strain / strain_rate - input_delay"""
    return g_pulse(_tt(t) - strain / strain_rate, amplitude, loading_rate, input_delay)


def g_table(t, amplitude, delay, table):
    """amplitude * interp(t - delay; times, values), piecewise linear, end values held"""
    T, Y = table
    tau = _tt(t) - delay
    tf = float(tau.detach())
    if tf <= T[0]:
        y = Y[0] + 0.0 * tau
    elif tf >= T[-1]:
        y = Y[-1] + 0.0 * tau
    else:
        lo = int(np.searchsorted(T, tf, side="right")) - 1
        y = Y[lo] + (Y[lo + 1] - Y[lo]) / (T[lo + 1] - T[lo]) * (tau - T[lo])
    return amplitude * y


def _pulse_branch(tau, f, off=True):
    return "before" if tau <= 0 else ("inside" if (tau * f < 1 or not off) else "after")


# names: the library's parameter names, the amplitude-like one (the value is linear in it) first; g: the twin; kinks(p): times where d/dt
# or d/dp jumps; branch(t, p): which piece t is on; branches: every piece there is
FUNCTIONS = {
    "Pulse": dict(names=("amplitude", "loading_rate", "input_delay"), g=g_pulse, kinks=lambda p: [],
                  branch=lambda t, p: _pulse_branch(t - p[2], p[1]), branches={"before", "inside", "after"}),
    "Harmonic": dict(names=("amplitude", "loading_rate", "input_delay"), g=g_harmonic, kinks=lambda p: [],
                     branch=lambda t, p: _pulse_branch(t - p[2], p[1], off=False), branches={"before", "inside"}),
    "Ramp": dict(names=("amplitude", "rate"), g=g_ramp, kinks=lambda p: [1 / p[1]],
                 branch=lambda t, p: "below" if t * p[1] < 1 else "above", branches={"below", "above"}),
    "Sech2Tanh": dict(names=("amplitude", "width"), g=g_sech2tanh, kinks=lambda p: [], branch=lambda t, p: "all", branches={"all"}),
    "Constant": dict(names=("amplitude",), g=g_constant, kinks=lambda p: [], branch=lambda t, p: "all", branches={"all"}),
    "CappedRamp": dict(names=("length", "rate", "cap"), g=g_capped_ramp, kinks=lambda p: [p[2] / p[1]],
                       branch=lambda t, p: "below" if t * p[1] < p[2] else "above", branches={"below", "above"}),
    "DelayedPulse": dict(names=("amplitude", "loading_rate", "input_delay", "strain", "strain_rate"), g=g_delayed_pulse, kinks=lambda p: [],
                         branch=lambda t, p: _pulse_branch(t - p[3] / p[4] - p[2], p[1]), branches={"before", "inside", "after"}),
    "Table": dict(names=("amplitude", "delay"), g=g_table, kinks=None, branch=None, branches={"before", "between", "after"}),
}

_rng = np.random.default_rng(11)
TABLE = (np.sort(_rng.uniform(0.45e-4, 2.3e-4, 6)), _rng.normal(size=6))          # 6 breakpoints inside the horizon, both ends held
TABLE2 = (np.array([0.613e-4, 1.937e-4]), np.array([0.4, -1.1]))                  # exactly 2 breakpoints
TABLE_PAST = (np.array([-3.1e-4, -2.2e-4, -0.4e-4]), np.array([0.0, 0.7, -0.9]))  # the whole horizon beyond the last breakpoint

# values that take every branch inside HORIZON and keep every kink off the stage times of the 4 x 6 grid (asserted by the checkers);
# amplitudes: a displacement of ~1 mm, a force of a few N (accelerations ~1e6 mm/s^2 on these 1e-6 Mg blocks)
VALUES = {
    "Pulse": dict(disp=(3.0, 5000.0, 0.3137e-4), force=(5.0, 5000.0, 0.3137e-4)),
    "Harmonic": dict(disp=(2.0, 7000.0, 0.4211e-4), force=(4.0, 7000.0, 0.4211e-4)),
    "Ramp": dict(disp=(1.2, 6131.0), force=(6.0, 6131.0)),
    "Sech2Tanh": dict(disp=(1.5e-9, 3.1e-5), force=(6e-9, 3.1e-5)),
    "Constant": dict(disp=(0.3,), force=(4.0,)),
    "CappedRamp": dict(disp=(45.0, 41.3, 0.004), force=(1500.0, 41.3, 0.004)),
    "Table": dict(disp=(1.5, 0.2e-4), force=(4.0, 0.2e-4)),
}


class Term:
    """One library function with values: the engine's object, its torch twin, its kinks and branches.  ``names``: the keys of the
    params dict (None: the value is a constant of the solver); default: the library's own names behind ``prefix``."""

    def __init__(self, fn, values, vector=1.0, prefix="", names=None, table=None):
        self.fn, self.spec = fn, FUNCTIONS[fn]
        self.values = tuple(float(v) for v in values)
        self.vector = np.asarray(vector, dtype=float)
        self.names = tuple(prefix + n for n in self.spec["names"]) if names is None else tuple(names)
        self.table = (TABLE if table is None else table) if fn == "Table" else None
        assert len(self.values) == len(self.names) == len(self.spec["names"])

    def lib(self):
        kw = {k: (v if n is None else n) for k, n, v in zip(self.spec["names"], self.names, self.values)}
        if self.fn == "Table":
            return ld.Table(self.table[0], self.table[1], self.vector, **kw)
        return getattr(ld, self.fn)(self.vector, **kw)

    def params(self):
        return {n: v for n, v in zip(self.names, self.values) if n is not None}

    def _p(self, d):
        return [v if n is None else d[n] for n, v in zip(self.names, self.values)]

    def value(self, t, d):
        """The twin: g(t; d) * vector with d a dict of torch scalars (or floats)."""
        extra = (self.table,) if self.fn == "Table" else ()
        return self.spec["g"](t, *self._p(d), *extra) * torch.as_tensor(self.vector)

    def kinks(self, d):
        p = [float(x) for x in self._p(d)]
        if self.fn == "Table":
            return [p[1] + b for b in self.table[0]]
        return self.spec["kinks"](p)

    def branch(self, t, d):
        p = [float(x) for x in self._p(d)]
        if self.fn == "Table":
            tau = t - p[1]
            return "before" if tau <= self.table[0][0] else ("after" if tau >= self.table[0][-1] else "between")
        return self.spec["branch"](t, p)


def term(fn, role, vector, prefix="", **kw):
    return Term(fn, VALUES[fn][role], vector, prefix, **kw)


LOADED = np.array([[5, 0], [5, 1], [10, 2]])
LOAD_VEC = np.array([1.0, -0.6, 0.3])


class Problem:
    """The lattice, boundary conditions and mechanical parameters of tests/common.Case with time functions of choice: ``con_terms`` drive
    the Case's constrained DOFs (its ``vec``: x of the middle block of the left edge, the rest held), ``load_terms`` are forces on
    ``loaded`` (default: x and y of block 5 and theta of block 10).  One solver for the engine under test, one for the oracle."""

    def __init__(self, lib, con_terms=(), load_terms=(), lattice="quads", n=4, batch=1, seed=7, con=None, loaded=LOADED):
        self.c = c = Case(lattice, n, True, True, seed=seed, lib=lib, cutoff_deg=125.0 if lattice == "kagome" else 42.0)
        self.con_terms, self.load_terms, self.batch, self.lattice, self.seed = list(con_terms), list(load_terms), batch, lattice, seed
        self.con = c.con if con is None else np.asarray(con)
        self.loaded = np.asarray(loaded) if self.load_terms else None
        con_fn = sum((t.lib() for t in self.con_terms[1:]), self.con_terms[0].lib()) if self.con_terms else None
        load_fn = sum((t.lib() for t in self.load_terms[1:]), self.load_terms[0].lib()) if self.load_terms else None
        self.solver = setup_dynamic_solver(c.geo, c.energy, loaded_block_DOF_pairs=self.loaded, loading_fn=load_fn,
                                           constrained_block_DOF_pairs=self.con, constrained_DOFs_fn=con_fn, damped_blocks=c.damped,
                                           batch=batch, _lib=lib)
        n_con = len(self.con)
        args = dict(constrained_block_DOF_pairs=self.con, damped_blocks=c.damped,
                    constrained_DOFs_fn=lambda t, **d: sum((x.value(t, d) for x in self.con_terms), torch.zeros(n_con, dtype=torch.float64)))
        if self.load_terms:
            args.update(loaded_block_DOF_pairs=self.loaded,
                        loading_fn=lambda state, t, **d: sum((x.value(t, d) for x in self.load_terms), torch.zeros(len(self.loaded), dtype=torch.float64)))
        self.oracle_args = args
        self.y0 = c.random_state(0.05, 0.02, 5.0)

    def params(self, **over):
        """(constraint_params, loading_params) of one member: the terms' values, entries of ``over`` replaced by name."""
        out = []
        for terms in (self.con_terms, self.load_terms):
            d = {}
            for t in terms:
                d.update(t.params())
            d.update({k: float(v) for k, v in over.items() if k in d})
            out.append(d)
        assert set(over) <= set(out[0]) | set(out[1]), sorted(over)
        return tuple(out)

    def cp(self, pm):
        return self.c.cp._replace(constraint_params=dict(pm[0]), loading_params=dict(pm[1]))

    def oracle_solver(self, **kw):
        return OD.setup_dynamic_solver(self.c.ogeo, self.c.oenergy, **self.oracle_args, **kw)

    def oracle_cp(self, con, load):
        return self.c.oracle_cp()._replace(constraint_params=con, loading_params=load)

    def terms(self):
        return [(t, 0) for t in self.con_terms] + [(t, 1) for t in self.load_terms]

    def signature(self):
        """What the oracle's result depends on besides the member's parameters, the grid and the cotangent."""
        return (self.lattice, self.c.geo.n_blocks, self.seed, _b(self.con), _b(self.loaded),
                tuple((t.fn, slot, t.names, t.values if None in t.names else None, _b(t.vector), None if t.table is None else _b(np.stack(t.table)))
                      for t, slot in self.terms()))


def single(lib, fn, role, lattice="quads", n=4, batch=1, values=None, table=None, seed=7):
    """One function in one role on the Case's boundary conditions (force: its constrained DOFs are held at zero)."""
    c_vec = np.array([1.0] + [0.0] * 6) if lattice == "quads" else np.array([1.0] + [0.0] * 5)
    vals = VALUES[fn][role] if values is None else values
    if role == "disp":
        return Problem(lib, con_terms=[Term(fn, vals, c_vec, table=table)], lattice=lattice, n=n, batch=batch, seed=seed)
    return Problem(lib, load_terms=[Term(fn, vals, LOAD_VEC, table=table)], lattice=lattice, n=n, batch=batch, seed=seed)


def harmonic_plus_ramp(lib, batch=1):
    """Slot 0: Harmonic displacement; slot 1: Ramp force (names with a prefix, so that every name is in one dict only)."""
    return Problem(lib, con_terms=[term("Harmonic", "disp", np.array([1.0] + [0.0] * 6))],
                   load_terms=[term("Ramp", "force", LOAD_VEC, prefix="load_")], batch=batch)


def static_tuning(lib, n=4, batch=1, seed=7):
    """loading.static_tuning_drive: CappedRamp (slot 0) on the held y of the far corner + DelayedPulse (slot 1) on the driven x, sharing
    ``compressive_strain`` / ``compressive_strain_rate`` (the pulse starts when the ramp ends, + input_delay)."""
    nc = 7
    static_vec, dyn_vec = np.zeros(nc), np.zeros(nc)
    static_vec[-1], dyn_vec[0] = -1.0, 1.0
    strain, rate = 0.004, 41.3
    ramp = Term("CappedRamp", (45.0, rate, strain), static_vec, names=(None, "compressive_strain_rate", "compressive_strain"))
    pulse = Term("DelayedPulse", (3.0, 8000.0, 0.2137e-4, strain, rate), dyn_vec,
                 names=("amplitude", "loading_rate", "input_delay", "compressive_strain", "compressive_strain_rate"))
    p = Problem(lib, n=n, batch=batch, seed=seed)
    p.con_terms = [ramp, pulse]
    p.solver = setup_dynamic_solver(p.c.geo, p.c.energy, constrained_block_DOF_pairs=p.con,
                                    constrained_DOFs_fn=ld.static_tuning_drive(static_vec, dyn_vec, 45.0), damped_blocks=p.c.damped,
                                    batch=batch, _lib=lib)
    return p


def two_roles_in_one_block(lib):
    """x of the driven block follows a Pulse, y of the SAME block carries a Sech2Tanh force: two lanes of one quad, two table rows."""
    c0 = Case("quads", 4, True, True, seed=7, lib=lib, cutoff_deg=42.0)
    mid = int(c0.con[0, 0])
    con = np.array([[mid, 0], [mid, 2], [0, 0], [0, 1], [0, 2], [15, 1]])
    return Problem(lib, con_terms=[term("Pulse", "disp", np.array([1.0, 0, 0, 0, 0, 0]))],
                   load_terms=[term("Sech2Tanh", "force", np.array([1.0]), prefix="load_")], con=con, loaded=np.array([[mid, 1]]))


# -- stage times, kinks, branches -----------------------------------------------------------------------------------------------------------
def fixed_step_bounds(ts, spi, step_times=None):
    if step_times is not None:
        return np.asarray(step_times, dtype=float)
    spis = np.broadcast_to(spi, (len(ts) - 1,))
    return np.concatenate([a + (b - a) * np.arange(k) / k for a, b, k in zip(ts[:-1], ts[1:], spis)] + [ts[-1:]])


def stage_times(bounds):
    """t_n + c_r h of every step of a grid (the step ends included: the first stage of the next step, and the output rows)."""
    bounds = np.asarray(bounds, dtype=float)
    return (bounds[:-1, None] + np.diff(bounds)[:, None] * STAGE_C[None, :]).reshape(-1)


def check_premises(p, pm, times, ts, branches=True):
    """No stage time within KINK_GAP of the output interval of a kink; every branch of every function visited by some stage time."""
    gap = KINK_GAP * float(np.diff(ts).min())
    for t, slot in p.terms():
        d = pm[slot]
        for k in t.kinks(d):
            near = np.abs(times - k).min()
            assert near > gap, (t.fn, "a stage time lies on a kink", k, near)
        if branches:
            seen = {t.branch(float(x), d) for x in times}
            assert seen == t.spec["branches"], (t.fn, "branches visited", sorted(seen))


# -- engine against oracle --------------------------------------------------------------------------------------------------------------------
def scalar_err(a, b):
    a, b = float(a), float(b)
    if b == 0.0:
        return 0.0 if a == 0.0 else float("inf")
    return abs(a - b) / abs(b)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.abs(b).max()
    if scale == 0.0:
        return 0.0 if np.abs(a).max() == 0.0 else float("inf")
    return float(np.abs(a - b).max() / scale)


_ORACLE = {}        # the oracle's results by content of the case: computed once per process, shared by the tests that need them, never written to


def _b(x):
    return None if x is None else np.ascontiguousarray(x, dtype=float).tobytes()


def tangent_of(pm, seed=5):
    """A direction that moves every function parameter by 10-40 % of its size (a parameter that is 0: by 0.1-0.4)."""
    rng = np.random.default_rng(seed)
    return tuple({k: (0.1 + 0.3 * rng.random()) * rng.choice([-1.0, 1.0]) * (v if v != 0.0 else 1.0) for k, v in d.items()} for d in pm)


def oracle_reference(p, key, pm, ts, fb_free, spi=SPI, step_times=None, adaptive_steps=None, tangent=None):
    """The oracle on one member: full fields (fixed grids), the differentiable history on the free DOFs, d sum(fb * hist) / d(every
    function parameter), and the tangent of the history along ``tangent``."""
    key = (p.signature(), tuple(tuple(sorted(d.items())) for d in pm), _b(ts), _b(fb_free), _b(np.broadcast_to(spi, (len(ts) - 1,))), _b(step_times),
           _b(adaptive_steps), None if tangent is None else tuple(tuple(sorted(d.items())) for d in tangent))
    if key in _ORACLE:
        return _ORACLE[key]
    c = p.c
    osol = p.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5", step_times=step_times) if adaptive_steps is None \
        else p.oracle_solver(integrator="adaptive")
    names = [(s, k) for s in (0, 1) for k in pm[s]]

    def hist_of(*xs):
        d = ({}, {})
        for (s, k), x in zip(names, xs):
            d[s][k] = x
        cp = p.oracle_cp(*d)
        if adaptive_steps is None:
            return OD.solve_fixed_differentiable(osol, c.ogeo, T64(p.y0), ts, cp, spi, "dopri5", step_times=step_times)[0]
        return OD.solve_adaptive_replay_differentiable(osol, c.ogeo, T64(p.y0), ts, cp, adaptive_steps)[0]
    out = {}
    if adaptive_steps is None:
        out["fields"] = osol(p.y0, ts, p.oracle_cp(*[{k: T64(v) for k, v in d.items()} for d in pm])).numpy()
    leaves = [T64(pm[s][k], True) for s, k in names]
    hist = hist_of(*leaves)
    out["hist"] = hist.detach().numpy()
    gr = torch.autograd.grad((hist * T64(fb_free)).sum(), leaves, allow_unused=True)
    out["grad"] = {nk: (0.0 if g is None else g.item()) for nk, g in zip(names, gr)}
    if tangent is not None:
        _, jv = torch.autograd.functional.jvp(hist_of, tuple(T64(pm[s][k]) for s, k in names), tuple(T64(tangent[s][k]) for s, k in names))
        out["dot"] = jv.numpy()
    _ORACLE[key] = out
    return out


def fields_bar(p, n_t, seed=3):
    # (member m's cotangent does not depend on the batch it sits in: a member met again in another test finds its oracle run)
    fb = np.stack([np.random.default_rng(seed + m).normal(size=(n_t, 2, p.c.geo.n_blocks, 3)) for m in range(p.batch)])
    fb.reshape(p.batch, n_t, 2, -1)[:, :, :, p.solver.constrained_DOF_ids] = 0.0      # as everywhere in the suite: free DOFs only
    return fb


def engine_grads(p, trees):
    """Per member {(slot, name): gradient} out of vjp's tree(s)."""
    trees = trees if isinstance(trees, list) else [trees]
    return [{**{(0, k): v for k, v in t.constraint_params.items()}, **{(1, k): v for k, v in t.loading_params.items()}} for t in trees]


def check_fixed(p, key, members=None, ts=None, spi=SPI, step_times=None, jvp=True, branches=True, label=None):
    """Engine against oracle on a fixed grid, member by member: full fields (RTOL_TRAJ), the gradient of every function parameter
    (RTOL_GRAD each) and -- where the library has forward mode -- fields_dot along a direction that moves every function parameter
    (RTOL_GRAD).  Returns {(member, what): error} and the engine's outputs."""
    s = p.solver
    ts = np.linspace(0, HORIZON, N_OUT) if ts is None else ts
    members = [p.params()] * p.batch if members is None else members
    assert len(members) == p.batch
    times = stage_times(fixed_step_bounds(ts, spi, step_times))
    for pm in members:
        check_premises(p, pm, times, ts, branches=branches)
    cps = [p.cp(pm) for pm in members]
    arg = cps if p.batch > 1 else cps[0]
    fields = s(p.y0, ts, arg, keep_trajectory=True, steps_per_interval=spi, step_times=step_times)
    stats = dict(s.stats)
    fb = fields_bar(p, len(ts))
    trees, s0 = s.vjp(fb if p.batch > 1 else fb[0])
    grads = engine_grads(p, trees)
    fields = np.asarray(fields).reshape(p.batch, len(ts), 2, -1)
    free = s.free_DOF_ids
    jvp = jvp and s.engine.has_forward_tangent          # (the CPU port is reverse mode only)
    tangents = [tangent_of(pm) if jvp else None for pm in members]
    fdot = None
    if jvp:
        dots = [tangent_tree(p, t) for t in tangents]
        f2, fdot = s.jvp(p.y0, ts, arg, None, dots if p.batch > 1 else dots[0], steps_per_interval=spi, step_times=step_times)
        fdot = np.asarray(fdot).reshape(p.batch, len(ts), 2, -1)
        assert rel(np.asarray(f2).reshape(fields.shape), fields) < 1e-13
    errs, refs = {}, []
    for m, pm in enumerate(members):
        ref = oracle_reference(p, f"{key}/{m}", pm, ts, fb[m].reshape(len(ts), 2, -1)[:, :, free], spi, step_times, tangent=tangents[m])
        refs.append(ref)
        errs[(m, "fields")] = rel(fields[m], ref["fields"].reshape(len(ts), 2, -1))
        assert np.abs(ref["hist"]).max() > 0
        for nk, g in ref["grad"].items():
            errs[(m, "d/d" + nk[1])] = scalar_err(grads[m][nk], g)
        if fdot is not None:
            assert np.abs(ref["dot"]).max() > 0
            errs[(m, "fields_dot")] = rel(fdot[m][:, :, free], ref["dot"])
    report(label or key, errs)
    bad = {k: v for k, v in errs.items() if not v < (RTOL_TRAJ if k[1] == "fields" else RTOL_GRAD)}
    assert not bad, (key, bad)
    return errs, dict(fields=fields, grads=grads, fdot=fdot, stats=stats, state0_bar=np.asarray(s0), refs=refs)


def check_adaptive(p, key, n_out=41, rtol=1e-5, atol=1e-5, label=None):
    """The adaptive solve with its accepted steps kept (as parity.check_adaptive_records_adjoint): the oracle's replay of the engine's
    accepted steps reproduces the fields to 1e-11, autograd through the replay gives the parameter gradients (RTOL_GRAD)."""
    s = p.solver
    ts = np.linspace(0, HORIZON, n_out)
    pm = p.params()
    s.rtol, s.atol = rtol, atol
    fields = s(p.y0, ts, p.cp(pm), keep_trajectory=True)
    assert s.stats["step_control"] == "adaptive-records", s.stats["step_control"]
    st = np.concatenate([ts[:1], s.engine.adaptive_step_times(0)])
    check_premises(p, pm, stage_times(st), ts)
    fb = fields_bar(p, len(ts))
    trees, _ = s.vjp(fb[0])
    grads = engine_grads(p, trees)[0]
    free = s.free_DOF_ids
    ref = oracle_reference(p, key, pm, ts, fb[0].reshape(len(ts), 2, -1)[:, :, free], adaptive_steps=st)
    errs = {(0, "replayed fields"): rel(np.asarray(fields).reshape(len(ts), 2, -1)[:, :, free], ref["hist"])}
    for nk, g in ref["grad"].items():
        errs[(0, "d/d" + nk[1])] = scalar_err(grads[nk], g)
    report(label or key, errs, extra=f"steps {len(st) - 1}")
    bad = {k: v for k, v in errs.items() if not v < (1e-11 if k[1] == "replayed fields" else RTOL_GRAD)}
    assert not bad, (key, bad)
    return errs


def report(label, errs, extra=""):
    """The worst error per kind of quantity, as the neighbouring test files print theirs."""
    worst = {}
    for (m, what), v in errs.items():
        kind = what if not what.startswith("d/d") else "grad"
        if kind not in worst or v > worst[kind][0]:
            worst[kind] = (v, m, what)
    print(f"time_functions: {label}: " + ", ".join(f"{k} {v:.2e} ({w}, member {m})" for k, (v, m, w) in worst.items()) + (" " + extra if extra else ""))


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tangent_tree(p, tan):
    """A ControlParams-shaped tangent that moves the function parameters only (every other leaf None: a zero tangent)."""
    return p.c.cp._replace(geometrical_params=None, mechanical_params=None, constraint_params=dict(tan[0]), loading_params=dict(tan[1]))


def check_rhs(p, key, t, rtol, label=None):
    """The rhs / rhs_vjp (/ rhs_jvp where the library has it) hooks at time ``t`` against autograd of the oracle's rhs: the rate, the state
    cotangent, the gradient of every function parameter, and the tangent along (a state direction, every function parameter)."""
    s, pm = p.solver, p.params()
    cp = p.cp(pm)
    s.engine.set_params(**{k: v[None] for k, v in s._flatten(cp).items()})
    rng = np.random.default_rng(17)
    nb = p.c.geo.n_blocks
    y = rng.normal(size=(2, nb, 3)) * np.array([0.3, 0.3, 0.1])
    y[1] *= 50.0
    lam, yd = rng.normal(size=y.shape), rng.normal(size=y.shape)
    dy = s.engine.rhs(y[None], t)[0]
    yb, g = s.engine.rhs_vjp(y[None], t, lam[None])
    bars = ({}, {})
    for f, tm in enumerate(s.con_terms):
        tm.scatter_grad(g["fn_params"][0][f], bars[0], cp.constraint_params)
    for f, tm in enumerate(s.load_terms):
        tm.scatter_grad(g["fn_params"][0][len(s.con_terms) + f], bars[1], cp.loading_params)
    osol = p.oracle_solver()
    free = osol.free_DOF_ids
    names = [(sl, k) for sl in (0, 1) for k in pm[sl]]

    def rhs_of(yf, *xs):
        d = ({}, {})
        for (sl, k), x in zip(names, xs):
            d[sl][k] = x
        ocp = p.oracle_cp(*d)
        return osol.rhs(yf, t, ocp, osol.reduced_inertia(ocp), create_graph=True)
    yf = T64(y.reshape(2, -1)[:, free], True)
    leaves = [T64(pm[sl][k], True) for sl, k in names]
    r = rhs_of(yf, *leaves)
    gr = torch.autograd.grad((r * T64(lam.reshape(2, -1)[:, free])).sum(), [yf] + leaves, allow_unused=True)
    errs = {(0, "rhs"): rel(dy.reshape(2, -1)[:, free], r.detach().numpy()), (0, "y_bar"): rel(yb[0].reshape(2, -1)[:, free], gr[0].numpy())}
    for nk, og in zip(names, gr[1:]):
        errs[(0, "d/d" + nk[1])] = scalar_err(bars[nk[0]][nk[1]], 0.0 if og is None else og.item())
    if s.engine.has_rhs_jvp:
        tan = tangent_of(pm)
        pd = {k: v[None] for k, v in s._flatten_tangent(cp, tangent_tree(p, tan)).items()}
        ydc = yd.copy()
        ydc.reshape(2, -1)[:, s.constrained_DOF_ids] = 0.0
        dy2, dd = s.engine.rhs_jvp(y[None], t, np.stack([np.zeros_like(y), ydc])[None], [pd, pd], 2)
        assert rel(dy2[0], dy) < 1e-13
        z = torch.zeros_like(yf)
        for k, ydk in enumerate((z, T64(ydc.reshape(2, -1)[:, free]))):
            _, jv = torch.autograd.functional.jvp(rhs_of, (T64(y.reshape(2, -1)[:, free]),) + tuple(T64(pm[sl][n]) for sl, n in names),
                                                  (ydk,) + tuple(T64(tan[sl][n]) for sl, n in names))
            errs[(0, f"rhs_dot{k}")] = rel(dd[0, k].reshape(2, -1)[:, free], jv.numpy())
    report(label or key, errs)
    bad = {k: v for k, v in errs.items() if not v < rtol}
    assert not bad, (key, t, bad)
    return errs


# -- the engine against itself: one case on several kernel paths --------------------------------------------------------------------------
def run_path(make, env, ts, spi=SPI, step_times=None, members=None, adaptive=False, jvp=True, rtol=1e-5, multi=(), as_member=0):
    """One case (``make()``: a fresh Problem, built under ``env``) through a forward solve that keeps its trajectory, the reverse sweep
    and forward mode; returns fields, every gradient leaf, fields_dot, the columns of jvp_multi for each K of ``multi``, and the stats
    that say which kernels ran.  ``as_member``: a batch-1 run takes the cotangent that member has in a batch."""
    def run():
        p = make()
        s = p.solver
        members_ = [p.params()] * p.batch if members is None else members
        cps = [p.cp(pm) for pm in members_]
        arg = cps if p.batch > 1 else cps[0]
        if adaptive:
            s.rtol = s.atol = rtol
            fields = s(p.y0, ts, arg, keep_trajectory=True)
        else:
            fields = s(p.y0, ts, arg, keep_trajectory=True, steps_per_interval=spi, step_times=step_times)
        nt, shape = ts.shape[-1], (p.batch, ts.shape[-1], 2, p.c.geo.n_blocks, 3)
        out = dict(fields=np.array(fields).reshape(shape), stats=dict(s.stats))
        fb = fields_bar(p, nt, seed=3 + as_member)
        # the raw sweep asks for no ligament gradients: the build the persistent reverse loops serve (vjp below: the whole tree)
        raw = s.vjp_raw(fb if p.batch > 1 else fb[0], which=RAW_WHICH)
        out["raw_stats"] = dict(s.adjoint_stats)
        raw = {"raw:" + k: np.array(v) for k, v in raw.items()}
        for m, cp in enumerate(cps):          # the raw sweep's function-parameter gradients under their names, as vjp's tree has them
            bars = ({}, {})
            for f, tm in enumerate(s.con_terms):
                tm.scatter_grad(raw["raw:fn_params"][m][f], bars[0], cp.constraint_params)
            for f, tm in enumerate(s.load_terms):
                tm.scatter_grad(raw["raw:fn_params"][m][len(s.con_terms) + f], bars[1], cp.loading_params)
            raw.update({f"{m}:raw{sl}:{k}": np.array(v) for sl in (0, 1) for k, v in bars[sl].items()})
        if adaptive:
            out["step_bounds"] = [np.concatenate([ts[:1], s.engine.adaptive_step_times(m)]) for m in range(p.batch)]
        if adaptive:
            s(p.y0, ts, arg, keep_trajectory=True)
        else:
            s(p.y0, ts, arg, keep_trajectory=True, steps_per_interval=spi, step_times=step_times)
        trees, s0 = s.vjp(fb if p.batch > 1 else fb[0])
        out["adjoint_stats"] = dict(s.adjoint_stats)
        tl = trees if isinstance(trees, list) else [trees]
        out["grads"] = dict(state0=np.array(s0).reshape((p.batch,) + shape[2:]), cnv=np.stack([t.geometrical_params.centroid_node_vectors for t in tl]),
                            damping=np.stack([np.asarray(t.mechanical_params.damping) for t in tl]))
        out["grads"].update(raw)
        for m, gm in enumerate(engine_grads(p, trees)):
            for (sl, k), v in gm.items():
                out["grads"][f"{m}:{sl}:{k}"] = np.array(v)
        if jvp and s.engine.has_forward_tangent:
            dots = [tangent_tree(p, tangent_of(pm)) for pm in members_]
            kw = dict(adaptive=True) if adaptive else dict(steps_per_interval=spi, step_times=step_times)
            f2, fdot = s.jvp(p.y0, ts, arg, None, dots if p.batch > 1 else dots[0], **kw)
            out["jvp_fields"], out["fdot"], out["jvp_stats"] = np.array(f2).reshape(shape), np.array(fdot).reshape(shape), dict(s.stats)
            for K in multi:
                tans = [(None, [tangent_tree(p, tangent_of(pm, seed=50 + k)) for pm in members_]) for k in range(K)]
                tans = tans if p.batch > 1 else [(None, t[0]) for _, t in tans]
                _, fd = s.jvp_multi(p.y0, ts, arg, tans, **kw)
                cols = []
                for k in range(K):
                    dk = [tangent_tree(p, tangent_of(pm, seed=50 + k)) for pm in members_]
                    cols.append(np.array(s.jvp(p.y0, ts, arg, None, dk if p.batch > 1 else dk[0], **kw)[1]))
                out[f"multi{K}"] = (np.array(fd), np.stack(cols, axis=0 if p.batch == 1 else 1), dict(s.stats))
        return out
    return with_env(env, run)


def member_view(out, m):
    """Member m of a run_path result, laid out as a batch-1 result."""
    grads = {k: v[m:m + 1] for k, v in out["grads"].items() if not k.split(":")[0].isdigit()}
    grads.update({"0:" + k.split(":", 1)[1]: v for k, v in out["grads"].items() if k.startswith(f"{m}:")})
    view = dict(fields=out["fields"][m:m + 1], grads=grads)
    if "fdot" in out:
        view.update(fdot=out["fdot"][m:m + 1], jvp_fields=out["jvp_fields"][m:m + 1])
    return view


def compare_paths(label, ref, out, tol_fields=1e-13, tol_grad=1e-12, tol_dot=1e-12):
    """Two kernels evaluating the same expressions: fields to 1e-13, every gradient leaf to 1e-12 (the bars of
    test_four_checkpoint_levels_give_the_same_gradient), tangent columns to 1e-12."""
    errs = {(0, "fields"): rel(out["fields"], ref["fields"])}
    assert set(out["grads"]) == set(ref["grads"])
    for k in ref["grads"]:
        errs[(0, "d/d" + k)] = rel(out["grads"][k], ref["grads"][k])
    if "fdot" in ref and "fdot" in out:
        errs[(0, "fields_dot")] = rel(out["fdot"], ref["fdot"])
        errs[(0, "jvp fields")] = rel(out["jvp_fields"], ref["fields"])
    report(label, errs)
    bad = {k: v for k, v in errs.items() if not v < (tol_fields if "fields" in k[1] and "dot" not in k[1] else tol_dot if "dot" in k[1] else tol_grad)}
    assert not bad, (label, bad)
    return errs


# -- cases shared by the CPU-port and the HIP suites ------------------------------------------------------------------------------------------
def unequal_steps(ts, spi):
    """Caller-chosen step boundaries: unequal steps inside every output interval (as parity.check_trajectory_and_adjoint's)."""
    return np.concatenate([a + (b - a) * np.linspace(0, 1, spi + 1)[:-1] ** 1.7 for a, b in zip(ts[:-1], ts[1:])] + [ts[-1:]])


def staggered_members(p, fn, t_out):
    """Three members whose function is before, inside and after its pulse (below, close under and above the ramp's cap) at ``t_out``."""
    if fn == "Pulse":
        members = [p.params(input_delay=2.1137e-4), p.params(), p.params(loading_rate=12000.0)]
        want = ["before", "inside", "after"]
    else:
        name = [k for d in p.params() for k in d if k.endswith("rate")][0]
        members = [p.params(**{name: 3011.0}), p.params(), p.params(**{name: 9173.0})]
        want = ["below", "below", "above"]
    (t, slot), = p.terms()
    assert [t.branch(float(t_out), pm[slot]) for pm in members] == want
    return members


def check_zero_amplitude(lib, fn, role):
    """Amplitude 0 is an ordinary input: the fields are those of the undriven solve, every gradient and tangent is finite and equals
    autograd's (check_fixed), and the amplitude gradient is non-zero where the oracle's is."""
    vals = (0.0,) + tuple(VALUES[fn][role][1:])
    key = f"{fn}/{role}/zero amplitude"
    p = single(lib, fn, role, values=vals)
    errs, out = check_fixed(p, key)
    ts = np.linspace(0, HORIZON, N_OUT)
    q = Problem(lib)
    undriven = q.solver(q.y0, ts, q.c.cp, steps_per_interval=SPI)
    assert np.array_equal(p.y0, q.y0) and np.array_equal(out["fields"][0], undriven.reshape(len(ts), 2, -1)), key
    slot = 0 if role == "disp" else 1
    amp = (slot, FUNCTIONS[fn]["names"][0])
    assert all(np.isfinite(v) for v in out["grads"][0].values()) and (out["fdot"] is None or np.all(np.isfinite(out["fdot"])))
    ref = out["refs"][0]["grad"]
    assert ref[amp] != 0.0 and out["grads"][0][amp] != 0.0, (key, ref[amp], out["grads"][0][amp])
    assert all(ref[k] == 0.0 and out["grads"][0][k] == 0.0 for k in ref if k != amp), (key, ref, out["grads"][0])


def check_pulse_end_on_output(lib, role):
    """A continuous coincidence: the pulse ends exactly on an output time (and on a step boundary).  Value and rate are continuous
    there, so whichever side either code takes, the comparison holds to the same tolerances."""
    ts = np.linspace(0, HORIZON, N_OUT)
    vals = (VALUES["Pulse"][role][0], 8000.0, 1e-4)
    assert vals[2] + 1 / vals[1] == ts[3]
    return check_fixed(single(lib, "Pulse", role, values=vals), f"Pulse/{role}/ends on an output time")


def check_table_edge(lib, edge, role):
    """Exactly two breakpoints; the whole horizon beyond the last breakpoint (the end value held: d/dt and d/d delay are zero)."""
    if edge == "two breakpoints":
        return check_fixed(single(lib, "Table", role, table=TABLE2), f"Table/{role}/two breakpoints")
    errs, out = check_fixed(single(lib, "Table", role, table=TABLE_PAST), f"Table/{role}/past the end", branches=False)
    g, slot = out["grads"][0], 0 if role == "disp" else 1
    assert g[(slot, "delay")] == 0.0 and g[(slot, "amplitude")] != 0.0 and out["refs"][0]["grad"][(slot, "delay")] == 0.0
    return errs, out


def check_constant_force(lib):
    """Constant as a force: the amplitude gradient sums the response to a static load (a step applied at t = 0)."""
    errs, out = check_fixed(single(lib, "Constant", "force"), "Constant/force")
    assert out["grads"][0][(1, "amplitude")] != 0.0
    return errs, out


def check_zero_member_in_batch(lib, fn, role):
    """A batch in which only the middle member has amplitude 0: every member against its own oracle run, and the other two bit-identical
    to the same solve with an ordinary member in the middle."""
    name = FUNCTIONS[fn]["names"][0]
    a = VALUES[fn][role][0]
    ts = np.linspace(0, HORIZON, N_OUT)
    p = single(lib, fn, role, batch=3)
    with_zero = [p.params(), p.params(**{name: 0.0}), p.params(**{name: 0.5 * a})]
    errs, out = check_fixed(p, f"{fn}/{role}/batch with a zero member", members=with_zero)
    assert all(np.isfinite(v) for g in out["grads"] for v in g.values())
    without = [with_zero[0], p.params(**{name: 0.7 * a}), with_zero[2]]
    one = run_path(lambda: single(lib, fn, role, batch=3), {}, ts, members=with_zero)
    two = run_path(lambda: single(lib, fn, role, batch=3), {}, ts, members=without)
    for m in (0, 2):
        assert np.array_equal(one["fields"][m], two["fields"][m]), m
        for k in one["grads"]:
            if k.startswith(f"{m}:"):
                assert np.array_equal(one["grads"][k], two["grads"][k]), (m, k)
            elif not k.split(":")[0].isdigit():
                assert np.array_equal(one["grads"][k][m], two["grads"][k][m]), (m, k)
        if "fdot" in one:
            assert np.array_equal(one["fdot"][m], two["fdot"][m]), m
    assert np.all(np.isfinite(one["fields"])) and all(np.all(np.isfinite(v)) for v in one["grads"].values())


# the hooks at one time inside and one time after the active window of every function of the case
RHS_CASES = {
    "Table as displacement": (lambda lib: single(lib, "Table", "disp"), (1.1e-4, 2.9e-4)),
    "Sech2Tanh as force": (lambda lib: single(lib, "Sech2Tanh", "force"), (2.3 * 3.1e-5, 5.5 * 3.1e-5)),
    "Harmonic + Ramp": (harmonic_plus_ramp, (1.0e-4, 2.5e-4)),
    "CappedRamp + DelayedPulse": (static_tuning, (1.9e-4, 2.8e-4)),
}


def check_adaptive_path(label, make, out, ts):
    """An adaptive run_path result (batch 1) against the oracle's replay of the steps THAT run accepted: fields 1e-11, the parameter
    gradients of the whole-tree sweep and of the raw sweep RTOL_GRAD each, and -- ``out`` holds a tangent -- fields_dot of
    jvp(adaptive=True) against torch.autograd.functional.jvp through the replay (RTOL_GRAD)."""
    p = make()
    pm, st = p.params(), out["step_bounds"][0]
    check_premises(p, pm, stage_times(st), ts)
    free = p.solver.free_DOF_ids
    nt = len(ts)
    fb = fields_bar(p, nt)[0].reshape(nt, 2, -1)[:, :, free]
    ref = oracle_reference(p, label, pm, ts, fb, adaptive_steps=st, tangent=tangent_of(pm) if "fdot" in out else None)
    errs = {(0, "replayed fields"): rel(out["fields"][0].reshape(nt, 2, -1)[:, :, free], ref["hist"])}
    for (sl, k), g in ref["grad"].items():
        errs[(0, f"d/d{k}")] = scalar_err(out["grads"][f"0:{sl}:{k}"], g)
        errs[(0, f"d/d{k} (raw sweep)")] = scalar_err(out["grads"][f"0:raw{sl}:{k}"], g)
    if "fdot" in out:
        errs[(0, "fields_dot")] = rel(out["fdot"][0].reshape(nt, 2, -1)[:, :, free], ref["dot"])
        errs[(0, "replayed fields (tangent pass)")] = rel(out["jvp_fields"][0].reshape(nt, 2, -1)[:, :, free], ref["hist"])
    report(label, errs, extra=f"steps {len(st) - 1}")
    bad = {k: v for k, v in errs.items() if not v < (1e-11 if "replayed" in k[1] else RTOL_GRAD)}
    assert not bad, (label, bad)
    return errs
