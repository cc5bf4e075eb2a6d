"""-m gpu: forward-mode signals on the device (include/dfx.h: dfx_forward_tangent_signals_multi, dfx_forward_tangent_signals_dense_multi;
kernels k_tan_signal_channels / k_tan_signal_combine / k_tan_finite_flags in difflexmm_amd/csrc/dfx_tangent.h, per-ligament arithmetic
dfx_tangent_signal.h; DynamicSolver.signal_jvp_multi / signal_jacfwd, problems.SignalCalibration, the hinge fit's on_device Jacobian).

Shapes are those of test_gpu_signal_misfit.py and its ``make_terms`` (force terms on the driven, a clamped and a corner block, x, y and the
moment, signals that share a block, a signal of several terms of both signs, displacement and velocity terms) plus one signal on the
displacement and one on the velocity of a prescribed DOF: quads 6x6 with the angle contact engaged (cutoff 42 deg), kagome 4x4 (a padded
fourth slot), 3 members with different designs, 4 Dopri5 steps per interval, K = 5 directions (a pass of 4 and a tail of 1), both pass
forms, 23 outputs: T x force blocks is 92 (quads) and 69 (kagome) items, more than the 64 of one workgroup and no multiple of it.
Bars: 1e-12 of a column's largest entry against the identical pass (``jvp_multi`` runs the same kernels on the same inputs) and for K = 1
against column 0 of K = 5; 1e-6 for the two prescribed-DOF signals (``jvp_multi`` assembles those rows from central differences, the
device position tangent is exact); TOL_SIGNAL for the signals; RTOL_RHS (1e-12) against ``torch.autograd.functional.jvp`` of the yardstick's
signals with the oracle's energies; 1e-11 for the transposition identity; 1e-6 against central differences; 1e-9 for the hinge samples.
The directions of the ensemble carry tangents of the drive's amplitude and loading_rate but not of input_delay: the host rows ``jvp_multi``
is compared on come from ``TimeFunction.param_partials``, whose step of 1e-6 * max(1, |p|) is a tenth of a delay of 1e-5 (2.3e-5 seen with
it, the truncation error of that difference); the delay is held to the closed form of the pulse instead, at 1e-12.  "RuntimeError ...
adaptive=True with a grid": that refusal is ``jvp_multi``'s own, a ``ValueError`` raised before the engine is reached, and is tested as such.
Every comparison prints its worst case before it asserts.  Worst cases seen on an MI355X (profiles/r21_signal_tangent.txt): identical pass
2.1e-16, prescribed-DOF signals 1.2e-10, closed form 3.2e-16, signals 2.7e-16; autograd jvp 2.1e-14 (nonlinear); transposition 2.8e-13 on the
fixed grid and 5.1e-13 on the kept adaptive steps; K = 1 against column 0 1.6e-15; central differences k_stretch 3.5e-10, damping 3.6e-10,
k_contact 1.4e-8, amplitude 5.9e-7; hinge 4.9e-16 / 1.1e-16 / 7.8e-16, LM 5 evaluations on both paths; calibration condition number 2.98e5,
5 evaluations, truth to 2.0e-9.  No comparison missed its bar."""
import math

import numpy as np
import pytest
import torch

import difflexmm_amd as dm
from difflexmm_amd import _binding as b
from difflexmm_amd import geometry as G
from difflexmm_amd import hinge as H
from difflexmm_amd import objective as O
from difflexmm_amd import problems as P
from difflexmm_amd.dynamics import with_leaf

from .hinge_common import NT, K as HINGE_K, forwards
from .model_matrix import ModelCase
from .parity import RTOL_RHS
from .signal_yardstick import elastic_energy, signals
from .strain_yardstick import T64
from .test_gpu_objective import BATCH, FAST, Ensemble
from .test_gpu_signal_misfit import MODEL_NAMES, TOL_SIGNAL, make_terms, member_leaves
from .test_gpu_tangent import _case, _tangent_tree
from .test_gpu_tangent_multi import WIDEST, _leaves, form  # noqa: F401  (form: the fixture, both pass forms)

pytestmark = pytest.mark.gpu

SPI, T, KDIRS = 4, 23, 5
TS = np.linspace(0.0, 4e-4, T)
ALL = ("centroid_node_vectors", "void_angle0", "inertia", "state0", "fn_params", "reference_vector", "k_bond", "contact", "damping")
ITEMS_PER_WORKGROUP = 64                                                                # kTanSigQuads
OMEGA = np.array([1.0, 0.5, 2.0, 0.25, 1.5, 1e-8])


def _per_bond_cp(c, cp):
    bp, nbd = cp.mechanical_params.bond_params, len(c.bonds)
    bp = bp._replace(**{k: np.broadcast_to(getattr(bp, k), (nbd,)).copy() for k in ("k_stretch", "k_shear", "k_rot")})
    return cp._replace(mechanical_params=cp.mechanical_params._replace(bond_params=bp))


class Setup:
    """The ensemble of test_gpu_objective.py, the terms above, K = 5 directions on every leaf and on state0, and the results of the
    identical pass per form (computed once, shared by the tests that need them)."""

    def __init__(self, lattice):
        e = self.e = Ensemble(lattice)
        c = self.c = e.c
        self.s = c.solver
        self.cps = [_per_bond_cp(c, cp) for cp in e.cps]
        terms, self.force_blocks, self.listed = make_terms(c)
        self.driven = (int(c.con[0, 0]), int(c.con[0, 1]))
        self.terms = terms + [(4, self.driven[0], self.driven[1], 1.5), (5, self.driven[0], 3 + self.driven[1], -0.5)]
        self.ns = 6
        self.spec = O.SignalSpec(self.terms, self.ns)
        rng = np.random.default_rng(31)
        nb = c.geo.n_blocks
        self.y0 = np.stack([c.random_state(0.05, 0.02, 5.0)] * BATCH)
        self.tangents = []
        for k in range(KDIRS):
            y0d = rng.normal(size=(BATCH, 2, nb, 3)) * np.abs(self.y0).max()
            y0d.reshape(BATCH, 2, -1)[:, :, self.s.constrained_DOF_ids] = 0.0           # (state0 of prescribed DOFs is not read)
            # (no tangent of input_delay here: TimeFunction.param_partials, which jvp_multi assembles the prescribed rows from, steps by
            # 1e-6 * max(1, |p|) -- for a delay of 1e-5 a tenth of the parameter, a truncation error of (2 pi rate h)^2 / 6 = 5.9e-5 at
            # this drive.  The delay is checked against the closed form below instead.)
            trees = [_tangent_tree(c, rng, scale=1.0 + m + 0.3 * k) for m in range(BATCH)]
            trees = [t._replace(constraint_params={n: v for n, v in t.constraint_params.items() if n != "input_delay"}) for t in trees]
            self.tangents.append((y0d, trees))
        self.no_drive = [(y0d, [t._replace(constraint_params={}) for t in trees]) for y0d, trees in self.tangents]
        self.cache = {}

    def passes(self, form_name):
        """(fields, fields_dot) of jvp_multi and (S, S_dot) of signal_jvp_multi on the same grid, under the form the fixture forced"""
        if form_name not in self.cache:
            f, fd = self.s.jvp_multi(self.y0, TS, self.cps, self.tangents, steps_per_interval=SPI)
            S, Sd = self.s.signal_jvp_multi(self.y0, TS, self.cps, self.tangents, self.spec, steps_per_interval=SPI)
            assert self.s.stats["step_control"] == "fixed"
            self.cache[form_name] = (f, fd, S, Sd)
        return self.cache[form_name]


@pytest.fixture(scope="module", params=["quads", "kagome"])
def setup(request, hip_lib):
    return Setup(request.param)


def _col_err(got, want):
    """worst error of (..., T, ns) columns, each signal of each column on the scale of its own largest entry"""
    scale = np.abs(want).max(axis=-2, keepdims=True)
    assert np.all(scale > 0)
    return float((np.abs(got - want) / scale).max())


def test_the_setup_is_the_one_the_kernels_can_go_wrong_on(setup, form):  # noqa: F811
    c = setup.c
    n_fb = len(setup.force_blocks)
    assert (T * n_fb) > ITEMS_PER_WORKGROUP and (T * n_fb) % ITEMS_PER_WORKGROUP != 0, (T, n_fb)
    assert {setup.driven[0], 0, c.geo.n_blocks - 1} <= set(setup.force_blocks)
    assert KDIRS == WIDEST + 1                                              # a pass of 4 and a tail of 1 in the chunked form
    f, fd, S, Sd = setup.passes(form)
    assert S.shape == (BATCH, T, setup.ns) and Sd.shape == (BATCH, KDIRS, T, setup.ns)
    # every tangent column is non-zero
    assert np.all(np.abs(Sd).max(axis=2) > 0), np.abs(Sd).max(axis=2)
    # the contact penalty is active on at least one listed force slot (quads: cutoff 42 deg)
    active = 0
    bonds = np.asarray(c.bonds)
    blocks = bonds // c.geo.n_npb
    on_force = np.isin(blocks, setup.force_blocks).any(1)
    for m in range(BATCH):
        lv = member_leaves(c, setup.cps, m)
        if "am" not in lv:
            continue
        phi0 = G.void_angles0(lv["cnv"], c.bonds)
        th = f[m, :, 0, :, 2]
        kap = th[:, blocks[:, 1]] - th[:, blocks[:, 0]]
        wrap = lambda a: a - 2 * math.pi * np.round(a / (2 * math.pi))     # noqa: E731
        for a in (wrap(phi0[None, :, 0] - kap), wrap(phi0[None, :, 1] + kap)):
            active += int(((a >= lv["am"]) & (a < lv["ac"]))[:, on_force].sum())
    print(f"[signal tangent] {c.geo.__class__.__name__} {form}: (output, void angle) pairs of force-block ligaments inside the penalty window: {active}")
    if c.geo.n_npb == 4:
        assert active > 0


# ---- 1. against the identical pass -----------------------------------------------------------------------------------------------------------
def test_columns_equal_the_signals_of_the_identical_pass(setup, form):  # noqa: F811
    s, tag = setup.s, f"{setup.c.geo.__class__.__name__} {form}"
    f, fd, S, Sd = setup.passes(form)
    # field terms on free DOFs: signal 2 (a displacement and a velocity of an interior block)
    free = O.SignalSpec([(0, bk, comp, co) for sg, bk, comp, co in setup.terms if sg == 2], 1)
    want = np.stack([[O.host_signal_values(free, fd[m, k]) for k in range(KDIRS)] for m in range(BATCH)])
    e_free = _col_err(Sd[..., 2:3], want)
    # the two prescribed-DOF signals: jvp_multi's rows are central differences of the time function
    drv = O.SignalSpec([(sg - 4, bk, comp, co) for sg, bk, comp, co in setup.terms if sg >= 4], 2)
    want = np.stack([[O.host_signal_values(drv, fd[m, k]) for k in range(KDIRS)] for m in range(BATCH)])
    e_drv = _col_err(Sd[..., 4:6], want)
    # the signals against signal_values of a forward solve on the same grid
    s(setup.y0, TS, setup.cps, steps_per_interval=SPI)
    ref = s.signal_values(setup.spec)
    e_S = float(np.abs(S - ref).max() / np.abs(ref).max())
    per = [float(np.abs(S[..., i] - ref[..., i]).max() / np.abs(ref[..., i]).max()) for i in range(setup.ns)]
    print(f"[signal tangent] {tag}: field terms on free DOFs {e_free:.2e} (bar 1e-12), prescribed-DOF signals {e_drv:.2e} (bar 1e-6), "
          f"signals against signal_values {e_S:.2e} of the largest (bar {TOL_SIGNAL}), each of its own largest: " + ", ".join(f"{v:.2e}" for v in per))
    assert e_free <= 1e-12 and e_drv <= 1e-6 and e_S <= TOL_SIGNAL and max(per) <= 1e-11


def test_prescribed_position_tangent_is_the_closed_form_of_the_pulse(setup, form):  # noqa: F811
    """The signal on the displacement of the driven DOF along tangents of amplitude, loading_rate AND input_delay, against the derivative of
    g = A (1 - cos(2 pi r (t - d))) / 2 on 0 < t - d < 1 / r written out: both sides are exact, so the bar is 1e-12 of the largest entry."""
    s = setup.s
    dA, dr, dd = 0.3, -45.0, 2e-6
    zero = dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None))
    tang = [(None, zero._replace(constraint_params=dict(amplitude=dA, loading_rate=dr, input_delay=dd)))]
    spec = O.SignalSpec([(0, setup.driven[0], setup.driven[1], 1.5)], 1)
    S, Sd = s.signal_jvp_multi(setup.y0, TS, setup.cps, tang, spec, steps_per_interval=SPI)
    A, r, d = FAST["amplitude"], FAST["loading_rate"], FAST["input_delay"]
    tau = TS - d
    on = (tau > 0) & (tau < 1 / r)
    g = np.where(on, A * (1 - np.cos(2 * math.pi * r * tau)) / 2, 0.0)
    dg = np.where(on, dA * g / A + A * math.pi * np.sin(2 * math.pi * r * tau) * (tau * dr - r * dd), 0.0)
    e_v = float(np.abs(S[..., 0] - 1.5 * g).max() / np.abs(1.5 * g).max())
    e_d = float(np.abs(Sd[:, 0, :, 0] - 1.5 * dg).max() / np.abs(1.5 * dg).max())
    print(f"[signal tangent] {setup.c.geo.__class__.__name__} {form}: prescribed displacement against the closed form: value {e_v:.2e}, tangent {e_d:.2e} (bar 1e-12)")
    assert on.sum() > 10 and e_v <= 1e-12 and e_d <= 1e-12


# ---- 2. against autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contact", [None, "angle"])
@pytest.mark.parametrize("model", list(MODEL_NAMES))
def test_columns_match_autograd_jvp_of_the_yardstick(hip_lib, model, contact, monkeypatch):
    """Quads 4x4, one member, per-ligament stiffnesses, K = 3 directions in one pass of width 4: node vectors, reference vectors,
    stiffnesses, contact constants and state0 (no drive tangent: jvp_multi's prescribed rows are central differences)."""
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", "chunked")
    mc = ModelCase("quads", model, contact, 4, "per_bond", batch=1, seed=5)
    s, cp, p = mc.solver, mc.cps[0], mc.members[0]
    nb, nbd = mc.geo.n_blocks, len(mc.bonds)
    driven, corner = int(mc.con[0, 0]), nb - 1
    terms = [(0, driven, 6, 1.0), (0, driven, 8, 0.7), (1, 0, 7, -1.3), (1, corner, 8, 0.9), (1, 5, 8, 0.5), (1, 5, 6, -0.2), (2, 6, 1, 2.0), (2, 6, 3, 1e-4),
             (3, 6, 2, 1.0), (3, driven, 6, 0.01)]
    spec = O.SignalSpec(terms, 4)
    rng = np.random.default_rng(23)
    bp = cp.mechanical_params.bond_params
    y0 = 0.02 * rng.normal(size=(2, nb, 3))
    y0.reshape(2, -1)[:, s.constrained_DOF_ids] = 0.0
    tangents = []
    for k in range(3):
        bd = type(bp)(**{f: 0.1 * rng.normal(size=np.shape(getattr(bp, f))) * np.abs(np.asarray(getattr(bp, f), dtype=float)) for f in bp._fields})
        cd = dm.ContactParams(*[0.05 * rng.normal() for _ in range(3)]) if contact else None
        y0d = 0.02 * rng.normal(size=(2, nb, 3))
        y0d.reshape(2, -1)[:, s.constrained_DOF_ids] = 0.0
        tangents.append((y0d, dm.ControlParams(dm.GeometricalParams(None, 0.02 * rng.normal(size=mc.cnv.shape)), dm.MechanicalParams(bd, None, None, None, cd))))
    ts = np.linspace(0.0, 4e-4, 5)
    f, fd = s.jvp_multi(y0, ts, cp, tangents, steps_per_interval=SPI)
    S, Sd = s.signal_jvp_multi(y0, ts, cp, tangents, spec, steps_per_interval=SPI)
    lv = dict(cnv=mc.cnv, refv=p.get("refv", np.zeros((nbd, 2))), ks=p["ks"], ksh=p.get("ksh", np.zeros(nbd)), kr=p.get("kr", np.zeros(nbd)))
    names = ["cnv", "refv", "ks", "ksh", "kr"]
    if contact:
        lv.update(phi0=G.void_angles0(mc.cnv, mc.bonds), am=mc.contact_params[0], ac=mc.contact_params[1], kc=mc.contact_params[2])
        names += ["phi0", "am", "ac", "kc"]

    def fn(u, v, *leaves):
        t = dict(zip(names, leaves))
        con = (t["phi0"], t["am"], t["ac"], t["kc"]) if contact else None
        E = elastic_energy(u, t["cnv"], mc.bonds, t["refv"], t["ks"], t["ksh"], t["kr"], MODEL_NAMES[model], con)
        force, = torch.autograd.grad(E, u, create_graph=True)
        return signals(terms, 4, u, v, force)
    primal = (T64(f[:, 0]), T64(f[:, 1])) + tuple(T64(lv[n]) for n in names)
    worst = 0.0
    for k, (y0d, tree) in enumerate(tangents):
        tf = s._flatten_tangent(cp, tree)
        dl = dict(cnv=tf["centroid_node_vectors"], refv=tf["reference_vector"], ks=tf["k_bond"][:, 0], ksh=tf["k_bond"][:, 1], kr=tf["k_bond"][:, 2])
        if contact:
            dl.update(phi0=tf["void_angle0"], am=tf["contact"][0], ac=tf["contact"][1], kc=tf["contact"][2])
        tang = (T64(fd[k][:, 0]), T64(fd[k][:, 1])) + tuple(T64(dl[n]) for n in names)
        val, ref = torch.autograd.functional.jvp(fn, primal, tang)
        e_v = float(np.abs(S - val.detach().numpy()).max() / np.abs(val.detach().numpy()).max())
        e = _col_err(Sd[k], ref.numpy())
        print(f"[signal tangent] quads 4x4 {model} contact={contact} direction {k}: columns against autograd jvp {e:.2e}, signals {e_v:.2e}")
        assert e_v <= TOL_SIGNAL
        worst = max(worst, e)
    assert np.abs(Sd).max() > 0 and worst <= RTOL_RHS, worst


# ---- 3. transposition ------------------------------------------------------------------------------------------------------------------------
def _flat_dot(s, raw, cps, trees, y0d, m):
    tf = s._flatten_tangent(cps[m], trees[m])
    tot = float(np.sum(np.asarray(raw["state0"])[m] * y0d[m]))
    for name, t in tf.items():
        if name in raw:
            tot += float(np.sum(np.asarray(raw[name], dtype=float)[m].reshape(np.shape(t)) * t))
    return tot


def _transposition(setup, tag, **grid):
    s = setup.s
    S, Sd = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.no_drive, setup.spec, **grid)
    stats_fwd = dict(s.stats)
    rng = np.random.default_rng(5)
    tau = rng.uniform(0.5, 1.5, T)
    spec = setup.spec.with_targets(S * rng.uniform(0.5, 1.5, S.shape), OMEGA, tau)
    s(setup.y0, TS, setup.cps, keep_trajectory=True, **{k: v for k, v in grid.items() if k != "adaptive"})
    stats_rev = dict(s.stats)
    obj, raw = s.signal_misfit_value_and_raw(spec, which=ALL)
    raw = {k: np.array(v) for k, v in raw.items()}
    c = tau[None, :, None] * OMEGA[None, None, :] * (S - spec.targets)
    worst = 0.0
    for k, (y0d, trees) in enumerate(setup.no_drive):
        for m in range(BATCH):
            lhs = float(np.sum(c[m] * Sd[m, k]))
            rhs = _flat_dot(s, raw, setup.cps, trees, y0d, m)
            worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    print(f"[signal tangent] {tag}: transposition gap {worst:.2e} (bar 1e-11), misfit {np.asarray(obj)}")
    assert np.abs(c).max() > 0 and worst <= 1e-11, worst
    return stats_fwd, stats_rev


def test_columns_are_the_transpose_of_the_signal_misfit_gradient(setup, form):  # noqa: F811
    _transposition(setup, f"{setup.c.geo.__class__.__name__} {form} fixed grid", steps_per_interval=SPI)


def test_adaptive_columns_are_the_transpose_on_the_kept_steps(setup, form):  # noqa: F811
    s = setup.s
    old = (s.rtol, s.atol)
    s.rtol = s.atol = 1e-5
    try:
        fwd, rev = _transposition(setup, f"{setup.c.geo.__class__.__name__} {form} adaptive", adaptive=True)
    finally:
        s.rtol, s.atol = old
    assert fwd["step_control"] == "adaptive-dense" and rev["step_control"] == "adaptive-records", (fwd["step_control"], rev["step_control"])


# ---- 4. central differences ------------------------------------------------------------------------------------------------------------------
def _scalar_case(seed=8):
    c = _case("quads", 6, True, True, seed=seed)
    mp = c.cp.mechanical_params
    c.cp = c.cp._replace(mechanical_params=mp._replace(damping=5e-4))
    return c


def test_signal_jacfwd_matches_central_differences(hip_lib):
    c = _scalar_case()
    s = c.solver
    driven = (int(c.con[0, 0]), int(c.con[0, 1]))
    terms = make_terms(c)[0] + [(4, driven[0], driven[1], 1.5), (5, driven[0], 3 + driven[1], -0.5)]
    spec = O.SignalSpec(terms, 6)
    ts, spi = np.linspace(0.0, 4e-4, 5), 12
    y0 = c.random_state(0.05, 0.02, 5.0)
    wrt = ["k_stretch", "damping", "k_contact", "amplitude"]
    S, jac = s.signal_jacfwd(y0, ts, c.cp, wrt, spec, steps_per_interval=spi)
    assert sorted(jac) == sorted(wrt) and all(jac[n].shape == S.shape == (5, 6) for n in wrt)
    x0 = dict(k_stretch=120.0, damping=5e-4, k_contact=1.5, amplitude=FAST["amplitude"])

    def solve(cp):
        s(y0, ts, cp, steps_per_interval=spi)
        return s.signal_values(spec)[0]
    # central differences with the relative steps 1e-4 and 2e-4, extrapolated, (4 D(h) - D(2h)) / 3: truncation h^4 f^(5) / 30, rounding
    # ~ 1e-16 |S| / h.  With one step of 1e-6 the rounding term alone is 1e-10 |S| / |x dS/dx|, which passes 1e-6 for a leaf the signals
    # barely feel (k_contact here: 1.8e-6 seen with that step).
    for name in wrt:
        h = 1e-4 * abs(x0[name])
        d1 = (solve(with_leaf(c.cp, name, x0[name] + h)) - solve(with_leaf(c.cp, name, x0[name] - h))) / (2 * h)
        d2 = (solve(with_leaf(c.cp, name, x0[name] + 2 * h)) - solve(with_leaf(c.cp, name, x0[name] - 2 * h))) / (4 * h)
        fd = (4.0 * d1 - d2) / 3.0
        live = np.abs(fd).max(axis=0) > 0
        e = _col_err(jac[name][:, live], fd[:, live])
        print(f"[signal tangent] signal_jacfwd d/d{name} against central differences: {e:.2e} (bar 1e-6); signals that move: {int(live.sum())} of 6")
        assert live.any() and np.abs(jac[name]).max() > 0 and np.all(jac[name][:, ~live] == 0.0)
        assert e <= 1e-6, (name, e)


# ---- 5. contract -----------------------------------------------------------------------------------------------------------------------------
def test_contract(setup, monkeypatch):
    monkeypatch.setenv("DFX_TANGENT_MULTI_FORM", "chunked")
    s, e = setup.s, setup.s.engine
    # bit-equal results on a repeated call
    a = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents, setup.spec, steps_per_interval=SPI)
    a2 = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents, setup.spec, steps_per_interval=SPI)
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
    # K = 1 equals column 0 of K = 5
    one = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents[:1], setup.spec, steps_per_interval=SPI)
    e1 = _col_err(one[1][:, 0], a[1][:, 0])
    print(f"[signal tangent] {setup.c.geo.__class__.__name__}: K = 1 against column 0 of K = 5: {e1:.2e} (bar 1e-12)")
    assert float(np.abs(one[0] - a[0]).max() / np.abs(a[0]).max()) <= 1e-13 and e1 <= 1e-12      # (the 1-wide and the 4-wide build)
    # the handle's kept solve survives: a vjp after the call equals the vjp before it, to the bit
    nb = setup.c.geo.n_blocks

    def solve_and_vjp(between):
        fields = s(setup.y0, TS, setup.cps, keep_trajectory=True, steps_per_interval=SPI)
        fb = np.random.default_rng(2).normal(size=fields.shape)
        between()
        return s.vjp(fb)
    seen = {}

    def between():
        seen["out"] = e.forward_tangent_signals_multi(setup.y0, np.random.default_rng(3).normal(size=(BATCH, 2, 2, nb, 3)), None, 2, TS, SPI,
                                                      setup.terms, setup.ns)
    t1, s1 = solve_and_vjp(between)
    t0, s0 = solve_and_vjp(lambda: None)
    assert np.array_equal(np.asarray(s1), np.asarray(s0)) and np.abs(seen["out"][1]).max() > 0
    for tm, tr in zip(t1, t0):
        for x, y in zip(_leaves(tm), _leaves(tr)):
            assert np.array_equal(x, y)
    # refusals name the entry
    args = (setup.y0, None, None, 1, TS, SPI)
    with pytest.raises(RuntimeError, match="dfx_forward_tangent_signals_multi.*block 9999 out of range"):
        e.forward_tangent_signals_multi(*args, [(0, 9999, 0, 1.0)], 1)
    with pytest.raises(RuntimeError, match="dfx_forward_tangent_signals_multi.*signal 1 is empty"):
        e.forward_tangent_signals_multi(*args, [(0, 1, 0, 1.0)], 2)
    grid, nst = b.padded_step_times([np.array([TS[0], TS[-1]])] * BATCH, TS[0])
    with pytest.raises(RuntimeError, match="dfx_forward_tangent_signals_dense_multi.*component 9 out of range"):
        e.forward_tangent_signals_dense_multi(setup.y0, None, None, 1, TS, grid, nst, [(0, 1, 9, 1.0)], 1)
    with pytest.raises(ValueError, match="signal_jvp_multi: adaptive=True.*steps_per_interval"):
        s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents, setup.spec, steps_per_interval=SPI, adaptive=True)
    # one NaN in state0_dot on a block that no term lists: return code 3
    unlisted = [bk for bk in range(nb) if bk not in {t[1] for t in setup.terms} and bk not in set(setup.c.con[:, 0])]
    s0d = np.zeros((BATCH, 1, 2, nb, 3))
    s0d[1, 0, 0, unlisted[-1], 1] = np.nan
    codes = []
    orig = e._check
    monkeypatch.setattr(e, "_check", lambda rc, what: (codes.append(rc), orig(rc, what)))
    with pytest.raises(RuntimeError, match="dfx_forward_tangent_signals_multi.*non-finite state or tangent"):
        e.forward_tangent_signals_multi(setup.y0, s0d, None, 1, TS, SPI, setup.terms, setup.ns)
    assert codes[-1] == 3, codes
    monkeypatch.undo()
    ok = e.forward_tangent_signals_multi(setup.y0, np.zeros_like(s0d), None, 1, TS, SPI, setup.terms, setup.ns)
    assert np.all(np.isfinite(ok[0])) and np.all(ok[1] == 0.0)


def test_force_terms_with_the_distance_contact_are_refused(hip_lib):
    from .test_distance_contact import DistCase
    c = DistCase("quads", None, n=4, seed=5)
    s = c.solver
    s.prepare(c.cp)
    ts = np.linspace(0.0, 1e-4, 3)
    with pytest.raises(RuntimeError, match="dfx_forward_tangent_signals_multi.*distance-based contact"):
        s.engine.forward_tangent_signals_multi(None, None, None, 1, ts, 2, [(0, 1, 6, 1.0)], 1)
    S, Sd, _ = s.engine.forward_tangent_signals_multi(None, None, None, 1, ts, 2, [(0, 1, 0, 1.0)], 1)      # field terms alone are served
    assert S.shape == (1, 3, 1) and np.all(np.isfinite(S)) and np.all(Sd == 0.0)


# ---- 6. hinge --------------------------------------------------------------------------------------------------------------------------------
HINGE_TRUTH = (110.0, 1.3, 1.35)
LOWER, UPPER = [50.0, 0.5, 0.5], [200.0, 3.0, 3.0]


@pytest.fixture(scope="module")
def sample(hip_lib):
    fws, _ = forwards(None)
    for fw in fws:
        fw.setup()
    return fws


def test_hinge_jacobian_on_the_device(sample):
    fws = sample
    rng = np.random.default_rng(4)
    targets = {}
    for fw in fws:
        u = np.linspace(0, 1.2, 9) * (-1.0 if fw.loading_type == "compression" else 1.0)
        targets[fw.loading_type] = np.array([u, 3.0 * np.abs(u) + rng.uniform(-0.2, 0.2, 9), 0.1 * np.ones(9)])
    opt = H.HingeResponseError(fws, targets)
    r0, J0 = opt.residuals_and_jacobian(HINGE_K)
    r1, J1 = opt.residuals_and_jacobian(HINGE_K, on_device=True)
    e_r = float(np.abs(r1 - r0).max() / np.abs(r0).max())
    e_J = max(float(np.abs(J1[:, j] - J0[:, j]).max() / np.abs(J0[:, j]).max()) for j in range(3))
    v, g = opt.value_and_grad_device(HINGE_K)
    grad = 2.0 * J1.T @ r1 / r1.size
    e_g = float(np.abs(grad - np.array(g)).max() / np.abs(g).max())
    print(f"[signal tangent] hinge: residuals {e_r:.2e}, Jacobian {e_J:.2e} against the host path; 2 J^T r / n against value_and_grad_device {e_g:.2e} (bars 1e-9)")
    assert r1.shape == (3 * NT,) and J1.shape == (3 * NT, 3)
    assert e_r <= 1e-9 and e_J <= 1e-9 and e_g <= 1e-9


def test_hinge_lm_on_the_device(sample):
    fws = sample
    targets = {fw.loading_type: np.vstack([fw.force_displacement(*fw.solve(HINGE_TRUTH)), np.ones(NT)]) for fw in fws}
    runs = {}
    for on_device in (False, True):
        opt = H.HingeResponseError(fws, targets)
        opt.run_optimization_lm(HINGE_K, 8, lower_bound=LOWER, upper_bound=UPPER, on_device=on_device)
        best = opt.design_values[int(np.argmin(opt.objective_values))]
        err = float(np.abs(np.array(best) / np.array(HINGE_TRUTH) - 1).max())
        print(f"[signal tangent] hinge LM on_device={on_device}: {len(opt.objective_values)} evaluations, max relative error {err:.2e}")
        assert len(opt.objective_values) <= 8 and err <= 1e-6
        assert all(lo <= x <= hi for d in opt.design_values for x, lo, hi in zip(d, LOWER, UPPER))
        assert set(opt.fitted_responses) == {"tension", "compression", "shear"}
        runs[on_device] = len(opt.objective_values)
    assert runs[True] <= runs[False], runs


# ---- 7. calibration --------------------------------------------------------------------------------------------------------------------------
def test_signal_calibration_recovers_the_parameters(hip_lib):
    """Targets generated by the engine at known (k_stretch, k_rot, damping, amplitude) on quads 6x6: two displacements, one velocity and
    the reaction force on the driven DOF, each weighted by the inverse square of its own size."""
    c = _scalar_case(seed=12)
    s = c.solver
    wrt = ["k_stretch", "k_rot", "damping", "amplitude"]
    truth = np.array([120.0, 1.5, 5e-4, 1.5])
    c.cp = with_leaf(c.cp, "amplitude", 1.5)
    driven = (int(c.con[0, 0]), int(c.con[0, 1]))
    spec0 = O.SignalSpec([(0, 14, 0, 1.0), (1, 21, 2, 1.0), (2, 15, 3, 1.0), (3, driven[0], 6 + driven[1], 1.0)], 4)
    ts, grid = np.linspace(0.0, 4e-4, 17), dict(steps_per_interval=4)
    y0 = np.zeros((2, c.geo.n_blocks, 3))
    s(y0, ts, c.cp, **grid)
    targets = s.signal_values(spec0)[0]
    omega = 1.0 / np.abs(targets).max(axis=0) ** 2
    spec = spec0.with_targets(targets, omega)
    cal = P.SignalCalibration(s, y0, ts, c.cp, spec, wrt, **grid)
    r, J = cal.residuals_and_jacobian(truth)
    cond = float(np.linalg.cond(J))
    print(f"[signal tangent] calibration: residual at the truth {np.abs(r).max():.2e}, condition number of the weighted Jacobian {cond:.3e} (bar 1e6), "
          f"column norms {np.linalg.norm(J, axis=0)}")
    assert np.abs(r).max() <= 1e-10 and cond < 1e6
    cal.objective_values.clear(), cal.design_values.clear()
    hist = cal.run_lm(truth * np.array([1.15, 0.85, 1.15, 0.85]))
    err = float(np.abs(hist["x"][-1] / truth - 1).max())
    print(f"[signal tangent] calibration: {hist['n_eval']} evaluations, status {hist['status']}, objectives {cal.objective_values}, max relative error {err:.2e}")
    assert hist["n_eval"] <= 20 and err <= 1e-6
    assert all(f1 < f0 for f0, f1 in zip(hist["fun"][:-1], hist["fun"][1:]))          # every accepted iterate lowers the objective
