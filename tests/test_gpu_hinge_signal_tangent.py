"""-m gpu: forward-mode signals with hinge-force terms (components 9 + 3 node + dof; kernel k_tan_hinge_channels in
difflexmm_amd/csrc/dfx_tangent.h behind dfx_forward_tangent_signals_multi / _dense_multi; DynamicSolver.signal_jvp_multi / signal_jacfwd).

The setup is tests/test_gpu_signal_tangent.py's (its ``Setup``: the ensemble of test_gpu_objective.py, 3 members, 23 outputs, 4 Dopri5
steps per interval, K = 5 directions on every leaf and on state0 -- one full pass of 4 plus a remainder of 1 -- both pass forms) with the
terms of tests/test_gpu_hinge_signal.py (signals 0..5: hinges on the driven, a clamped, a corner and two bonded interior blocks, the moment,
both hinges of a bond, a signal mixing a hinge, a block force and a velocity).  T x listed hinges is 345 (quads) and 230 (kagome) items, more
than the 64 of one workgroup of k_tan_hinge_channels and no multiple of it.
Bars, each the one tests/test_gpu_signal_tangent.py holds the same construction to:
  S against ``signal_values`` of a forward solve on the same grid          TOL_SIGNAL = 1e-12 of the largest signal    (its line 163)
  S_dot against the transpose identity with ``signal_misfit_value_and_raw``  1e-11, fixed grid and adaptive=True        (its line 272)
  S_dot against extrapolated central differences (4 D(h) - D(2h)) / 3      1e-6                                       (its lines 315-327)
Every comparison prints its worst case before it asserts; the worst cases seen on an MI355X are in profiles/r24_hinge_signal.txt."""
import numpy as np
import pytest

from difflexmm_amd import objective as O
from difflexmm_amd.dynamics import with_leaf

from .test_gpu_hinge_signal import make_terms
from .test_gpu_objective import BATCH, FAST
from .test_gpu_signal_misfit import TOL_SIGNAL
from .test_gpu_signal_tangent import KDIRS, SPI, TS, T, Setup, _col_err, _scalar_case, _transposition
from .test_gpu_tangent_multi import WIDEST, form  # noqa: F401  (form: the fixture, both pass forms)

pytestmark = pytest.mark.gpu

ITEMS_PER_WORKGROUP = 64                                  # kTanHingeThreads
NS = 6


def hinge_terms(c):
    terms, listed, _ = make_terms(c)
    return [t for t in terms if t[0] < NS], listed


@pytest.fixture(scope="module", params=["quads", "kagome"])
def setup(request, hip_lib):
    st = Setup(request.param)
    st.terms, st.listed = hinge_terms(st.c)
    st.ns, st.spec = NS, O.SignalSpec(st.terms, NS, hinge_channels=True)
    return st


def test_signals_equal_the_reverse_entries_and_every_column_moves(setup, form):  # noqa: F811
    s, c = setup.s, setup.c
    n_items = T * len(setup.listed)
    assert n_items > ITEMS_PER_WORKGROUP and n_items % ITEMS_PER_WORKGROUP != 0 and KDIRS == WIDEST + 1
    S, Sd = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents, setup.spec, steps_per_interval=SPI)
    assert S.shape == (BATCH, T, NS) and Sd.shape == (BATCH, KDIRS, T, NS) and np.all(np.abs(Sd).max(axis=2) > 0)
    s(setup.y0, TS, setup.cps, steps_per_interval=SPI)
    ref = s.signal_values(setup.spec)
    e_S = float(np.abs(S - ref).max() / np.abs(ref).max())
    one = s.signal_jvp_multi(setup.y0, TS, setup.cps, setup.tangents[:1], setup.spec, steps_per_interval=SPI)
    e1 = _col_err(one[1][:, 0], Sd[:, 0])
    print(f"[hinge signal tangent] {c.geo.__class__.__name__} {form}: signals against signal_values {e_S:.2e} of the largest (bar {TOL_SIGNAL}); "
          f"K = 1 against column 0 of K = 5: {e1:.2e} (bar 1e-12)")
    assert e_S <= TOL_SIGNAL and e1 <= 1e-12


def test_columns_are_the_transpose_of_the_signal_misfit_gradient(setup, form):  # noqa: F811
    _transposition(setup, f"hinge terms, {setup.c.geo.__class__.__name__} {form} fixed grid", steps_per_interval=SPI)


def test_adaptive_columns_are_the_transpose_on_the_kept_steps(setup, form):  # noqa: F811
    s = setup.s
    old = (s.rtol, s.atol)
    s.rtol = s.atol = 1e-5
    try:
        fwd, rev = _transposition(setup, f"hinge terms, {setup.c.geo.__class__.__name__} {form} adaptive", adaptive=True)
    finally:
        s.rtol, s.atol = old
    assert fwd["step_control"] == "adaptive-dense" and rev["step_control"] == "adaptive-records", (fwd["step_control"], rev["step_control"])


def test_signal_jacfwd_matches_central_differences(hip_lib):
    """The scalar case of tests/test_gpu_signal_tangent.py (quads 6x6, one member) with the hinge terms, the same four leaves, the same
    extrapolated central differences and the same bar."""
    c = _scalar_case()
    s = c.solver
    spec = O.SignalSpec(hinge_terms(c)[0], NS, hinge_channels=True)
    ts, spi = np.linspace(0.0, 4e-4, 5), 12
    y0 = c.random_state(0.05, 0.02, 5.0)
    wrt = ["k_stretch", "damping", "k_contact", "amplitude"]
    S, jac = s.signal_jacfwd(y0, ts, c.cp, wrt, spec, steps_per_interval=spi)
    assert sorted(jac) == sorted(wrt) and all(jac[n].shape == S.shape == (5, NS) for n in wrt)
    x0 = dict(k_stretch=120.0, damping=5e-4, k_contact=1.5, amplitude=FAST["amplitude"])

    def solve(cp):
        s(y0, ts, cp, steps_per_interval=spi)
        return s.signal_values(spec)[0]
    for name in wrt:
        h = 1e-4 * abs(x0[name])
        d1 = (solve(with_leaf(c.cp, name, x0[name] + h)) - solve(with_leaf(c.cp, name, x0[name] - h))) / (2 * h)
        d2 = (solve(with_leaf(c.cp, name, x0[name] + 2 * h)) - solve(with_leaf(c.cp, name, x0[name] - 2 * h))) / (4 * h)
        fd = (4.0 * d1 - d2) / 3.0
        live = np.abs(fd).max(axis=0) > 0
        e = _col_err(jac[name][:, live], fd[:, live])
        print(f"[hinge signal tangent] signal_jacfwd d/d{name} against central differences: {e:.2e} (bar 1e-6); signals that move: {int(live.sum())} of {NS}")
        assert live.any() and np.abs(jac[name]).max() > 0 and np.all(jac[name][:, ~live] == 0.0)
        assert e <= 1e-6, (name, e)
