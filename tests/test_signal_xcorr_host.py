"""No GPU: the host side of the signal cross-correlation objective (difflexmm_amd/objective.py: CorrelationSpec, xcorr_of_signals,
host_xcorr_value_and_cotangent; include/dfx.h: dfx_signal_xcorr, dfx_signal_xcorr_value[_and_grad]).

  * xcorr_of_signals against the module's own port of the reference's measures: compute_xcorr2d on random (n_pairs, T) records to 1e-13
    of the largest entry (delay d sits at index T - 1 - d of the reference's slice), and compute_space_time_xcorr on the reference's own
    test_xcorr (shapes (10, 20): a record against itself gives 1 at delay 0, against itself rolled by 3 along time delay 3);
  * host_xcorr_value_and_cotangent against torch autograd of an independent fp64 restatement written here (explicit loops over pairs,
    lags and outputs; torch.logsumexp / softmax / max for the reductions): three normalisations x three reductions, a delay term under
    "softmax", T = 5 and T = 70, D in {0, 3, T - 1}, a signal paired with itself, a signal in two pairs, a template pair; bar 1e-12 of
    the largest reference entry.  One case also against central differences;
  * every ValueError of the spec, and NotImplementedError from the binding on the CPU port's library.
Every comparison prints its worst case before it asserts."""
import numpy as np
import pytest
import torch

from difflexmm_amd import objective as O

TOL = 1e-12
NORMS, REDUCES = ("reference", "coefficient", "none"), ("at", "max", "softmax")
# signal 0 with itself, signal 1 in two pairs, a template pair
PAIRS = [(0, 0), (1, 2), (3, 1), (2, -2)]
NS, NT, NB = 4, 2, 6


def sig_spec():
    # four signals of field components: displacement and velocity rows, one signal with two terms
    return O.SignalSpec([(0, 1, 0, 1.0), (1, 2, 4, 0.5), (1, 3, 1, -2.0), (2, 4, 2, 1.5), (3, 5, 3, 1.0)], NS)


def restated(fields, templates, pairs, D, norm, reduce, lag, beta, w_peak, w_delay, target, terms):
    """J, M, delta from the fields in torch fp64, nothing shared with the module under test: explicit sums over pairs, lags and outputs"""
    T = fields.shape[0]
    S = [sum(coef * fields[:, c // 3, b, c % 3] for s2, b, c, coef in terms if s2 == s) for s in range(NS)]
    A = [S[a] for a, _ in pairs]
    B = [S[b] if b >= 0 else templates[:, -1 - b] for _, b in pairs]
    R = []
    for d in range(-D, D + 1):
        acc = torch.zeros((), dtype=torch.float64)
        for Ap, Bp in zip(A, B):
            for k in range(T):
                if 0 <= k + d < T:
                    acc = acc + Ap[k] * Bp[k + d]
        R.append(acc)
    R = torch.stack(R)
    EA, EB = sum((a * a).sum() for a in A), sum((b * b).sum() for b in B)
    N = EA if norm == "reference" else torch.sqrt(EA * EB) if norm == "coefficient" else torch.ones((), dtype=torch.float64)
    rho = R / N
    lags = torch.arange(-D, D + 1, dtype=torch.float64)
    if reduce == "at":
        M, delta = rho[lag + D], torch.tensor(float(lag), dtype=torch.float64)
    elif reduce == "max":
        M, at = torch.max(rho, 0)
        delta = lags[at]
    else:
        M = torch.logsumexp(beta * rho, 0) / beta
        delta = (torch.softmax(beta * rho, 0) * lags).sum()
    return w_peak * M + 0.5 * w_delay * (delta - target) ** 2, M, delta, rho


def cases():
    for T in (5, 70):
        for D in (0, 3, T - 1):
            for norm in NORMS:
                for reduce in REDUCES:
                    yield T, D, norm, reduce, 0.0
                yield T, D, norm, "softmax", 0.7


def make(T, D, norm, reduce, w_delay, seed=0):
    rng = np.random.default_rng(seed + 7 * T + D)
    t = np.arange(T)[:, None, None, None]
    fields = rng.normal(size=(T, 2, NB, 3)) * 0.3 + np.sin(0.4 * t + rng.uniform(0, 3, (1, 2, NB, 3)))
    templates = rng.normal(size=(T, NT))
    lag = {0: 0, 3: -2}.get(D, 1 - (T // 3))
    spec = O.CorrelationSpec(sig_spec(), PAIRS, D, templates, norm, reduce, lag if reduce == "at" else None, 3.0 if reduce == "softmax" else None,
                             -1.3, w_delay, 0.8)
    return fields, templates, spec


def test_rho_against_compute_xcorr2d():
    rng = np.random.default_rng(1)
    worst = 0.0
    for n_pairs, T in ((1, 5), (3, 20), (10, 20), (4, 70)):
        A, B = rng.normal(size=(n_pairs, T)), rng.normal(size=(n_pairs, T))
        ref = O.compute_xcorr2d(A, B, shift=(0, None))                       # (2 T - 1,): delay d at index T - 1 - d
        S = np.concatenate([A, B]).T                                        # (T, 2 n_pairs): signals A_0.., B_0..
        spec = O.CorrelationSpec(O.SignalSpec.fields_of([(i, 0) for i in range(2 * n_pairs)]), [(i, n_pairs + i) for i in range(n_pairs)], T - 1)
        rho = O.xcorr_of_signals(spec, S)
        err = float(np.abs(rho - ref[::-1]).max() / np.abs(ref).max())
        worst = max(worst, err)
        print(f"[signal xcorr host] {n_pairs} pairs, T = {T}: rho against compute_xcorr2d {err:.2e} of the largest entry")
        assert rho.shape == (2 * T - 1,) and err <= 1e-13
    assert worst <= 1e-13


def test_max_against_compute_space_time_xcorr():
    """the reference's own test_xcorr: shapes (10, 20)"""
    rng = np.random.default_rng(0)
    st0 = rng.uniform(size=(10, 20))
    spec = O.CorrelationSpec(O.SignalSpec.fields_of([(i, 0) for i in range(20)]), [(i, 10 + i) for i in range(10)], 19, reduce="max")
    for st1, delay in ((st0, 0), (np.roll(st0, 3, axis=1), 3)):
        ref_max, ref_delay = O.compute_space_time_xcorr(st0, st1)
        J, M, delta, _ = O.xcorr_value_and_signal_cotangent(spec, np.concatenate([st0, st1]).T)
        print(f"[signal xcorr host] roll {delay}: peak {M:.15f} (reference {ref_max:.15f}), delay {delta} (reference {ref_delay})")
        assert ref_delay == delay == delta and abs(M - ref_max) <= 1e-13 * abs(ref_max) and J == M
    assert abs(O.xcorr_value_and_signal_cotangent(spec, np.concatenate([st0, st0]).T)[1] - 1.0) <= 1e-15


@pytest.mark.parametrize("T,D,norm,reduce,w_delay", list(cases()))
def test_cotangent_against_autograd(T, D, norm, reduce, w_delay):
    fields, templates, spec = make(T, D, norm, reduce, w_delay)
    f = torch.tensor(fields, dtype=torch.float64, requires_grad=True)
    J, M, delta, rho = restated(f, torch.tensor(templates, dtype=torch.float64), PAIRS, D, norm, reduce, spec.lag, spec.beta, spec.w_peak, w_delay,
                                spec.delay_target, spec.signal_spec.terms)
    ref, = torch.autograd.grad(J, f)
    ref = ref.numpy()
    Jh, Mh, dh, fb = O.host_xcorr_value_and_cotangent(spec, fields)
    rho_h = O.xcorr_of_signals(spec, O.host_signal_values(spec.signal_spec, fields))
    e = dict(rho=float(np.abs(rho_h - rho.detach().numpy()).max() / np.abs(rho.detach().numpy()).max()), J=abs(Jh - J.item()) / abs(J.item()),
             M=abs(Mh - M.item()) / abs(M.item()), delta=abs(dh - delta.item()) / max(D, 1),
             fields_bar=float(np.abs(fb - ref).max() / np.abs(ref).max()))
    print(f"[signal xcorr host] T={T} D={D} {norm} {reduce} w_delay={w_delay}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert np.abs(ref).max() > 0 and fb.shape == fields.shape
    assert all(v <= TOL for v in e.values()), e
    # a member axis gives the same numbers per member
    Jb, Mb, db, fbb = O.host_xcorr_value_and_cotangent(spec, np.stack([fields, 2.0 * fields]))
    assert Jb.shape == (2,) and Jb[0] == Jh and Mb[0] == Mh and db[0] == dh and np.array_equal(fbb[0], fb)


def test_one_case_against_central_differences():
    fields, templates, spec = make(5, 3, "coefficient", "softmax", 0.7)
    J, _, _, fb = O.host_xcorr_value_and_cotangent(spec, fields)
    rng = np.random.default_rng(5)
    for trial in range(3):
        v = rng.normal(size=fields.shape)
        h = 1e-6
        fd = (O.host_xcorr_value_and_cotangent(spec, fields + h * v)[0] - O.host_xcorr_value_and_cotangent(spec, fields - h * v)[0]) / (2 * h)
        mine = float(np.sum(fb * v))
        err = abs(mine - fd) / abs(fd)
        print(f"[signal xcorr host] direction {trial}: cotangent against central differences {err:.2e}")
        assert err <= 1e-8


def test_zero_normalisation_gives_nan_values_and_a_zero_cotangent():
    fields, templates, spec = make(5, 3, "reference", "softmax", 0.7)
    dead = fields.copy()
    dead[:, 0, 1, 0] = 0.0                                                   # signal 0 is side A of pair 0 ...
    spec = O.CorrelationSpec(spec.signal_spec, [(0, 1)], 3, None, "reference", "softmax", None, 3.0, 1.0, 0.7, 0.8)
    J, M, d, fb = O.host_xcorr_value_and_cotangent(spec, np.stack([fields, dead]))
    assert np.isfinite([J[0], M[0], d[0]]).all() and np.abs(fb[0]).max() > 0
    assert np.isnan([J[1], M[1], d[1]]).all() and not fb[1].any()


def test_spec_refusals():
    s = sig_spec()
    tp = np.zeros((5, 2))
    bad = [dict(pairs=[]), dict(pairs=[(0, 1, 2)]), dict(pairs=[(0.5, 1)]), dict(pairs=[(4, 0)]), dict(pairs=[(0, 4)]), dict(pairs=[(-1, 0)]),
           dict(pairs=[(0, -1)], templates=None), dict(pairs=[(0, -3)]), dict(max_lag=-1), dict(max_lag=5), dict(max_lag=1.5),
           dict(templates=np.zeros(5)), dict(templates=np.where(np.arange(10).reshape(5, 2) == 3, np.nan, 0.0)),
           dict(normalisation="energy"), dict(reduce="mean"), dict(reduce="at", lag=3), dict(reduce="at", lag=0.5),
           dict(reduce="softmax"), dict(reduce="softmax", beta=0.0), dict(reduce="softmax", beta=-1.0), dict(reduce="softmax", beta=np.inf),
           dict(w_delay=1.0), dict(reduce="at", lag=1, w_delay=1.0), dict(w_peak=np.nan), dict(reduce="softmax", beta=1.0, w_delay=np.inf),
           dict(delay_target=np.nan)]
    for kw in bad:
        args = dict(pairs=[(0, 1), (2, -2)], max_lag=2, templates=tp)
        args.update(kw)
        with pytest.raises(ValueError):
            O.CorrelationSpec(s, **args)
    ok = O.CorrelationSpec(s, [(0, 1), (2, -2)], 2, tp, "coefficient", "softmax", None, 2.0, -1.0, 0.5, 1.0)
    other = ok.with_templates(np.ones((3, 5, 2)))
    assert other.templates.shape == (3, 5, 2) and other.pairs == ok.pairs and other.beta == 2.0 and other.w_delay == 0.5 and ok.n_lags == 5
    assert O.CorrelationSpec(s, [(0, 1)], 2, reduce="at").lag == 0
    with pytest.raises(ValueError):
        O.xcorr_of_signals(ok, np.zeros((4, NS)))                                # templates of another T
    with pytest.raises(ValueError):
        O.xcorr_of_signals(other, np.zeros((5, NS)))                             # per-member templates against one member
    with pytest.raises(ValueError, match="force components"):
        O.host_xcorr_value_and_cotangent(O.CorrelationSpec(O.SignalSpec([(0, 1, 6, 1.0)], 1), [(0, 0)], 1), np.zeros((5, 2, NB, 3)))


def test_cpu_port_has_no_cross_correlation(cpu_lib):
    from .common import Case
    c = Case("quads", 4, True, False, seed=3, lib=cpu_lib)
    eng = c.solver.engine
    assert not eng.has_signal_xcorr
    for call in (lambda: eng.signal_xcorr([(0, 1, 0, 1.0)], 1, [(0, 0)], 0), lambda: eng.signal_xcorr_value([(0, 1, 0, 1.0)], 1, [(0, 0)], 0),
                 lambda: eng.signal_xcorr_value_and_grad([(0, 1, 0, 1.0)], 1, [(0, 0)], 0)):
        with pytest.raises(NotImplementedError, match="dfx_signal_xcorr_value_and_grad"):
            call()
