"""No GPU: the host layers of the signal projections (difflexmm_amd/objective.py: ProjectionSpec, fourier_basis,
host_projection_values, host_projection_value_and_cotangent; include/dfx.h: dfx_signal_projection*): argument checks, the Fourier rows
against numpy.fft.rfft, the projections against an einsum over host_signal_values, the cotangent against torch.autograd on the formula,
and the identity that turns the projection objective into the signal misfit (B = I, W_sk = tau_k omega_s, Ptarget = Starget)."""
import numpy as np
import pytest
import torch

from difflexmm_amd import objective as O

T, NB = 23, 7
TERMS = [(0, 1, 0, 1.0), (0, 2, 4, -0.5), (1, 3, 2, 2.0), (2, 6, 5, 1e-2), (2, 1, 1, 0.25)]


def _fields(batch=None, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, 2, NB, 3) if batch is None else (batch, T, 2, NB, 3))


def _spec(n_rows=4, targets=None, seed=1, signal_targets=None):
    rng = np.random.default_rng(seed)
    return O.ProjectionSpec(O.SignalSpec(TERMS, 3, signal_targets), rng.normal(size=(n_rows, T)), rng.normal(size=(3, n_rows)), targets)


def test_projection_spec_checks_shapes_and_finiteness():
    sig = O.SignalSpec(TERMS, 3)
    B, W = np.ones((4, T)), np.ones((3, 4))
    sp = O.ProjectionSpec(sig, B, W)
    assert sp.n_rows == 4 and sp.targets is None and sp.basis.shape == (4, T)
    with pytest.raises(ValueError, match="targets of the signal spec have T"):
        O.ProjectionSpec(O.SignalSpec(TERMS, 3, np.zeros((T + 1, 3))), B, W)
    for bad in (np.ones((4, 4)), np.ones((4,)), np.ones((3, 4, 1)), np.ones((2, 4))):
        with pytest.raises(ValueError, match="row_weights must be"):
            O.ProjectionSpec(sig, B, bad)
    with pytest.raises(ValueError, match="n_rows >= 1"):
        O.ProjectionSpec(sig, np.ones((0, T)), np.ones((3, 0)))
    with pytest.raises(ValueError, match="basis must be"):
        O.ProjectionSpec(sig, np.ones(T), W)
    for name, args in (("basis", (np.where(np.arange(T) == 3, np.nan, B), W)), ("row_weights", (B, np.where(W > 0, np.inf, W))),
                       ("targets", (B, W, np.full((3, 4), np.nan)))):
        with pytest.raises(ValueError, match=f"{name}: non-finite"):
            O.ProjectionSpec(sig, *args)
    with pytest.raises(ValueError, match="targets must be"):
        O.ProjectionSpec(sig, B, W, np.zeros((4, 3)))
    per_member = sp.with_targets(np.ones((5, 3, 4)))
    assert per_member.targets.shape == (5, 3, 4) and per_member.basis is not None and np.array_equal(per_member.row_weights, W)
    assert sp.with_targets(None).targets is None


def test_fourier_basis_is_dt_times_rfft_on_a_uniform_grid():
    n, dt = 48, 2.5e-4
    t = dt * np.arange(n)
    freqs = np.fft.rfftfreq(n, dt)
    rng = np.random.default_rng(3)
    s = rng.normal(size=n)
    Bm = O.fourier_basis(t, freqs, quadrature="rectangle")
    assert Bm.shape == (2 * len(freqs), n)
    P = Bm @ s
    mine = P[0::2] - 1j * P[1::2]
    ref = dt * np.fft.rfft(s)
    err = np.abs(mine - ref).max() / np.abs(ref).max()
    print(f"[signal projection] fourier_basis against dt * rfft: {err:.2e}")
    assert err <= 1e-13
    # the trapezoid rule differs from the rectangle rule in the two end weights only
    Bt = O.fourier_basis(t, freqs[1:3])
    assert np.allclose(Bt[:, 1:-1], Bm[2:6, 1:-1], rtol=1e-12, atol=0) and np.allclose(Bt[:, 0], 0.5 * Bm[2:6, 0], rtol=1e-12, atol=0)
    # a non-uniform grid: trapezoid weights integrate a linear function exactly
    tn = np.sort(rng.uniform(0.0, 1.0, 17))
    q = O.fourier_basis(tn, [0.0])[0]
    assert abs(q @ (3.0 * tn + 1.0) - (1.5 * (tn[-1] ** 2 - tn[0] ** 2) + tn[-1] - tn[0])) < 1e-14


def test_fourier_basis_windows_and_refusals():
    t = np.linspace(0.2, 1.7, 31)
    f = [0.7, 3.1]
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * (t - t[0]) / (t[-1] - t[0]))
    assert np.array_equal(O.fourier_basis(t, f, window="hann"), O.fourier_basis(t, f, window=hann))
    assert np.array_equal(O.fourier_basis(t, f, window=np.ones(31)), O.fourier_basis(t, f))
    assert not np.array_equal(O.fourier_basis(t, f, window="hann"), O.fourier_basis(t, f))
    assert abs(hann[0]) < 1e-15 and abs(hann[-1]) < 1e-15 and abs(hann[15] - 1.0) < 1e-15
    for kw in (dict(window="hamming"), dict(window=np.ones(30)), dict(quadrature="simpson")):
        with pytest.raises(ValueError):
            O.fourier_basis(t, f, **kw)
    with pytest.raises(ValueError):
        O.fourier_basis(t[::-1], f)
    with pytest.raises(ValueError):
        O.fourier_basis(t, [])


@pytest.mark.parametrize("batch", [None, 3])
def test_host_projection_values_are_the_einsum_of_the_signals(batch):
    f, sp = _fields(batch), _spec()
    P = O.host_projection_values(sp, f)
    assert P.shape == ((3, 4) if batch is None else (3, 3, 4))
    assert np.array_equal(P, np.einsum("jk,...ks->...sj", sp.basis, O.host_signal_values(sp.signal_spec, f)))
    with pytest.raises(ValueError, match="force components"):
        O.host_projection_values(O.ProjectionSpec(O.SignalSpec([(0, 1, 6, 1.0)], 1), np.ones((2, T)), np.ones((1, 2))), f)
    with pytest.raises(ValueError, match="basis has T"):
        O.host_projection_values(sp, f[..., :-1, :, :, :])


def _torch_value(sp, f, targets):
    ft = torch.tensor(f, requires_grad=True)
    cols = [None] * sp.signal_spec.n_signals
    for s, b, c, coef in sp.signal_spec.terms:
        src = coef * ft[..., c // 3, b, c % 3]
        cols[s] = src if cols[s] is None else cols[s] + src
    S = torch.stack(cols, dim=-1)
    P = torch.einsum("jk,...ks->...sj", torch.tensor(sp.basis), S)
    J = 0.5 * torch.sum(torch.tensor(sp.row_weights) * (P - torch.tensor(targets)) ** 2, dim=(-2, -1))
    g, = torch.autograd.grad(J.sum(), ft)
    return J.detach().numpy(), g.numpy()


@pytest.mark.parametrize("targets", ["none", "shared", "per_member"])
def test_host_cotangent_is_autograd_of_the_formula(targets):
    f = _fields(3)
    rng = np.random.default_rng(5)
    tg = None if targets == "none" else rng.normal(size=(3, 4) if targets == "shared" else (3, 3, 4))
    sp = _spec(targets=tg)
    val, fb = O.host_projection_value_and_cotangent(sp, f)
    ref_v, ref_g = _torch_value(sp, f, np.zeros((3, 4)) if tg is None else tg)
    assert val.shape == (3,) and fb.shape == f.shape and np.abs(ref_g).max() > 0
    assert np.abs(val - ref_v).max() <= 1e-13 * np.abs(ref_v).max()
    assert np.abs(fb - ref_g).max() <= 1e-13 * np.abs(ref_g).max()
    if targets != "per_member":
        v1, fb1 = O.host_projection_value_and_cotangent(sp, f[1])
        assert isinstance(v1, float) and v1 == val[1] and np.array_equal(fb1, fb[1])
    else:
        with pytest.raises(ValueError, match="per-member targets"):
            O.host_projection_value_and_cotangent(sp, f[1])


def test_identity_basis_gives_the_signal_misfit():
    f = _fields(2, seed=8)
    rng = np.random.default_rng(9)
    Starget, omega, tau = rng.normal(size=(2, T, 3)), np.array([1.0, 0.5, 2.0]), rng.uniform(0.0, 2.0, T)
    sig = O.SignalSpec(TERMS, 3)
    sp = O.ProjectionSpec(sig, np.eye(T), omega[:, None] * tau[None, :], np.swapaxes(Starget, 1, 2))
    val, fb = O.host_projection_value_and_cotangent(sp, f)
    S = O.host_signal_values(sig, f)
    c = tau[None, :, None] * omega[None, None, :] * (S - Starget)
    misfit = 0.5 * np.sum(c * (S - Starget), axis=(1, 2))
    fb_ref = np.zeros_like(f)
    for s, b, comp, coef in TERMS:
        fb_ref[:, :, comp // 3, b, comp % 3] += coef * c[:, :, s]
    assert np.abs(val - misfit).max() <= 1e-14 * np.abs(misfit).max()
    assert np.abs(fb - fb_ref).max() <= 1e-14 * np.abs(fb_ref).max()


def test_the_binding_lists_the_three_entries_with_the_hip_only_names(hip_lib):
    from difflexmm_amd._binding import COMM_EXPORTS
    names = ["dfx_signal_projections", "dfx_signal_projection_value", "dfx_signal_projection_value_and_grad"]
    assert all(n in COMM_EXPORTS and hasattr(hip_lib, n) for n in names)
