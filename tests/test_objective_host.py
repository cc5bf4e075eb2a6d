"""The host side of the weighted objectives (difflexmm_amd/objective.py): ``block_weights_from_targets`` and the NumPy yardstick
``host_value_and_cotangent`` of the two kinds the engine evaluates on the device (include/dfx.h: DFX_OBJ_KINETIC, DFX_OBJ_ANGULAR_MOMENTUM).
Value, cotangent and explicit terms against torch.autograd of the same formula in float64 (bar: 1e-13 of the largest entry -- both sides
are a handful of float64 products per entry); with 0/1 weights against ``energy.kinetic_energy`` / ``energy.angular_momentum`` and against
the cotangents ``SplitTargetKineticEnergy`` / ``TargetAngularMomentum`` build inline (the reference's problems/quads_energy_splitting.py:66-88,
quads_spin.py:380-430).  No engine involved."""
import numpy as np
import pytest
import torch

from difflexmm_amd import energy as E
from difflexmm_amd import objective as O

B, T, NB = 3, 5, 11
TOL = 1e-13


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(12)
    fields = rng.normal(size=(B, T, 2, NB, 3)) * np.array([0.4, 0.4, 0.15])
    fields[:, :, 1] *= 50.0
    inertia = rng.uniform(0.5, 2.0, size=(B, NB, 3)) * np.array([1e-6, 1e-6, 1e-5])
    inertia[..., 1] = inertia[..., 0]
    targets = [np.array([2, 3, 6, 7]), np.array([3, 4, 9])]           # overlap on block 3
    weights = np.array([[1.0, -0.5], [0.25, 2.0], [-1.5, 0.75]])      # per member, both signs
    tau = np.array([0.0, 1.0, 0.37, 2.0, 1.0])
    lever0 = rng.normal(size=(B, NB, 2)) * 15.0
    return fields, inertia, targets, weights, tau, lever0


def test_block_weights_from_targets_adds_overlaps_and_stacks_members():
    w = O.block_weights_from_targets(6, [[0, 1], [1, 2]], [1.0, 2.0])
    assert w.shape == (6,) and np.array_equal(w, [1.0, 3.0, 2.0, 0.0, 0.0, 0.0])
    wm = O.block_weights_from_targets(6, [[0, 1], [1, 2]], [[1.0, 2.0], [0.5, -1.0]])
    assert wm.shape == (2, 6) and np.array_equal(wm, [[1.0, 3.0, 2.0, 0, 0, 0], [0.5, -0.5, -1.0, 0, 0, 0]])
    with pytest.raises(ValueError):
        O.block_weights_from_targets(6, [[0, 6]], [1.0])
    with pytest.raises(ValueError):
        O.block_weights_from_targets(6, [[-1]], [1.0])
    with pytest.raises(ValueError):
        O.block_weights_from_targets(6, [[0], [1]], [1.0])


def _torch_value(kind, f, p, w, tau, a):
    tw = tau[None, :, None] * w[:, None, :]
    u, v = f[:, :, 0], f[:, :, 1]
    if kind == O.KINETIC:
        return (tw[..., None] * p[:, None] * v ** 2 / 2).sum(dim=(1, 2, 3))
    rx, ry = a[:, None, :, 0] + u[..., 0], a[:, None, :, 1] + u[..., 1]
    return (tw * (rx * p[:, None, :, 1] * v[..., 1] - ry * p[:, None, :, 0] * v[..., 0] + p[:, None, :, 2] * v[..., 2])).sum(dim=(1, 2))


@pytest.mark.parametrize("kind", [O.KINETIC, O.ANGULAR_MOMENTUM])
@pytest.mark.parametrize("with_tau", [False, True])
def test_host_yardstick_against_autograd(data, kind, with_tau):
    fields, inertia, targets, weights, tau, lever0 = data
    w = O.block_weights_from_targets(NB, targets, weights)
    spec = O.ObjectiveSpec(kind, w, tau if with_tau else None, lever0 if kind == O.ANGULAR_MOMENTUM else None)
    val, fb, m_bar, c_bar = O.host_value_and_cotangent(spec, fields, inertia)
    assert val.shape == (B,) and fb.shape == fields.shape and m_bar.shape == (B, NB, 3) and c_bar.shape == (B, NB, 2)
    ft, pt, at = (torch.tensor(x, requires_grad=True) for x in (fields, inertia, lever0))
    tv = _torch_value(kind, ft, pt, torch.tensor(w), torch.tensor(tau if with_tau else np.ones(T)), at)
    gf, gp, ga = torch.autograd.grad(tv.sum(), (ft, pt, at), allow_unused=True)
    assert relerr(val, tv.detach().numpy()) < TOL
    assert np.abs(fb).max() > 0 and relerr(fb, gf.numpy()) < TOL
    assert relerr(m_bar, gp.numpy()) < TOL
    if kind == O.ANGULAR_MOMENTUM:
        assert np.abs(fb[:, :, 0]).max() > 0 and relerr(c_bar, ga.numpy()) < TOL       # position rows carry cotangents too
    else:
        assert ga is None and not c_bar.any() and not fb[:, :, 0].any()
    # blocks outside every target, and outputs whose time weight is zero, carry nothing
    off = np.setdiff1d(np.arange(NB), np.concatenate(targets))
    assert not fb[:, :, :, off].any() and not m_bar[:, off].any()
    if with_tau:
        assert not fb[:, 0].any()
    # one member without the member axis
    v0, fb0, m0, c0 = O.host_value_and_cotangent(spec._replace(block_weights=w[1], lever0=None if spec.lever0 is None else lever0[1]),
                                                 fields[1], inertia[1])
    assert isinstance(v0, float) and v0 == val[1] and np.array_equal(fb0, fb[1]) and np.array_equal(m0, m_bar[1]) and np.array_equal(c0, c_bar[1])


def test_unit_weights_are_the_energy_functions_and_the_inline_cotangents(data):
    """0/1 weights: the values of energy.kinetic_energy / energy.angular_momentum summed over the output times, and the cotangents and
    explicit terms exactly as the two problem classes write them for one design."""
    fields, inertia, targets, _, _, lever0 = data
    f, p = fields[0], inertia[0]
    # energy splitting: weights of both signs on overlapping targets (SplitTargetKineticEnergy.value_and_grad)
    wts = np.array([0.599, -0.401])
    spec = O.ObjectiveSpec(O.KINETIC, O.block_weights_from_targets(NB, targets, wts))
    val, fb, m_bar, c_bar = O.host_value_and_cotangent(spec, f, p)
    vals = np.array([E.kinetic_energy(f[:, 1, tb, :], p[tb]) for tb in targets])
    fb_in, raw_m = np.zeros_like(f), np.zeros((NB, 3))
    for w, tb in zip(wts, targets):
        v = f[:, 1, tb, :]
        fb_in[:, 1, tb, :] += w * p[tb] * v
        np.add.at(raw_m, tb, w * 0.5 * (v ** 2).sum(0))
    assert abs(val - wts @ vals) < TOL * np.abs(vals).max()
    assert relerr(fb, fb_in) < TOL and relerr(m_bar, raw_m) < TOL and not c_bar.any()
    for i, tb in enumerate(targets):        # one target alone, weight 1: its own kinetic energy
        one = O.host_value_and_cotangent(O.ObjectiveSpec(O.KINETIC, O.block_weights_from_targets(NB, [tb], [1.0])), f, p)[0]
        assert abs(one - vals[i]) < TOL * vals[i]
    # angular momentum of one target about a point (TargetAngularMomentum._value / value_and_grad)
    tb = targets[0]
    cen, centre = lever0[0] + np.array([3.0, -2.0]), np.array([3.0, -2.0])
    spec = O.ObjectiveSpec(O.ANGULAR_MOMENTUM, O.block_weights_from_targets(NB, [tb], [1.0]), None, cen - centre)
    val, fb, m_bar, c_bar = O.host_value_and_cotangent(spec, f, p)
    ref = sum(E.angular_momentum(cen[tb] + f[k, 0, tb, :2], f[k, 1, tb, :], p[tb], reference_point=centre).sum() for k in range(T))
    assert abs(val - ref) < TOL * max(abs(ref), np.abs(fb).max())
    pos, vel, it = cen[tb][None] + f[:, 0, tb, :2] - centre, f[:, 1, tb, :], p[tb]
    fb_in = np.zeros_like(f)
    fb_in[:, 0, tb, 0] = vel[..., 1] * it[:, 1]
    fb_in[:, 0, tb, 1] = -vel[..., 0] * it[:, 0]
    fb_in[:, 1, tb, 0] = -pos[..., 1] * it[:, 0]
    fb_in[:, 1, tb, 1] = pos[..., 0] * it[:, 1]
    fb_in[:, 1, tb, 2] = it[:, 2]
    cen_in, m_in = np.zeros((NB, 2)), np.zeros((NB, 3))
    cen_in[tb, 0], cen_in[tb, 1] = (vel[..., 1] * it[:, 1]).sum(0), (-vel[..., 0] * it[:, 0]).sum(0)
    m_in[tb, 0], m_in[tb, 1], m_in[tb, 2] = (-pos[..., 1] * vel[..., 0]).sum(0), (pos[..., 0] * vel[..., 1]).sum(0), vel[..., 2].sum(0)
    assert relerr(fb, fb_in) < TOL and relerr(c_bar, cen_in) < TOL and relerr(m_bar, m_in) < TOL


def test_spec_is_checked():
    f, p = np.zeros((T, 2, NB, 3)), np.ones((NB, 3))
    with pytest.raises(ValueError):
        O.host_value_and_cotangent(O.ObjectiveSpec(O.ANGULAR_MOMENTUM, np.ones(NB)), f, p)          # no lever0
    with pytest.raises(ValueError):
        O.host_value_and_cotangent(O.ObjectiveSpec(7, np.ones(NB)), f, p)
    with pytest.raises(ValueError):
        O.host_value_and_cotangent(O.ObjectiveSpec(O.KINETIC, np.ones(NB), np.ones(T + 1)), f, p)


def test_binding_declares_the_device_entries(hip_lib):
    """The two entries are HIP-library-only exports of include/dfx.h (the CPU port of the oracle keeps the kinetic entries only): an
    engine on a library without them raises NotImplementedError, as forward mode does."""
    from difflexmm_amd import _binding as b
    for name in ("dfx_objective_value", "dfx_objective_value_and_grad"):
        assert name in b.COMM_EXPORTS and name in b.EXPORTS and hasattr(hip_lib, name)
    assert (b.OBJ_KINETIC, b.OBJ_ANGULAR_MOMENTUM) == (O.KINETIC, O.ANGULAR_MOMENTUM) == (0, 1)


def test_cpu_port_engine_refuses_device_objectives(cpu_lib):
    from .common import Case
    c = Case("quads", 4, True, False, lib=cpu_lib)
    assert not c.solver.engine.has_objective
    with pytest.raises(NotImplementedError, match="dfx_objective_value_and_grad"):
        c.solver.engine.objective_value(O.KINETIC, np.ones(16))
