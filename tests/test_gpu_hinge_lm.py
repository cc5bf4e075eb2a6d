"""The hinge characterisation in forward mode (difflexmm_amd/hinge.py: force_jvp, force_jacobian, residuals_and_jacobian,
run_optimization_lm) on the samples of tests/hinge_common.py: the Jacobian of the force histories against autograd through the oracle
twin, 2 J^T r / r.size against the reverse-mode gradient, the adaptive form, and the Levenberg-Marquardt fit."""
import math

import numpy as np
import pytest
import torch

from difflexmm_amd import hinge as H
from oracle import ref_problems as RP

from .hinge_common import KW, NT, SPI, K, forwards

pytestmark = pytest.mark.gpu

TOL = 1e-9             # the bar of the fit gradient (hinge_common.check_force_displacement_and_fit_gradient)
TRUTH = (110.0, 1.3, 1.35)
LOWER, UPPER = [50.0, 0.5, 0.5], [200.0, 3.0, 3.0]


def _oracle_jacobian(of, k):
    kt = tuple(torch.tensor(v, dtype=torch.float64) for v in k)
    cols = torch.autograd.functional.jacobian(lambda *ks: of.force_displacement(list(ks), SPI)[1], kt)
    return of.force_displacement(list(kt), SPI)[1].detach().numpy(), np.stack([c.numpy() for c in cols], 1)


def _check_gradient_identity(opt, k, tol_value=1e-12):
    r, J = opt.residuals_and_jacobian(k)
    v, g = opt.value_and_grad(k)
    assert r.shape == (opt.target_forces.size,) and J.shape == (r.size, 3)
    e_v = abs(float(np.mean(r ** 2)) - v) / abs(v)
    grad = 2.0 * J.T @ r / r.size
    e_g = np.abs(grad - np.array(g)).max() / np.abs(g).max()
    print("objective", e_v, "2 J^T r / n vs value_and_grad", e_g)
    assert e_v < tol_value and e_g < TOL, (e_v, e_g)
    return r, J


@pytest.fixture(scope="module")
def sample():
    fws, ofs = forwards(None)
    for fw in fws:
        fw.setup()
    return fws, ofs


def _random_targets(fws, seed=4):
    rng = np.random.default_rng(seed)
    targets = {}
    for fw in fws:
        u = np.linspace(0, KW["amplitude"], 9) * (-1.0 if fw.loading_type == "compression" else 1.0)
        targets[fw.loading_type] = np.array([u, 3.0 * np.abs(u) + rng.uniform(-0.2, 0.2, 9), 0.1 * np.ones(9)])
    return targets


def test_force_jacobian_of_the_three_tests_against_the_oracle(sample):
    fws, ofs = sample
    for fw, of in zip(fws, ofs):
        forces, jac = fw.force_jacobian(K)
        assert forces.shape == (NT,) and jac.shape == (NT, 3)
        assert fw.solve_dynamics.stats["step_control"] == "fixed"
        ref_f, ref_j = _oracle_jacobian(of, K)
        assert np.abs(forces - ref_f).max() < TOL * np.abs(ref_f).max()
        for j in range(3):
            err = np.abs(jac[:, j] - ref_j[:, j]).max() / np.abs(ref_j[:, j]).max()
            print(fw.loading_type, "column", j, err)
            assert np.abs(ref_j[:, j]).max() > 0 and err < TOL, (fw.loading_type, j, err)
        # force_jvp is linear in its directions: one combined direction equals the combination of the columns
        w = np.array([0.3, -1.1, 0.7])
        sol, cp = fw.solve(K)
        _, cols = fw.solve_dynamics.jacfwd(fw.state0, fw.timepoints, cp, ["k_stretch", "k_shear", "k_rot"], steps_per_interval=SPI)
        mixed = sum(wi * cols[n] for wi, n in zip(w, ("k_stretch", "k_shear", "k_rot")))
        one = fw.force_jvp(sol, cp, [mixed], [w])
        assert one.shape == (1, NT) and np.abs(one[0] - jac @ w).max() < 1e-11 * np.abs(jac @ w).max()


def test_gradient_identity_on_the_three_tests(sample):
    fws, _ = sample
    opt = H.HingeResponseError(fws, _random_targets(fws))
    r, J = _check_gradient_identity(opt, K)
    # the order of forward_problems
    f0, j0 = fws[0].force_jacobian(K)
    assert np.array_equal(r[:NT], f0 - opt.target_forces[0]) and np.array_equal(J[:NT], j0)


def test_quads_sample_in_shear():
    from difflexmm_amd.geometry import QuadGeometry
    n1, n2 = 4, 4
    g = QuadGeometry(n1, n2, KW["spacing"], KW["bond_length"])
    rng = np.random.default_rng(8)
    hs, vs = (b + rng.uniform(-0.3, 0.3, b.shape) for b in g.get_design_from_rotated_square(25 * math.pi / 180))
    fw = H.HingeQuadsForward(n1_blocks=n1, n2_blocks=n2, horizontal_shifts=hs, vertical_shifts=vs, loading_type="shear",
                             steps_per_interval=SPI, **KW)
    of = RP.HingeForward("quads", n1, n2, KW["spacing"], KW["bond_length"], (hs, vs), KW["k_stretch"], KW["density"], KW["damping"], "shear",
                         KW["amplitude"], KW["loading_rate"], NT, use_contact=True, k_contact=1.5, min_angle=KW["min_angle"],
                         cutoff_angle=KW["cutoff_angle"])
    u = np.linspace(0, KW["amplitude"], 7)
    opt = H.HingeResponseError([fw], {"shear": np.array([u, 2.0 * u, np.ones(7)])})
    r, J = _check_gradient_identity(opt, K)
    ref_f, ref_j = _oracle_jacobian(of, K)
    assert np.abs(r + opt.target_forces[0] - ref_f).max() < TOL * np.abs(ref_f).max()
    for j in range(3):
        err = np.abs(J[:, j] - ref_j[:, j]).max() / np.abs(ref_j[:, j]).max()
        print("quads, shear, column", j, err)
        assert err < TOL, (j, err)


def test_adaptive_form():
    """Problems set up without steps_per_interval: the Jacobian goes through the adaptive solve on its own accepted steps, and its
    gradient is the one the reverse sweep returns for that same adaptive solve."""
    fws = [H.HingeForward(n1_cells=2, n2_cells=2, initial_angle=25 * math.pi / 180, loading_type=lt,
                          force_multiplier=-1.0 if lt == "compression" else 1.0, **KW) for lt in ("tension", "compression", "shear")]
    for fw in fws:
        fw.setup()
        assert fw.steps_per_interval is None
    opt = H.HingeResponseError(fws, _random_targets(fws))
    r, J = opt.residuals_and_jacobian(K)
    for fw in fws:
        st = fw.solve_dynamics.stats
        print(fw.loading_type, st["step_control"], "kept", st.get("kept_trajectory"), "steps", st.get("steps_per_member"))
        assert st["step_control"] == "adaptive-dense", st["step_control"]
    # the objective of two adaptive solves of the same problem: the forward pass and the tangent pass agree to rounding
    _check_gradient_identity(opt, K, tol_value=1e-12)
    for fw in fws:
        assert fw.solve_dynamics.stats["step_control"] == "adaptive-records", fw.solve_dynamics.stats["step_control"]


def _fit(sample, start, n_iterations):
    fws, _ = sample
    targets = {fw.loading_type: np.vstack([fw.force_displacement(*fw.solve(TRUTH)), np.ones(NT)]) for fw in fws}
    opt = H.HingeResponseError(fws, targets)
    opt.run_optimization_lm(start, n_iterations, lower_bound=LOWER, upper_bound=UPPER)
    best = opt.design_values[int(np.argmin(opt.objective_values))]
    err = np.abs(np.array(best) / np.array(TRUTH) - 1).max()
    print("start", start, "evaluations", len(opt.objective_values), "objectives", opt.objective_values, "max relative error", err)
    return opt, err


def test_run_optimization_lm(sample):
    opt, err = _fit(sample, K, 8)
    assert len(opt.objective_values) <= 8 and err <= 1e-6
    assert len(opt.design_values) == len(opt.objective_values) and opt.design_values[0] == tuple(float(k) for k in K)
    assert all(lo <= x <= hi for d in opt.design_values for x, lo, hi in zip(d, LOWER, UPPER))
    assert set(opt.fitted_responses) == {"tension", "compression", "shear"} and opt.fitted_responses["shear"].shape == (2, NT)
    for fw, target in zip(opt.forward_problems, opt.target_forces):
        assert np.abs(opt.fitted_responses[fw.loading_type][1] - target).max() < 1e-5 * np.abs(target).max()
    d = H.HingeResponseError.from_dict(opt.to_dict())
    assert len(d.forward_problems) == 3 and d.objective_values == opt.objective_values and d.design_values == opt.design_values


def test_run_optimization_lm_from_the_upper_bounds(sample):
    """(200, 3, 3): the same loop on the CPU port's arithmetic with a central-difference Jacobian is below 1e-6 after its sixth
    evaluation (two of the first three steps end on a bound of k_rot); ten leave margin."""
    opt, err = _fit(sample, tuple(UPPER), 10)
    assert len(opt.objective_values) <= 10 and err <= 1e-6
