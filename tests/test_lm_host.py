"""optimize.levenberg_marquardt on closed-form problems and on the hinge fit of tests/hinge_common.py (CPU port, central-difference
Jacobian), and the forward-mode entries the CPU port does not have.  No GPU."""
import numpy as np
import pytest

from difflexmm_amd import hinge as H
from difflexmm_amd.optimize import levenberg_marquardt

from .hinge_common import K, NT, forwards


def test_a_linear_problem_converges_in_one_step():
    rng = np.random.default_rng(0)
    A, x_true = rng.normal(size=(7, 3)), np.array([1.5, -2.0, 0.25])
    calls = []

    def fun(x):
        calls.append(x.copy())
        return A @ (x - x_true), A
    # lam0 = 0: the Gauss-Newton step, exact on a linear problem
    res = levenberg_marquardt(fun, np.zeros(3), lam0=0.0)
    assert np.abs(res.x[1] - x_true).max() < 1e-13 and len(res.x) >= 2
    # the default damping: each accepted step leaves lam / (1 + lam) of the error in every scaled direction
    res = levenberg_marquardt(fun, np.zeros(3), max_evaluations=6)
    assert res.fun[1] < 1e-3 * res.fun[0] and np.abs(res.x[-1] - x_true).max() < 1e-12
    assert all(b < a for a, b in zip(res.fun, res.fun[1:])) and res.n_eval <= 6 and len(res.evaluated) == res.n_eval
    assert res.status in ("xtol", "maxeval")


def test_a_bounded_exponential_fit_ends_on_its_bound():
    t = np.linspace(0.0, 2.0, 15)
    y = 2.0 * np.exp(-1.5 * t)

    def fun(x):
        e = np.exp(-x[1] * t)
        return x[0] * e - y, np.stack([e, -x[0] * t * e], 1)
    # the unconstrained optimum (2, 1.5) lies outside: the rate may not exceed 1
    res = levenberg_marquardt(fun, [1.0, 0.5], lower=[0.0, 0.0], upper=[5.0, 1.0], max_evaluations=40)
    x = res.x[-1]
    assert x[1] == 1.0 and all(0.0 <= a[0] <= 5.0 and 0.0 <= a[1] <= 1.0 for a, _, _ in res.evaluated)
    # on the bound the amplitude is the linear least-squares one
    e = np.exp(-t)
    assert abs(x[0] - (e @ y) / (e @ e)) < 1e-8
    assert all(b < a for a, b in zip(res.fun, res.fun[1:]))
    # without bounds it finds the generating parameters
    free = levenberg_marquardt(fun, [1.0, 0.5], max_evaluations=40)
    assert np.abs(free.x[-1] - [2.0, 1.5]).max() < 1e-8


def test_a_rank_deficient_jacobian_ends_by_the_lambda_cap():
    # the second unknown does not enter: a zero column, J^T J + lam diag(J^T J) is singular for every lam
    a = np.array([1.0, 2.0, 3.0])

    def fun(x):
        return a * x[0] - 1.0, np.stack([a, np.zeros(3)], 1)
    res = levenberg_marquardt(fun, [0.0, 0.7], max_evaluations=50)
    assert res.status == "lambda" and res.lam > 1e8 and res.n_eval == 1 and np.array_equal(res.x[-1], [0.0, 0.7])
    # two equal columns: singular only at lam = 0; the damped steps reach the minimum, then no trial decreases it and lam runs up
    def fun2(x):
        return a * (x[0] + x[1]) - np.array([1.0, 2.0, 2.0]), np.stack([a, a], 1)
    res = levenberg_marquardt(fun2, [0.0, 0.0], max_evaluations=200, xtol=0.0)
    assert res.status in ("lambda", "xtol") and abs(res.x[-1].sum() - (a @ [1.0, 2.0, 2.0]) / (a @ a)) < 1e-9


@pytest.fixture(scope="module")
def hinge_fit(cpu_lib):
    fws, _ = forwards(cpu_lib)
    for fw in fws:
        fw.setup()
    truth = (110.0, 1.3, 1.35)
    targets = {fw.loading_type: np.vstack([fw.force_displacement(*fw.solve(truth)), np.ones(NT)]) for fw in fws}
    return H.HingeResponseError(fws, targets), truth


def test_hinge_fit_by_levenberg_marquardt_on_the_cpu_port(hinge_fit):
    """The fit of check_fit_loops (2 x 2 cells, 5 outputs, 10 steps per interval) with a central-difference Jacobian, relative step 1e-6:
    max relative error of k <= 1e-6 within 8 evaluations (the same arithmetic reaches 1.4e-7 after 3 accepted steps)."""
    opt, truth = hinge_fit
    opt.setup_objective()

    def residuals(x):
        return np.concatenate([p.force_displacement(*p.solve(tuple(x)))[1] - t for p, t in zip(opt.forward_problems, opt.target_forces)])

    def fun(x):
        J = np.empty((opt.target_forces.size, 3))
        for j in range(3):
            h = 1e-6 * x[j]
            xp, xm = x.copy(), x.copy()
            xp[j] += h
            xm[j] -= h
            J[:, j] = (residuals(xp) - residuals(xm)) / (2 * h)
        return residuals(x), J
    res = levenberg_marquardt(fun, np.array(K), lower=[50.0, 0.5, 0.5], upper=[200.0, 3.0, 3.0], max_evaluations=8)
    err = np.abs(res.x[-1] / np.array(truth) - 1).max()
    print("evaluations", res.n_eval, "objectives", res.fun, "max relative error", err)
    assert res.n_eval <= 8 and err <= 1e-6
    assert abs(res.fun[0] - opt.objective_fn(K)) < 1e-12 * res.fun[0]          # the objective keeps the reference's definition


def test_forward_mode_entries_are_missing_on_the_cpu_port(hinge_fit):
    opt, _ = hinge_fit
    p = opt.forward_problems[0]
    e = p._force.engine
    assert not e.has_rhs_jvp
    y = np.zeros((e.batch, 2, e.n_blocks, 3))
    with pytest.raises(NotImplementedError, match="dfx_rhs_jvp"):
        e.rhs_jvp(y, 0.0, None, None, 1)
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent_multi"):
        opt.residuals_and_jacobian(K)
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent_multi"):
        opt.run_optimization_lm(K, 3)
    assert opt.objective_values == [] and opt.design_values == []
