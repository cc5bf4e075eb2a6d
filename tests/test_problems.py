"""Problem layer: BC index patterns, objectives, multi-input weighting, constraints,
the optimisation loop -- exercised through the CPU port (host logic; the same code drives the HIP engine)."""
import math

import numpy as np
import pytest

from difflexmm_amd import problems as P
from difflexmm_amd.geometry import KagomeGeometry, QuadGeometry


def _quads(lib, side="left", shift=0, n=6):
    fw = P.QuadsFocusingForward(
        n1_blocks=n, n2_blocks=n, spacing=15.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19, k_rot=1.5,
        density=6.18e-9, damping=1e-4 * np.ones((n * n, 3)), amplitude=7.5, loading_rate=3000.0, input_delay=1e-5,
        n_excited_blocks=2, loaded_side=side, input_shift=shift, simulation_time=4e-4, n_timepoints=5,
        use_contact=True, k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180,
        steps_per_interval=10, _lib=lib)
    fw.setup()
    return fw


def _design(fw, seed=0, amp=0.2):
    rng = np.random.default_rng(seed)
    base = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    return tuple(b + rng.uniform(-amp, amp, b.shape) for b in base)


def test_quads_bc_patterns_match_reference_counts():
    """24x16 paper lattice: 6 driven + 36 clamped = 42 constrained DOFs, ordering as in
    problems/quads_focusing.py:104-197 (driven pairs first, first n_excited entries carry the pulse)."""
    g = QuadGeometry(24, 16, 15.0, 2.25)
    pairs, vec, driven, clamped = P.quads_focusing_constraints(g, 2, "left", 0, 2)
    assert len(pairs) == 42 and vec.sum() == 2 and np.all(vec[:2] == 1)
    assert list(driven) == [7 * 24, 8 * 24] and len(clamped) == 12
    assert list(pairs[:6, 1]) == [0, 0, 1, 1, 2, 2]
    pb, _, drb, _ = P.quads_focusing_constraints(g, 2, "bottom", -2, 2)
    assert list(drb) == [9, 10] and list(pb[:6, 1]) == [1, 1, 0, 0, 2, 2]
    with pytest.raises(ValueError):
        P.quads_focusing_constraints(g, 2, "diagonal")
    assert list(P.quads_target_blocks(g, (2, 2), (4, 3))) == [10 * 24 + 15, 11 * 24 + 15, 10 * 24 + 16, 11 * 24 + 16]


def test_kagome_bc_patterns():
    g = KagomeGeometry(20, 12, 20.0 * np.array([[1.0, 0.0], [0.5, math.sqrt(3) / 2]]), 2.25)
    pairs, vec, driven, clamped = P.kagome_focusing_constraints(g, 2, 2)
    assert len(np.unique(pairs[:, 0] * 3 + pairs[:, 1])) == len(pairs) == 6 + 3 * (3 + 4 + 3 + 4)
    assert list(driven) == [2 * 20 * 5, 2 * 20 * 6]


def test_kagome_forward_problem_runs(cpu_lib):
    # 6 x 6 cells: on fewer rows the two driven blocks are also corner-clamped blocks (the clamp wins, as in the reference's index
    # lists) and nothing moves
    fw = P.KagomeFocusingForward(n1_cells=6, n2_cells=6, cell_size=20.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19,
                                 k_rot=1.5, density=6.18e-9, damping=1e-4 * np.ones((72, 3)), amplitude=5.0, loading_rate=3000.0,
                                 input_delay=1e-5, n_excited_blocks=2, simulation_time=4e-4, n_timepoints=5, use_contact=True,
                                 k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180,
                                 steps_per_interval=10, _lib=cpu_lib)
    obj = P.TargetKineticEnergy(fw, (2, 2), (-1, 0))
    design = tuple(np.zeros(s) for s in fw.geometry.design_shapes())
    v, g = obj.value_and_grad(design)
    assert v > 1e-6 and all(np.isfinite(a).all() for a in g) and len(g) == 3 and max(np.abs(a).max() for a in g) > 1e-8
    assert abs(obj.value(design) - v) / v < 1e-12


def test_multi_input_objective_is_weighted_sum_and_gradient_matches_fd(cpu_lib):
    fws = [_quads(cpu_lib, "left", 0), _quads(cpu_lib, "bottom", -1)]
    mi = P.MultiInputTargetKineticEnergy(fws, (2, 2), (1, 1), weights=(1.0, 0.5))
    d = _design(fws[0])
    v, g = mi.value_and_grad(d)
    ind = mi.individual(d)
    assert abs(v - (ind[0] + 0.5 * ind[1])) / v < 1e-12 and np.all(ind > 0)
    rng = np.random.default_rng(1)
    dirn = tuple(rng.normal(size=a.shape) for a in d)
    eps = 1e-5
    vp = mi.value(tuple(a + eps * b for a, b in zip(d, dirn)))
    vm = mi.value(tuple(a - eps * b for a, b in zip(d, dirn)))
    fd = (vp - vm) / (2 * eps)
    an = sum((a * b).sum() for a, b in zip(g, dirn))
    assert abs(fd - an) / abs(fd) < 1e-6


def test_optimisation_loop_increases_objective_and_stays_feasible(cpu_lib):
    fw = _quads(cpu_lib)
    obj = P.TargetKineticEnergy(fw, (2, 2), (1, 1))
    opt = P.OptimizationProblem(obj)
    x0 = _design(fw, amp=0.05)
    x = opt.run_optimization(x0, 3, lower_bound=-3.0, upper_bound=3.0, min_void_angle=5 * math.pi / 180,
                             min_block_angle=5 * math.pi / 180, min_edge_length=1.0, verbose=False)
    assert opt.objective_values[-1] > opt.objective_values[0]
    assert all(b > a for a, b in zip(opt.objective_values, opt.objective_values[1:]))
    assert P.angle_constraints(fw.geometry, x, 5 * math.pi / 180, 5 * math.pi / 180).max() <= 1e-8
    assert P.edge_length_constraints(fw.geometry, x, 1.0).max() <= 1e-8
    d = opt.to_dict()
    assert len(d["design_values"]) == len(d["objective_values"])


def check_response_data(lib, batch=1):
    """problems/quads_focusing.py:319-372: per-bond strain energies and per-block kinetic energy histories.  The engine reduces them
    from its resident history (dfx_response_data); checked against the oracle's strains (torch restatement of energy.py:120-155,
    522-534), against the host NumPy formulas, and against the engine's own potential energy (no contact active here)."""
    import torch
    from oracle import ref_energy as OE, ref_geometry as OG
    fw = _quads(lib) if batch == 1 else None
    if batch > 1:
        fw = P.QuadsFocusingForward(
            n1_blocks=6, n2_blocks=6, spacing=15.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19, k_rot=1.5,
            density=6.18e-9, damping=1e-4 * np.ones((36, 3)), amplitude=7.5, loading_rate=3000.0, input_delay=1e-5,
            n_excited_blocks=2, loaded_side="left", input_shift=0, simulation_time=4e-4, n_timepoints=5,
            use_contact=True, k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180,
            steps_per_interval=10, batch=batch, _lib=lib)
        fw.setup()
    designs = [_design(fw, seed=s) for s in range(batch)]
    sols = fw.solve(designs if batch > 1 else designs[0])
    sols = sols if batch > 1 else [sols]
    T, nb = len(fw.timepoints), fw.geometry.n_blocks
    for m, sol in enumerate(sols):
        r = fw.compute_response_data(sol)                                  # device path: a solution of the last solve
        assert r["strain_energy_stretch"].shape == (T, len(fw.bond_connectivity)) and r["kinetic_energy"].shape == (T, nb)
        bonds = torch.as_tensor(np.asarray(fw.bond_connectivity, dtype=np.int64))
        cnv = torch.as_tensor(np.array(sol.centroid_node_vectors))
        refv = torch.as_tensor(fw.reference_bond_vectors)
        for k in range(T):
            nodes = OE.block_to_node_kinematics(torch.as_tensor(sol.fields[k, 0]), cnv).reshape(-1, 3)
            ax, sh, be = OE.ligament_strains(nodes[bonds[:, 0]], nodes[bonds[:, 1]], refv)
            for name, strain, stiff, scale in (("stretch", ax, fw.k_stretch, fw.bond_length), ("shear", sh, fw.k_shear, fw.bond_length),
                                               ("bending", be, fw.k_rot, 1.0)):
                want = 0.5 * stiff * (strain.numpy() * scale) ** 2
                assert np.abs(r["strain_energy_" + name][k] - want).max() <= 1e-12 * max(want.max(), 1e-300) + 1e-30
        inertia = OG.compute_inertia(cnv, 6.18e-9).numpy()
        assert np.abs(r["kinetic_energy"] - np.sum(0.5 * sol.fields[:, 1] ** 2 * inertia, axis=-1)).max() <= 1e-12 * r["kinetic_energy"].max()
        host = fw.compute_response_data(sol._replace(timepoints=sol.timepoints.copy()))     # another object: host NumPy path
        for key in ("strain_energy_stretch", "strain_energy_shear", "strain_energy_bending", "kinetic_energy"):
            assert np.abs(host[key] - r[key]).max() <= 1e-11 * max(np.abs(r[key]).max(), 1e-300)
    r0 = fw.compute_response_data()                                         # the reference's call without arguments
    assert np.array_equal(r0["kinetic_energy"], fw.compute_response_data(sols[0])["kinetic_energy"])
    if batch == 1:
        cp = fw.control_params(designs[0])
        flat = fw.solve_dynamics._flatten(cp)
        fw.solve_dynamics.engine.set_params(**{k: v[None] for k, v in flat.items()})
        e = fw.solve_dynamics.engine.energy(sols[0].fields[-1, 0][None])[0]
        tot = (r0["strain_energy_stretch"] + r0["strain_energy_shear"] + r0["strain_energy_bending"])[-1].sum()
        assert abs(e - tot) / tot < 1e-10


@pytest.mark.parametrize("batch", [1, 3])
def test_response_data_energies(cpu_lib, batch):
    check_response_data(cpu_lib, batch)


def test_mma_reproduces_the_nlopt_tutorial_optimum():
    """The worked example of NLopt's documentation for LD_MMA: min sqrt(x2) s.t. x2 >= (2 x1)^3, x2 >= (1 - x1)^3;
    optimum x = (1/3, 8/27), f = 0.5443310..."""
    from difflexmm_amd.optimize import mma_minimize

    def f(x):
        return np.sqrt(x[1]), np.array([0.0, 0.5 / np.sqrt(x[1])])

    def c(x):
        return np.array([(2 * x[0]) ** 3 - x[1], (1 - x[0]) ** 3 - x[1]])

    def jc(x):
        return np.array([[6 * (2 * x[0]) ** 2, -1.0], [-3 * (1 - x[0]) ** 2, -1.0]])

    r = mma_minimize(f, [1.234, 5.678], lower=[-np.inf, 1e-12], constraints=[(c, jc)], maxeval=100, xtol_rel=1e-8,
                     constraint_tol=1e-8)      # the tutorial passes tol = 1e-8 to add_inequality_constraint
    assert abs(r.fun - 0.5443310539518174) < 1e-7 and np.allclose(r.x, [1 / 3, 8 / 27], atol=1e-6)
    assert r.n_eval < 30 and r.feasible


def test_mma_second_problem_with_bounds_and_two_constraints():
    """A second problem with a known optimum (KKT point by hand): min (x0-2)^2 + (x1-1)^2 + x2^2 subject to
    x0 + x1 <= 2, x0^2 - x1 <= 0, 0 <= x <= 3.  The optimum is x = (1, 1, 0), f = 1 (both constraints active)."""
    from difflexmm_amd.optimize import mma_minimize

    def f(x):
        return (x[0] - 2) ** 2 + (x[1] - 1) ** 2 + x[2] ** 2, np.array([2 * (x[0] - 2), 2 * (x[1] - 1), 2 * x[2]])

    cons = [(lambda x: np.array([x[0] + x[1] - 2.0]), lambda x: np.array([[1.0, 1.0, 0.0]])),
            (lambda x: np.array([x[0] ** 2 - x[1]]), lambda x: np.array([[2 * x[0], -1.0, 0.0]]))]
    r = mma_minimize(f, [0.5, 1.0, 1.7], lower=0.0, upper=3.0, constraints=cons, maxeval=200, xtol_rel=1e-10,
                     constraint_tol=1e-9)     # feasible start, as NLopt's MMA (no artificial variables) expects
    assert r.feasible and abs(r.fun - 1.0) < 1e-6 and np.allclose(r.x, [1.0, 1.0, 0.0], atol=1e-4)


def test_mma_reaches_svanbergs_cantilever_optimum():
    """The test problem of the paper that introduced MMA (K. Svanberg, Int. J. Numer. Meth. Engng 24 (1987), sec. 6): weight of a
    five-segment cantilever  0.0624 (x1 + ... + x5)  under the tip-deflection bound  61/x1^3 + 37/x2^3 + 19/x3^3 + 7/x4^3 + 1/x5^3 <= 1,
    start x = 5 (feasible).  Published optimum: x = (6.016, 5.309, 4.494, 3.502, 2.153), weight 1.340."""
    from difflexmm_amd.optimize import mma_minimize
    a = np.array([61.0, 37.0, 19.0, 7.0, 1.0])
    r = mma_minimize(lambda x: (0.0624 * x.sum(), np.full(5, 0.0624)), np.full(5, 5.0), lower=1e-3, upper=10.0,
                     constraints=[(lambda x: np.array([(a / x ** 3).sum() - 1.0]), lambda x: (-3 * a / x ** 4)[None])],
                     maxeval=200, xtol_rel=1e-10, constraint_tol=1e-9)
    assert r.feasible and abs(r.fun - 1.340) < 5e-4 and np.allclose(r.x, [6.016, 5.309, 4.494, 3.502, 2.153], atol=2e-3)


def test_mma_one_rho_update_makes_the_approximation_conservative():
    """nlopt/mma.c: g(x + d) = f + sum (f' s^2 d + (|f'| s + rho/2) d^2) / (s^2 - d^2) and w = sum d^2 / (s^2 - d^2) / 2, so
    raising rho by (f_new - g) / w closes the gap exactly -- for sigma != 1 too (a stray sigma^2 on the rho term
    broke this).  Checked on the approximation formulas the module uses, through a non-conservative first candidate."""
    from difflexmm_amd import optimize as O
    evals = []

    def f(x):
        evals.append(x.copy())
        return float(np.sum(x ** 4)), 4 * x ** 3

    gen = O.mma_steps(np.array([2.0, -1.5]), lower=-8.0, upper=8.0, maxeval=50)     # sigma = 8: far from 1
    x = next(gen)
    vals = []
    try:
        while True:
            v, g = f(x)
            vals.append(v)
            x = gen.send((v, g))
    except StopIteration as stop:
        res = stop.value
    assert res.fun < 1e-6 * vals[0] and res.n_eval <= 50
    assert min(vals) == pytest.approx(res.fun)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_constraint_jacobians_match_finite_differences(lattice):
    if lattice == "quads":
        g = QuadGeometry(4, 3, 15.0, 2.25)
        base = g.get_design_from_rotated_square(25 * math.pi / 180)
        design = tuple(b + np.random.default_rng(0).uniform(-0.3, 0.3, b.shape) for b in base)
    else:
        g = KagomeGeometry(3, 2, bond_length=0.1)
        design = tuple(np.random.default_rng(0).uniform(-0.02, 0.02, sh) for sh in g.design_shapes())
    x = P._flatten_design(design)
    for f, J in ((lambda d: P.angle_constraints(g, d, 0.1, 0.2), P.angle_constraints_jac(g, design)),
                 (lambda d: P.edge_length_constraints(g, d, 0.5), P.edge_length_constraints_jac(g, design))):
        fd = np.zeros(J.shape)
        for j in range(len(x)):
            e = np.zeros(len(x)); e[j] = 1e-6
            fd[:, j] = (f(P._unflatten_design(g, x + e)) - f(P._unflatten_design(g, x - e))) / 2e-6
        assert np.abs(J.toarray() - fd).max() < 1e-7 * max(1.0, np.abs(fd).max())


def test_mma_loop_with_reference_signature(cpu_lib):
    """run_optimization_nlopt(initial_guess, n_iterations, ..., min_void_angle, min_block_angle, min_edge_length):
    the objective grows, the returned design is feasible, and the bookkeeping lists have one entry per evaluation."""
    fw = _quads(cpu_lib)
    obj = P.TargetKineticEnergy(fw, (2, 2), (1, 1))
    opt = P.OptimizationProblem(obj)
    x0 = _design(fw, amp=0.05)
    amin = 5 * math.pi / 180
    x = opt.run_optimization_nlopt(x0, 8, lower_bound=-3.0, upper_bound=3.0, min_void_angle=amin, min_block_angle=amin,
                                   min_edge_length=1.0, verbose=False)
    assert len(opt.objective_values) == len(opt.design_values) == 8
    assert opt.mma_result.fun > opt.objective_values[0] and opt.mma_result.feasible
    assert P.angle_constraints(fw.geometry, x, amin, amin).max() <= 2e-8
    assert P.edge_length_constraints(fw.geometry, x, 1.0).max() <= 2e-8
    assert max(np.abs(a).max() for a in x) <= 3.0


def test_angular_momentum_objective_gradient_matches_fd(cpu_lib):
    """quads_spin objective through the generic cotangent path (host objective -> solve_dynamics.vjp -> geometry.vjp)."""
    fw = _quads(cpu_lib)
    x0 = _design(fw, amp=0.05)
    obj = P.TargetAngularMomentum(fw, (2, 2), (1, 1), spin_center="center", reference_design=x0)
    v, g = obj.value_and_grad(x0)
    rng = np.random.default_rng(3)
    d = tuple(rng.normal(size=a.shape) for a in x0)
    eps = 1e-6
    vp = obj.value(tuple(a + eps * b for a, b in zip(x0, d)))
    vm = obj.value(tuple(a - eps * b for a, b in zip(x0, d)))
    fd = (vp - vm) / (2 * eps)
    an = sum((a * b).sum() for a, b in zip(g, d))
    assert abs(v) > 0 and abs(an - fd) < 2e-5 * abs(fd), (an, fd)


def test_ensemble_optimisation_in_lock_step_equals_members_alone(cpu_lib):
    """BASELINE config 5 in small: an ensemble of multi-input focusing designs optimised side by side (one batched
    forward + reverse sweep per round) goes through exactly the iterates each member would visit alone."""
    amin = 5 * math.pi / 180
    kw = dict(lower_bound=-3.0, upper_bound=3.0, min_void_angle=amin, min_block_angle=amin, min_edge_length=1.0)

    def objective(batch):
        fws = []
        for side, shift in (("left", 0), ("bottom", -1)):
            fw = P.QuadsFocusingForward(
                n1_blocks=5, n2_blocks=5, spacing=15.0, bond_length=2.25, k_stretch=120.0, k_shear=1.19, k_rot=1.5,
                density=6.18e-9, damping=1e-4 * np.ones((25, 3)), amplitude=7.5, loading_rate=3000.0, input_delay=1e-5,
                n_excited_blocks=1, loaded_side=side, input_shift=shift, simulation_time=3e-4, n_timepoints=4,
                use_contact=True, k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180,
                steps_per_interval=8, batch=batch, _lib=cpu_lib)
            fw.setup()
            fws.append(fw)
        return P.MultiInputTargetKineticEnergy(fws, (1, 1), (1, 1), weights=[1.0, 0.5]), fws[0]

    obj3, fw = objective(3)
    x0s = [_design(fw, seed=s, amp=0.05) for s in (0, 1, 2)]
    best, logs = P.run_ensemble_optimization(obj3, x0s, 5, **kw)
    assert all(len(l["objective_values"]) == 5 for l in logs)
    obj1, _ = objective(1)
    for m in (0, 2):
        opt = P.OptimizationProblem(obj1)
        x = opt.run_optimization_nlopt(x0s[m], 5, verbose=False, **kw)
        assert np.allclose(opt.objective_values, logs[m]["objective_values"], rtol=1e-9)
        assert all(np.allclose(a, b, rtol=0, atol=1e-10) for a, b in zip(x, best[m]))
    assert all(l["mma"].fun >= l["objective_values"][0] for l in logs)
    # the members' host work (constraints, MMA sub-problems) in two worker processes: same iterates, same histories
    from difflexmm_amd.optimize import MemberWorkers
    with MemberWorkers(2) as workers:
        best_w, logs_w = P.run_ensemble_optimization(obj3, x0s, 5, workers=workers, **kw)
    # pipelined: the two halves of a 4-member ensemble take turns on the engine (batch 2), the workers run one half's MMA steps
    # while the other half is integrated -- the same iterates as the members alone
    obj2, _ = objective(2)
    x0s4 = x0s + [_design(fw, seed=7, amp=0.05)]
    with MemberWorkers(2) as workers:
        best_p, logs_p = P.run_ensemble_optimization(obj2, x0s4, 5, workers=workers, pipeline=True, **kw)
    for m in range(3):
        assert logs_p[m]["objective_values"] == logs[m]["objective_values"]
        assert all(np.array_equal(a, b) for a, b in zip(best_p[m], best[m]))
    assert len(logs_p[3]["objective_values"]) == 5
    with pytest.raises(ValueError, match="batch=2"):
        P.run_ensemble_optimization(obj3, x0s4, 5, workers=None, pipeline=True, **kw)
    for m in range(3):
        assert logs_w[m]["objective_values"] == logs[m]["objective_values"]
        assert logs_w[m]["constraints_violation"] == logs[m]["constraints_violation"] and logs[m]["constraints_violation"]["angles"]
        assert all(np.array_equal(a, b) for a, b in zip(best_w[m], best[m])) and logs_w[m]["mma"].n_eval == logs[m]["mma"].n_eval


def test_member_workers_report_a_failing_member():
    from difflexmm_amd.optimize import MemberWorkers, drive_ensemble
    with MemberWorkers(2) as workers:
        with pytest.raises(RuntimeError, match="ensemble worker"):
            drive_ensemble(lambda xs: [(0.0, np.zeros(1))] * len(xs), [(_failing_member, (), {}), (_failing_member, (), {})], workers)


def _failing_member():
    yield np.zeros(1)
    raise ValueError("boom")


def _big_member(n, rounds, seed):
    """Asks for `rounds` evaluations at points of n doubles (n = 70 000: 560 KB per message, beyond any pipe buffer)."""
    x = np.full(n, float(seed))
    total = 0.0
    for _ in range(rounds):
        value, grad = yield x
        total += value
        x = x + grad
    return total, x[:3].copy()


@pytest.mark.timeout(120)
def test_pipelined_ensemble_survives_messages_larger_than_a_pipe_buffer():
    """round-3 advice: with groups=2 the caller posted one half's (value, gradient) to a worker that was still blocked sending the
    other half's reply -- both sides stuck in Connection.send once a message outgrew the socket buffer (~208 KB; one 128 x 128 design
    is 528 KB).  Four members of 560 KB each on two workers that own members of BOTH halves, against the same run without workers."""
    from difflexmm_amd.optimize import MemberWorkers, drive_ensemble
    n, rounds = 70_000, 4
    specs = [(_big_member, (n, rounds, k), {}) for k in range(4)]

    def batch_fun(xs, ids=None):
        return [(float(x[0]), np.ones_like(x)) for x in xs]
    ref = drive_ensemble(batch_fun, specs)
    with MemberWorkers(2) as workers:
        out = drive_ensemble(batch_fun, specs, workers, groups=2)
    with MemberWorkers(1) as workers:
        out1 = drive_ensemble(batch_fun, specs, workers, groups=2)
    for a, b, c in zip(ref, out, out1):
        assert a[0] == b[0] == c[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])


def test_bench_host_path_on_cpu_port(cpu_lib):
    """bench.py's workload builder and its prepare / execute split (the timed region) through the CPU port on a small
    lattice: same code path as on the GPU box up to the library behind the C ABI."""
    import bench
    fw, obj, designs = bench.c3_problem(8, 3, 2, lib=cpu_lib)
    assert len(designs) == 2 and fw.solve_dynamics.engine.batch == 2
    bench.prepare(fw, designs, 4, spi=2)
    res = bench.execute(fw, obj, spi=2)
    # the pulse starts at t = 0 and the target sits next to the driven blocks: already a few steps give a non-zero objective and
    # a non-zero gradient (round-1 verdict: the timed job must not differentiate a zero)
    assert res["objective"].shape == (2,) and np.all(res["objective"] > 0) and bench.grad_norm(res) > 0
    assert set(obj.target_blocks) == {3 * 8 + 1, 3 * 8 + 2, 4 * 8 + 1, 4 * 8 + 2} and list(fw.driven_blocks_ids) == [3 * 8, 4 * 8]
    assert res["fwd_launches"] == 0 and res["streams"] >= 1                          # the CPU port launches no kernels
    line = bench.cpu_baseline(8, 3, n_steps=20, repeats=3)
    assert line["kind"] == "port" and line["value"] > 0 and line["cores"] >= 1 and line["one_thread"] > 0
    t = bench.load_pmc_traffic()
    # counters of another engine build are not reported: the file carries a hash of the sources it was collected for
    assert t is None or t["source"].startswith("STALE") or t["k_adj_stage_bytes_per_member_launch"] > bench.BYTES_ADJ_STAGE * 128 * 128 * 0.9
    assert t is None or t["source"].startswith("STALE") or t["csrc_sha256"] == bench.csrc_digest()
    assert "build" in line and "march" in line["build"]


def test_bench_gpus_flag_starts_its_own_ranks(tmp_path):
    """`bench.py --gpus 2` without a launcher starts 2 rank processes itself (before any GPU call) and gives each the
    environment the ranks read; with a launcher whose WORLD_SIZE disagrees it refuses.  (No GPU here: the ranks are replaced by a
    stub that reports its environment.)"""
    import subprocess, sys, textwrap, bench, os
    stub = tmp_path / "stub.py"
    stub.write_text(textwrap.dedent("""
        import os, sys
        open(os.path.join(os.path.dirname(__file__), "rank%s.txt" % os.environ["RANK"]), "w").write(
            " ".join(os.environ[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "DFX_UID_FILE")) + " " + " ".join(sys.argv[1:]))
        sys.exit(3 if os.environ["RANK"] == "1" else 0)
    """))
    real = bench.__file__
    try:
        bench.__file__ = str(stub)                       # launch_ranks starts `python <this file> argv`
        import types
        launch = types.FunctionType(bench.launch_ranks.__code__, dict(bench.__dict__, __file__=str(stub)))
        rc = launch(2, ["--gpus", "2", "--steps", "20"])
    finally:
        bench.__file__ = real
    assert rc == 3                                       # the worst exit code is propagated
    r0, r1 = (tmp_path / "rank0.txt").read_text().split(), (tmp_path / "rank1.txt").read_text().split()
    assert r0[:4] == ["0", "0", "2", "127.0.0.1"] and r1[:4] == ["1", "1", "2", "127.0.0.1"] and r0[4] == r1[4]
    assert r0[5:] == ["--gpus", "2", "--steps", "20"]
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, real, "--gpus", "2", "--steps", "1"], env=env, capture_output=True, text=True)
    assert p.returncode != 0 and "WORLD_SIZE=4" in p.stderr


def test_bench_times_exactly_k_steps():
    import bench
    for k in (1, 20, 250, 251, 777, 5000):
        ts, counts = bench.step_grid(k)
        total = int(np.sum(np.broadcast_to(counts, (len(ts) - 1,))))
        assert total == k and abs(ts[-1] - k * bench.DT) < 1e-18 and np.all(np.diff(ts) > 0)


def test_bench_dump_outputs_is_repeatable_and_bounded(tmp_path):
    """`bench.py --dump-outputs DIR`: one float64 .npy per array; an array of more than DUMP_MAX_VALUES values comes out as the same
    seeded sample of its entries in every run, so that two builds can be compared file by file."""
    import bench
    rng = np.random.default_rng(0)
    small, big = rng.standard_normal((4, 3)), rng.standard_normal(bench.DUMP_MAX_VALUES + 1000)
    for d in ("a", "b"):
        n = bench.dump_outputs(str(tmp_path / d), {"objective": small.astype(np.float32), "grad_x": big})
        assert n <= 64e6
    for name in ("objective", "grad_x"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "objective.npy"), small.astype(np.float32).astype(np.float64))
    s = np.load(tmp_path / "a" / "grad_x.npy")
    assert s.shape == (bench.DUMP_MAX_VALUES,) and np.isin(s, big).all() and len(np.unique(s)) == s.size


def test_geometry_cache_tells_kagome_lattices_with_different_bases_apart():
    """the per-design geometry cache keyed kagome lattices by their scalar attributes only; two lattices that
    differ in direct_basis (cell_size / cell_angle) must not share centroids and node vectors for one design object."""
    ga = KagomeGeometry(3, 2, 20.0 * np.array([[1.0, 0.0], [0.5, math.sqrt(3) / 2]]), 2.25)
    gb = KagomeGeometry(3, 2, 26.0 * np.array([[1.0, 0.0], [0.5, math.sqrt(3) / 2]]), 2.25)
    design = tuple(np.random.default_rng(0).uniform(-0.3, 0.3, sh) for sh in ga.design_shapes())
    ca, na = P.geometry_from_design_cached(ga, design)
    cb, nb = P.geometry_from_design_cached(gb, design)
    ea, ena = ga.geometry_from_design(*design)
    eb, enb = gb.geometry_from_design(*design)
    assert np.array_equal(ca, ea) and np.array_equal(na, ena)
    assert np.array_equal(cb, eb) and np.array_equal(nb, enb)
    assert not np.array_equal(ca, cb)


def test_optimization_problem_round_trips_through_a_dict_and_resumes(cpu_lib, tmp_path):
    """problems/quads_focusing.py:677-690: to_dict -> save_data -> load_data -> from_dict gives back the problem with its histories;
    the loop then continues from the last design and appends to them."""
    from difflexmm_amd.utils import load_data, save_data
    fw = _quads(cpu_lib)
    opt = P.OptimizationProblem(P.TargetKineticEnergy(fw, (2, 2), (1, 1)))
    x0 = _design(fw, amp=0.05)
    amin = 5 * math.pi / 180
    kw = dict(lower_bound=-3.0, upper_bound=3.0, min_void_angle=amin, min_block_angle=amin, min_edge_length=1.0, verbose=False)
    opt.run_optimization_nlopt(x0, 3, **kw)
    fw.solve(opt.design_values[-1])
    d = opt.to_dict()
    assert d["forward_problem"]["n1_blocks"] == 6 and d["target_size"] == (2, 2) and isinstance(d["forward_problem"]["solution_data"], dict)
    save_data(tmp_path / "opt.pkl", d)
    back = P.OptimizationProblem.from_dict(load_data(tmp_path / "opt.pkl"), _lib=cpu_lib)
    assert back.objective_values == opt.objective_values and len(back.design_values) == 3
    assert np.array_equal(back.objective.target_blocks, opt.objective.target_blocks)
    assert np.array_equal(back.objective.forward.solution_data.fields, fw.solution_data.fields)
    v, _ = back.objective.value_and_grad(back.design_values[-1])
    assert abs(v - opt.objective_values[-1]) <= 1e-12 * abs(v)          # same problem, same design, same objective
    back.run_optimization_nlopt(back.design_values[-1], 2, **kw)
    assert len(back.objective_values) == 5 and len(back.design_values) == 5
    mi = P.MultiInputTargetKineticEnergy([_quads(cpu_lib, "left", 0), _quads(cpu_lib, "bottom", -1)], (2, 2), (1, 1), weights=(1.0, 0.5))
    md = P.OptimizationProblem(mi).to_dict()
    mb = P.OptimizationProblem.from_dict(md, _lib=cpu_lib)
    assert [o.forward.loaded_side for o in mb.objective.objectives] == ["left", "bottom"] and list(mb.objective.weights) == [1.0, 0.5]


@pytest.mark.parametrize("n", [3, 4, 5])
def test_closed_form_polygon_cotangents_match_the_complex_step_jacobians(n):
    """geometry.polygon_props_vjp (closed form, used by the design loop) against polygon_props_jac (complex step through
    polygon_props itself), for counter-clockwise polygons (the lattices) and clockwise ones (where polygon_props, like the reference,
    divides by |S| and the reference point is not the centroid)."""
    from difflexmm_amd import geometry as G
    rng = np.random.default_rng(n)
    th = np.sort(rng.uniform(0, 2 * np.pi, (40, n)), axis=1)
    r = rng.uniform(0.5, 1.5, (40, n))
    v = np.stack([r * np.cos(th) + rng.normal(size=(40, 1)), r * np.sin(th) + rng.normal(size=(40, 1))], -1)
    for vv in (v, v[:, ::-1].copy()):
        dA, dC, dI = G.polygon_props_jac(vv)
        ab, cb, ib = rng.normal(size=40), rng.normal(size=(40, 2)), rng.normal(size=40)
        ref = ab[:, None, None] * dA + np.einsum("bc,bcnk->bnk", cb, dC) + ib[:, None, None] * dI
        got = G.polygon_props_vjp(vv, ab, cb, ib)
        assert (np.abs(got - ref).reshape(40, -1).max(1) / np.abs(ref).reshape(40, -1).max(1)).max() < 1e-11
        assert np.allclose(G.polygon_props_vjp(vv, area_bar=ab), ab[:, None, None] * dA, rtol=0, atol=1e-13)


def test_to_data_and_from_data_round_trip(cpu_lib):
    """problems/quads_focusing.py:372-379, 664-672: the object-level twins of to_dict / from_dict (what the notebooks pickle)."""
    from . import callers_common as C
    fw, _, x = C.quads_forward(cpu_lib)
    sol = fw.solve(x)
    copy = fw.to_data()
    assert copy.is_setup is False and copy.n1_blocks == fw.n1_blocks and np.array_equal(copy.solution_data.fields, sol.fields)
    again = P.QuadsFocusingForward.from_data(fw, _lib=cpu_lib)
    again.setup()
    assert np.array_equal(again.solve(x).fields, sol.fields)
    opt = P.OptimizationProblem(P.TargetKineticEnergy(fw, (2, 2), (1, 0)))
    opt.run_optimization_nlopt(x, 1, verbose=False)
    assert P.OptimizationProblem.from_data(opt, _lib=cpu_lib).objective_values == opt.objective_values
    assert len(opt.to_data().design_values) == 1


def test_grid_refine_brings_the_frozen_grid_gradient_closer_to_exact(cpu_lib, monkeypatch):
    """`grid_refine = k` (setup_dynamic_solver / the forward problems): every step of the grid frozen from the adaptive controller is
    split into k before the reverse sweep differentiates it.  At the paper's loose tolerances (atol = 1e-4) the default grid's gradient is
    further from the exact one than the reference's continuous adjoint; k = 2 brings it closer at twice the steps
    (python -m tests.adjoint_semantics: 6.9e-3 -> 2.2e-5 on the paper lattice).  Here: 10 x 6 quads, exact = rtol = atol = 1e-11."""
    from tests.adjoint_semantics import paper_problem, relerr as rel
    monkeypatch.setenv("DFX_ADAPTIVE_RECORDS", "0")        # the frozen grid at k = 1 too (the default keeps the adaptive pass's own records)
    res = {}
    for key, (rtol, atol, k) in {"loose": (1e-8, 1e-4, 1), "refined": (1e-8, 1e-4, 2), "exact": (1e-11, 1e-11, 1)}.items():
        fw = paper_problem(10, 6, 6, rtol, atol, cpu_lib, grid_refine=k)
        if not res:
            rng = np.random.default_rng(7)
            design = tuple(b + rng.uniform(-0.3, 0.3, b.shape) for b in fw.geometry.get_design_from_rotated_square(25 * math.pi / 180))
        obj = P.TargetKineticEnergy(fw, (2, 2), (2, 1))
        v, g = obj.value_and_grad(design)
        res[key] = (v, g, int(np.sum(fw.solve_dynamics.stats["steps_per_interval"])))
        fw.solve_dynamics.engine.close()
    assert res["refined"][2] == 2 * res["loose"][2]
    e1, e2 = rel(res["loose"][1], res["exact"][1]), rel(res["refined"][1], res["exact"][1])
    assert res["exact"][0] > 0 and e2 < 0.2 * e1 and e1 > 1e-5, (e1, e2)
    with pytest.raises(ValueError):
        paper_problem(10, 6, 6, 1e-8, 1e-4, cpu_lib, grid_refine=0)
