"""Parity checks shared by the CPU-port suite (no GPU) and the HIP suite (-m gpu): the engine under test
against the torch-autograd / NumPy oracle on identical seeded inputs.  Tolerances are for fp64."""
import numpy as np
import torch

from difflexmm_amd import geometry as geo
from oracle import ref_dynamics as OD

from .common import Case, relerr

RTOL_RHS = 1e-12       # one RHS evaluation / one VJP
RTOL_TRAJ = 1e-10      # short fixed-step trajectories (same tableau, same grid)
RTOL_GRAD = 1e-9       # discrete-adjoint gradients vs autograd through the unrolled oracle


def T64(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=grad)


def check_rhs_and_vjp(lib, lattice, n, nonlinear, contact, seed=3, per_bond_k=True, scale_th=0.15, rtol=None, cutoff_deg=None,
                      extra_bonds=None, scramble=None):
    cut = cutoff_deg if cutoff_deg is not None else (125.0 if lattice == "kagome" else 42.0)
    c = Case(lattice, n, nonlinear, contact, seed=seed, lib=lib, cutoff_deg=cut, per_bond_k=per_bond_k, extra_bonds=extra_bonds,
             scramble=scramble)
    s = c.solver
    flat = s._flatten(c.cp)
    s.engine.set_params(**{k: v[None] for k, v in flat.items()})
    y = c.random_state(scale_th=scale_th)
    lam = c.rng.normal(size=y.shape)
    t = 0.012
    dy = s.engine.rhs(y[None], t)[0]
    yb, g = s.engine.rhs_vjp(y[None], t, lam[None])
    names = ["cnv", "refv", "ks", "ksh", "kr", "damping", "amplitude", "loading_rate", "input_delay"]
    src = dict(cnv=c.cnv, refv=c.refv, ks=c.ks, ksh=c.ksh, kr=c.kr, damping=c.dval, amplitude=7.5, loading_rate=30.0,
               input_delay=0.1 / 30, min_angle=c.contact_params[0], cutoff_angle=c.contact_params[1],
               k_contact=c.contact_params[2])
    if contact:
        names += ["min_angle", "cutoff_angle", "k_contact"]
    leaves = {k: T64(src[k], True) for k in names}
    inertia = T64(flat["inertia"], True)
    leaves["inertia"] = inertia
    osol = c.oracle_solver()
    free = osol.free_DOF_ids
    yf = T64(y.reshape(2, -1)[:, free], True)
    r = osol.rhs(yf, t, c.oracle_cp(leaves), inertia.reshape(-1)[torch.as_tensor(free)], create_graph=True)
    L = (r * T64(lam.reshape(2, -1)[:, free])).sum()
    gr = torch.autograd.grad(L, [yf] + [leaves[k] for k in names] + [inertia], allow_unused=True)
    og = dict(zip(names + ["inertia"], gr[1:]))
    errs = {"rhs": relerr(dy.reshape(2, -1)[:, free], r.detach().numpy()),
            "y_bar": relerr(yb[0].reshape(2, -1)[:, free], gr[0].numpy())}
    cnv_bar = g["centroid_node_vectors"][0]
    if contact:
        cnv_bar = cnv_bar + geo.void_angles0_vjp(c.cnv, c.bonds, g["void_angle0"][0])
    errs["cnv"] = relerr(cnv_bar, og["cnv"].numpy())
    errs["refv"] = relerr(g["reference_vector"][0], og["refv"].numpy())
    errs["k"] = relerr(g["k_bond"][0], np.stack([og["ks"].numpy(), og["ksh"].numpy(), og["kr"].numpy()], 1))
    errs["inertia"] = relerr(g["inertia"][0], og["inertia"].numpy())
    errs["damping"] = relerr(g["damping"][0], og["damping"].numpy())
    errs["pulse"] = relerr(g["fn_params"][0][0][:3], np.array([og[k].item() for k in ("amplitude", "loading_rate", "input_delay")]))
    if contact:
        ref = np.array([og[k].item() for k in ("min_angle", "cutoff_angle", "k_contact")])
        assert np.abs(ref).max() > 0, "contact inactive: the test would be vacuous"
        errs["contact"] = relerr(g["contact"][0], ref)
    # constrained DOFs report zero rate / cotangent
    con = osol.constrained_DOF_ids
    assert np.all(dy.reshape(2, -1)[:, con] == 0.0) and np.all(yb[0].reshape(2, -1)[:, con] == 0.0)
    for k, v in errs.items():
        assert v < (rtol or RTOL_RHS), (lattice, nonlinear, contact, k, v)
    return errs


def check_trajectory_and_adjoint(lib, lattice, n, integrator, nonlinear=True, contact=True, seed=5, spi=6, n_out=5, batch=1,
                                 own_step_times=False, extra_bonds=None, scramble=None):
    cut = (125.0 if lattice == "kagome" else 42.0)
    c = Case(lattice, n, nonlinear, contact, seed=seed, lib=lib, cutoff_deg=cut, integrator=integrator, extra_bonds=extra_bonds,
             scramble=scramble)
    fast = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)   # a full pulse inside the short window
    c.cp = c.cp._replace(constraint_params=fast)
    ts = np.linspace(0, 3e-4, n_out)
    s = c.solver
    y0 = c.random_state(0.05, 0.02, 5.0)
    step_times = None
    if own_step_times:      # unequal steps inside every interval
        counts = np.broadcast_to(spi, (n_out - 1,))
        step_times = np.concatenate([a + (b - a) * np.linspace(0, 1, int(k) + 1)[:-1] ** 1.7 for a, b, k in zip(ts[:-1], ts[1:], counts)]
                                    + [ts[-1:]])
    fields = s(y0, ts, c.cp, keep_trajectory=True, steps_per_interval=spi, step_times=step_times)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau=integrator, step_times=step_times)
    lv = dict(loading_rate=T64(3000.0), input_delay=T64(1e-5))
    of = osol(y0, ts, c.oracle_cp(lv)).numpy()
    e_fwd = relerr(fields, of)
    assert e_fwd < RTOL_TRAJ, ("forward", lattice, integrator, e_fwd)
    assert s.stats["steps"] == int(np.sum(np.broadcast_to(spi, (n_out - 1,))))
    fb = c.rng.normal(size=fields.shape)
    # the oracle's differentiable history holds the free DOFs only: keep the cotangent off the prescribed DOFs here
    # (their direct contribution is covered by test_cotangents_on_prescribed_dof_outputs_reach_constraint_params)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    tree, s0 = s.vjp(fb)
    design = [T64(d, True) for d in c.design]
    cnv = c.ogeo.centroid_node_vectors(*design)
    cen = c.ogeo.block_centroids(*design)
    amp, y0t = T64(7.5, True), T64(y0, True)
    free = osol.free_DOF_ids
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(dict(cnv=cnv, cen=cen, amplitude=amp, **lv)),
                                            spi, integrator, step_times=step_times)
    L = (hist * T64(fb.reshape(len(ts), 2, -1)[:, :, free])).sum()
    gr = torch.autograd.grad(L, design + [amp, y0t])
    mine = c.geo.vjp(c.design, tree.geometrical_params.centroid_node_vectors, tree.geometrical_params.block_centroids)
    errs = {"fwd": e_fwd}
    for i, (a, b) in enumerate(zip(mine, gr)):
        errs[f"design{i}"] = relerr(a, b.numpy())
    errs["amplitude"] = abs(tree.constraint_params["amplitude"] - gr[len(design)].item()) / abs(gr[len(design)].item())
    errs["state0"] = relerr(s0.reshape(2, -1)[:, free], gr[-1].numpy().reshape(2, -1)[:, free])
    for k, v in errs.items():
        assert v < RTOL_GRAD, (lattice, integrator, k, v)
    return errs


def check_adaptive_records_adjoint(lib, lattice="quads", n=4, nonlinear=True, contact=True, seed=9, n_out=61, rtol=1e-5, atol=1e-5, horizon=3e-4,
                                   batch=1):
    """The reference's default call made differentiable as it stands (``dfx_forward_adaptive_keep``): adaptive Dormand-Prince with jax's
    controller, outputs interpolated inside the steps, and the reverse sweep = the exact discrete adjoint of THAT solve, output cotangents
    entering through the quartic dense output.  Checked against the oracle's ``odeint`` restatement (forward, accepted step boundaries)
    and against ``torch.autograd`` through the oracle's replay of the same accepted steps with jax's dense-output formulas
    (``solve_adaptive_replay_differentiable``).  The tolerances are chosen so that steps hold none, one and several outputs."""
    cut = (125.0 if lattice == "kagome" else 42.0)
    c = Case(lattice, n, nonlinear, contact, seed=seed, lib=lib, cutoff_deg=cut, batch=batch)
    fast = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
    c.cp = c.cp._replace(constraint_params=fast)
    ts = np.linspace(0, horizon, n_out)
    s = c.solver
    s.rtol, s.atol = rtol, atol
    y0 = c.random_state(0.05, 0.02, 5.0)
    out = s(y0, ts, [c.cp] * batch if batch > 1 else c.cp, keep_trajectory=True)
    assert s.stats["step_control"] == "adaptive-records", s.stats["step_control"]
    fields = out[0] if batch > 1 else out
    osol = c.oracle_solver(integrator="adaptive", rtol=rtol, atol=atol)
    lv = dict(loading_rate=T64(3000.0), input_delay=T64(1e-5))
    of = osol(y0, ts, c.oracle_cp(lv)).numpy()
    st = osol.stats["step_times"]
    e_fwd = relerr(fields, of)
    assert e_fwd < 1e-8, ("adaptive forward", e_fwd)       # (two controllers: rounding in the error estimate moves the step sizes by ~1e-8)
    mine_t = s.engine.adaptive_step_times(0)
    # (the controller amplifies rounding: the error estimate is a difference of nearly equal numbers, so two correct implementations
    # agree on the step boundaries to ~1e-8, not to 1e-15; the decisions -- how many steps, which attempts fail -- are the same)
    assert len(mine_t) == len(st) - 1 and relerr(mine_t, st[1:]) < 1e-6, (len(mine_t), len(st) - 1)
    st = np.concatenate([ts[:1], mine_t])                  # the replay below freezes the steps the ENGINE took
    per_step = np.histogram(ts[1:], bins=st)[0]
    assert per_step.max() >= 2 and (per_step == 0).any() and (per_step == 1).any(), per_step      # the three kinds of step
    fb = c.rng.normal(size=fields.shape)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    trees, s0s = s.vjp(np.stack([fb] * batch) if batch > 1 else fb)
    tree, s0 = (trees[0], s0s[0]) if batch > 1 else (trees, s0s)
    design = [T64(d, True) for d in c.design]
    cnv, cen = c.ogeo.centroid_node_vectors(*design), c.ogeo.block_centroids(*design)
    amp, y0t = T64(7.5, True), T64(y0, True)
    free = osol.free_DOF_ids
    hist, _ = OD.solve_adaptive_replay_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(dict(cnv=cnv, cen=cen, amplitude=amp, **lv)), st)
    assert relerr(hist.detach().numpy(), fields.reshape(len(ts), 2, -1)[:, :, free]) < 1e-11    # the replay IS the engine's adaptive solve
    L = (hist * T64(fb.reshape(len(ts), 2, -1)[:, :, free])).sum()
    gr = torch.autograd.grad(L, design + [amp, y0t])
    mine = c.geo.vjp(c.design, tree.geometrical_params.centroid_node_vectors, tree.geometrical_params.block_centroids)
    errs = {"fwd": e_fwd, "steps": len(st) - 1, "outputs_per_step_max": int(per_step.max())}
    for i, (a, b) in enumerate(zip(mine, gr)):
        errs[f"design{i}"] = relerr(a, b.numpy())
    errs["amplitude"] = abs(tree.constraint_params["amplitude"] - gr[len(design)].item()) / abs(gr[len(design)].item())
    errs["state0"] = relerr(s0.reshape(2, -1)[:, free], gr[-1].numpy().reshape(2, -1)[:, free])
    for k, v in errs.items():
        if k not in ("steps", "outputs_per_step_max", "fwd"):
            assert v < RTOL_GRAD, (lattice, "adaptive records", k, v)
    return errs


def torch_table(times, values, vector):
    """Oracle twin of loading.Table: amplitude * interp(t - input_delay; times, values) (jnp.interp semantics)."""
    T, Y = np.asarray(times, dtype=float), np.asarray(values, dtype=float)
    vt = torch.as_tensor(np.asarray(vector, dtype=float))

    def fn(t, amplitude, loading_rate=None, input_delay=0.0):
        tau = torch.as_tensor(t, dtype=torch.float64) - input_delay
        tf = float(tau.detach())
        if tf <= T[0]:
            y = Y[0] + 0.0 * tau
        elif tf >= T[-1]:
            y = Y[-1] + 0.0 * tau
        else:
            lo = int(np.searchsorted(T, tf, side="right")) - 1
            y = Y[lo] + (Y[lo + 1] - Y[lo]) / (T[lo + 1] - T[lo]) * (tau - T[lo])
        return amplitude * y * vt
    return fn


def check_table_drive(lib, spi=6, n_out=5):
    """Prescribed displacement from a recorded signal (DFX_FN_TABLE): trajectory and gradients (design, amplitude, delay)
    against the oracle driven by the same piecewise-linear function."""
    import difflexmm_amd.loading as ld
    from difflexmm_amd.dynamics import setup_dynamic_solver
    import difflexmm_amd.energy as en_mod
    c = Case("quads", 4, True, True, seed=7, lib=lib, cutoff_deg=42.0)
    rng = np.random.default_rng(11)
    times = np.concatenate([[0.0], np.sort(rng.uniform(0.1e-4, 2.9e-4, 9)), [3.2e-4]])
    values = np.concatenate([[0.0], rng.normal(size=9), [0.3]])
    energy = en_mod.combine_block_energies(en_mod.build_strain_energy(c.bonds, en_mod.ligament_energy), en_mod.build_contact_energy(c.bonds))
    s = setup_dynamic_solver(c.geo, energy, constrained_block_DOF_pairs=c.con,
                             constrained_DOFs_fn=ld.Table(times, values, c.vec, amplitude="amplitude", delay="input_delay"),
                             damped_blocks=c.damped, _lib=lib)
    c.osolver_args["constrained_DOFs_fn"] = torch_table(times, values, c.vec)
    cp = c.cp._replace(constraint_params=dict(amplitude=2.5, input_delay=2e-5))
    ts = np.linspace(0, 3e-4, n_out)
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = s(y0, ts, cp, keep_trajectory=True, steps_per_interval=spi)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    of = osol(y0, ts, c.oracle_cp(dict(amplitude=T64(2.5), input_delay=T64(2e-5)))).numpy()
    e_fwd = relerr(fields, of)
    assert e_fwd < RTOL_TRAJ, ("table forward", e_fwd)
    fb = c.rng.normal(size=fields.shape)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    tree, _ = s.vjp(fb)
    design = [T64(d, True) for d in c.design]
    cnv, cen = c.ogeo.centroid_node_vectors(*design), c.ogeo.block_centroids(*design)
    amp, dly = T64(2.5, True), T64(2e-5, True)
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(y0), ts, c.oracle_cp(dict(cnv=cnv, cen=cen, amplitude=amp, input_delay=dly)),
                                            spi, "dopri5")
    L = (hist * T64(fb.reshape(len(ts), 2, -1)[:, :, osol.free_DOF_ids])).sum()
    gr = torch.autograd.grad(L, design + [amp, dly])
    mine = c.geo.vjp(c.design, tree.geometrical_params.centroid_node_vectors, tree.geometrical_params.block_centroids)
    errs = {f"design{i}": relerr(a, b.numpy()) for i, (a, b) in enumerate(zip(mine, gr))}
    errs["amplitude"] = abs(tree.constraint_params["amplitude"] - gr[-2].item()) / abs(gr[-2].item())
    errs["delay"] = abs(tree.constraint_params["input_delay"] - gr[-1].item()) / abs(gr[-1].item())
    for k, v in errs.items():
        assert v < RTOL_GRAD, ("table", k, v)
    return errs


def check_several_dofs_of_one_block_share_a_time_function(lib, spi=6, n_out=5):
    """x, y and theta of the driven block all follow the same pulse with different coefficients: their contributions to
    the time-function parameter gradients land on the same accumulator entries (three lanes of one quad in the kernel)."""
    import difflexmm_amd.loading as ld
    from difflexmm_amd.dynamics import setup_dynamic_solver
    import difflexmm_amd.energy as en_mod
    from .common import torch_pulse
    c = Case("quads", 4, True, False, seed=8, lib=lib)
    vec = np.array([1.0, 0.5, -0.02, 0, 0, 0, 0])
    energy = en_mod.build_strain_energy(c.bonds, en_mod.ligament_energy)
    s = setup_dynamic_solver(c.geo, energy, constrained_block_DOF_pairs=c.con, constrained_DOFs_fn=ld.Pulse(vec),
                             damped_blocks=c.damped, _lib=lib)
    c.osolver_args["constrained_DOFs_fn"] = torch_pulse(vec)
    fast = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
    cp = c.cp._replace(constraint_params=fast)
    ts = np.linspace(0, 3e-4, n_out)
    y0 = c.random_state(0.05, 0.02, 5.0)
    fields = s(y0, ts, cp, keep_trajectory=True, steps_per_interval=spi)
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    fb = c.rng.normal(size=fields.shape)
    fb.reshape(len(ts), 2, -1)[:, :, s.constrained_DOF_ids] = 0.0
    tree, _ = s.vjp(fb)
    amp, rate, dly = T64(7.5, True), T64(3000.0, True), T64(1e-5, True)
    hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, T64(y0), ts, c.oracle_cp(dict(amplitude=amp, loading_rate=rate, input_delay=dly)),
                                            spi, "dopri5")
    assert relerr(fields.reshape(len(ts), 2, -1)[:, :, osol.free_DOF_ids], hist.detach().numpy()) < RTOL_TRAJ
    L = (hist * T64(fb.reshape(len(ts), 2, -1)[:, :, osol.free_DOF_ids])).sum()
    gr = torch.autograd.grad(L, [amp, rate, dly])
    for name, g in zip(("amplitude", "loading_rate", "input_delay"), gr):
        e = abs(tree.constraint_params[name] - g.item()) / abs(g.item())
        assert e < RTOL_GRAD, (name, e)


# -- every parameter leaf, per member (tests/param_shapes.py builds the parameter images) ---------------------------------------------

RAW_WHICH = ("centroid_node_vectors", "void_angle0", "inertia", "damping", "fn_params")


def member_leaf_errors(mine, ref, prefix=""):
    """relerr of every leaf of every member on its own (``mine`` / ``ref``: one dict of arrays per member): a global maximum over a batch
    would hide a member whose entries are smaller than its neighbours'.  Returns {(member, leaf): error}."""
    assert len(mine) == len(ref)
    errs = {}
    for m, (a, b) in enumerate(zip(mine, ref)):
        assert set(a) == set(b), (sorted(a), sorted(b))
        for k in b:
            assert np.shape(a[k]) == np.shape(b[k]), (m, k, np.shape(a[k]), np.shape(b[k]))
            errs[(m, prefix + k)] = relerr(a[k], b[k])
    return errs


def _fields_bar(sc, n_t, seed=77):
    s, rng = sc.c.solver, np.random.default_rng(seed)
    fb = rng.normal(size=(len(sc.members), n_t, 2, sc.c.geo.n_blocks, 3))
    fb.reshape(len(sc.members), n_t, 2, -1)[:, :, :, s.constrained_DOF_ids] = 0.0
    return fb


def _y0(sc, seed=78):
    rng = np.random.default_rng(seed)
    y = rng.normal(size=(2, sc.c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02])
    y[1] *= 5.0
    return y


def run_engine_param_leaves(sc, ts, spi=None, adaptive=False, rtol=1e-5, atol=1e-5):
    """The engine on every leaf of ``sc`` (a ShapeCase): forward fields, then the reverse sweep twice -- ``vjp_raw`` (no ligament gradients:
    the persistent reverse loop where it applies) and ``vjp`` (the whole tree: the build that accumulates ligament / damping gradients),
    each after a forward solve of its own.  Returns per-member dicts of NumPy arrays in the oracle's layout plus the run's stats."""
    c, s = sc.c, sc.c.solver
    B, y0 = len(sc.members), _y0(sc)
    fb = _fields_bar(sc, len(ts))
    free = s.free_DOF_ids
    if adaptive:
        s.rtol, s.atol = rtol, atol

    def solve():
        out = s(y0, ts, sc.engine_params(), keep_trajectory=True, steps_per_interval=None if adaptive else spi)
        return np.array(out).reshape(B, len(ts), 2, c.geo.n_blocks, 3), dict(s.stats)

    fields, st_fwd = solve()
    step_times = [np.concatenate([ts[:1], s.engine.adaptive_step_times(m)]) for m in range(B)] if adaptive else None
    raw = {k: np.array(v) for k, v in s.vjp_raw(fb if B > 1 else fb[0], which=RAW_WHICH).items()}
    st_raw = dict(s.adjoint_stats)
    fields2, st_fwd2 = solve()
    trees, s0 = s.vjp(fb if B > 1 else fb[0])
    st_tree = dict(s.adjoint_stats)
    trees, s0 = (trees, s0) if B > 1 else ([trees], s0[None])
    out = []
    zc = np.zeros_like(c.cen)
    for m, (p, tree) in enumerate(zip(sc.members, trees)):
        d = {"fields": fields[m].reshape(len(ts), 2, -1)[:, :, free]}
        gp, mp = tree.geometrical_params, tree.mechanical_params
        for i, g in enumerate(c.geo.vjp(c.design, gp.centroid_node_vectors, gp.block_centroids)):
            d[f"design{i}"] = g
        bp = mp.bond_params
        d.update(ks=bp.k_stretch, ksh=bp.k_shear, kr=bp.k_rot, refv=bp.reference_vector, inertia=mp.inertia, damping=mp.damping)
        if c.contact:
            d.update(min_angle=mp.contact_params.min_angle, cutoff_angle=mp.contact_params.cutoff_angle, k_contact=mp.contact_params.k_contact)
        for k in ("amplitude", "loading_rate", "input_delay"):
            d[k] = tree.constraint_params[k]
        d["state0"] = s0[m].reshape(2, -1)[:, free]
        # the raw sweep, mapped onto the same leaves
        r = {}
        cnv_bar = raw["centroid_node_vectors"][m]
        if c.contact:
            cnv_bar = cnv_bar + geo.void_angles0_vjp(c.cnv, c.bonds, raw["void_angle0"][m])
        for i, g in enumerate(c.geo.vjp(c.design, cnv_bar, zc)):
            r[f"design{i}"] = g
        r["inertia"] = raw["inertia"][m].reshape(np.shape(p["inertia"]))
        rows = raw["damping"][m][c.damped]
        r["damping"] = rows.reshape(np.shape(p["damping"])) if np.shape(p["damping"]) == rows.shape else rows.sum(0)
        r["amplitude"], r["loading_rate"], r["input_delay"] = raw["fn_params"][m][0][:3]
        d["raw"] = r
        d["fields_again"] = fields2[m].reshape(len(ts), 2, -1)[:, :, free]
        out.append(d)
    return dict(members=out, fwd_stats=st_fwd, fwd_stats_again=st_fwd2, raw_stats=st_raw, tree_stats=st_tree, step_times=step_times)


def oracle_param_leaves(sc, ts, spi=None, step_times=None, integrator="dopri5", expanded=False):
    """torch.autograd through the oracle's unrolled fixed-grid solve (or its replay of the engine's accepted adaptive steps, one list of
    step boundaries per member) with every parameter leaf on the tape, member by member.  ``expanded``: the leaves a forward-mode
    tangent is given on -- the stiffnesses per ligament even where the member's are scalars, and also the gradient with respect to the node
    vectors themselves (key ``cnv``; inertia is a leaf of its own here, so this is their path through the energy and the void angles)."""
    c = sc.c
    B, y0 = len(sc.members), _y0(sc)
    fb = _fields_bar(sc, len(ts))
    out = []
    for m, p in enumerate(sc.members):
        design = [T64(d, True) for d in c.design]
        cnv, cen = c.ogeo.centroid_node_vectors(*design), c.ogeo.block_centroids(*design)
        names = ["ks", "ksh", "kr", "refv", "inertia", "damping", "amplitude", "loading_rate", "input_delay"]
        src = dict(ks=p["ks"], ksh=p["ksh"], kr=p["kr"], refv=p["refv"], inertia=p["inertia"], damping=p["damping"], amplitude=7.5,
                   loading_rate=3000.0, input_delay=1e-5, min_angle=c.contact_params[0], cutoff_angle=c.contact_params[1],
                   k_contact=c.contact_params[2])
        if c.contact:
            names += ["min_angle", "cutoff_angle", "k_contact"]
        if expanded:
            src.update({k: np.broadcast_to(p[k], (len(c.bonds),)) for k in ("ks", "ksh", "kr")})
        leaves = {k: T64(src[k], True) for k in names}
        y0t = T64(y0, True)
        cp = c.oracle_cp(dict(cnv=cnv, cen=cen, **leaves))
        if step_times is None:
            osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau=integrator)
            hist, _ = OD.solve_fixed_differentiable(osol, c.ogeo, y0t, ts, cp, spi, integrator)
        else:
            osol = c.oracle_solver(integrator="adaptive")
            hist, _ = OD.solve_adaptive_replay_differentiable(osol, c.ogeo, y0t, ts, cp, step_times[m])
        free = osol.free_DOF_ids
        L = (hist * T64(fb[m].reshape(len(ts), 2, -1)[:, :, free])).sum()
        gr = torch.autograd.grad(L, design + [leaves[k] for k in names] + [y0t] + ([cnv] if expanded else []))
        d = {"fields": hist.detach().numpy()}
        if expanded:
            d["cnv"], gr = gr[-1].numpy(), gr[:-1]
        for i, g in enumerate(gr[:len(design)]):
            d[f"design{i}"] = g.numpy()
        for k, g in zip(names, gr[len(design):-1]):
            d[k] = g.numpy()
        d["state0"] = gr[-1].numpy().reshape(2, -1)[:, free]
        if c.contact:
            assert np.abs([d[k] for k in ("min_angle", "cutoff_angle", "k_contact")]).max() > 0, "contact inactive: the test would be vacuous"
        out.append(d)
    return out


def raw_part(ref_members):
    """The leaves the raw sweep (``vjp_raw(which=RAW_WHICH)``) reaches, out of the oracle's per-member dicts."""
    keys = [k for k in ref_members[0] if k.startswith("design")] + ["inertia", "damping", "amplitude", "loading_rate", "input_delay"]
    return [{k: d[k] for k in keys} for d in ref_members]


def compare_param_leaves(eng, ref, rtol_fwd=RTOL_TRAJ, rtol_grad=RTOL_GRAD):
    """Every member, every leaf: the whole-tree sweep, the raw sweep and both forward solves against the oracle."""
    mine = [{k: v for k, v in d.items() if k not in ("raw", "fields_again")} for d in eng["members"]]
    errs = member_leaf_errors(mine, ref)
    errs.update(member_leaf_errors([d["raw"] for d in eng["members"]], raw_part(ref), prefix="raw:"))
    errs.update(member_leaf_errors([{"fields": d["fields_again"]} for d in eng["members"]], [{"fields": d["fields"]} for d in ref],
                                   prefix="again:"))
    bad = {k: v for k, v in errs.items() if not v < (rtol_fwd if k[1].endswith("fields") else rtol_grad)}
    assert not bad, bad
    return errs


def check_param_leaves(sc, ts, spi=None, adaptive=False, integrator="dopri5", rtol=1e-5, atol=1e-5):
    """Engine against the oracle on every parameter leaf of ``sc``; returns (engine result, errors)."""
    eng = run_engine_param_leaves(sc, ts, spi=spi, adaptive=adaptive, rtol=rtol, atol=atol)
    ref = oracle_param_leaves(sc, ts, spi=spi, step_times=eng["step_times"], integrator=integrator)
    return eng, compare_param_leaves(eng, ref)


# -- forward mode on the same parameter images --------------------------------------------------------------------------------------------

LEAF_OF_SHAPE = {"k_per_bond": ("ks", "ksh", "kr"), "uniform": ("ks", "ksh", "kr"), "damping_per_block": ("damping",)}     # else: refv
JVP_NAMES = ("cnv", "refv", "ks", "ksh", "kr", "inertia", "damping", "amplitude", "loading_rate", "input_delay", "state0")
CONTACT_NAMES = ("min_angle", "cutoff_angle", "k_contact")


def shape_leaf_names(shape):
    """The leaves a shape of tests/param_shapes.py is named after (oracle names)."""
    return LEAF_OF_SHAPE.get(shape, ("refv",))


def tangent_tree_of(sc, leaves):
    """(state0_dot, ControlParams-shaped tangent tree) out of a dict of oracle-named tangent leaves, following ``DynamicSolver.jvp``'s rules:
    a leaf the dict does not hold is None (a zero tangent), and so is state0_dot."""
    import difflexmm_amd as dm
    g = leaves.get
    contact = None
    if sc.c.contact and any(k in leaves for k in CONTACT_NAMES):
        contact = dm.ContactParams(*[g(k) for k in CONTACT_NAMES])
    con = {k: leaves[k] for k in ("amplitude", "loading_rate", "input_delay") if k in leaves}
    tree = dm.ControlParams(dm.GeometricalParams(None, g("cnv")),
                            dm.MechanicalParams(dm.LigamentParams(g("ks"), g("ksh"), g("kr"), g("refv")), None, g("inertia"), g("damping"), contact),
                            constraint_params=con or None)
    return g("state0"), tree


def shape_tangents(sc, seed):
    """Per member of a ShapeCase, named directions over the member's OWN leaves: ``out[m][name] = (state0_dot, tree, leaves)`` with
    ``(state0_dot, tree)`` what ``jvp`` takes for that member and ``leaves`` the same content under the oracle's names (a leaf that is
    missing there is a zero tangent).  ``"all"``: a random tangent of every leaf at relative size ~1 (as _tangent_tree of
    tests/test_gpu_tangent.py: node vectors, reference vectors and stiffnesses per ligament, inertia per block and DOF -- a ShapeCase gives
    it as a leaf, so it is seeded directly --, damping in the leaf's own shape, contact constants, pulse parameters, state0).  ``"leaf"``:
    only the leaves the shape is named after, with the values they have in ``"all"`` (so all - leaf is ``"all"`` without them): relerr
    normalises by the global maximum, and the tangent of e.g. the damping alone sits three decades under the all-leaf column."""
    c = sc.c
    rng = np.random.default_rng(seed)
    nbd = len(c.bonds)
    assert all(p["inertia"] is not None for p in sc.members), "shape_tangents seeds the inertia leaf directly"
    fast = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
    out = []
    for p in sc.members:
        def d(x):
            return rng.normal(size=np.shape(x)) * (np.abs(np.asarray(x, dtype=float)) + 1e-12)
        lv = dict(cnv=0.02 * rng.normal(size=np.shape(c.cnv)), refv=d(np.broadcast_to(p["refv"], (nbd, 2))),
                  ks=d(np.broadcast_to(p["ks"], (nbd,))), ksh=d(np.broadcast_to(p["ksh"], (nbd,))), kr=d(np.broadcast_to(p["kr"], (nbd,))),
                  inertia=d(p["inertia"]), damping=d(p["damping"]))
        assert np.shape(lv["damping"]) == np.shape(p["damping"])
        if c.contact:
            lv.update({k: 0.05 * rng.normal() for k in CONTACT_NAMES})
        lv.update({k: 0.1 * rng.normal() * v for k, v in fast.items()})
        y0d = rng.normal(size=(2, c.geo.n_blocks, 3)) * np.array([0.05, 0.05, 0.02])
        y0d[1] *= 5.0
        y0d.reshape(2, -1)[:, c.solver.constrained_DOF_ids] = 0.0          # (state0 of prescribed DOFs is not read)
        lv["state0"] = y0d
        only = {k: lv[k] for k in shape_leaf_names(sc.shape)}
        out.append({"all": tangent_tree_of(sc, lv) + (lv,), "leaf": tangent_tree_of(sc, only) + (only,)})
    return out


def oracle_member_leaves(sc, p):
    """The primal leaves of one member under the oracle's names (NumPy), state0 included."""
    c = sc.c
    nbd = len(c.bonds)
    lv = dict(cnv=c.cnv, refv=np.broadcast_to(p["refv"], (nbd, 2)), ks=np.broadcast_to(p["ks"], (nbd,)), ksh=np.broadcast_to(p["ksh"], (nbd,)),
              kr=np.broadcast_to(p["kr"], (nbd,)), inertia=p["inertia"], damping=p["damping"], amplitude=7.5, loading_rate=3000.0,
              input_delay=1e-5, state0=_y0(sc))
    if c.contact:
        lv.update(zip(CONTACT_NAMES, c.contact_params))
    return lv


def oracle_param_jvp(sc, ts, directions, spi=None, step_times=None, names=("all", "leaf"), members=None):
    """torch.autograd.functional.jvp through the oracle's unrolled fixed-grid solve (``step_times[m]``: through its replay of the accepted
    adaptive steps of member m), member by member and direction by direction; ``directions``: what :func:`shape_tangents` returns.
    Returns per member ``{"fields": (T, 2, n_free), name: fields_dot (T, 2, n_free), ...}`` on the free DOFs (None for a member that
    ``members`` leaves out)."""
    c = sc.c
    keys = list(JVP_NAMES) + (list(CONTACT_NAMES) if c.contact else [])
    out = []
    for m, p in enumerate(sc.members):
        if members is not None and m not in members:
            out.append(None)
            continue
        prim = oracle_member_leaves(sc, p)
        if step_times is None:
            osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
        else:
            osol = c.oracle_solver(integrator="adaptive")

        def f(*xs):
            lv = dict(zip(keys, xs))
            y0t = lv.pop("state0")
            if step_times is None:
                return OD.solve_fixed_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(lv), spi, "dopri5")[0]
            return OD.solve_adaptive_replay_differentiable(osol, c.ogeo, y0t, ts, c.oracle_cp(lv), step_times[m])[0]
        d = {}
        for name in names:
            tan = directions[m][name][2]
            assert set(tan) <= set(keys), sorted(set(tan) - set(keys))
            of, ojv = torch.autograd.functional.jvp(f, tuple(T64(prim[k]) for k in keys),
                                                    tuple(T64(tan[k]) if k in tan else torch.zeros_like(T64(prim[k])) for k in keys))
            d["fields"] = of.detach().numpy()
            d[name] = ojv.numpy()
        out.append(d)
    return out


def oracle_param_fields(sc, ts, spi, m, **replaced):
    """The oracle's own fixed-grid fields (free DOFs) of member m, with leaves of ``replaced`` instead of the member's."""
    c = sc.c
    lv = dict(oracle_member_leaves(sc, sc.members[m]), **replaced)
    y0 = lv.pop("state0")
    osol = c.oracle_solver(integrator="fixed", steps_per_interval=spi, tableau="dopri5")
    of = osol(y0, ts, c.oracle_cp({k: T64(v) for k, v in lv.items()})).numpy()
    return of.reshape(len(ts), 2, -1)[:, :, osol.free_DOF_ids]


def uniform_twin(sc, m):
    """The leaves that turn member m's image into its uniform twin: the leaf the shape is named after replaced by its mean (stiffnesses,
    damping per DOF) or by the lattice's own reference vectors."""
    c, p = sc.c, sc.members[m]
    names = shape_leaf_names(sc.shape)
    if names == ("refv",):
        return dict(refv=np.broadcast_to(c.refv, (len(c.bonds), 2)).copy())
    if names == ("damping",):
        return dict(damping=np.broadcast_to(p["damping"], (len(c.damped), 3)).mean(0))
    return {k: float(np.mean(p[k])) for k in names}
