"""What a tangent stage costs: DynamicSolver.jvp (primal + one tangent direction per member: jvp_multi along one direction, the
K-direction kernels of dfx_tangent.h at width 1) against the plain fixed-grid forward solve solve_dynamics(..., steps_per_interval=...) on the same grid, at
  * 128 x 128 quads with angle contact, 16 members, 250 dopri5 steps;
  * the paper's lattice (24 x 16 quads, spacing 15 mm, contact -15 / -10 deg, damping), 1 member, 250 steps.
Prints device ms per step of both (HIP events around the stage launches), the wall time per call, and the ratio.
    python tools/tangent_timing.py
--adaptive: the paper's lattice at the paper's tolerances (rtol 1e-8 / atol 1e-4, 200 outputs over 2 / 30 s), forward mode of the default
call both ways: jvp(adaptive=True) (adaptive pass + tangent pass on every member's own accepted steps with the dense output) beside the
no-grid jvp (adaptive pass + tangent pass on the frozen grid of the slowest member).  Wall ms per call and device ms of the tangent pass.
    python tools/tangent_timing.py --adaptive"""
import math
import os
import sys
import time

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)

import difflexmm_amd as dm                                   # noqa: E402
from difflexmm_amd import energy as en_mod                   # noqa: E402
from difflexmm_amd import geometry as geo                    # noqa: E402
from difflexmm_amd import loading as ld                      # noqa: E402
from difflexmm_amd.dynamics import setup_dynamic_solver      # noqa: E402

RHO, KS, KSH, KR = 6.18e-9, 120.0, 1.19, 1.5


def quads_problem(n1, n2, batch, spacing=15.0, angle_deg=25.0, seed=0):
    g = geo.QuadGeometry(n1, n2, spacing, 0.15 * spacing)
    rng = np.random.default_rng(seed)
    base = g.get_design_from_rotated_square(angle_deg * math.pi / 180)
    bonds = g.bond_connectivity()
    energy = en_mod.combine_block_energies(en_mod.build_strain_energy(bonds, en_mod.ligament_energy), en_mod.build_contact_energy(bonds))
    left = np.arange(0, n1 * n2, n1)[n2 // 2 - 1:n2 // 2 + 1]             # two excited blocks on the left edge
    con = np.array([[b, d] for b in left for d in range(3)])
    vec = np.array([1.0 if d == 0 else 0.0 for b in left for d in range(3)])
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * RHO * spacing ** 2 * KSH)] * 2 + [2 * math.sqrt(0.02175026 * RHO * spacing ** 4 * KR)])
    s = setup_dynamic_solver(g, energy, constrained_block_DOF_pairs=con, constrained_DOFs_fn=ld.Pulse(vec), damped_blocks=np.arange(n1 * n2),
                             batch=batch)
    cps, dots = [], []
    for m in range(batch):
        design = tuple(b + rng.uniform(-0.02 * spacing, 0.02 * spacing, b.shape) for b in base)
        cps.append(dm.ControlParams(dm.GeometricalParams(g.block_centroids(*design), g.centroid_node_vectors(*design)),
                                    dm.MechanicalParams(dm.LigamentParams(KS, KSH, KR, g.reference_bond_vectors()), RHO, None, damping,
                                                        dm.ContactParams(-15 * math.pi / 180, -10 * math.pi / 180, KR)),
                                    constraint_params=dict(amplitude=0.5 * spacing, loading_rate=30.0, input_delay=0.1 / 30.0)))
        # one direction per member: design node vectors, stiffnesses, damping and pulse amplitude at once
        dots.append(dm.ControlParams(dm.GeometricalParams(None, 0.01 * rng.normal(size=np.shape(cps[-1].geometrical_params.centroid_node_vectors))),
                                     dm.MechanicalParams(dm.LigamentParams(1.0, 0.01, 0.01, None), None, None, 0.1 * damping, None),
                                     constraint_params=dict(amplitude=1.0)))
    return s, cps, dots


def time_case(label, n1, n2, batch, steps, reps=3):
    s, cps, dots = quads_problem(n1, n2, batch)
    ts = np.array([0.0, 0.5 / 30.0])
    spi = steps
    y0 = np.zeros((batch, 2, n1 * n2, 3))
    fwd, tan = [], []
    for rep in range(reps + 1):                              # (the first round warms up: module loads, allocations)
        t0 = time.perf_counter()
        s(y0, ts, cps, steps_per_interval=spi)
        w_f = time.perf_counter() - t0
        st_f = dict(s.stats)
        t0 = time.perf_counter()
        fields, fdot = s.jvp(y0, ts, cps, None, dots, steps_per_interval=spi)
        w_t = time.perf_counter() - t0
        st_t = dict(s.stats)
        if rep:
            fwd.append((st_f["kernel_ms"], w_f))
            tan.append((st_t["kernel_ms"], w_t))
    assert np.all(np.isfinite(fdot)) and np.abs(fdot[:, -1]).max() > 0
    f_ms = min(x[0] for x in fwd) / steps
    t_ms = min(x[0] for x in tan) / steps
    print(f"{label}: {n1 * n2} blocks x {batch} members, {steps} dopri5 steps | forward {f_ms:.4f} ms/step (wall {1e3 * min(x[1] for x in fwd) / steps:.4f}), "
          f"{st_f['launches']} launches | tangent {t_ms:.4f} ms/step (wall {1e3 * min(x[1] for x in tan) / steps:.4f}), {st_t['launches']} launches, "
          f"{1e3 * t_ms / 6:.1f} us per tangent stage | ratio tangent / forward {t_ms / f_ms:.2f}")
    return t_ms / f_ms


def time_adaptive(reps=3):
    n1, n2 = 24, 16
    s, cps, dots = quads_problem(n1, n2, 1)
    s.rtol, s.atol = 1e-8, 1e-4
    ts = np.linspace(0.0, 2.0 / 30.0, 200)
    y0 = np.zeros((1, 2, n1 * n2, 3))
    rows = {"adaptive=True": [], "no grid": []}
    for rep in range(reps + 1):                              # (the first round warms up)
        for label, kw in (("adaptive=True", dict(adaptive=True)), ("no grid", {})):
            t0 = time.perf_counter()
            fields, fdot = s.jvp(y0, ts, cps, None, dots, **kw)
            wall = time.perf_counter() - t0
            assert np.all(np.isfinite(fdot)) and np.abs(fdot[:, -1]).max() > 0
            if rep:
                rows[label].append((wall, s.stats["kernel_ms"], s.stats["steps"], s.stats["launches"], s.stats["step_control"]))
    for label, r in rows.items():
        wall, ms, steps, launches, control = min(r)
        print(f"paper 24x16 quads + contact, rtol 1e-8 / atol 1e-4, 200 outputs | jvp {label} ({control}): wall {1e3 * wall:.1f} ms per call, "
              f"tangent pass {ms:.1f} ms on the device, {steps} steps, {launches} launches")


if __name__ == "__main__":
    if "--adaptive" in sys.argv[1:]:
        time_adaptive()
        sys.exit(0)
    time_case("128x128 quads + contact", 128, 128, 16, 250)
    time_case("paper 24x16 quads + contact", 24, 16, 1, 250)
