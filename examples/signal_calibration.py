"""A calibration of four scalars against signal histories by Levenberg-Marquardt: stretching and bending stiffness of the ligaments, the
damping and the amplitude of the drive of a 6 x 6 rotating-squares sample, from two tracked displacements, one tracked velocity and the
reaction force on the driven block.  No measurements ship with this repository, so the "experiment" is the response of a sample with
known parameters; the fit starts 15 % away from them.

    python examples/signal_calibration.py [--blocks 6] [--outputs 17] [--iterations 20]

Every evaluation is ONE forward-mode solve (problems.SignalCalibration -> DynamicSolver.signal_jacfwd): the signals and their four
tangent columns are formed on the device at the end of the tangent pass (include/dfx.h: dfx_forward_tangent_signals_multi), so what
comes back is (4, T, 4) numbers, not five histories; the reaction force is differentiated where the solve ran.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import difflexmm_amd as dm  # noqa: E402
from difflexmm_amd import energy as en  # noqa: E402
from difflexmm_amd import loading as ld  # noqa: E402
from difflexmm_amd import objective as O  # noqa: E402
from difflexmm_amd.geometry import QuadGeometry  # noqa: E402
from difflexmm_amd.problems import SignalCalibration  # noqa: E402

WRT = ["k_stretch", "k_rot", "damping", "amplitude"]
TRUTH = np.array([120.0, 1.5, 5e-4, 1.5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--outputs", type=int, default=17)
    ap.add_argument("--iterations", type=int, default=20)
    a = ap.parse_args()
    n = a.blocks
    g = QuadGeometry(n, n, 15.0, 2.25)
    design = g.get_design_from_rotated_square(25 * math.pi / 180)
    bonds = g.bond_connectivity()
    energy = en.combine_block_energies(en.build_strain_energy(bonds, en.ligament_energy), en.build_contact_energy(bonds))
    driven = (n // 2) * n                                       # a block on the left edge: x driven, y and rotation held; a corner clamped
    con = np.array([[driven, 0], [driven, 1], [driven, 2], [0, 0], [0, 1], [0, 2]])
    solve = dm.setup_dynamic_solver(g, energy, constrained_block_DOF_pairs=con, constrained_DOFs_fn=ld.Pulse(np.array([1.0, 0, 0, 0, 0, 0])),
                                    damped_blocks=np.arange(n * n))
    cp = dm.ControlParams(dm.GeometricalParams(g.block_centroids(*design), g.centroid_node_vectors(*design)),
                          dm.MechanicalParams(dm.LigamentParams(TRUTH[0], 1.19, TRUTH[1], g.reference_bond_vectors()), 6.18e-9, None, TRUTH[2],
                                              dm.ContactParams(-15 * math.pi / 180, 42 * math.pi / 180, 1.5)),
                          constraint_params=dict(amplitude=TRUTH[3], loading_rate=3000.0, input_delay=1e-5))
    inner = driven + 2
    spec = O.SignalSpec([(0, inner, 0, 1.0), (1, inner + n + 1, 2, 1.0), (2, inner + 1, 3, 1.0), (3, driven, 6, 1.0)], 4)
    ts, grid = np.linspace(0.0, 4e-4, a.outputs), dict(steps_per_interval=4)
    state0 = np.zeros((2, n * n, 3))
    solve(state0, ts, cp, **grid)
    measured = solve.signal_values(spec)[0]                     # the "experiment"
    spec = spec.with_targets(measured, 1.0 / np.abs(measured).max(axis=0) ** 2)
    cal = SignalCalibration(solve, state0, ts, cp, spec, WRT, **grid)
    start = TRUTH * np.array([1.15, 0.85, 1.15, 0.85])
    t0 = time.perf_counter()
    hist = cal.run_lm(start, a.iterations)
    wall = time.perf_counter() - t0
    print(f"{hist['n_eval']} evaluations (one forward-mode solve with {len(WRT)} tangents each) in {wall:.2f} s, status {hist['status']}")
    print("misfit: first %.3e  best %.3e" % (cal.objective_values[0], min(cal.objective_values)))
    for name, x0, x, t in zip(WRT, start, hist["x"][-1], TRUTH):
        print(f"  {name:10s} start {x0:.6g}  fitted {x:.9g}  sample {t:.6g}")


if __name__ == "__main__":
    main()
