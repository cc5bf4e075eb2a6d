"""Maximise the energy delivered to a target region through its boundary hinges: a few iterations of the method of moving asymptotes on the
6 x 6 quads with ``problems.TargetCutEnergy`` around the 2 x 2 region in the middle of the lattice -- the work

    W = -dt * sum_k sum_h sum_d f_hd(t_k) v_{b(h) d}(t_k)

that the eight ligaments between the region and the rest of the lattice do on it (hinge-force channels against block velocities at lag 0,
``dfx_signal_xcorr_value_and_grad``: the history never leaves the device).  W is a rectangle rule on the output times.  Beside W, every
evaluation prints the kinetic energy summed over the output times in the same region (``TargetKineticEnergy``, the objective of the
focusing problems, which stands in for the delivered energy there) and the peak of the force transmitted through the cut.

    python examples/cut_energy.py [--iterations 6] [--outputs 200] [--bound 0.03]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import objective as O  # noqa: E402
from difflexmm_amd import problems as P  # noqa: E402

SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY, LOADING_RATE = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9, 30.0
N = 6


class Reported:
    """``TargetCutEnergy`` as the loops of ``OptimizationProblem`` take it (they maximise), with a line per evaluation."""

    def __init__(self, cut, kinetic):
        self.cut, self.kinetic, self.forward = cut, kinetic, cut.forward
        self.history = []

    def value_and_grad(self, design):
        w, g = self.cut.value_and_grad(design, on_device=True)
        sd = self.forward.solve_dynamics
        resultant = sd.signal_values(O.SignalSpec.cut_force(self.cut.hinges))[0]                # (T, 2), on the solve of this evaluation
        ke = self.kinetic.value(design)
        self.history.append((w, ke))
        print(f"evaluation {len(self.history)}: W = {w:.6e} (work on the region through its {len(self.cut.hinges)} boundary hinges), kinetic-energy "
              f"objective of the region {ke:.6e}, peak transmitted force {np.linalg.norm(resultant, axis=1).max():.4e}")
        return w, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--bound", type=float, default=0.03, help="box on the design variables, in units of the block spacing")
    a = ap.parse_args()
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                                [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((N * N, 1))
    fw = P.QuadsFocusingForward(n1_blocks=N, n2_blocks=N, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, use_contact=True, k_contact=K_ROT, min_angle=-15 * math.pi / 180,
                                cutoff_angle=-10 * math.pi / 180, amplitude=0.5 * SPACING, loading_rate=LOADING_RATE,
                                input_delay=0.1 / LOADING_RATE, n_excited_blocks=2, loaded_side="left", input_shift=0,
                                simulation_time=2 / LOADING_RATE, n_timepoints=a.outputs, atol=1e-4, rtol=1e-8)
    fw.setup()
    kinetic = P.TargetKineticEnergy(fw, (2, 2), (0, 0))
    cut = P.TargetCutEnergy(fw, kinetic.target_blocks)
    print(f"region {sorted(int(b) for b in kinetic.target_blocks)}, boundary hinges (block, node) {cut.hinges}, {a.outputs} outputs "
          f"{float(np.diff(fw.timepoints).mean()):.3e} s apart")
    wrapped = Reported(cut, kinetic)
    problem = P.OptimizationProblem(wrapped, name="cut_energy")
    start = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    problem.run_optimization_nlopt(start, a.iterations, lower_bound=-a.bound * SPACING, upper_bound=a.bound * SPACING, min_void_angle=0.0,
                                   min_block_angle=10 * math.pi / 180, min_edge_length=0.1 * SPACING, verbose=False)
    first, best = wrapped.history[0], max(wrapped.history, key=lambda h: h[0])
    print(f"W {first[0]:.6e} -> {best[0]:.6e}; kinetic-energy objective of the region {first[1]:.6e} -> {best[1]:.6e} in {len(wrapped.history)} evaluations")


if __name__ == "__main__":
    main()
