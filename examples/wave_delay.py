"""Tune the arrival time of a pulse: a few iterations of the method of moving asymptotes on a small quad lattice with
``problems.TargetWaveDelay`` -- the softmax peak of the correlation coefficient between the velocity of a block near the loaded side and
that of a block further along the same row, over time lags in output indices, plus the squared distance of the soft delay from a chosen
one (``dfx_signal_xcorr_value_and_grad``: the history never leaves the device).  Peak and delay are printed at every evaluation.

    python examples/wave_delay.py [--iterations 6] [--outputs 60] [--delay 1.5e-2] [--bound 0.03] [--host]
    python examples/wave_delay.py --cpu-port --outputs 30 --max-lag 10      # rehearsal without a GPU (host path)
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import problems as P  # noqa: E402

SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY, LOADING_RATE = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9, 30.0


class Minimised:
    """The loops of ``OptimizationProblem`` maximise: hand them -J, and report the peak and the delay of every evaluation."""

    def __init__(self, objective, on_device, dt):
        self.objective, self.forward, self.on_device, self.dt = objective, objective.forward, on_device, dt
        self.history = []

    def value_and_grad(self, design):
        v, g = self.objective.value_and_grad(design, on_device=self.on_device)
        peak, delay = self.objective.last_peak, self.objective.last_delay
        self.history.append((v, peak, delay))
        print(f"evaluation {len(self.history)}: J = {v:.6f}, peak of the correlation coefficient {peak:.4f}, delay {delay:.3f} outputs "
              f"= {delay * self.dt:.4e} s")
        return -v, tuple(-a for a in g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=8)
    ap.add_argument("--n2", type=int, default=6)
    ap.add_argument("--outputs", type=int, default=60)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--max-lag", type=int, default=20)
    ap.add_argument("--beta", type=float, default=20.0)
    ap.add_argument("--delay", type=float, default=1.5e-2, help="the wanted delay between the two blocks, in seconds")
    ap.add_argument("--bound", type=float, default=0.03, help="box on the design variables, in units of the block spacing")
    ap.add_argument("--host", action="store_true", help="history down, correlation in NumPy, cotangent up through vjp")
    ap.add_argument("--cpu-port", action="store_true", help="the CPU port of the oracle (host path only)")
    a = ap.parse_args()
    lib = None
    if a.cpu_port:
        from oracle.cpu import load
        lib, a.host = load(), True
    nb = a.n1 * a.n2
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                                [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((nb, 1))
    fw = P.QuadsFocusingForward(n1_blocks=a.n1, n2_blocks=a.n2, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, use_contact=True, k_contact=K_ROT, min_angle=-15 * math.pi / 180,
                                cutoff_angle=-10 * math.pi / 180, amplitude=0.5 * SPACING, loading_rate=LOADING_RATE,
                                input_delay=0.1 / LOADING_RATE, n_excited_blocks=2, loaded_side="left", input_shift=0,
                                simulation_time=2 / LOADING_RATE, n_timepoints=a.outputs, atol=1e-4, rtol=1e-8, _lib=lib)
    fw.setup()
    row = (a.n2 // 2) * a.n1
    source, target = row + 1, row + (3 * a.n1) // 4              # the second block of the middle row and one three quarters along it
    dt = float(np.diff(fw.timepoints).mean())
    objective = P.TargetWaveDelay(fw, [(source, 0)], [(target, 0)], "velocity", a.max_lag, a.beta, delay_target_seconds=a.delay, w_peak=-1.0,
                                  w_delay=2.0 / a.max_lag ** 2)
    print(f"blocks {source} -> {target}, {a.outputs} outputs {dt:.3e} s apart, lags -{a.max_lag} .. {a.max_lag}, wanted delay "
          f"{objective.spec.delay_target:.3f} outputs")
    wrapped = Minimised(objective, not a.host, dt)
    problem = P.OptimizationProblem(wrapped, name="wave_delay")
    start = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    problem.run_optimization_nlopt(start, a.iterations, lower_bound=-a.bound * SPACING, upper_bound=a.bound * SPACING, min_void_angle=0.0,
                                   min_block_angle=10 * math.pi / 180, min_edge_length=0.1 * SPACING, verbose=False)
    first, best = wrapped.history[0], min(wrapped.history, key=lambda h: h[0])
    print(f"J {first[0]:.6f} -> {best[0]:.6f}; peak {first[1]:.4f} -> {best[1]:.4f}; delay {first[2]:.3f} -> {best[2]:.3f} outputs "
          f"(wanted {objective.spec.delay_target:.3f}) in {len(wrapped.history)} evaluations")


if __name__ == "__main__":
    main()
