"""Shape the drive itself: the waveform that puts the most kinetic energy into a target region under an amplitude bound |Y_j| <= A.

8 x 8 quads with contact, driven on the left edge by a ``loading.Table`` whose samples are a leaf of ``constraint_params``
(``Table(times, "waveform")``); ``problems.DriveWaveformDesign`` maximises the kinetic energy summed over the output times in a 2 x 2 region
on the far side (``objective.ObjectiveSpec``, evaluated and differentiated on the device) by the method of moving asymptotes -- one kept solve
and one reverse sweep per evaluation, the sample gradient from the sweep's drive-cotangent trace.  The first and the last sample stay zero,
so the drive starts and ends at rest.  Every evaluation prints the objective beside that of the raised-cosine pulse of the same peak
amplitude A (the synthetic pulse of the focusing problems, sampled on the same breakpoints).

    python examples/waveform_design.py [--iterations 12] [--samples 25] [--amplitude 1.5] [--outputs 100]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import loading as L  # noqa: E402
from difflexmm_amd import objective as O  # noqa: E402
from difflexmm_amd import problems as P  # noqa: E402

SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY, LOADING_RATE = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9, 30.0
N = 8


class Reported(P.DriveWaveformDesign):
    """``DriveWaveformDesign`` with a line per evaluation: the objective beside that of the raised-cosine pulse."""
    reference = None

    def value_and_grad(self, y):
        v, g = super().value_and_grad(y)
        beside = "" if self.reference is None else f"   ({v / self.reference:.3f} x the raised-cosine pulse, {self.reference:.6e})"
        print(f"evaluation: kinetic energy in the target {v:.6e}{beside}")
        return v, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=100)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--samples", type=int, default=25, help="breakpoints of the waveform over the drive window 1 / loading_rate")
    ap.add_argument("--amplitude", type=float, default=1.5, help="the bound A on every sample, in mm")
    a = ap.parse_args()
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                                [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((N * N, 1))
    fw = P.QuadsFocusingForward(n1_blocks=N, n2_blocks=N, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, use_contact=True, k_contact=K_ROT, min_angle=-15 * math.pi / 180,
                                cutoff_angle=-10 * math.pi / 180, amplitude=a.amplitude, loading_rate=LOADING_RATE, input_delay=0.0,
                                n_excited_blocks=2, loaded_side="left", input_shift=0, simulation_time=2 / LOADING_RATE,
                                n_timepoints=a.outputs, atol=1e-6, rtol=1e-6)
    times = np.linspace(0.0, 1.0 / LOADING_RATE, a.samples)
    fw.setup(excited_blocks_fn=L.Table(times, "waveform"))
    target = P.quads_target_blocks(fw.geometry, (2, 2), (2, 0))
    spec = O.ObjectiveSpec(O.KINETIC, O.block_weights_from_targets(fw.geometry.n_blocks, [target], np.ones(1)))
    pulse = 0.5 * a.amplitude * (1.0 - np.cos(2 * np.pi * LOADING_RATE * times))          # the raised cosine of the same peak amplitude
    cp = fw.control_params(fw.geometry.get_design_from_rotated_square(25 * math.pi / 180))
    cp = cp._replace(constraint_params=dict(cp.constraint_params, waveform=pulse))
    design = Reported(fw.solve_dynamics, fw.state0, fw.timepoints, cp, "waveform", spec, fixed=(0, -1), maximize=True)
    design.reference, _ = design.value_and_grad(pulse)
    print(f"target blocks {sorted(int(b) for b in target)}; {a.samples} samples over {times[-1]:.3e} s, |Y_j| <= {a.amplitude}")
    best = design.run_mma(pulse, a.iterations, lower_bound=-a.amplitude, upper_bound=a.amplitude)
    print(f"best of {len(design.objective_values)} evaluations: {max(design.objective_values):.6e} against {design.reference:.6e}; "
          f"peak |Y| {np.abs(best).max():.3f}, samples at the bound: {int(np.sum(np.abs(best) > 0.999 * a.amplitude))} of {a.samples}")


if __name__ == "__main__":
    main()
