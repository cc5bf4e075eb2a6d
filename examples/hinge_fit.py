"""`problems/hinge_characterization.py` on the engine: the ligament stiffnesses of a rotating-squares sample fitted to force-displacement
curves of a tension, a compression and a shear test.  No measured curves ship with this repository, so the "experiment" is the response
of a sample with known stiffnesses; the fit starts elsewhere and must walk towards them.

    python examples/hinge_fit.py [--iterations 12] [--cells 3] [--method mma|lm] [--on-device]

--method mma (the default) is the reference's loop: the method of moving asymptotes on the reverse-mode gradient.  --method lm treats the
fit as the least-squares problem it is: Levenberg-Marquardt on the residual Jacobian, which forward mode delivers in one pass per test
(an addition, HingeResponseError.run_optimization_lm).  --on-device (with mma) evaluates and differentiates the misfit on the kept solve
of every test (HingeResponseError.value_and_grad_device: the signal misfit of include/dfx.h): the histories stay on the device and the
second, reaction-force handle is not used.  --on-device with lm takes the reaction force and its three tangents at the end of every
tangent pass on the device (DynamicSolver.signal_jacfwd: the forward-mode signals of include/dfx.h): the same fit, no history downloaded.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import hinge as H  # noqa: E402


TRUTH, START = (120.0, 1.19, 1.5), (80.0, 2.0, 0.8)
LOWER, UPPER = [20.0, 0.2, 0.2], [400.0, 6.0, 6.0]


def build_fit(cells=3, timepoints=21):
    """The three tests and the fit against the responses of the sample with the stiffnesses TRUTH."""
    kw = dict(n1_cells=cells, n2_cells=cells, spacing=15.0, bond_length=2.25, initial_angle=25 * math.pi / 180, k_stretch=120.0,
              k_shear=1.19, k_rot=1.5, density=6.18e-9, damping=0.2, amplitude=1.5, loading_rate=100.0, n_timepoints=timepoints,
              use_contact=True, k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180)
    tests = [H.HingeForward(loading_type=lt, force_multiplier=-1.0 if lt == "compression" else 1.0, **kw) for lt in ("tension", "compression", "shear")]
    for fw in tests:
        fw.setup()
    targets = {fw.loading_type: np.vstack([fw.force_displacement(*fw.solve(TRUTH)), np.ones(timepoints)]) for fw in tests}
    return H.HingeResponseError(tests, targets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--cells", type=int, default=3)
    ap.add_argument("--timepoints", type=int, default=21)
    ap.add_argument("--method", choices=("mma", "lm"), default="mma")
    ap.add_argument("--on-device", action="store_true", help="mma: the misfit and its gradient on the kept solve of every test; lm: the force Jacobian at the end of the tangent pass")
    a = ap.parse_args()
    fit = build_fit(a.cells, a.timepoints)
    t0 = time.perf_counter()
    if a.method == "lm":
        fit.run_optimization_lm(START, a.iterations, lower_bound=LOWER, upper_bound=UPPER, on_device=a.on_device)
        what = "3 forward-mode solves with 3 tangents each" + (", force Jacobian on the device" if a.on_device else "")
    else:
        fit.run_optimization_nlopt(START, a.iterations, lower_bound=LOWER, upper_bound=UPPER, on_device=a.on_device)
        what = "3 forward + 3 reverse solves each" + (", misfit on the device" if a.on_device else "")
    wall = time.perf_counter() - t0
    best = int(np.argmin(fit.objective_values))
    print(f"{len(fit.objective_values)} evaluations ({what}) in {wall:.2f} s")
    print("squared error: first %.3e  best %.3e" % (fit.objective_values[0], fit.objective_values[best]))
    print("stiffnesses  : start", START, " best", tuple(round(k, 4) for k in fit.design_values[best]), " sample", TRUTH)


if __name__ == "__main__":
    main()
