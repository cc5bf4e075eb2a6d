"""Focus a pulse without breaking a hinge: the 6 x 6 focusing problem (kinetic energy in a 2 x 2 target, maximised with the method of
moving asymptotes under the geometric constraints) once as it is and once under a stretch-strain limit on the ligaments of the 3 x 3
region around the target (the ligaments next to the driven blocks follow the prescribed pulse whatever the design) --
``problems.PeakLigamentStrain`` handed to ``run_optimization_nlopt(state_constraints=[...])``: a smooth maximum over all output times and
ligaments of the squared utilisation (eps / eps_lim)^2, evaluated and differentiated on the device (``dfx_strain_peak_value_and_grad``).
The limit is set to a fraction of the peak stretch strain of the initial design, so that the unconstrained optimum violates it.  The peak
utilisation of both results is printed.

    python examples/strain_limited_focusing.py [--iterations 10] [--fraction 0.9] [--beta 30] [--bound 0.02]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import problems as P  # noqa: E402

SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9
WATCHED = dict(target_sizes=((3, 3),), target_shifts=((1, 0),), ends="any")


def forward(n=6):
    damping = 0.05 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                              [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((n * n, 1))
    fw = P.QuadsFocusingForward(n1_blocks=n, n2_blocks=n, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, amplitude=5.0, loading_rate=2500.0, input_delay=2e-5,
                                n_excited_blocks=2, loaded_side="left", input_shift=0, simulation_time=6e-4, n_timepoints=40, use_contact=True,
                                k_contact=1.5, min_angle=5 * math.pi / 180, cutoff_angle=45 * math.pi / 180, steps_per_interval=8)
    fw.setup()
    return fw


def utilisation(limit, design):
    """sqrt of the hard maximum of q: the largest eps / eps_lim over the watched ligaments and all output times"""
    limit.value(design)
    return math.sqrt(limit.last_peak), tuple(int(x) for x in limit.last_peak_at)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--fraction", type=float, default=0.9, help="stretch-strain limit as a fraction of the initial design's peak stretch strain")
    ap.add_argument("--beta", type=float, default=30.0, help="sharpness of the KS aggregate (q is of the order of 1 at the limit)")
    ap.add_argument("--bound", type=float, default=0.02, help="box on the design variables, in units of the block spacing")
    a = ap.parse_args()
    box = a.bound * SPACING
    # (the loop clips its start into the box: the initial design is the clipped one)
    start = tuple(np.clip(d, -box, box) for d in forward().geometry.get_design_from_rotated_square(25 * math.pi / 180))
    # the peak stretch strain of the initial design: utilisation against a limit of 1
    probe = P.PeakLigamentStrain(forward(), (1.0, None, None), beta=a.beta, **WATCHED)
    eps0, _ = utilisation(probe, start)
    eps_lim = a.fraction * eps0
    print(f"initial design: peak stretch strain {eps0:.4e}; limit {eps_lim:.4e}")
    kw = dict(lower_bound=-box, upper_bound=box, min_void_angle=0.0, min_block_angle=10 * math.pi / 180,
              min_edge_length=0.1 * SPACING, verbose=False)
    results = {}
    for name, limited in (("unconstrained", False), ("strain-limited", True)):
        objective = P.TargetKineticEnergy(forward(), (2, 2), (2, 0))
        limit = P.PeakLigamentStrain(forward(), (eps_lim, None, None), beta=a.beta, **WATCHED)
        problem = P.OptimizationProblem(objective, name=f"strain_limited_focusing ({name})")
        best = problem.run_optimization_nlopt(start, a.iterations, state_constraints=[limit] if limited else None, **kw)
        u, at = utilisation(limit, best)
        results[name] = (max(problem.objective_values), u)
        state = problem.constraints_violation.get("state", [])
        print(f"{name:15s}: kinetic energy in the target {problem.objective_values[0]:.5e} -> {float(objective.value_and_grad(best)[0]):.5e} in "
              f"{len(problem.objective_values)} evaluations; peak utilisation eps / eps_lim of the result {u:.4f} at (output, bond) {at}"
              + (f"; J - 1 along the way: {np.array2string(np.array(state), precision=3)}" if state else ""))
    print(f"peak utilisation: unconstrained {results['unconstrained'][1]:.4f}, strain-limited {results['strain-limited'][1]:.4f}")


if __name__ == "__main__":
    main()
