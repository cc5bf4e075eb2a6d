"""A band gap in a design loop: minimise the worst-case transmission over a band of frequencies on a small quad lattice
(``problems.TargetTransmission(worst_case=True)``: per frequency the log ratio of the band power of the displacements on the far edge to
that on the driven edge, their KS smooth maximum over the band -- ``dfx_signal_spectrum_value_and_grad``; the history never leaves the
device).  A pulse on the left edge, displacement signals on both sides, a few evaluations of the method of moving asymptotes between bounds
on the design; the dB spectrum over the band is printed before and after.

    python examples/band_gap.py [--evaluations 6] [--n1 8] [--n2 6] [--outputs 60]
    python examples/band_gap.py --cpu-port            # rehearsal without a GPU (host path)
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difflexmm_amd import problems as P  # noqa: E402
from difflexmm_amd.optimize import mma_minimize  # noqa: E402

SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY, LOADING_RATE = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9, 30.0
DB = 10.0 / math.log(10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=8)
    ap.add_argument("--n2", type=int, default=6)
    ap.add_argument("--outputs", type=int, default=60)
    ap.add_argument("--evaluations", type=int, default=6)
    ap.add_argument("--cpu-port", action="store_true", help="the CPU port of the oracle (host path only)")
    a = ap.parse_args()
    lib = None
    if a.cpu_port:
        from oracle.cpu import load
        lib = load()
    nb = a.n1 * a.n2
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                                [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((nb, 1))
    fw = P.QuadsFocusingForward(n1_blocks=a.n1, n2_blocks=a.n2, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, use_contact=True, k_contact=K_ROT, min_angle=-15 * math.pi / 180,
                                cutoff_angle=-10 * math.pi / 180, amplitude=0.5 * SPACING, loading_rate=LOADING_RATE,
                                input_delay=0.1 / LOADING_RATE, n_excited_blocks=2, loaded_side="left", input_shift=0,
                                simulation_time=2 / LOADING_RATE, n_timepoints=a.outputs, atol=1e-4, rtol=1e-8, _lib=lib)
    fw.setup()
    # displacement x of the second column (behind the driven edge) in, of the last column out; the band around the drive frequency
    rows = range(1, a.n2 - 1)
    inside, outside = [(r * a.n1 + 1, 0) for r in rows], [(r * a.n1 + a.n1 - 1, 0) for r in rows]
    band = LOADING_RATE * np.array([0.75, 1.0, 1.25, 1.5])
    spread = 2.0                                                 # the transmissions of the start design differ by about this much (in l)
    objective = P.TargetTransmission(fw, inside, outside, "displacement", band, window="hann", worst_case=True, beta=10.0 / spread)
    geo = fw.geometry
    start = geo.get_design_from_rotated_square(25 * math.pi / 180)
    x0 = P._flatten_design(start)
    history = []

    def fun(x):
        v, g = objective.value_and_grad(P._unflatten_design(geo, x), on_device=not a.cpu_port)
        history.append((v, np.array(objective.last_measures, dtype=float).reshape(-1)))
        print(f"evaluation {len(history)}: worst-case transmission (KS) {DB * v:+.3f} dB")
        return v, P._flatten_design(g)

    mma_minimize(fun, x0, lower=x0 - 0.1 * SPACING, upper=x0 + 0.1 * SPACING, maxeval=a.evaluations)
    best = min(range(len(history)), key=lambda i: history[i][0])
    print("frequency [Hz]   transmission before [dB]   after [dB]")
    for f, l0, l1 in zip(band, history[0][1], history[best][1]):
        print(f"{f:14.2f}   {DB * l0:+24.3f}   {DB * l1:+10.3f}")
    print(f"worst in-band transmission: {DB * history[0][1].max():+.3f} dB -> {DB * history[best][1].max():+.3f} dB "
          f"(KS value {DB * history[0][0]:+.3f} -> {DB * history[best][0]:+.3f} dB) in {len(history)} evaluations")


if __name__ == "__main__":
    main()
