"""Wall time of one value-and-gradient of the energy-splitting objective (``SplitTargetKineticEnergy``): the host path (history
downloaded, cotangent built in NumPy and uploaded through ``dfx_adjoint``, one design per call) against the device path
(``dfx_objective_value_and_grad``: the history stays in HBM, a list of designs is one ensemble), on an MI355X.  Both share the forward
solve and the reverse sweep.  Medians of 5 alternating rounds after one warm-up each.

  * the paper lattice of the energy-splitting notebook (24 x 16 quads, 200 outputs, adaptive solve), 1 design and 32 designs (the
    host path runs the 32 one after the other);
  * 128 x 128 quads, 4 designs, 201 outputs on the fixed grid of the flagship benchmark (its step size; --spi steps per output).

    python tools/objective_timing.py [--rows paper1,paper32,big] [--rounds 5] [--spi 5] [--out profiles/r12_device_objectives.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import problems as P  # noqa: E402

WEIGHTS = (0.599, 0.401)
SIZES, SHIFTS = ((2, 2), (2, 2)), ((5, 3), (-3, -3))


def paper_forward(batch):
    from tests import notebook_kat as K
    return P.QuadsFocusingForward(n1_blocks=K.N1, n2_blocks=K.N2, spacing=K.SPACING, bond_length=K.HINGE, k_stretch=K.K_STRETCH, k_shear=K.K_SHEAR,
                                  k_rot=K.K_ROT, density=K.DENSITY, damping=K.damping(), use_contact=True, k_contact=K.K_ROT,
                                  min_angle=-15 * np.pi / 180, cutoff_angle=-10 * np.pi / 180, amplitude=0.5 * K.SPACING,
                                  loading_rate=K.LOADING_RATE, input_delay=0.1 / K.LOADING_RATE, n_excited_blocks=2, loaded_side="left",
                                  input_shift=0, simulation_time=2 / K.LOADING_RATE, n_timepoints=200, atol=1e-4, rtol=1e-8, batch=batch)


def big_forward(batch, spi, size=128):
    spacing, rho, ksh, kr, freq = 15.0, 6.18e-9, 1.19, 1.5, 30.0
    dt = (2.0 / freq) / 50000.0                    # the flagship benchmark's step
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * rho * spacing ** 2 * ksh)] * 2 +
                                [2 * math.sqrt(0.02175026 * rho * spacing ** 4 * kr)]) * np.ones((size * size, 1))
    return P.QuadsFocusingForward(n1_blocks=size, n2_blocks=size, spacing=spacing, bond_length=2.25, k_stretch=120.0, k_shear=ksh, k_rot=kr,
                                  density=rho, damping=damping, amplitude=7.5, loading_rate=freq, input_delay=0.0, n_excited_blocks=2,
                                  loaded_side="left", input_shift=0, simulation_time=200 * spi * dt, n_timepoints=201, use_contact=True,
                                  k_contact=1.5, min_angle=-15 * math.pi / 180, cutoff_angle=-10 * math.pi / 180, steps_per_interval=spi,
                                  batch=batch)


def designs_of(fw, n, seed=0):
    base = fw.geometry.get_design_from_rotated_square(25 * math.pi / 180)
    out = []
    for m in range(n):
        rng = np.random.default_rng(seed + m)
        out.append(tuple(b + rng.uniform(-0.3, 0.3, b.shape) for b in base))
    return out


def measure(name, fw_host, fw_dev, n, rounds, sizes=SIZES, shifts=SHIFTS):
    host, dev = P.SplitTargetKineticEnergy(fw_host, sizes, shifts, WEIGHTS), P.SplitTargetKineticEnergy(fw_dev, sizes, shifts, WEIGHTS)
    designs = designs_of(fw_host, n)

    def run_host():
        return [host.value_and_grad(d) for d in designs]

    def run_dev():
        return dev.value_and_grad(designs) if n > 1 else [dev.value_and_grad(designs[0], on_device=True)]
    rh, rd = run_host(), run_dev()                 # warm-up: allocations, graphs
    vd = rd[0] if n > 1 else [rd[0][0]]
    gd = rd[1] if n > 1 else [rd[0][1]]
    e_v = max(abs(vd[m] - rh[m][0]) / max(abs(rh[m][0]), 1e-300) for m in range(n))
    e_g = max(np.abs(a - r).max() / max(np.abs(r).max(), 1e-300) for m in range(n) for a, r in zip(gd[m], rh[m][1]))
    th, td = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        run_host()
        t1 = time.perf_counter()
        run_dev()
        t2 = time.perf_counter()
        th.append(t1 - t0)
        td.append(t2 - t1)
    T, nb = fw_host.n_timepoints, fw_host.geometry.n_blocks
    moved = 2 * T * 2 * nb * 3 * 8                 # history down + cotangent up, per design
    mh, md = statistics.median(th), statistics.median(td)
    return (f"{name:38s} host {1e3 * mh:9.2f} ms (min {1e3 * min(th):.2f}, max {1e3 * max(th):.2f})   device {1e3 * md:9.2f} ms "
            f"(min {1e3 * min(td):.2f}, max {1e3 * max(td):.2f})   host / device {mh / md:5.2f}   PCIe bytes no longer moved per evaluation "
            f"{n * moved / 1e6:8.2f} MB   agreement: value {e_v:.1e}, design gradient {e_g:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="paper1,paper32,big")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spi", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = a.rows.split(",")
    lines = ["value-and-gradient of the energy-splitting objective, wall time per evaluation of ALL designs of the row: host path (one design "
             f"per call) against device path (one ensemble); medians of {a.rounds} alternating rounds after one warm-up"]
    fw1 = None
    if "paper1" in rows or "paper32" in rows:
        fw1 = paper_forward(1)
        fw1.setup()
    if "paper1" in rows:
        lines.append(measure("24 x 16, 200 outputs, adaptive, 1 design", fw1, fw1, 1, a.rounds))
    if "paper32" in rows:
        fw32 = paper_forward(32)
        fw32.setup()
        lines.append(measure("24 x 16, 200 outputs, adaptive, 32 designs", fw1, fw32, 32, a.rounds))
    if "big" in rows:
        fb1, fb4 = big_forward(1, a.spi), big_forward(4, a.spi)
        fb1.setup()
        fb4.setup()
        lines.append(measure(f"128 x 128, 201 outputs, {200 * a.spi} fixed steps, 4 designs", fb1, fb4, 4, a.rounds,
                             sizes=((2, 2), (2, 2)), shifts=((-62, 0), (-60, 3))))      # (next to the driven blocks: the wave gets there)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
