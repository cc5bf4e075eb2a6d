"""What the sample gradients of a table drive cost the reverse sweep, on an MI355X: the device time of the sweep (HIP events around it,
``dfx_stats.kernel_ms``) with and without the request of ``dfx_fn_table_grads`` on the SAME kept solve, and what ran (``dfx_stats``
``tile_kernels``: 3 the persistent loop, 2 the per-stage builds, 0 the generic builds the request routes to).  The raw sweep asks for what a
design reaches (node vectors, void angles, inertia) plus the function parameters.  One more sweep per row runs with DFX_TIMING set: the
library then reports on stderr the device time of the reduction onto the samples alone (k_stage_times + k_table_grad behind the sweep).

  * chip: 128 x 128 quads x 32 members with contact (the shape of ``bench.py``), fixed grid of bench.py's step 1.333e-6 s;
  * paper: the 24 x 16 lattice x 1 and x 32 members, fixed grid -- without the request its sweep runs on the persistent loop.

    python tools/waveform_timing.py [--rows chip,paper1,paper32] [--steps 200] [--calls 5] [--samples 64] [--out profiles/waveform_gradient.txt]
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import loading as L  # noqa: E402
from difflexmm_amd import problems as P  # noqa: E402

WHICH = ("centroid_node_vectors", "void_angle0", "inertia", "fn_params")
SPACING, BOND_LENGTH, K_STRETCH, K_SHEAR, K_ROT, DENSITY, LOADING_RATE = 15.0, 2.25, 120.0, 1.19, 1.5, 6.18e-9, 30.0
DT = 4e-6 / 3          # the fixed step of bench.py's flagship workload


def forward(n1, n2, batch, outputs, steps, samples):
    damping = 0.0186 * np.array([2 * math.sqrt(0.36125 * DENSITY * SPACING ** 2 * K_SHEAR)] * 2 +
                                [2 * math.sqrt(0.02175026 * DENSITY * SPACING ** 4 * K_ROT)]) * np.ones((n1 * n2, 1))
    fw = P.QuadsFocusingForward(n1_blocks=n1, n2_blocks=n2, spacing=SPACING, bond_length=BOND_LENGTH, k_stretch=K_STRETCH, k_shear=K_SHEAR,
                                k_rot=K_ROT, density=DENSITY, damping=damping, use_contact=True, k_contact=K_ROT, min_angle=-15 * math.pi / 180,
                                cutoff_angle=-10 * math.pi / 180, amplitude=0.5 * SPACING, loading_rate=LOADING_RATE, input_delay=0.0,
                                n_excited_blocks=2, loaded_side="left", input_shift=0, simulation_time=steps * DT,
                                n_timepoints=outputs, steps_per_interval=max(1, steps // (outputs - 1)), batch=batch)
    times = np.linspace(0.0, 0.5 * steps * DT, samples)          # a raised cosine over the first half of the horizon
    fw.setup(excited_blocks_fn=L.Table(times, "waveform"))
    pulse = 0.005 * SPACING * (1.0 - np.cos(2 * np.pi * times / times[-1]))
    cp = fw.control_params(fw.geometry.get_design_from_rotated_square(25 * math.pi / 180))
    cp = cp._replace(constraint_params=dict(cp.constraint_params, waveform=pulse))
    return fw, cp


def row(name, n1, n2, batch, outputs, steps, samples, calls):
    fw, cp = forward(n1, n2, batch, outputs, steps, samples)
    s = fw.solve_dynamics
    s(fw.state0, fw.timepoints, [cp] * batch if batch > 1 else cp, keep_trajectory=True, want_fields=False)
    fb = np.zeros((batch, outputs, 2, n1 * n2, 3))
    fb[:, -1, 1] = 1.0
    out = {}
    for on in (False, True, False, True):
        s.engine.fn_table_grads(on)
        ms = []
        for _ in range(calls + 1):          # (the first: warm-up)
            st = s.engine.adjoint(fb, which=WHICH)[1]
            ms.append(st["kernel_ms"])
        out.setdefault(on, []).append((statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]), st["tile_kernels"], st["launches"]))
    sys.stderr.write(f"{name}: ")
    sys.stderr.flush()
    os.environ["DFX_TIMING"] = "1"
    s.engine.adjoint(fb, which=WHICH)
    del os.environ["DFX_TIMING"]
    off, req = out[False], out[True]
    fmt = lambda r: f"{r[0]:9.3f} ms (min {r[1]:.3f}, max {r[2]:.3f}; tile_kernels {r[3]}, {r[4]} launches)"      # noqa: E731
    steps_run = max(1, steps // (outputs - 1)) * (outputs - 1)
    return (f"{name:34s} {steps_run} steps, {samples} samples\n"
            f"    without the request   {fmt(off[0])}   again {fmt(off[1])}\n"
            f"    with the request      {fmt(req[0])}   again {fmt(req[1])}\n"
            f"    ratio (medians of the second pair) {req[1][0] / off[1][0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="chip,paper1,paper32")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = a.rows.split(",")
    lines = [f"reverse sweep on one kept solve, want = {WHICH}: device time between the HIP events around the sweep (dfx_stats.kernel_ms), medians "
             f"of {a.calls} sweeps; the request is switched off, on, off, on"]
    if "chip" in rows:
        lines.append(row("128 x 128 quads x 32 members", 128, 128, 32, 5, a.steps, a.samples, a.calls))
    if "paper1" in rows:
        lines.append(row("24 x 16 quads x 1 member", 24, 16, 1, 5, a.steps, a.samples, a.calls))
    if "paper32" in rows:
        lines.append(row("24 x 16 quads x 32 members", 24, 16, 32, 5, a.steps, a.samples, a.calls))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
