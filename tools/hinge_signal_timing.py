"""Wall time of a signal value-and-gradient with HINGE terms beside the same call with BLOCK-FORCE terms on the same blocks, on ONE kept
solve each, on an MI355X: the paper lattice (24 x 16 quads, 200 outputs, adaptive solve), 1 design and 32 designs.  The cut is the
boundary of the 4 x 4 target region in the middle of the lattice (``objective.bonds_across``: 16 hinges on 12 blocks).

  hinge   the misfit of ``problems.TargetTransmittedForce`` (the resultant through the cut, x and y, zero targets) and the value of
          ``problems.TargetCutEnergy`` (48 hinge-force signals against 48 velocities, lag 0)
  block   the yardstick, whose code the hinge channels left as it was: ``SignalSpec.force_sum`` per dof on the blocks that own those
          hinges, as a misfit on zero targets

Both run the same reverse sweep with the same ``want`` (the raw gradients a design reaches); the hinge call adds one launch for the hinge
channels and seeds fewer ligaments in the cotangent.  The value-only entries isolate what runs in front of the sweep.  Medians of 5 calls
after one warm-up each.  There is no bar: this is a record.

    python tools/hinge_signal_timing.py [--batches 1,32] [--calls 5] [--out profiles/r24_hinge_signal_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import objective as O  # noqa: E402
from difflexmm_amd import problems as P  # noqa: E402
from tools.objective_timing import designs_of, paper_forward  # noqa: E402
from tools.peak_strain_timing import median_ms  # noqa: E402

WHICH = ("centroid_node_vectors", "void_angle0", "inertia")


def row(batch, calls):
    fw = paper_forward(batch)
    fw.setup()
    designs = designs_of(fw, batch)
    fw.solve(designs if batch > 1 else designs[0], keep_trajectory=True, want_fields=False)
    sd = fw.solve_dynamics
    inside = P.quads_target_blocks(fw.geometry, (4, 4), (0, 0))
    T = len(fw.timepoints)
    force = P.TargetTransmittedForce(fw, inside).spec
    energy = P.TargetCutEnergy(fw, inside)
    blocks = sorted({b for b, _ in energy.hinges})
    block = O.SignalSpec([(d, b, O.FORCE + d, 1.0) for d in (0, 1) for b in blocks], 2, np.zeros((T, 2)))
    t_h = median_ms(lambda: sd.signal_misfit_value_and_raw(force, which=WHICH), calls)
    t_b = median_ms(lambda: sd.signal_misfit_value_and_raw(block, which=WHICH), calls)
    t_e = median_ms(lambda: sd.signal_xcorr_value_and_raw(energy.spec, which=WHICH), calls)
    v_h = median_ms(lambda: sd.signal_misfit_value(force), calls)
    v_b = median_ms(lambda: sd.signal_misfit_value(block), calls)
    v_e = median_ms(lambda: sd.signal_xcorr_value(energy.spec), calls)
    name = f"24 x 16, 200 outputs, adaptive, {batch} design{'s' if batch > 1 else ''}, {len(energy.hinges)} hinges on {len(blocks)} blocks"
    return (f"{name:72s} block force {t_b[0]:8.2f} ms (min {t_b[1]:.2f}, max {t_b[2]:.2f})   cut force {t_h[0]:8.2f} ms (min {t_h[1]:.2f}, max "
            f"{t_h[2]:.2f})   cut energy {t_e[0]:8.2f} ms (min {t_e[1]:.2f}, max {t_e[2]:.2f})   cut force / block force {t_h[0] / t_b[0]:5.2f}   "
            f"value only: block force {v_b[0]:6.2f} ms, cut force {v_h[0]:6.2f} ms, cut energy {v_e[0]:6.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["signal value-and-gradient with hinge terms (the resultant through a cut; the energy through it) beside the same misfit with block-force "
             f"terms on the blocks that own the hinges, on one kept solve: want = {WHICH}; wall time per call, medians of {a.calls} calls after one warm-up"]
    lines += [row(int(b), a.calls) for b in a.batches.split(",")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
