"""Time of one value-and-gradient of the signal-projection objective (``dfx_signal_projection_value_and_grad``) against the signal misfit
(``dfx_signal_misfit_value_and_grad``) on the SAME kept solve, on an MI355X: the paper lattice (24 x 16 quads, 200 outputs, adaptive
solve), 1 design and 32 designs, 8 velocity signals, 6 basis rows (cos / sin at the drive frequency, at twice it and at 0.59 of it).
Both calls share everything behind the cotangent on the signals -- the reverse sweep above all; the projection adds two small launches
(the time reduction, the cotangent from the coefficients).  The question: is the difference within the run-to-run spread of the misfit call?

The calls are host-synchronous (they return once the gradients are in host-visible memory); each is bracketed by HIP events recorded on
an otherwise idle stream, which complete as soon as they are recorded: their device timestamps bracket the whole call, launches, sweep
and the waits of the host included (the engine's own streams are non-blocking, no event can be put on them from here).  The two calls
alternate; warm-up rounds are discarded; medians of ``--rounds`` (at least 20).

    python tools/projection_timing.py [--designs 1,32] [--rounds 20] [--out profiles/r20_signal_projection_timing.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import objective as O  # noqa: E402
from tools.objective_timing import designs_of, paper_forward  # noqa: E402

WARMUP = 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)                      # ms


def specs(fw, seed=5):
    nb, T = fw.geometry.n_blocks, fw.n_timepoints
    blocks = np.linspace(nb // 5, nb - nb // 5, 8).astype(int)
    rng = np.random.default_rng(seed)
    bd = [(int(b), 0) for b in blocks]
    misfit = O.SignalSpec.fields_of(bd, "velocity", rng.normal(size=(T, 8)), omega=rng.uniform(0.5, 2.0, 8), tau=rng.uniform(0.5, 2.0, T))
    f0 = fw.loading_rate
    basis = O.fourier_basis(fw.timepoints, [f0, 2 * f0, 0.59 * f0], window="hann")
    proj = O.ProjectionSpec(O.SignalSpec.fields_of(bd, "velocity"), basis, rng.uniform(-1.0, 2.0, (8, 6)), rng.normal(size=(8, 6)) * 1e-3)
    return misfit, proj


def measure(n, rounds):
    fw = paper_forward(n)
    fw.setup()
    misfit, proj = specs(fw)
    designs = designs_of(fw, n)
    fw.solve(designs if n > 1 else designs[0], keep_trajectory=True, want_fields=False)
    sd = fw.solve_dynamics
    run_m = lambda: sd.signal_misfit_value_and_raw(misfit)          # noqa: E731
    run_p = lambda: sd.signal_projection_value_and_raw(proj)        # noqa: E731
    tm, tp = [], []
    for r in range(WARMUP + rounds):
        a, b = timed(run_m), timed(run_p)
        if r >= WARMUP:
            tm.append(a)
            tp.append(b)
    mm, mp = statistics.median(tm), statistics.median(tp)
    q = lambda t: (sorted(t)[len(t) // 4], sorted(t)[(3 * len(t)) // 4])        # noqa: E731
    return (f"24 x 16, 200 outputs, adaptive, {n:2d} design(s): misfit {mm:8.3f} ms (min {min(tm):.3f}, quartiles {q(tm)[0]:.3f} .. {q(tm)[1]:.3f}, "
            f"max {max(tm):.3f})   projection {mp:8.3f} ms (min {min(tp):.3f}, quartiles {q(tp)[0]:.3f} .. {q(tp)[1]:.3f}, max {max(tp):.3f})   "
            f"projection - misfit {mp - mm:+.3f} ms = {100 * (mp - mm) / mm:+.2f} %   interquartile range of the misfit call "
            f"{q(tm)[1] - q(tm)[0]:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--designs", default="1,32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rounds = max(20, a.rounds)
    lines = ["value-and-gradient on one kept solve, HIP-event time per call: dfx_signal_misfit_value_and_grad against "
             f"dfx_signal_projection_value_and_grad (8 signals, 6 rows); alternating, {WARMUP} warm-up rounds discarded, medians of {rounds}"]
    for n in (int(x) for x in a.designs.split(",")):
        lines.append(measure(n, rounds))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
