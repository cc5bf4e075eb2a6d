"""Time of one value-and-gradient of the spectral-ratio objective (``dfx_signal_spectrum_value_and_grad``) against the signal projections
(``dfx_signal_projection_value_and_grad``, the yardstick: its code is not the code under test) on the SAME kept solve, on an MI355X: the
paper lattice (24 x 16 quads, 200 outputs, adaptive solve), 1 design and 32 designs, 8 velocity signals, 6 basis rows, G = 3 and 64 groups.
Both calls share everything behind the cotangent on the signals -- the reverse sweep above all; the spectrum replaces the value finish by the
forms and the reduction and adds the effective-weight launch.  The value-only columns (no sweep) give the cost of those launches on the
machine.  The question: is the difference within the interquartile range of the projection call?

Timed as tools/projection_timing.py times: HIP events on an otherwise idle stream around the host-synchronous calls, the calls
alternating, warm-up rounds discarded, medians of ``--rounds`` (at least 20).

    python tools/spectrum_timing.py [--designs 1,32] [--rounds 20] [--out profiles/spectrum_timing.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import objective as O  # noqa: E402
from tools.objective_timing import designs_of, paper_forward  # noqa: E402
from tools.projection_timing import WARMUP, timed  # noqa: E402


def specs(fw, seed=5):
    nb = fw.geometry.n_blocks
    blocks = np.linspace(nb // 5, nb - nb // 5, 8).astype(int)
    rng = np.random.default_rng(seed)
    sig = O.SignalSpec.fields_of([(int(b), 0) for b in blocks], "velocity")
    f0 = fw.loading_rate
    basis = O.fourier_basis(fw.timepoints, [f0, 2 * f0, 0.59 * f0], window="hann")
    proj = O.ProjectionSpec(sig, basis, rng.uniform(-1.0, 2.0, (8, 6)), rng.normal(size=(8, 6)) * 1e-3)
    out = {}
    for G in (3, 64):
        wn, wd = rng.uniform(0.0, 2.0, (G, 8, 6)), rng.uniform(0.0, 2.0, (G, 8, 6))
        wn[:, :4], wd[:, 4:] = 0.0, 0.0                         # the last four signals over the first four
        out[G] = O.SpectrumSpec(sig, basis, wn, wd, None, None, rng.uniform(-1.0, 1.0, G), "log", "ks", 2.0)
    return proj, out


def measure(n, rounds):
    fw = paper_forward(n)
    fw.setup()
    proj, spectra = specs(fw)
    designs = designs_of(fw, n)
    fw.solve(designs if n > 1 else designs[0], keep_trajectory=True, want_fields=False)
    sd = fw.solve_dynamics
    runs = {"projection": lambda: sd.signal_projection_value_and_raw(proj), "projection value": lambda: sd.signal_projection_value(proj)}
    for G, sp in spectra.items():
        runs[f"spectrum G={G}"] = lambda sp=sp: sd.signal_spectrum_value_and_raw(sp)
        runs[f"spectrum G={G} value"] = lambda sp=sp: sd.signal_spectrum_value(sp)
    t = {k: [] for k in runs}
    for r in range(WARMUP + rounds):
        for k, fn in runs.items():
            ms = timed(fn)
            if r >= WARMUP:
                t[k].append(ms)
    med = {k: statistics.median(v) for k, v in t.items()}
    q = sorted(t["projection"])
    iqr = q[(3 * len(q)) // 4] - q[len(q) // 4]
    lines = [f"24 x 16, 200 outputs, adaptive, {n:2d} design(s): projection {med['projection']:8.3f} ms (interquartile range {iqr:.3f} ms), "
             f"value only {med['projection value']:.3f} ms"]
    for G in spectra:
        d = med[f"spectrum G={G}"] - med["projection"]
        dv = med[f"spectrum G={G} value"] - med["projection value"]
        lines.append(f"    spectrum G = {G:2d}: {med[f'spectrum G={G}']:8.3f} ms, spectrum - projection {d:+.3f} ms = {100 * d / med['projection']:+.2f} %; "
                     f"value only {med[f'spectrum G={G} value']:.3f} ms, spectrum - projection {dv:+.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--designs", default="1,32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rounds = max(20, a.rounds)
    lines = ["value-and-gradient on one kept solve, HIP-event time per call: dfx_signal_projection_value_and_grad against "
             f"dfx_signal_spectrum_value_and_grad (8 signals, 6 rows, log / KS); alternating, {WARMUP} warm-up rounds discarded, medians of {rounds}"]
    for n in (int(x) for x in a.designs.split(",")):
        lines += measure(n, rounds)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
