"""Wall time of one value-and-gradient of a signal misfit: the host path against the device path
(``dfx_signal_misfit_value_and_grad``: channels, residuals, the Hessian-vector product of the force terms and their explicit terms are
formed on the kept solve), on an MI355X.  Both share the forward solve and the reverse sweep.  Medians of 5 alternating rounds after one
warm-up each.

  * the hinge fit of examples/hinge_fit.py (three tests, 3 x 3 cells, 21 outputs): ``HingeResponseError.value_and_grad`` (history down,
    a second handle with one member per output time for the reaction forces and their vjp, cotangent up) against
    ``value_and_grad_device``;
  * the paper lattice (24 x 16 quads, 200 outputs, adaptive solve), 1 design and 32 designs: ``TargetSignalMisfit`` on tracked block
    motions (displacements of 8 blocks: the host path downloads the history and uploads a dense cotangent, one design per call; the device
    path runs the 32 as one ensemble), and -- device only, it has no host path -- the same lattice with reaction-force signals.

    python tools/signal_misfit_timing.py [--rows hinge,paper1,paper32] [--rounds 5] [--out profiles/r17_signal_misfit_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difflexmm_amd import objective as O  # noqa: E402
from difflexmm_amd import problems as P  # noqa: E402
from tools.objective_timing import designs_of, paper_forward  # noqa: E402


def alternate(run_host, run_dev, rounds):
    th, td = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        run_host()
        t1 = time.perf_counter()
        run_dev()
        t2 = time.perf_counter()
        th.append(t1 - t0)
        td.append(t2 - t1)
    return th, td


def row(name, th, td, moved, launches, agreement):
    mh, md = statistics.median(th), statistics.median(td)
    return (f"{name:46s} host {1e3 * mh:9.2f} ms (min {1e3 * min(th):.2f}, max {1e3 * max(th):.2f})   device {1e3 * md:9.2f} ms "
            f"(min {1e3 * min(td):.2f}, max {1e3 * max(td):.2f})   host / device {mh / md:5.2f}   PCIe bytes no longer moved per evaluation "
            f"{moved / 1e6:8.3f} MB   objective launches beside the sweep {launches}   agreement: {agreement}")


def hinge_row(rounds):
    from examples.hinge_fit import START, build_fit
    fit = build_fit()
    v, g = fit.value_and_grad(START)                   # warm-up
    vd, gd = fit.value_and_grad_device(START)
    e_v = abs(vd - v) / abs(v)
    e_g = max(abs(a - b) for a, b in zip(gd, g)) / max(abs(b) for b in g)
    th, td = alternate(lambda: fit.value_and_grad(START), lambda: fit.value_and_grad_device(START), rounds)
    p = fit.forward_problems[0]
    T, nb = p.n_timepoints, p.geometry.n_blocks
    # per test: history down, T states up and T accelerations down for the forces, the same again and a (T, ...) cotangent down for their
    # vjp, the cotangent of the sweep up
    moved = 3 * (2 * T * nb * 6 + 4 * T * nb * 6) * 8
    return row("hinge fit, 3 tests, 3 x 3 cells, 21 outputs", th, td, moved, "3 x 6 (host path: 3 x 2 calls on the second handle)",
               f"value {e_v:.1e}, gradient {e_g:.1e}")


def tracked(fw, n_designs, seed=3):
    """displacements x, y of 8 blocks spread over the lattice against targets of their own scale"""
    nb = fw.geometry.n_blocks
    blocks = np.linspace(nb // 5, nb - nb // 5, 8).astype(int)
    bd = [(int(b), d) for b in blocks for d in (0, 1)]
    rng = np.random.default_rng(seed)
    targets = 0.05 * rng.normal(size=(fw.n_timepoints, len(bd)))
    return O.SignalSpec.fields_of(bd, "displacement", targets)


def reaction(fw):
    """one signal: the x force summed over the driven blocks' neighbours' column (8 blocks of the second column)"""
    n1 = fw.n1_blocks
    bd = [(r * n1 + 1, 0) for r in range(4, 12)]
    rng = np.random.default_rng(4)
    return O.SignalSpec.force_sum(bd, 1.0, rng.normal(size=(fw.n_timepoints, 1)))


def paper_row(name, fw_host, fw_dev, n, rounds):
    host, dev = P.TargetSignalMisfit(fw_host, tracked(fw_host, n)), P.TargetSignalMisfit(fw_dev, tracked(fw_dev, n))
    designs = designs_of(fw_host, n)
    run_host = lambda: [host.value_and_grad(d) for d in designs]                                                    # noqa: E731
    run_dev = lambda: dev.value_and_grad(designs) if n > 1 else [dev.value_and_grad(designs[0], on_device=True)]      # noqa: E731
    rh, rd = run_host(), run_dev()
    vd = rd[0] if n > 1 else [rd[0][0]]
    gd = rd[1] if n > 1 else [rd[0][1]]
    e_v = max(abs(vd[m] - rh[m][0]) / max(abs(rh[m][0]), 1e-300) for m in range(n))
    e_g = max(np.abs(a - r).max() / max(np.abs(r).max(), 1e-300) for m in range(n) for a, r in zip(gd[m], rh[m][1]))
    th, td = alternate(run_host, run_dev, rounds)
    T, nb = fw_host.n_timepoints, fw_host.geometry.n_blocks
    out = [row(name + ", tracked motions", th, td, n * 2 * T * 2 * nb * 3 * 8, "3", f"value {e_v:.1e}, design gradient {e_g:.1e}")]
    force = P.TargetSignalMisfit(fw_dev, reaction(fw_dev))
    run_force = lambda: force.value_and_grad(designs) if n > 1 else force.value_and_grad(designs[0], on_device=True)  # noqa: E731
    run_force()
    tf = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        run_force()
        tf.append(time.perf_counter() - t0)
    out.append(f"{name + ', reaction-force signal':46s} host      (none)   device {1e3 * statistics.median(tf):9.2f} ms (min {1e3 * min(tf):.2f}, "
               f"max {1e3 * max(tf):.2f})   objective launches beside the sweep 6")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="hinge,paper1,paper32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = a.rows.split(",")
    lines = ["value-and-gradient of a signal misfit, wall time per evaluation of ALL designs / tests of the row: host path against device path; "
             f"medians of {a.rounds} alternating rounds after one warm-up"]
    if "hinge" in rows:
        lines.append(hinge_row(a.rounds))
    fw1 = None
    if "paper1" in rows or "paper32" in rows:
        fw1 = paper_forward(1)
        fw1.setup()
    if "paper1" in rows:
        lines += paper_row("24 x 16, 200 outputs, adaptive, 1 design", fw1, fw1, 1, a.rounds)
    if "paper32" in rows:
        fw32 = paper_forward(32)
        fw32.setup()
        lines += paper_row("24 x 16, 200 outputs, adaptive, 32 designs", fw1, fw32, 32, a.rounds)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
