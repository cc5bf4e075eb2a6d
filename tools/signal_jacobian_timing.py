"""What one Jacobian evaluation of a least-squares fit over K = 3 scalar leaves (k_stretch, k_shear, k_rot) costs, two ways:
  (host)    the route before the forward-mode signal entries: DynamicSolver.jacfwd downloads fields and K tangent histories and
            objective.host_signal_values reads the field terms out of them; for the reaction force of the hinge samples
            hinge.force_jacobian's host path on top (a second handle, the history uploaded again, dfx_rhs_jvp);
  (device)  DynamicSolver.signal_jacfwd (dfx_forward_tangent_signals_multi): channels, signals and their tangents formed at the end of every
            pass on the device, (1 + K) x T x n_signals numbers downloaded;
on three shapes: the three hinge samples (2 x 2 cells, 9 outputs, the reaction force), the paper's lattice (24 x 16 quads, contact, damping,
200 outputs, four tracked displacements) and one 128 x 128 design with 200 outputs.  Per shape: one warm-up round, then --reps rounds in
which the two routes alternate; printed are the median and the spread (min .. max) of the wall time and of stats["kernel_ms"] (device
time of the pass, HIP events), the bytes each route moves over PCIe for its results (counted from the shapes), and the largest relative
difference of the two Jacobians in the warm-up round.  Every shape runs in a child process of its own under a time limit; a child that
fails ends the run.
    python tools/signal_jacobian_timing.py [--reps 5] >> profiles/r21_signal_tangent.txt"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tools"))

NAMES = ["k_stretch", "k_shear", "k_rot"]
CASES = {"hinge": 240, "paper": 240, "128x128": 420}          # time limit of each child, seconds


def line(label, xs):
    xs = np.sort(np.asarray(xs, dtype=float))
    return f"{label} median {np.median(xs):9.3f}  (min {xs[0]:9.3f} .. max {xs[-1]:9.3f})"


def report(tag, host, device, bytes_host, bytes_device, gap):
    print(f"== {tag} ==")
    for name, (wall, kern) in (("host  ", host), ("device", device)):
        print(f"  {name} wall ms   {line('', wall)}")
        print(f"  {name} kernel ms {line('', kern)}")
    print(f"  PCIe bytes for the results: host {bytes_host:,}  device {bytes_device:,}  ({bytes_host / max(bytes_device, 1):.0f} x)")
    print(f"  wall: device / host = {np.median(device[0]) / np.median(host[0]):.3f}   largest relative difference of the Jacobians: {gap:.2e}", flush=True)


def run_lattice(n1, n2, outputs, reps):
    from tangent_timing import quads_problem
    from difflexmm_amd import objective as O
    s, cps, _ = quads_problem(n1, n2, 1)
    cp = cps[0]
    nb = n1 * n2
    ts = np.linspace(0.0, 0.5 / 30.0, outputs)
    y0 = np.zeros((2, nb, 3))
    mid = (n2 // 2) * n1
    spec = O.SignalSpec.fields_of([(mid + n1 // 4, 0), (mid + n1 // 2, 0), (mid + n1 // 2, 2), (mid + 3 * n1 // 4, 1)], "displacement")
    host, device, gap = ([], []), ([], []), 0.0
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        f, cols = s.jacfwd(y0, ts, cp, NAMES, steps_per_interval=2)
        Jh = np.stack([O.host_signal_values(spec, cols[n]) for n in NAMES])
        w_h, k_h = time.perf_counter() - t0, s.stats["kernel_ms"]
        t0 = time.perf_counter()
        S, dcols = s.signal_jacfwd(y0, ts, cp, NAMES, spec, steps_per_interval=2)
        Jd = np.stack([dcols[n] for n in NAMES])
        w_d, k_d = time.perf_counter() - t0, s.stats["kernel_ms"]
        if rep == 0:
            gap = float(np.abs(Jd - Jh).max() / np.abs(Jh).max())
            continue
        host[0].append(1e3 * w_h), host[1].append(k_h), device[0].append(1e3 * w_d), device[1].append(k_d)
    K = len(NAMES)
    report(f"{n1} x {n2} quads, 1 design, {outputs} outputs, {2 * (outputs - 1)} dopri5 steps, K = {K}, {spec.n_signals} displacement signals, {reps} rounds",
           host, device, (1 + K) * outputs * nb * 6 * 8, (1 + K) * outputs * spec.n_signals * 8 + 4 * 1024, gap)


def run_hinge(reps):
    sys.path.insert(0, os.path.join(root, "examples"))
    from hinge_fit import TRUTH, build_fit
    fit = build_fit(cells=2, timepoints=9)
    host, device, gap = ([], []), ([], []), 0.0
    for rep in range(reps + 1):
        out = {}
        for on_device, acc in ((False, host), (True, device)):
            t0, kern, J = time.perf_counter(), 0.0, []
            for p in fit.forward_problems:
                J.append(p.force_jacobian(TRUTH, on_device=on_device)[1])
                kern += p.solve_dynamics.stats["kernel_ms"]
            out[on_device] = np.concatenate(J)
            if rep:
                acc[0].append(1e3 * (time.perf_counter() - t0)), acc[1].append(kern)
        if rep == 0:
            gap = float(np.abs(out[True] - out[False]).max() / np.abs(out[False]).max())
    p = fit.forward_problems[0]
    nb, T, K = p.geometry.n_blocks, p.n_timepoints, 3
    hist = (1 + K) * T * nb * 6 * 8
    report(f"hinge samples: 3 tests of {nb} blocks, {T} outputs, adaptive solve, K = {K}, the reaction force, {reps} rounds (kernel ms: the tangent passes only)",
           host, device, 3 * (hist + hist + (1 + K) * T * nb * 6 * 8), 3 * ((1 + K) * T * 8 + 4 * 1024), gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=list(CASES))
    a = ap.parse_args()
    if a.case == "hinge":
        return run_hinge(a.reps)
    if a.case == "paper":
        return run_lattice(24, 16, 200, a.reps)
    if a.case == "128x128":
        return run_lattice(128, 128, 200, a.reps)
    for case, limit in CASES.items():
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)]).returncode
        if rc:
            print(f"{case}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
