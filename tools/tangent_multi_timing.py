"""What K tangent directions cost: DynamicSolver.jvp_multi (dfx_forward_tangent_multi) --
  (a)  as the library runs it: passes of the widest chunk (the primal once per stage, 4 epsilon parts per lane), or, where batch x blocks
       x K lanes do not fill the chip, all directions spread over lanes in one pass (width 1);
  (a') the chunked form forced (DFX_TANGENT_MULTI_FORM=chunked), to show what the choice is worth;
against the two ways K directions were had before it --
  (b1) K calls of DynamicSolver.jvp on the same solver: K passes of width 1 (jvp is jvp_multi along one direction; in
       profiles/r09_tangent_multi.txt it was still a single-direction kernel of its own);
  (b2) one jvp on a solver of batch x K members, every design replicated K times (where batch x K <= --max-members, default 64: the host
       side of wider replicated ensembles takes longer than the measurement is worth)
-- on tools/tangent_timing.py's two configurations:
  * 128 x 128 quads with angle contact, 16 members, 250 dopri5 steps;
  * the paper's lattice (24 x 16 quads, contact, damping), 1 member, 250 steps,
for K = 1, 2, 4, 8.  Every figure is device time of the stage launches (HIP events, stats["kernel_ms"]; for (b1) the sum over the K
calls): one warm-up round, then --reps rounds (default 5) in which the three forms ALTERNATE; printed are the median and the spread
(min .. max) of ms per step, the median in ns per (member . direction . step), and the ratios of the medians (a) / min(b1, b2) and
(a') / min(b1, b2).
The columns of (a) are compared with (b1)'s in the warm-up round (max relative difference printed).
    python tools/tangent_multi_timing.py [--reps 5] [--small] > profiles/r09_tangent_multi.txt"""
import os
import sys
import time

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tools"))

from tangent_timing import quads_problem                     # noqa: E402

import difflexmm_amd as dm                                   # noqa: E402


def directions(cps, dots, K, seed=1):
    """K directions per member: member m's direction of tangent_timing.py, its leaves rescaled per direction (all of them dense)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        trees = []
        for cp, d in zip(cps, dots):
            g = d.geometrical_params.centroid_node_vectors
            bp = d.mechanical_params.bond_params
            trees.append(d._replace(
                geometrical_params=dm.GeometricalParams(None, g * (1.0 + 0.25 * k) + 0.002 * rng.normal(size=g.shape)),
                mechanical_params=d.mechanical_params._replace(bond_params=bp._replace(k_stretch=bp.k_stretch * (1.0 - 0.1 * k))),
                constraint_params=dict(amplitude=1.0 + k)))
        out.append(trees)
    return out            # [direction][member]


def stats_line(xs):
    xs = np.sort(np.asarray(xs))
    return float(np.median(xs)), float(xs[0]), float(xs[-1])


def time_case(label, n1, n2, batch, steps, Ks, reps, max_members):
    s, cps, dots = quads_problem(n1, n2, batch)
    ts = np.array([0.0, 0.5 / 30.0])
    y0 = np.zeros((batch, 2, n1 * n2, 3))
    print(f"== {label}: {n1 * n2} blocks x {batch} members, {steps} dopri5 steps, {reps} timed rounds after one warm-up ==")
    for K in Ks:
        dirs = directions(cps, dots, K)
        tangents = [(None, trees) for trees in dirs]
        wide = None
        if batch * K <= max_members and K > 1:
            wide, _, _ = quads_problem(n1, n2, batch * K)
            wide_cps = [cp for cp in cps for _ in range(K)]                      # member m * K + k = design m, direction k
            wide_dots = [dirs[k][m] for m in range(batch) for k in range(K)]
            y0w = np.zeros((batch * K, 2, n1 * n2, 3))
        rows = {"a": [], "ac": [], "b1": [], "b2": []}
        walls = {"a": [], "ac": [], "b1": [], "b2": []}
        for rep in range(reps + 1):
            os.environ.pop("DFX_TANGENT_MULTI_FORM", None)
            t0 = time.perf_counter()
            _, fd_a = s.jvp_multi(y0, ts, cps, tangents, steps_per_interval=steps)
            w_a, ms_a, launches_a = time.perf_counter() - t0, s.stats["kernel_ms"], s.stats["launches"]
            os.environ["DFX_TANGENT_MULTI_FORM"] = "chunked"
            t0 = time.perf_counter()
            _, fd_ac = s.jvp_multi(y0, ts, cps, tangents, steps_per_interval=steps)
            w_ac, ms_ac, launches_ac = time.perf_counter() - t0, s.stats["kernel_ms"], s.stats["launches"]
            os.environ.pop("DFX_TANGENT_MULTI_FORM", None)
            ms_b1, w_b1, worst = 0.0, 0.0, 0.0
            for k in range(K):
                t0 = time.perf_counter()
                _, fd1 = s.jvp(y0, ts, cps, None, dirs[k], steps_per_interval=steps)
                w_b1 += time.perf_counter() - t0
                ms_b1 += s.stats["kernel_ms"]
                if rep == 0:
                    worst = max(worst, float(np.abs(fd_a[:, k] - fd1).max() / np.abs(fd1).max()),
                                float(np.abs(fd_ac[:, k] - fd1).max() / np.abs(fd1).max()))
            if wide is not None:
                t0 = time.perf_counter()
                _, fdw = wide.jvp(y0w, ts, wide_cps, None, wide_dots, steps_per_interval=steps)
                w_b2, ms_b2 = time.perf_counter() - t0, wide.stats["kernel_ms"]
            if rep == 0:
                assert np.all(np.isfinite(fd_a)) and np.abs(fd_a[:, :, -1]).max() > 0
                print(f"   K = {K}: columns of jvp_multi (both forms) against K jvp calls: max relative difference {worst:.2e}; launches: (a) {launches_a}"
                      f"{' (spread: one pass)' if launches_a < launches_ac else ''}, (a') {launches_ac}")
                continue
            rows["a"].append(ms_a / steps); walls["a"].append(w_a)
            rows["ac"].append(ms_ac / steps); walls["ac"].append(w_ac)
            rows["b1"].append(ms_b1 / steps); walls["b1"].append(w_b1)
            if wide is not None:
                rows["b2"].append(ms_b2 / steps); walls["b2"].append(w_b2)
        per = 1e6 / (batch * K)
        med = {}
        for key, name in (("a", "(a)  jvp_multi"), ("ac", "(a') jvp_multi, chunked"), ("b1", f"(b1) {K} x jvp"), ("b2", f"(b2) jvp, batch {batch * K}")):
            if not rows[key]:
                if key == "b2":
                    print(f"   K = {K} {name:24s}: not run" + (" (K = 1: the same as (b1))" if K == 1 else f" (more than {max_members} members)"))
                continue
            m, lo, hi = stats_line(rows[key])
            med[key] = m
            print(f"   K = {K} {name:24s}: {m:.4f} ms/step (min {lo:.4f} .. max {hi:.4f}), {m * per:.2f} ns per member.direction.step, "
                  f"wall {np.median(walls[key]):.2f} s per call" + ("s" if key == "b1" else ""))
        best = min(v for k2, v in med.items() if k2 not in ("a", "ac"))
        spread = max(stats_line(rows["a"])[2] / stats_line(rows["a"])[1], 1.0) - 1.0
        print(f"   K = {K} ratio (a) / min(b): {med['a'] / best:.3f}, (a') / min(b): {med['ac'] / best:.3f}   (spread of (a)'s rounds: {100 * spread:.1f} %)")
        if wide is not None:
            wide.engine.close()
    s.engine.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    max_members = int(args[args.index("--max-members") + 1]) if "--max-members" in args else 64
    Ks = [int(x) for x in args[args.index("--K") + 1].split(",")] if "--K" in args else [1, 2, 4, 8]
    if "--small" in args:            # a rehearsal of the script itself, not a measurement
        time_case("rehearsal 8x8 quads + contact", 8, 8, 2, 250, Ks, reps, max_members)
        sys.exit(0)
    if "--paper-only" not in args:
        time_case("128x128 quads + contact", 128, 128, 16, 250, Ks, reps, max_members)
    time_case("paper 24x16 quads + contact", 24, 16, 1, 250, Ks, reps, max_members)
