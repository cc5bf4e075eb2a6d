"""The hinge fit of examples/hinge_fit.py (its default sample) in reverse and in forward mode, on an MI355X:

  * wall time of one ``residuals_and_jacobian`` (3 forward-mode solves with 3 tangents each + 3 ``dfx_rhs_jvp`` calls) against one
    ``value_and_grad`` (3 forward + 3 reverse solves + 3 ``dfx_rhs_vjp`` calls): medians of 5 alternating rounds after one warm-up each;
  * evaluations and wall time the method of moving asymptotes and Levenberg-Marquardt need to bring the objective below 1e-6 of its start.

    python tools/hinge_fit_timing.py [--max-evaluations 60] [--out profiles/r11_hinge_lm.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import hinge_fit as ex  # noqa: E402


def timed(fit, name, stamps):
    """Wrap a method of the fit so that the time of every return is recorded."""
    inner = getattr(fit, name)

    def call(*a, **kw):
        out = inner(*a, **kw)
        stamps.append(time.perf_counter())
        return out
    setattr(fit, name, call)


def until(fit, stamps, t0, factor=1e-6):
    """(evaluations, seconds) until the objective first drops below factor * its start, or None."""
    for i, v in enumerate(fit.objective_values):
        if v < factor * fit.objective_values[0]:
            return i + 1, stamps[i] - t0
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-evaluations", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["hinge fit, the default sample of examples/hinge_fit.py (3 x 3 cells, 21 outputs, adaptive solves), start "
             f"{ex.START}, sample {ex.TRUTH}"]
    fit = ex.build_fit()
    fit.value_and_grad(ex.START)
    fit.residuals_and_jacobian(ex.START)
    t_rev, t_fwd = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        fit.value_and_grad(ex.START)
        t1 = time.perf_counter()
        fit.residuals_and_jacobian(ex.START)
        t2 = time.perf_counter()
        t_rev.append(t1 - t0)
        t_fwd.append(t2 - t1)
    steps = [p.solve_dynamics.stats.get("steps_per_member") for p in fit.forward_problems]
    lines.append(f"one value_and_grad           : median {1e3 * statistics.median(t_rev):8.2f} ms  (min {1e3 * min(t_rev):.2f}, max {1e3 * max(t_rev):.2f})")
    lines.append(f"one residuals_and_jacobian   : median {1e3 * statistics.median(t_fwd):8.2f} ms  (min {1e3 * min(t_fwd):.2f}, max {1e3 * max(t_fwd):.2f})"
                 f"   ratio {statistics.median(t_fwd) / statistics.median(t_rev):.2f}")
    lines.append(f"accepted steps per test (tension, compression, shear): {steps}")
    for method in ("mma", "lm"):
        fit = ex.build_fit()
        stamps = []
        timed(fit, "value_and_grad" if method == "mma" else "residuals_and_jacobian", stamps)
        t0 = time.perf_counter()
        if method == "mma":
            fit.run_optimization_nlopt(ex.START, a.max_evaluations, lower_bound=ex.LOWER, upper_bound=ex.UPPER)
        else:
            fit.run_optimization_lm(ex.START, a.max_evaluations, lower_bound=ex.LOWER, upper_bound=ex.UPPER)
        hit = until(fit, stamps, t0)
        best = min(fit.objective_values)
        lines.append(f"{method:3s}: {len(fit.objective_values)} evaluations run in {stamps[-1] - t0:.2f} s, best objective {best:.3e} "
                     f"(start {fit.objective_values[0]:.3e}); below 1e-6 of the start after "
                     + (f"{hit[0]} evaluations, {hit[1]:.2f} s" if hit else f"-- not within {a.max_evaluations} evaluations"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
