"""Wall time of ``dfx_strain_peak_value_and_grad`` beside ``dfx_strain_objective_value_and_grad`` on ONE kept solve each, with the same
weighted ligaments and the same ``want`` (the raw gradients a design reaches), on an MI355X.  The second call is the yardstick: both run the
same reverse sweep; the peak adds a maximum, a sum and a second evaluation of the weighted ligaments in front of it ("sweep time plus
three cheap passes").  The value-only entries are timed too: they isolate the passes in front of the sweep.  Medians of 5 calls after one
warm-up each.

  * the paper lattice (24 x 16 quads, 200 outputs, adaptive solve), 1 design and 32 designs, every ligament watched;
  * the large case of tests/objective_shapes.py (quads 17 x 17, 257 outputs, 2 members, 1 161 workgroups of the 64-item kernels).

    python tools/peak_strain_timing.py [--rows paper1,paper32,large] [--calls 5] [--out profiles/r23_peak_strain_timing.txt]
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

WHICH = ("centroid_node_vectors", "void_angle0", "inertia")
PARTS = (1.0, 1.0, 1.0, 0.0)


def median_ms(fn, calls):
    fn()                                           # warm-up: allocations, graphs
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(t), 1e3 * min(t), 1e3 * max(t)


def row(name, eng, coef, bw, tau, calls):
    """the four entries on the history the engine holds; beta from the hard maximum (beta q_hat = 15 for the first member)"""
    _, peak, _ = eng.strain_peak_value(coef, bw, tau, "ks", 1.0)
    beta = 15.0 / float(peak[0])
    t_se = median_ms(lambda: eng.strain_objective_value_and_grad(bw, tau, PARTS, which=WHICH), calls)
    t_pk = median_ms(lambda: eng.strain_peak_value_and_grad(coef, bw, tau, "ks", beta, which=WHICH), calls)
    t_pn = median_ms(lambda: eng.strain_peak_value_and_grad(coef, bw, tau, "pnorm", 6.0, which=WHICH), calls)
    v_se = median_ms(lambda: eng.strain_objective_value(bw, tau, PARTS), calls)
    v_pk = median_ms(lambda: eng.strain_peak_value(coef, bw, tau, "ks", beta), calls)
    return (f"{name:46s} strain energy {t_se[0]:8.2f} ms (min {t_se[1]:.2f}, max {t_se[2]:.2f})   peak KS {t_pk[0]:8.2f} ms (min {t_pk[1]:.2f}, max "
            f"{t_pk[2]:.2f})   peak p-norm {t_pn[0]:8.2f} ms   peak KS / strain energy {t_pk[0] / t_se[0]:5.2f}   value only: strain energy "
            f"{v_se[0]:6.2f} ms, peak KS {v_pk[0]:6.2f} ms   extra of the peak {t_pk[0] - t_se[0]:7.2f} ms")


def paper_row(batch, calls):
    from tools.objective_timing import designs_of, paper_forward
    fw = paper_forward(batch)
    fw.setup()
    designs = designs_of(fw, batch)
    fw.solve(designs if batch > 1 else designs[0], keep_trajectory=True, want_fields=False)
    eng = fw.solve_dynamics.engine
    coef = O.strain_limit_coefficients(fw.reference_bond_vectors, 0.02, 0.2, 0.2)
    bw = np.ones(len(fw.bond_connectivity))
    return row(f"24 x 16, 200 outputs, adaptive, {batch} design{'s' if batch > 1 else ''}", eng, coef, bw, None, calls)


def large_row(calls):
    from tests import objective_shapes as OS
    from tests import peak_strain_cases as PC
    L = OS.LargeCase("quads")
    os.environ["DFX_CHECKPOINT"] = "records"
    L.solve()
    coef, bw, tau = PC.large_inputs(L)
    return row("17 x 17, 257 outputs, fixed grid, 2 members", L.c.solver.engine, coef, bw, tau, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="paper1,paper32,large")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = a.rows.split(",")
    lines = ["dfx_strain_peak_value_and_grad beside dfx_strain_objective_value_and_grad on one kept solve: the same weighted ligaments, want = "
             f"{WHICH}; wall time per call, medians of {a.calls} calls after one warm-up"]
    if "paper1" in rows:
        lines.append(paper_row(1, a.calls))
    if "paper32" in rows:
        lines.append(paper_row(32, a.calls))
    if "large" in rows:
        lines.append(large_row(a.calls))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
