// dfx_drive.h -- the samples of a table drive as a differentiable leaf: the two small kernels behind a reverse sweep that kept the
// drive-cotangent trace (TraceCtx, the TRACE builds of the reverse stage in dfx_kernels.h).
//
// g_f(t) = A interp(t - delay; T, Y) is linear in the samples Y: d g_f / d Y[j] = A hat_j(t - delay), the piecewise-linear hat of
// breakpoint j (the end samples hold everything at or beyond T[0] / T[n-1], as eval_time_fn does).  The sweep leaves gbar = dL / d g_f at
// every stage time, so
//     dL / d Y[j] = A sum_{n, i} gbar[n][i] hat_j(t_n + c_i h_n - delay)
// -- a gather per (member, sample) over the stage times, no search (sample j owns (T[j-1], T[j+1])), no atomics: one wave per sample, a
// strided sum per lane and a butterfly over the lanes, the same order every time.
#pragma once
#include "dfx_kernels.h"

namespace {

// t_n + c_i h_n of every (member, step ordinal, stage), by the expressions of the stage kernels: the uniform grid of the segment table,
// caller-chosen step boundaries, or every member's own accepted steps (n_acc: their counts; the row N_m is the evaluation at the final
// state, a step of size zero).  Rows beyond a member's last step repeat its final time (their trace entries are zero).
__global__ __launch_bounds__(64) void k_stage_times(DevCtx c, StageTimes st, const Seg* segs, int n_seg, long long rows, long long n_total,
                                                    const int* n_acc, double* times) {
  const int m = blockIdx.y;
  const long long n = (long long)blockIdx.x * 64 + threadIdx.x;
  if (n >= rows) return;
  double t, h;
  if (c.t_steps) {
    const double* ts = steps_of(c, m);
    const long long N = n_acc ? (long long)n_acc[m] : n_total;
    if (n < N) { t = ts[n]; h = ts[n + 1] - t; }
    else { t = ts[N]; h = 0.0; }
  } else {
    int si = 0;
    while (si + 1 < n_seg && n >= segs[si].base_step + segs[si].n_steps) ++si;
    const Seg sg = segs[si];
    const int j = (int)(n - sg.base_step);
    t = sg.t_interval + (sg.j0 + j) * sg.h;
    h = n < n_total ? sg.h : 0.0;
  }
  double* out = times + ((size_t)m * (size_t)rows + (size_t)n) * (u32)c.s;
  for (int i = 0; i < c.s; ++i) out[i] = t + st.c[i] * h;
}

// weight of sample j in interp(tau; T, .) -- the branches of eval_time_fn's table: tau <= T[0] and tau >= T[n-1] hold the end samples,
// a breakpoint belongs to the piece that starts there
__device__ __forceinline__ double table_hat(const double* T, int n, int j, double tau) {
  if (tau <= T[0]) return j == 0 ? 1.0 : 0.0;
  if (tau >= T[n - 1]) return j == n - 1 ? 1.0 : 0.0;
  if (j > 0 && tau >= T[j - 1] && tau < T[j]) return (tau - T[j - 1]) / (T[j] - T[j - 1]);
  if (j + 1 < n && tau >= T[j] && tau < T[j + 1]) return 1.0 - (tau - T[j]) / (T[j + 1] - T[j]);
  return 0.0;
}

// grad[m][j] = A_m sum gbar[m][f][q] hat_j(times[m][q] - delay_m) over the n_stage = rows * s stage evaluations; grid (n_tab, batch)
__global__ __launch_bounds__(64) void k_table_grad(const TimeFn* fns, int f, int n_fns, const double* gbar, const double* times, long long n_stage,
                                                   double* grad) {
  const int m = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
  const TimeFn tf = fns[(size_t)m * DFX_MAX_FNS + f];
  if (j >= tf.n_tab) return;
  const double* g = gbar + ((size_t)m * n_fns + f) * (size_t)n_stage;
  const double* tm = times + (size_t)m * (size_t)n_stage;
  double acc = 0.0;
  for (long long q = lane; q < n_stage; q += 64) {
    const double gb = g[q];
    if (gb != 0.0) acc += gb * table_hat(tf.tab, tf.n_tab, j, tm[q] - tf.p[1]);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) grad[(size_t)m * tf.n_tab + j] = tf.p[0] * acc;
}

}  // namespace
