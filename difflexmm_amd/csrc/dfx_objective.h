// dfx_objective.h -- objectives that are weighted sums over blocks and output times, evaluated and differentiated on the device-resident
// history (include/dfx.h: dfx_objective_value[_and_grad]).  Only engine_objective.hip reads this header.
//
//   DFX_OBJ_KINETIC            J_m = sum_k tau_k sum_b w_mb sum_d p_mbd v_mkbd^2 / 2                                   (energy.py:494-499)
//   DFX_OBJ_ANGULAR_MOMENTUM   J_m = sum_k tau_k sum_b w_mb [ (a_x + u_x) m_y v_y - (a_y + u_y) m_x v_x + J omega ]     (energy.py:502-519)
//
// with p = (m_x, m_y, J) = 1 / inv_m, a = lever0[m][b] = block centroid - spin centre, (u, v) the history.  The host compacts the blocks
// whose weight is non-zero in any member into an index list; an item is one (output time k, listed block j) pair of one member.
//   k_objective           fills the cotangent G (T, batch, n_blocks, 6) of the reverse sweep -- position rows as well as velocity rows --
//                         on the items whose tau_k w_mb is non-zero (G was zeroed by the prelude launch) and leaves one partial sum of the
//                         value per workgroup
//   k_objective_finish    one workgroup per member adds that member's partials: fixed order, no atomics -- the same history gives the
//                         same bits
//   k_objective_explicit  after the sweep: the direct dependence on the inertia (into blk_m) and, for the angular kind, on the block
//                         centroids (into g_c), one lane per (member, listed block), output times in order
#pragma once
#include "dfx_kernels.h"

namespace {

constexpr int kObjThreads = 256;
constexpr int kObjWaves = kObjThreads / 64;

struct ObjArgs {
  const double* fields;     // batch * T * n_blocks*6   (q | v planes per output time)
  const int32_t* blocks;    // n_act listed blocks
  const double* w;          // w_members * n_blocks
  const double* tau;        // T, or null: all ones
  const double* lever;      // lever_members * n_blocks*2, or null (kinetic kind)
  int n_act, w_stride, lever_stride;     // strides between members: 0 when one array serves all
};

// wave sum in the fixed order of the shuffle tree (the idiom of the error norm in dfx_kernels.h); lane 0 holds the result
__device__ __forceinline__ double obj_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid (chunks of kObjThreads items, members)
template <int KIND>
__global__ __launch_bounds__(kObjThreads) void k_objective(DevCtx c, ObjArgs a, double* G, double* partial) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_act;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  double val = 0.0;
  if (item < total) {
    const int k = (int)(item / a.n_act), j = (int)(item % a.n_act);
    const int b = a.blocks[j];
    const double tw = (a.tau ? a.tau[k] : 1.0) * a.w[(size_t)m * a.w_stride + b];
    if (tw != 0.0) {
      const size_t nd = (size_t)c.n_blocks * 3;
      const double* f = a.fields + ((size_t)m * c.n_timepoints + k) * nd * 2;
      const double* im = c.inv_m + (size_t)m * nd + (size_t)b * 3;
      const double px = 1.0 / im[0], py = 1.0 / im[1], pz = 1.0 / im[2];
      const double vx = f[nd + (size_t)b * 3], vy = f[nd + (size_t)b * 3 + 1], vz = f[nd + (size_t)b * 3 + 2];
      double* g = G ? G + ((size_t)k * c.batch + m) * nd * 2 + (size_t)b * 6 : nullptr;
      if (KIND == DFX_OBJ_KINETIC) {
        val = tw * (0.5 * px * vx * vx + 0.5 * py * vy * vy + 0.5 * pz * vz * vz);
        if (g) { g[3] = tw * px * vx; g[4] = tw * py * vy; g[5] = tw * pz * vz; }
      } else {
        const double* l = a.lever + (size_t)m * a.lever_stride + (size_t)b * 2;
        const double rx = l[0] + f[(size_t)b * 3], ry = l[1] + f[(size_t)b * 3 + 1];
        val = tw * (rx * py * vy - ry * px * vx + pz * vz);
        if (g) { g[0] = tw * py * vy; g[1] = -tw * px * vx; g[3] = -tw * ry * px; g[4] = tw * rx * py; g[5] = tw * pz; }
      }
    }
  }
  __shared__ double red[kObjWaves];
  val = obj_wave_sum(val);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = val;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int wv = 1; wv < kObjWaves; ++wv) s += red[wv];
    partial[(size_t)m * gridDim.x + blockIdx.x] = s;
  }
}

// grid (members): the member's partials, strided over the lanes in order, then the same tree
__global__ __launch_bounds__(kObjThreads) void k_objective_finish(const double* partial, int n_partial, double* objective, double* objective_host) {
  const int m = blockIdx.x;
  double v = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kObjThreads) v += partial[(size_t)m * n_partial + i];
  __shared__ double red[kObjWaves];
  v = obj_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int wv = 1; wv < kObjWaves; ++wv) s += red[wv];
    if (objective) objective[m] = s;
    if (objective_host) objective_host[m] = s;       // pinned host memory: no copy engine hop inside the stream (as k_kinetic)
  }
}

// grid (chunks of 64 listed blocks, members); every (member, block) entry of blk_m / g_c belongs to one lane
template <int KIND>
__global__ __launch_bounds__(64) void k_objective_explicit(DevCtx c, ObjArgs a) {
  const int m = blockIdx.y;
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= a.n_act) return;
  const int b = a.blocks[j];
  const double w = a.w[(size_t)m * a.w_stride + b];
  if (w == 0.0) return;
  const size_t nd = (size_t)c.n_blocks * 3;
  double mx = 0.0, my = 0.0, mz = 0.0, cx = 0.0, cy = 0.0;
  double lx = 0.0, ly = 0.0, px = 0.0, py = 0.0;
  if (KIND == DFX_OBJ_ANGULAR_MOMENTUM) {
    const double* l = a.lever + (size_t)m * a.lever_stride + (size_t)b * 2;
    const double* im = c.inv_m + (size_t)m * nd + (size_t)b * 3;
    lx = l[0]; ly = l[1]; px = 1.0 / im[0]; py = 1.0 / im[1];
  }
  for (int k = 0; k < c.n_timepoints; ++k) {
    const double tw = (a.tau ? a.tau[k] : 1.0) * w;
    const double* f = a.fields + ((size_t)m * c.n_timepoints + k) * nd * 2;
    const double vx = f[nd + (size_t)b * 3], vy = f[nd + (size_t)b * 3 + 1], vz = f[nd + (size_t)b * 3 + 2];
    if (KIND == DFX_OBJ_KINETIC) {
      mx += tw * 0.5 * vx * vx; my += tw * 0.5 * vy * vy; mz += tw * 0.5 * vz * vz;
    } else {
      const double rx = lx + f[(size_t)b * 3], ry = ly + f[(size_t)b * 3 + 1];
      mx -= tw * ry * vx; my += tw * rx * vy; mz += tw * vz;
      cx += tw * py * vy; cy -= tw * px * vx;
    }
  }
  double* bm = c.blk_m + ((size_t)m * c.n_blocks + b) * 3;
  bm[0] += mx; bm[1] += my; bm[2] += mz;
  if (KIND == DFX_OBJ_ANGULAR_MOMENTUM) {
    double* gc = c.g_c + ((size_t)m * c.n_blocks + b) * 2;
    gc[0] += cx; gc[1] += cy;
  }
}

}  // namespace
