// dfx_tangent.h -- the forward-mode (tangent) solve: one Runge-Kutta stage of the primal and of K directional derivatives together.
//
// What it differentiates is the fixed-grid solve of dfx_forward_grid / dfx_forward_grid_members with its steps frozen -- the map dfx_adjoint
// transposes.  One lane per (member, block); the scalar is DualN<K>, one value and K epsilon parts, so every primal operation (the
// half-angle records, atan2 / sqrt / rsqrt and their expansions, the branch decisions, every parameter and record load) happens once and
// every epsilon operation K times.  The physics is not restated: bond_grad_p / contact_grad / distance_contact_grad (dfx_physics.h) are
// instantiated with T = P = DualN<K>:
//   * the block's stage record and those of its partners are seeded with the tangent stage states (seed_rec: the half-angle pair follows
//     theta), and every per-ligament parameter with its tangents: the epsilon parts of the forces those functions return are exactly
//     H_uu du + H_up dp  for the block's own DOFs, per direction;
//   * DOF part, as fwd_dof (dfx_stage.h) plus its derivative: a = F / m  =>  da = (dF - a dm) / m, with F = F_load - dE/du - c v,
//     dF = dF_load - (dE/du).e - dc v - c dv;  driven DOFs  du_c = sum coef (dg/dp . dp)  (eval_time_fn's gp),  loaded DOFs
//     dF_load = sum load_coef (dg/dp . dp);  the RK combine of the next stage record is linear and takes every tangent alike.
// Branch decisions (angle-contact window, closest edge of the distance-based contact, time-function phases) are taken on the primal values
// only: the tangents follow the primal's branch, as the reverse sweep does.  Nothing is culled: every ligament is evaluated.  No atomics,
// nothing depends on the launch geometry.
// The velocities of driven DOFs enter no force; their tangents are left at 0 here and the rows of prescribed DOFs in fields_dot are
// assembled on the host (difflexmm_amd/dynamics.py, DynamicSolver.jvp_multi).
//
// The dense pass (dfx_forward_tangent_dense[_multi]) differentiates the ADAPTIVE solve instead -- the map dfx_adjoint transposes after
// dfx_forward_adaptive_keep: the same stage kernel on every member's own frozen accepted steps (TanCtx::n_steps: a member that is done
// leaves; one more stage 0 at its final state, a step of size zero, gives A_6 of its last step), and k_tan_dense_multi forms the outputs
// inside the steps and their tangents by the quartic dense output of the adaptive pass, which is linear in (q_n, v_n, A_0 .. A_6) with
// coefficients that hold primal step data only.  A_0 of step n + 1 is A_6 of step n, so the place of A_0 alternates between rows 0 and 6
// of A / DA with the step's parity (TanStage::a0) and nothing is copied.
//
// The parameter image is a plain per-slot layout of its own, NOT the packed image of dfx_plan.h:pack_params, which is not linear in the
// parameters (it stores 1/m, a dictionary of reference vectors, uniform stiffnesses once per member).  Layouts (KC = the chunk width, a
// template parameter; the host runs ceil(K / KC) passes, engine_tangent.hip):
//   * parameter images, value then tangents -- the primal half once, then KC tangent halves:
//       slot    9 * (1 + KC):  r(2) l(2) k(3) phi(2), then the same nine per direction
//       block   6 * (1 + KC):  1/m(3) c(3), then d(1/m)(3) dc(3) per direction
//       member  3 + kTanMemDir * KC:  contact(3), then dcontact(3) dfn_params per direction
//       centre  2 * (1 + KC):  centroid(2), then its tangent per direction                        (distance-based contact)
//   * primal records S / Y and A: B * nb * kRec and B * a_rows * nb * 3; tangent records and DA: one such plane per direction (d_plane /
//     da_plane elements apart; tangent records hold q at 0..2, v at 5..7);
//   * fields_dot of a pass: (B, KT, T, 2, nb, 3), KT = the directions of the pass.
// A pass may hold several SLICES of KC directions each, one per blockIdx.y (TanSlices): every slice has an image of its own and its own
// planes, and runs the same arithmetic; slice 0 alone stores the primal results (all slices compute the same ones).  Lattices too small to
// fill the chip take all their directions as slices of width 1 in one pass -- the replicated-members form, which is cheaper there
// (profiles/r09_tangent_multi.txt); everything else takes one slice of the widest width per pass.  A single direction is KC = 1 with one
// slice in either form: dfx_forward_tangent and dfx_forward_tangent_dense are these kernels at that width.
//
// The signal sink (dfx_forward_tangent_signals[_dense]_multi): instead of downloading fields / fields_dot, a pass ends in three launches on
// its own buffers -- the history never leaves the device, what is downloaded is (B, KT, T, n_signals):
//   k_tan_signal_channels  items (output k, force block j), the four slots of an item on one DPP quad, slices along grid.z: each lane its
//                          own side of its ligament on DualN<KC> (dfx_tangent_signal.h) -- primal rows of fields, tangent rows of the
//                          slice's directions of fields_dot, the slot's entry of the slice's parameter image and the contact constants
//                          with their tangents; quad_sum of the value and of every epsilon part in direction order; lane 0 stores chan
//                          (slice 0) and chan_dot
//   k_tan_hinge_channels   items (output k, listed hinge), one lane each: the same evaluation of ONE ligament (a hinge channel, component
//                          9 + 3 node + dof, is the summand of a force channel), stored behind the block channels
//   k_tan_signal_combine   one lane per (member, direction, output, signal): the signal's terms in list order, field terms from
//                          fields_dot, force terms from chan_dot; the pass's first direction also writes S from fields and chan
//   k_tan_finite_flags     one flag per workgroup: a non-finite entry of fields / of the pass's fields_dot met on its stride; ordinary
//                          stores into a buffer of the call, ORed by the host
// Rows of prescribed DOFs: the position rows of fields_dot hold the exact tangent of c(t) (k_tan_init_multi, the stage, the dense output),
// so force terms on or beside a driven block are complete here; the velocity rows are 0 and the caller adds dc'/dp . dp to field terms on
// them (include/dfx.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dfx_kernels.h"
#include "dfx_stage.h"
#include "dfx_tangent_signal.h"

namespace dfx {


constexpr int kTanSlotVals = 9;                                    // the primal half of a slot (and of every tangent half)
constexpr int kTanBlkVals = 6;                                     // likewise of a block: 1/m(3), c(3)
constexpr int kTanMemDir = 3 + DFX_MAX_FNS * DFX_FN_PARAMS;        // dcontact(3), dfn_params
constexpr int kTanMaxWidth = 4;                                    // the widest chunk the library ships (profiles/r09_tangent_multi.txt)
DFX_HD constexpr int tan_slot_n(int kc) { return kTanSlotVals * (1 + kc); }
DFX_HD constexpr int tan_blk_n(int kc) { return kTanBlkVals * (1 + kc); }
DFX_HD constexpr int tan_mem_n(int kc) { return 3 + kTanMemDir * kc; }
DFX_HD constexpr int tan_cen_n(int kc) { return 2 * (1 + kc); }

struct TanCtx {
  int B, nb, n_fns, n_stages;
  const int32_t* slot_info;      // n_slots (shared)
  const int32_t* block_special;  // nb (shared)
  const dfx_special* special;
  const TimeFn* fns;             // B * DFX_MAX_FNS (the primal time functions: dfx_set_params' upload)
  const double* tp;              // slices * B * n_slots * tan_slot_n(KC)
  const double* blk;             // slices * B * nb * tan_blk_n(KC)
  const double* mem;             // slices * B * tan_mem_n(KC)
  const double* cen;             // slices * B * nb * tan_cen_n(KC), or null
  const double* tgrid;           // n_grids * n_steps * 2: (t, h) of every step
  const double* t0;              // n_grids: the first output time
  long long grid_stride;         // elements between the grids of two members in tgrid (0: one grid)
  int t0_stride;                 // 1: one t0 per member, 0: shared
  int a_rows;                    // places per member in A / DA: n_stages, or 7 in the dense pass (A_6 = the FSAL acceleration)
  const long long* n_steps;      // B: the step count N_m of every member (dense pass), or null: every member takes every step
  // sample tangents of table drives (dfx_fn_table_tangents): per function (tab_dirs, B, n_tab) or null; tab_k0: the call's direction that
  // is direction 0 of this pass (a spare direction of the last chunk, tab_k0 + k >= tab_dirs, has no tangent)
  const double* tabdot[DFX_MAX_FNS];
  int tab_k0, tab_dirs;
};

struct TanStage {
  const double *S_in, *D_in;     // primal / tangent records of this stage (tangent: one plane per direction)
  const double *Y, *DY;          // step base
  double *S_out, *D_out;         // next stage records (stage s-1: the next step base)
  double *A, *DA;                // stage accelerations and their tangents (DA: one plane per direction)
  long long n;                   // step ordinal
  int i;                         // stage index
  int a0;                        // place of A_0 of this step: 0, or in the dense pass 0 / 6 by the step's parity (A_0 of step n + 1 is A_6 of step n)
};

// the dense output of step n (the dense pass): launched after stage 0 of step n + 1 has left A_6
struct TanDense {
  const double *Y0, *DY0;        // step base of step n (records)
  const double *Y1, *DY1;        // step base of step n + 1
  const double *A, *DA;          // stage accelerations, 7 places per member
  const int32_t* out_ptr;        // B * op_stride: outputs [out_ptr[n], out_ptr[n + 1]) lie in step n
  const double* theta;           // B * Tn: relative position of every output in its step
  const double* ts;              // Tn output times
  double *fields, *fields_dot;   // B * Tn * 2 * nb * 3, and B * KT * Tn * 2 * nb * 3
  long long op_stride, n;
  int Tn, a0, a6;                // places of A_0 and A_6 of step n
  double cm[7], cma[7];          // mid-point weights (velocity / position form, Dopri of dfx_physics.h)
};

// where the directions of a pass lie: planes of the tangent buffers, and the images of the slices
struct TanSlices {
  long long d_plane, da_plane;                         // elements between the planes of two directions in D_in / DY / D_out, and in DA
  long long tp_plane, blk_plane, mem_plane, cen_plane; // elements between the images of two slices
  int kt;                                              // directions of the pass: slices * KC
};

// what the kernels take: a stage / a dense output, and where its directions lie
struct TanStageM {
  TanStage s;
  TanSlices sl;
};

struct TanDenseM {
  TanDense d;
  TanSlices sl;
};

template <int K>
DFX_HD BlockRec<DualN<K>> tan_rec_n(const double* S, const double* D, long long plane, int b) {
  const BlockRec<double> r = load_rec(S, b);
  double wx[K], wy[K], wth[K];
  DFX_DN_EACH {
    const double* d = D + (size_t)k * plane + (size_t)b * kRec;
    wx[k] = d[0]; wy[k] = d[1]; wth[k] = d[2];
  }
  return seed_rec(r, wx, wy, wth);
}

template <int K>
DFX_HD DualN<K> tan_par_n(const double* s, int j) {
  DualN<K> o; o.v = s[j];
  DFX_DN_EACH o.e[k] = s[kTanSlotVals * (1 + k) + j];
  return o;
}

// value (vi) and K tangents (ti + stride * k) of one scalar of an image
template <int K>
DFX_HD DualN<K> tan_scalar_n(const double* p, int vi, int ti, int stride) {
  DualN<K> o; o.v = p[vi];
  DFX_DN_EACH o.e[k] = p[ti + stride * k];
  return o;
}

// sum over f of coef_f * g_f(t), its time derivative, and per direction the tangent sum coef_f * dg_f/dp . dp_f; the time functions are
// evaluated once
// (dir0: direction 0 of this slice within the pass.  A table whose samples carry tangents adds A interp(tau; T, dY_k) per direction: the
// bin and the weight are found once per evaluation, by eval_time_fn's own branches, and serve all K directions)
template <int K>
DFX_HD void tan_drive_n(const TanCtx& c, int m, const double* mem /* the member's image of this slice */, const double* coef /* DFX_MAX_FNS */,
                        double t, double& g_sum, double& gt_sum, double (&dg_sum)[K], int dir0) {
  g_sum = 0.0; gt_sum = 0.0;
  DFX_DN_EACH dg_sum[k] = 0.0;
  const double* dfn = mem + 3 + 3;
  for (int f = 0; f < c.n_fns; ++f) {
    if (coef[f] == 0.0) continue;
    double g, gt, gp[kMaxFnParams];
    eval_time_fn(c.fns[(size_t)m * DFX_MAX_FNS + f], t, g, gt, gp);
    g_sum += coef[f] * g;
    gt_sum += coef[f] * gt;
    DFX_DN_EACH {
      double dg = 0.0;
      for (int j = 0; j < kMaxFnParams; ++j) dg += gp[j] * dfn[kTanMemDir * k + f * DFX_FN_PARAMS + j];
      dg_sum[k] += coef[f] * dg;
    }
    const TimeFn& tf = c.fns[(size_t)m * DFX_MAX_FNS + f];
    if (c.tabdot[f] && tf.type == kFnTable) {
      const int n = tf.n_tab;
      const double* T = tf.tab;
      const double tau = t - tf.p[1];
      int lo = 0;
      double w = 0.0;
      if (tau >= T[n - 1]) { lo = n - 2; w = 1.0; }
      else if (tau > T[0]) {
        int hi = n - 1;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (T[mid] <= tau) lo = mid; else hi = mid; }
        w = (tau - T[lo]) / (T[hi] - T[lo]);
      }
      DFX_DN_EACH {
        const int dir = c.tab_k0 + dir0 + k;
        if (dir < c.tab_dirs) {
          const double* dY = c.tabdot[f] + ((size_t)dir * c.B + m) * n;
          dg_sum[k] += coef[f] * tf.p[0] * (dY[lo] + w * (dY[lo + 1] - dY[lo]));
        }
      }
    }
  }
}

// state0_dot: (KT, B, 2, nb, 3) -- the directions of this pass (a padded direction is all zero), or null
template <int K>
__global__ void k_tan_init_multi(TanCtx c, const double* state0, const double* state0_dot, double* S, double* D, TanSlices sl) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  const int slice = blockIdx.y;
  const long long d_plane = sl.d_plane;
  const double* mem = c.mem + (size_t)slice * sl.mem_plane + (size_t)m * tan_mem_n(K);
  D += (size_t)slice * K * d_plane;
  if (state0_dot) state0_dot += (size_t)slice * K * c.B * 2 * c.nb * 3;
  const double t0 = c.t0[m * c.t0_stride];
  const int sidx = c.block_special[b];
  double rr[kRec];
  double* r = rr;
  const size_t nd = (size_t)c.nb * 3;
  const size_t s0_plane = (size_t)c.B * 2 * nd;
  for (int j = 0; j < 3; ++j) {
    double q = state0 ? state0[(size_t)m * 2 * nd + b * 3 + j] : 0.0;
    double v = state0 ? state0[(size_t)m * 2 * nd + nd + b * 3 + j] : 0.0;
    double dq[K], dv[K];
    DFX_DN_EACH {
      dq[k] = state0_dot ? state0_dot[k * s0_plane + (size_t)m * 2 * nd + b * 3 + j] : 0.0;
      dv[k] = state0_dot ? state0_dot[k * s0_plane + (size_t)m * 2 * nd + nd + b * 3 + j] : 0.0;
    }
    if (sidx >= 0 && ((c.special[sidx].con_mask >> j) & 1)) {
      tan_drive_n<K>(c, m, mem, c.special[sidx].con_coef[j], t0, q, v, dq, slice * K);
      DFX_DN_EACH dv[k] = 0.0;
    }
    r[j] = q; r[5 + j] = v;
    DFX_DN_EACH {
      double* d = D + (size_t)k * d_plane + (size_t)gid * kRec;
      d[j] = dq[k]; d[5 + j] = dv[k];
    }
  }
  double s, co;
  fast_sincos(0.5 * r[2], &s, &co);
  r[3] = co; r[4] = s;
  if (slice == 0) {
    double* out = S + (size_t)gid * kRec;
    for (int j = 0; j < kRec; ++j) out[j] = r[j];
  }
  DFX_DN_EACH {
    double* d = D + (size_t)k * d_plane + (size_t)gid * kRec;
    d[3] = 0.0; d[4] = 0.0;
  }
}

// node vectors of the bonded node, its next and its previous node on the block (distance-based contact)
template <int NPB, int K>
DFX_HD void tan_node_triple_n(const double* tp, int slot, DualN<K> (&r)[3][2]) {
  const int b = slot >> 2, k = slot & 3;
  const int ks[3] = {k, (k + 1) % NPB, (k + NPB - 1) % NPB};
  for (int i = 0; i < 3; ++i) {
    const double* s = tp + (size_t)(b * kSlots + ks[i]) * tan_slot_n(K);
    r[i][0] = tan_par_n<K>(s, 0); r[i][1] = tan_par_n<K>(s, 1);
  }
}

template <int MODEL, int CONTACT, int NPB, int KC>
__global__ void __launch_bounds__(256) k_tan_stage_multi(TanCtx c, Tableau T, TanStageM sm) {
  using D = DualN<KC>;
  constexpr int K = KC;
  const TanStage& st = sm.s;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  if (c.n_steps) {
    // dense pass: a member that has taken its N_m steps leaves (its step base stays put); at n == N_m only the evaluation at its final
    // state runs, as stage 0 of a step of size zero
    const long long N = c.n_steps[m];
    if (st.n > N || (st.n == N && st.i > 0)) return;
  }
  const size_t moff = (size_t)m * c.nb;                 // first block of this member in the record buffers
  const TanSlices& sl = sm.sl;
  const int slice = blockIdx.y;                         // this lane's KC directions: planes [slice * KC, (slice + 1) * KC), image `slice`
  const bool first = slice == 0;                        // the slice that stores the primal results
  const size_t doff = (size_t)slice * K * sl.d_plane, daoff = (size_t)slice * K * sl.da_plane;
  const double* S_in = st.S_in + moff * kRec;
  const double* D_in = st.D_in + doff + moff * kRec;
  const double* tp = c.tp + (size_t)slice * sl.tp_plane + moff * kSlots * tan_slot_n(K);
  const double* mem = c.mem + (size_t)slice * sl.mem_plane + (size_t)m * tan_mem_n(K);
  const BlockRec<D> o = tan_rec_n<K>(S_in, D_in, sl.d_plane, b);
  D f[3];
#pragma unroll
  for (int kk = 0; kk < NPB; ++kk) {
    const int slot = b * kSlots + kk;
    const int info = c.slot_info[slot];
    if (info < 0) continue;
    const int ps = info >> 1;
    const double sgn = (info & 1) ? 1.0 : -1.0;
    const double* sp = tp + (size_t)slot * tan_slot_n(K);
    const double* pp = tp + (size_t)ps * tan_slot_n(K);
    const BlockRec<D> p = tan_rec_n<K>(S_in, D_in, sl.d_plane, ps >> 2);
    const D lx = tan_par_n<K>(sp, 2), ly = tan_par_n<K>(sp, 3);
    const D l0 = tsqrt(lx * lx + ly * ly);
    const D il0 = 1.0 / l0;
    BondGrad<D> g;
    bond_grad_p<MODEL, D, D>(o, p, tan_par_n<K>(sp, 0), tan_par_n<K>(sp, 1), tan_par_n<K>(pp, 0), tan_par_n<K>(pp, 1), lx, ly, l0, il0,
                             tan_par_n<K>(sp, 4), tan_par_n<K>(sp, 5), tan_par_n<K>(sp, 6), sgn, g);
    f[0] = f[0] + g.fx; f[1] = f[1] + g.fy; f[2] = f[2] + g.fth;
    if (CONTACT == DFX_CONTACT_DISTANCE) {
      const D am = tan_scalar_n<K>(mem, 0, 3, kTanMemDir), ac = tan_scalar_n<K>(mem, 1, 4, kTanMemDir), kc = tan_scalar_n<K>(mem, 2, 5, kTanMemDir);
      D ro[3][2], rp[3][2];
      tan_node_triple_n<NPB, K>(tp, slot, ro);
      tan_node_triple_n<NPB, K>(tp, ps, rp);
      const double* cen = c.cen + (size_t)slice * sl.cen_plane;
      const double* co = cen + (moff + b) * tan_cen_n(K);
      const double* cp = cen + (moff + (ps >> 2)) * tan_cen_n(K);
      DistContactGrad<D> dc;
      distance_contact_grad<D, D>(o, p, tan_scalar_n<K>(co, 0, 2, 2), tan_scalar_n<K>(co, 1, 3, 2), tan_scalar_n<K>(cp, 0, 2, 2),
                                  tan_scalar_n<K>(cp, 1, 3, 2), ro, rp, info & 1, am, ac, kc, dc);
      f[0] = f[0] + dc.fx; f[1] = f[1] + dc.fy; f[2] = f[2] + dc.fth;
    } else if (CONTACT == DFX_CONTACT_ANGLE) {
      const D am = tan_scalar_n<K>(mem, 0, 3, kTanMemDir), ac = tan_scalar_n<K>(mem, 1, 4, kTanMemDir), kc = tan_scalar_n<K>(mem, 2, 5, kTanMemDir);
      ContactGrad<D> cg;
      const D kap = sgn * (o.th - p.th);
      contact_grad<D, D>(kap, tan_par_n<K>(sp, 7), tan_par_n<K>(sp, 8), am, ac, kc, cg);
      f[2] = f[2] + sgn * cg.dkap;
    }
  }
  // DOF part (fwd_dof of dfx_stage.h and its derivative, the tangent lines once per direction)
  const double* tg = c.tgrid + (size_t)m * c.grid_stride + 2 * (size_t)st.n;
  const double t = tg[0], h = tg[1];
  const int i = st.i, r = i + 1;
  const double t_i = t + T.c[i] * h, t_next = t + T.c[r] * h;
  const int sidx = c.block_special[b];
  const double* bk = c.blk + (size_t)slice * sl.blk_plane + (moff + b) * tan_blk_n(K);
  const size_t nd = (size_t)c.nb * 3;
  double* A = st.A + (size_t)m * c.a_rows * nd;
  double* DA = st.DA + daoff + (size_t)m * c.a_rows * nd;
  const double* rin = S_in + (size_t)b * kRec;
  const double* din = D_in + (size_t)b * kRec;
  const double* yb = st.Y + (moff + b) * kRec;
  const double* dyb = st.DY + doff + (moff + b) * kRec;
  double* ro = st.S_out + (moff + b) * kRec;
  double* dro = st.D_out + doff + (moff + b) * kRec;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const size_t dof = (size_t)b * 3 + d;
    bool constrained = false;
    double fload = 0.0, cnext = 0.0, cdnext = 0.0;
    double dfload[K], dcnext[K];
    DFX_DN_EACH { dfload[k] = 0.0; dcnext[k] = 0.0; }
    if (sidx >= 0) {
      const dfx_special& sp = c.special[sidx];
      constrained = (sp.con_mask >> d) & 1;
      double unused;
      if (constrained) tan_drive_n<K>(c, m, mem, sp.con_coef[d], t_next, cnext, cdnext, dcnext, slice * K);
      else tan_drive_n<K>(c, m, mem, sp.load_coef[d], t_i, fload, unused, dfload, slice * K);
    }
    const double v_i = rin[5 + d];
    const double inv_m = bk[d], damp = bk[3 + d];
    const double F = fload - f[d].v - damp * v_i;
    const double a = constrained ? 0.0 : F * inv_m;
    const size_t arow = (size_t)(i ? i : st.a0) * nd + dof;
    if (first) A[arow] = a;
    double sv = T.a[r][i] * a, sq = T.aa[r][i] * a;
    double dsv[K], dsq[K];
    DFX_DN_EACH {
      const double dv_i = din[(size_t)k * sl.d_plane + 5 + d];
      const double dinv_m = bk[kTanBlkVals * (1 + k) + d], ddamp = bk[kTanBlkVals * (1 + k) + 3 + d];
      // a = F / m: da = dF / m + F d(1/m)
      const double da = constrained ? 0.0 : (dfload[k] - f[d].e[k] - ddamp * v_i - damp * dv_i) * inv_m + F * dinv_m;
      DA[(size_t)k * sl.da_plane + arow] = da;
      dsv[k] = T.a[r][i] * da; dsq[k] = T.aa[r][i] * da;
    }
    for (int l = 0; l < i; ++l) {
      const size_t row = (size_t)(l ? l : st.a0) * nd + dof;
      const double al = A[row];
      sv += T.a[r][l] * al; sq += T.aa[r][l] * al;
      DFX_DN_EACH {
        const double dal = DA[(size_t)k * sl.da_plane + row];
        dsv[k] += T.a[r][l] * dal; dsq[k] += T.aa[r][l] * dal;
      }
    }
    double qnext = yb[d] + h * (T.c[r] * yb[5 + d] + h * sq);
    double vnext = yb[5 + d] + h * sv;
    if (constrained) { qnext = cnext; vnext = cdnext; }
    if (first) { ro[d] = qnext; ro[5 + d] = vnext; }
    DFX_DN_EACH {
      const double* dy = dyb + (size_t)k * sl.d_plane;
      double dqnext = dy[d] + h * (T.c[r] * dy[5 + d] + h * dsq[k]);
      double dvnext = dy[5 + d] + h * dsv[k];
      if (constrained) { dqnext = dcnext[k]; dvnext = 0.0; }
      double* dr = dro + (size_t)k * sl.d_plane;
      dr[d] = dqnext; dr[5 + d] = dvnext;
      if (d == 2) { dr[3] = 0.0; dr[4] = 0.0; }
    }
    if (d == 2) {
      double s, co;
      fast_sincos(0.5 * qnext, &s, &co);
      if (first) { ro[3] = co; ro[4] = s; }
    }
  }
}

// row j of fields (B, T, 2, nb, 3) and of this pass's fields_dot (B, KT, T, 2, nb, 3) from the step-base records
template <int K>
__global__ void k_tan_snapshot_multi(int B, int nb, int Tn, int j, const double* S, const double* D, TanSlices sl, double* fields,
                                     double* fields_dot) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)B * nb) return;
  const int m = (int)(gid / nb), b = (int)(gid % nb);
  const int slice = blockIdx.y;
  const size_t nd = (size_t)nb * 3;
  const size_t row = ((size_t)m * Tn + j) * 2 * nd;
  const double* r = S + (size_t)gid * kRec;
  if (slice == 0)
    for (int q = 0; q < 3; ++q) {
      fields[row + b * 3 + q] = r[q];
      fields[row + nd + b * 3 + q] = r[5 + q];
    }
  DFX_DN_EACH {
    const double* d = D + (size_t)(slice * K + k) * sl.d_plane + (size_t)gid * kRec;
    const size_t drow = (((size_t)m * sl.kt + slice * K + k) * Tn + j) * 2 * nd;
    for (int q = 0; q < 3; ++q) {
      fields_dot[drow + b * 3 + q] = d[q];
      fields_dot[drow + nd + b * 3 + q] = d[5 + q];
    }
  }
}

// The output of ONE right-hand-side evaluation (dfx_rhs_jvp) from what k_tan_init_multi and stage 0 of a step of size zero left behind: the
// step-base records Y / DY (velocities and their tangents) and row 0 of A / DA (accelerations and their tangents).  dy (B, 2, nb, 3) and this
// pass's dy_dots (B, KT, 2, nb, 3) are laid out as k_tan_snapshot_multi lays out one row of fields / fields_dot; the rows of prescribed DOFs
// are 0 (the stage already stores a = da = 0 there; their velocity is c'(t) in the records and is masked here).
template <int K>
__global__ void k_tan_rhs_out_multi(TanCtx c, const double* Y, const double* DY, const double* A, const double* DA, TanSlices sl, double* dy,
                                    double* dy_dots) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  const int slice = blockIdx.y;
  const size_t nd = (size_t)c.nb * 3;
  const size_t arow = (size_t)m * c.a_rows * nd + (size_t)b * 3;
  const size_t row = (size_t)m * 2 * nd;
  const int sidx = c.block_special[b];
  const int con_mask = sidx >= 0 ? c.special[sidx].con_mask : 0;
  const double* r = Y + (size_t)gid * kRec;
  if (slice == 0)
    for (int q = 0; q < 3; ++q) {
      dy[row + b * 3 + q] = ((con_mask >> q) & 1) ? 0.0 : r[5 + q];
      dy[row + nd + b * 3 + q] = A[arow + q];
    }
  DFX_DN_EACH {
    const double* d = DY + (size_t)(slice * K + k) * sl.d_plane + (size_t)gid * kRec;
    const double* da = DA + (size_t)(slice * K + k) * sl.da_plane + arow;
    const size_t drow = ((size_t)m * sl.kt + slice * K + k) * 2 * nd;
    for (int q = 0; q < 3; ++q) {
      dy_dots[drow + b * 3 + q] = ((con_mask >> q) & 1) ? 0.0 : d[5 + q];
      dy_dots[drow + nd + b * 3 + q] = da[q];
    }
  }
}

// rows [out_ptr[n], out_ptr[n + 1]) of fields and fields_dot from the dense output of step n: the quartic of the adaptive pass (k_prepare
// of dfx_kernels.h, the same expressions in the same order) on (q_n, q_n+1, q_mid, v_n, v_n+1) and on (v_n, v_n+1, v_mid, A_0, A_6), once,
// and the same linear formula on every tangent -- its coefficients hold primal step data only (h, theta).  One lane per (member, block).
template <int K>
__global__ void __launch_bounds__(256) k_tan_dense_multi(TanCtx c, TanDenseM dm) {
  const TanDense& dn = dm.d;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  if (dn.n >= c.n_steps[m]) return;
  const int32_t* op = dn.out_ptr + (size_t)m * dn.op_stride;
  const int lo = op[dn.n], hi = op[dn.n + 1];
  if (hi <= lo) return;
  const TanSlices& sl = dm.sl;
  const int slice = blockIdx.y;
  const double* mem = c.mem + (size_t)slice * sl.mem_plane + (size_t)m * tan_mem_n(K);
  const double h = c.tgrid[(size_t)m * c.grid_stride + 2 * (size_t)dn.n + 1];
  const size_t nd = (size_t)c.nb * 3;
  const double* A = dn.A + (size_t)m * c.a_rows * nd;
  const double* DA = dn.DA + (size_t)slice * K * sl.da_plane + (size_t)m * c.a_rows * nd;
  const double* y0 = dn.Y0 + (size_t)gid * kRec;
  const double* y1 = dn.Y1 + (size_t)gid * kRec;
  const int sidx = c.block_special[b];
  for (int d = 0; d < 3; ++d) {
    const size_t dof = (size_t)b * 3 + d;
    const bool constrained = sidx >= 0 && ((c.special[sidx].con_mask >> d) & 1);
    const double qn = y0[d], vn = y0[5 + d], q1 = y1[d], v1 = y1[5 + d];
    const double a0 = A[(size_t)dn.a0 * nd + dof], a6 = A[(size_t)dn.a6 * nd + dof];
    double sm = dn.cm[0] * a0 + dn.cm[6] * a6, sma = dn.cma[0] * a0 + dn.cma[6] * a6;
    for (int l = 1; l < 6; ++l) {
      const double al = A[(size_t)l * nd + dof];
      sm += dn.cm[l] * al; sma += dn.cma[l] * al;
    }
    const double qmid = qn + h * (0.5 * vn + h * sma), vmid = vn + h * sm;
    double dqn[K], dvn[K], dq1[K], dv1[K], da0[K], da6[K], dqmid[K], dvmid[K];
    DFX_DN_EACH {
      const double* dy0 = dn.DY0 + (size_t)(slice * K + k) * sl.d_plane + (size_t)gid * kRec;
      const double* dy1 = dn.DY1 + (size_t)(slice * K + k) * sl.d_plane + (size_t)gid * kRec;
      const double* DAk = DA + (size_t)k * sl.da_plane;
      dqn[k] = dy0[d]; dvn[k] = dy0[5 + d]; dq1[k] = dy1[d]; dv1[k] = dy1[5 + d];
      da0[k] = DAk[(size_t)dn.a0 * nd + dof]; da6[k] = DAk[(size_t)dn.a6 * nd + dof];
      double dsm = dn.cm[0] * da0[k] + dn.cm[6] * da6[k], dsma = dn.cma[0] * da0[k] + dn.cma[6] * da6[k];
      for (int l = 1; l < 6; ++l) {
        const double dal = DAk[(size_t)l * nd + dof];
        dsm += dn.cm[l] * dal; dsma += dn.cma[l] * dal;
      }
      dqmid[k] = dqn[k] + h * (0.5 * dvn[k] + h * dsma);
      dvmid[k] = dvn[k] + h * dsm;
    }
    for (int kk = lo; kk < hi; ++kk) {
      const double r = dn.theta[(size_t)m * dn.Tn + kk];
      double oq = dopri_dense(qn, q1, qmid, vn, v1, h, r), ov = dopri_dense(vn, v1, vmid, a0, a6, h, r);
      double doq[K], dov[K];
      DFX_DN_EACH {
        doq[k] = dopri_dense(dqn[k], dq1[k], dqmid[k], dvn[k], dv1[k], h, r);
        dov[k] = dopri_dense(dvn[k], dv1[k], dvmid[k], da0[k], da6[k], h, r);
      }
      if (constrained) {
        tan_drive_n<K>(c, m, mem, c.special[sidx].con_coef[d], dn.ts[kk], oq, ov, doq, slice * K);
        DFX_DN_EACH dov[k] = 0.0;
      }
      const size_t row = ((size_t)m * dn.Tn + kk) * 2 * nd;
      if (slice == 0) {
        dn.fields[row + dof] = oq;
        dn.fields[row + nd + dof] = ov;
      }
      DFX_DN_EACH {
        const size_t drow = (((size_t)m * sl.kt + slice * K + k) * dn.Tn + kk) * 2 * nd;
        dn.fields_dot[drow + dof] = doq[k];
        dn.fields_dot[drow + nd + dof] = dov[k];
      }
    }
  }
}

// ---- the signal sink ---------------------------------------------------------------------------------------------------------------------
constexpr int kTanSigThreads = 256;
constexpr int kTanSigQuads = kTanSigThreads / 4;      // items per workgroup (kObjQuads of dfx_objective.h)

struct TanSigArgs {
  const double *fields, *fields_dot;   // B * Tn * nb*6, and this pass's B * KT * Tn * nb*6
  const int32_t* fblocks;              // n_fb force blocks
  const int32_t* hslots;               // n_hg listed hinges: the slot block * 4 + node of each
  const int32_t* sig_ptr;              // n_sig + 1: the terms of signal s, in list order
  const int32_t* term_src;             // >= 0: offset of a field component inside one output time of the history; < 0: -(1 + channel)
  const double* term_coef;
  double *chan, *chan_dot;             // B * Tn * n_ch, and B * KT * Tn * n_ch
  double *S, *S_dot;                   // B * Tn * n_sig, and B * KT * Tn * n_sig
  int Tn, n_fb, n_sig;
  int n_hg, n_ch;                      // listed hinges; channels of one (member, output): (n_fb + n_hg) * 3, the hinges behind the blocks
};

// the own side of the ligament on `slot` (info = its slot_info, >= 0) of member m at output ko, for the directions of `slice`: the value and
// the KC epsilon parts of dE/d(x, y, theta) on the slot's block into f[0..2]
template <int MODEL, int CONTACT, int KC>
__device__ __forceinline__ void tan_signal_side(const TanCtx& c, const TanSlices& sl, const TanSigArgs& a, int m, int slice, int ko, int slot, int info,
                                                DualN<KC>* f) {
  constexpr int K = KC;
  const int b = slot >> 2;
  const int ps = info >> 1, pb = ps >> 2;
  const size_t nd = (size_t)c.nb * 3;
  const double* fr = a.fields + ((size_t)m * a.Tn + ko) * 2 * nd;
  TanSignalLigIn<KC> in;
  in.o.x = fr[(size_t)b * 3]; in.o.y = fr[(size_t)b * 3 + 1]; in.o.th = fr[(size_t)b * 3 + 2];
  in.p.x = fr[(size_t)pb * 3]; in.p.y = fr[(size_t)pb * 3 + 1]; in.p.th = fr[(size_t)pb * 3 + 2];
  fast_sincos(0.5 * in.o.th, &in.o.sh, &in.o.ch);
  fast_sincos(0.5 * in.p.th, &in.p.sh, &in.p.ch);
  DFX_DN_EACH {
    const double* fd = a.fields_dot + (((size_t)m * sl.kt + slice * K + k) * a.Tn + ko) * 2 * nd;
    in.dox[k] = fd[(size_t)b * 3]; in.doy[k] = fd[(size_t)b * 3 + 1]; in.doth[k] = fd[(size_t)b * 3 + 2];
    in.dpx[k] = fd[(size_t)pb * 3]; in.dpy[k] = fd[(size_t)pb * 3 + 1]; in.dpth[k] = fd[(size_t)pb * 3 + 2];
  }
  const double* tp = c.tp + (size_t)slice * sl.tp_plane + (size_t)m * c.nb * kSlots * tan_slot_n(K);
  const double* sp = tp + (size_t)slot * tan_slot_n(K);
  const double* pp = tp + (size_t)ps * tan_slot_n(K);
  in.rox = tan_par_n<K>(sp, 0); in.roy = tan_par_n<K>(sp, 1); in.rpx = tan_par_n<K>(pp, 0); in.rpy = tan_par_n<K>(pp, 1);
  in.lx = tan_par_n<K>(sp, 2); in.ly = tan_par_n<K>(sp, 3);
  in.ks = tan_par_n<K>(sp, 4); in.ksh = tan_par_n<K>(sp, 5); in.kr = tan_par_n<K>(sp, 6);
  if (CONTACT == 1) {
    const double* mem = c.mem + (size_t)slice * sl.mem_plane + (size_t)m * tan_mem_n(K);
    in.phi1 = tan_par_n<K>(sp, 7); in.phi2 = tan_par_n<K>(sp, 8);
    in.am = tan_scalar_n<K>(mem, 0, 3, kTanMemDir); in.ac = tan_scalar_n<K>(mem, 1, 4, kTanMemDir); in.kc = tan_scalar_n<K>(mem, 2, 5, kTanMemDir);
  }
  in.sgn = (info & 1) ? 1.0 : -1.0;
  tan_signal_lig<MODEL, CONTACT, KC>(in, f[0], f[1], f[2]);
}

// grid (chunks of kTanSigQuads items, members, slices of the pass)
template <int MODEL, int CONTACT, int KC>
__global__ __launch_bounds__(kTanSigThreads) void k_tan_signal_channels(TanCtx c, TanSlices sl, TanSigArgs a) {
  using D = DualN<KC>;
  constexpr int K = KC;
  const int m = blockIdx.y, slice = blockIdx.z;
  const long long total = (long long)a.Tn * a.n_fb;
  const long long item = (long long)blockIdx.x * kTanSigQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  const bool valid = item < total;
  D f[3];
  if (valid) {
    const int ko = (int)(item / a.n_fb);
    const int slot = a.fblocks[(int)(item % a.n_fb)] * kSlots + kk;
    const int info = c.slot_info[slot];
    if (info >= 0) tan_signal_side<MODEL, CONTACT, KC>(c, sl, a, m, slice, ko, slot, info, f);
  }
  // every lane of the quad takes part (slots without a ligament and the lanes of a padded item add zeros); direction order
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f[i].v = quad_sum(f[i].v);
    DFX_DN_EACH f[i].e[k] = quad_sum(f[i].e[k]);
  }
  if (valid && kk == 0) {
    if (slice == 0) {
      double* ch = a.chan + ((size_t)m * a.Tn + (size_t)(item / a.n_fb)) * (size_t)a.n_ch + (size_t)(item % a.n_fb) * 3;
      ch[0] = f[0].v; ch[1] = f[1].v; ch[2] = f[2].v;
    }
    DFX_DN_EACH {
      double* cd = a.chan_dot + (((size_t)m * sl.kt + slice * K + k) * a.Tn + (size_t)(item / a.n_fb)) * (size_t)a.n_ch + (size_t)(item % a.n_fb) * 3;
      cd[0] = f[0].e[k]; cd[1] = f[1].e[k]; cd[2] = f[2].e[k];
    }
  }
}

constexpr int kTanHingeThreads = 64;       // items per workgroup of k_tan_hinge_channels: one lane each

// grid (chunks of kTanHingeThreads (output, listed hinge) items, members, slices of the pass): the own side of ONE ligament, as a lane of
// k_tan_signal_channels evaluates it, with nothing summed: value (slice 0) and KC epsilon parts into the hinge's three channels, which sit
// behind the block channels of the (member, output) row.  Every listed slot carries a ligament (the host refuses the others).
template <int MODEL, int CONTACT, int KC>
__global__ __launch_bounds__(kTanHingeThreads) void k_tan_hinge_channels(TanCtx c, TanSlices sl, TanSigArgs a) {
  using D = DualN<KC>;
  constexpr int K = KC;
  const int m = blockIdx.y, slice = blockIdx.z;
  const long long total = (long long)a.Tn * a.n_hg;
  const long long item = (long long)blockIdx.x * kTanHingeThreads + threadIdx.x;
  if (item >= total) return;
  const int ko = (int)(item / a.n_hg), ih = (int)(item % a.n_hg);
  const int slot = a.hslots[ih];
  const int info = c.slot_info[slot];
  if (info < 0) return;
  D f[3];
  tan_signal_side<MODEL, CONTACT, KC>(c, sl, a, m, slice, ko, slot, info, f);
  const size_t at = (size_t)(a.n_fb + ih) * 3;
  if (slice == 0) {
    double* ch = a.chan + ((size_t)m * a.Tn + ko) * (size_t)a.n_ch + at;
    ch[0] = f[0].v; ch[1] = f[1].v; ch[2] = f[2].v;
  }
  DFX_DN_EACH {
    double* cd = a.chan_dot + (((size_t)m * sl.kt + slice * K + k) * a.Tn + ko) * (size_t)a.n_ch + at;
    cd[0] = f[0].e[k]; cd[1] = f[1].e[k]; cd[2] = f[2].e[k];
  }
}

// grid (chunks of kTanSigThreads (output, signal) pairs, members, directions of the pass)
__global__ __launch_bounds__(kTanSigThreads) void k_tan_signal_combine(TanSigArgs a, int nb, int kt) {
  const int m = blockIdx.y, d = blockIdx.z;
  const long long total = (long long)a.Tn * a.n_sig;
  const long long item = (long long)blockIdx.x * kTanSigThreads + threadIdx.x;
  if (item >= total) return;
  const int ko = (int)(item / a.n_sig), s = (int)(item % a.n_sig);
  const size_t nd = (size_t)nb * 3, row = (size_t)m * a.Tn + ko, drow = ((size_t)m * kt + d) * a.Tn + ko;
  const double* fd = a.fields_dot + drow * 2 * nd;
  const double* cd = a.chan_dot + drow * (size_t)a.n_ch;
  double Sd = 0.0;
  for (int t = a.sig_ptr[s]; t < a.sig_ptr[s + 1]; ++t) {
    const int src = a.term_src[t];
    Sd += a.term_coef[t] * (src >= 0 ? fd[src] : cd[-1 - src]);
  }
  a.S_dot[drow * a.n_sig + s] = Sd;
  if (d == 0) {
    const double* f = a.fields + row * 2 * nd;
    const double* ch = a.chan + row * (size_t)a.n_ch;
    double S = 0.0;
    for (int t = a.sig_ptr[s]; t < a.sig_ptr[s + 1]; ++t) {
      const int src = a.term_src[t];
      S += a.term_coef[t] * (src >= 0 ? f[src] : ch[-1 - src]);
    }
    a.S[row * a.n_sig + s] = S;
  }
}

// flags[blockIdx.x] = 1 when a non-finite entry of x[0, nx) or y[0, ny) lies on this workgroup's stride, else 0: every workgroup stores
// its own word, the host ORs them
__global__ __launch_bounds__(kTanSigThreads) void k_tan_finite_flags(const double* x, size_t nx, const double* y, size_t ny, int32_t* flags) {
  int bad = 0;
  for (size_t i = (size_t)blockIdx.x * kTanSigThreads + threadIdx.x; i < nx + ny; i += (size_t)gridDim.x * kTanSigThreads) {
    const double v = i < nx ? x[i] : y[i - nx];
    bad |= !isfinite(v);
  }
  __shared__ int red[kTanSigThreads / 64];
  const int any = __any(bad);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = any;
  __syncthreads();
  if (threadIdx.x == 0) {
    int r = 0;
    for (int wv = 0; wv < kTanSigThreads / 64; ++wv) r |= red[wv];
    flags[blockIdx.x] = r ? 1 : 0;
  }
}

#undef DFX_DN_EACH

}  // namespace dfx
