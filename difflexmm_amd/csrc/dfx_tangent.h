// dfx_tangent.h -- the forward-mode (tangent) solve: one Runge-Kutta stage of the primal and of its directional derivative together.
//
// What it differentiates is the fixed-grid solve of dfx_forward_grid / dfx_forward_grid_members with its steps frozen -- the map dfx_adjoint
// transposes.  One lane per (member, block):
//   * the block's stage record and those of its partners are seeded as Dual numbers with the tangent stage state (seed_rec: the half-angle
//     pair follows theta), and every per-ligament parameter as a Dual with its tangent (P = Dual): the epsilon parts of the forces that
//     bond_grad_p / contact_grad / distance_contact_grad return are exactly  H_uu du + H_up dp  for the block's own DOFs;
//   * DOF part, as fwd_dof (dfx_stage.h) plus its derivative: a = F / m  =>  da = (dF - a dm) / m, with F = F_load - dE/du - c v,
//     dF = dF_load - (dE/du).e - dc v - c dv;  driven DOFs  du_c = sum coef (dg/dp . dp)  (eval_time_fn's gp),  loaded DOFs
//     dF_load = sum load_coef (dg/dp . dp);  the RK combine of the next stage record is linear and takes the tangents alike.
// Branch decisions (angle-contact window, closest edge of the distance-based contact, time-function phases) are taken on the primal values
// only: the tangent follows the primal's branch, as the reverse sweep does.  Nothing is culled: every ligament is evaluated.
// The velocities of driven DOFs enter no force; their tangents are left at 0 here and the rows of prescribed DOFs in fields_dot are
// assembled on the host (difflexmm_amd/dynamics.py, DynamicSolver.jvp).
//
// dfx_forward_tangent_dense differentiates the ADAPTIVE solve instead -- the map dfx_adjoint transposes after dfx_forward_adaptive_keep: the
// same stage kernel on every member's own frozen accepted steps (TanCtx::n_steps: a member that is done leaves; one more stage 0 at its
// final state gives A_6 of its last step), and k_tan_dense forms the outputs inside the steps and their tangents by the quartic dense
// output of the adaptive pass, which is linear in (q_n, v_n, A_0 .. A_6) with coefficients that hold primal step data only.
//
// The parameter image is a plain per-slot layout of its own (value, then tangent), NOT the packed image of dfx_plan.h:pack_params, which
// is not linear in the parameters (it stores 1/m, a dictionary of reference vectors, uniform stiffnesses once per member).
#pragma once
#include <hip/hip_runtime.h>

#include "dfx_stage.h"

namespace dfx {

constexpr int kTanSlot = 18;     // per (member, slot): r(2) l(2) k(3) phi(2), then their tangents in the same order
constexpr int kTanBlk = 12;      // per (member, block): 1/m(3), d(1/m)(3), c(3), dc(3)
constexpr int kTanMem = 16;      // per member: contact(3), dcontact(3), dfn_params(DFX_MAX_FNS * DFX_FN_PARAMS)
constexpr int kTanCen = 4;       // per (member, block): block centroid(2), its tangent(2)   (distance-based contact)
static_assert(6 + DFX_MAX_FNS * DFX_FN_PARAMS <= kTanMem, "kTanMem");

struct TanCtx {
  int B, nb, n_fns, n_stages;
  const int32_t* slot_info;      // n_slots (shared)
  const int32_t* block_special;  // nb (shared)
  const dfx_special* special;
  const TimeFn* fns;             // B * DFX_MAX_FNS (the primal time functions: dfx_set_params' upload)
  const double* tp;              // B * n_slots * kTanSlot
  const double* blk;             // B * nb * kTanBlk
  const double* mem;             // B * kTanMem
  const double* cen;             // B * nb * kTanCen, or null
  const double* tgrid;           // n_grids * n_steps * 2: (t, h) of every step
  const double* t0;              // n_grids: the first output time
  long long grid_stride;         // elements between the grids of two members in tgrid (0: one grid)
  int t0_stride;                 // 1: one t0 per member, 0: shared
  int a_rows;                    // places per member in A / DA: n_stages, or 7 in the dense pass (A_6 = the FSAL acceleration)
  const long long* n_steps;      // B: the step count N_m of every member (dense pass), or null: every member takes every step
};

struct TanStage {
  const double *S_in, *D_in;     // primal / tangent records of this stage, B * nb * kRec (tangent: q at 0..2, v at 5..7)
  const double *Y, *DY;          // step base
  double *S_out, *D_out;         // next stage records (stage s-1: the next step base)
  double *A, *DA;                // stage accelerations and their tangents, B * a_rows * nb * 3
  long long n;                   // step ordinal
  int i;                         // stage index
  int a0;                        // place of A_0 of this step: 0, or in the dense pass 0 / 6 by the step's parity (A_0 of step n + 1 is A_6 of step n)
};

// the dense output of step n (dfx_forward_tangent_dense): launched after stage 0 of step n + 1 has left A_6
struct TanDense {
  const double *Y0, *DY0;        // step base of step n (records)
  const double *Y1, *DY1;        // step base of step n + 1
  const double *A, *DA;          // stage accelerations, 7 places per member
  const int32_t* out_ptr;        // B * op_stride: outputs [out_ptr[n], out_ptr[n + 1]) lie in step n
  const double* theta;           // B * Tn: relative position of every output in its step
  const double* ts;              // Tn output times
  double *fields, *fields_dot;   // B * Tn * 2 * nb * 3
  long long op_stride, n;
  int Tn, a0, a6;                // places of A_0 and A_6 of step n
  double cm[7], cma[7];          // mid-point weights (velocity / position form, Dopri of dfx_physics.h)
};

// (the kernels that are no templates are static: dfx_tangent_multi.h's translation unit reads this header too)
DFX_HD BlockRec<Dual> tan_rec(const double* S, const double* D, int b) {
  const BlockRec<double> r = load_rec(S, b);
  const double* d = D + (size_t)b * kRec;
  return seed_rec(r, d[0], d[1], d[2]);
}

DFX_HD Dual tan_par(const double* s, int j) { return Dual(s[j], s[9 + j]); }

// sum over f of coef_f * g_f(t) (and the tangent sum coef_f * dg_f/dp . dp_f)
DFX_HD void tan_drive(const TanCtx& c, int m, const double* coef /* DFX_MAX_FNS */, double t, double& g_sum, double& gt_sum, double& dg_sum) {
  g_sum = 0.0; gt_sum = 0.0; dg_sum = 0.0;
  const double* dfn = c.mem + (size_t)m * kTanMem + 6;
  for (int f = 0; f < c.n_fns; ++f) {
    if (coef[f] == 0.0) continue;
    double g, gt, gp[kMaxFnParams];
    eval_time_fn(c.fns[(size_t)m * DFX_MAX_FNS + f], t, g, gt, gp);
    double dg = 0.0;
    for (int k = 0; k < kMaxFnParams; ++k) dg += gp[k] * dfn[f * DFX_FN_PARAMS + k];
    g_sum += coef[f] * g;
    gt_sum += coef[f] * gt;
    dg_sum += coef[f] * dg;
  }
}

static __global__ void k_tan_init(TanCtx c, const double* state0, const double* state0_dot, double* S, double* D) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  const double t0 = c.t0[m * c.t0_stride];
  const int sidx = c.block_special[b];
  double* r = S + (size_t)gid * kRec;
  double* d = D + (size_t)gid * kRec;
  const size_t nd = (size_t)c.nb * 3;
  for (int k = 0; k < 3; ++k) {
    double q = state0 ? state0[(size_t)m * 2 * nd + b * 3 + k] : 0.0;
    double v = state0 ? state0[(size_t)m * 2 * nd + nd + b * 3 + k] : 0.0;
    double dq = state0_dot ? state0_dot[(size_t)m * 2 * nd + b * 3 + k] : 0.0;
    double dv = state0_dot ? state0_dot[(size_t)m * 2 * nd + nd + b * 3 + k] : 0.0;
    if (sidx >= 0 && ((c.special[sidx].con_mask >> k) & 1)) {
      tan_drive(c, m, c.special[sidx].con_coef[k], t0, q, v, dq);
      dv = 0.0;
    }
    r[k] = q; r[5 + k] = v;
    d[k] = dq; d[5 + k] = dv;
  }
  double s, co;
  fast_sincos(0.5 * r[2], &s, &co);
  r[3] = co; r[4] = s;
  d[3] = 0.0; d[4] = 0.0;
}

// node vectors of the bonded node, its next and its previous node on the block, as Duals (distance-based contact)
template <int NPB>
DFX_HD void tan_node_triple(const double* tp, int slot, Dual (&r)[3][2]) {
  const int b = slot >> 2, k = slot & 3;
  const int ks[3] = {k, (k + 1) % NPB, (k + NPB - 1) % NPB};
  for (int i = 0; i < 3; ++i) {
    const double* s = tp + (size_t)(b * kSlots + ks[i]) * kTanSlot;
    r[i][0] = tan_par(s, 0); r[i][1] = tan_par(s, 1);
  }
}

template <int MODEL, int CONTACT, int NPB>
__global__ void __launch_bounds__(256) k_tan_stage(TanCtx c, Tableau T, TanStage st) {
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
  const double* S_in = st.S_in + moff * kRec;
  const double* D_in = st.D_in + moff * kRec;
  const double* tp = c.tp + moff * kSlots * kTanSlot;
  const double* mem = c.mem + (size_t)m * kTanMem;
  const BlockRec<Dual> o = tan_rec(S_in, D_in, b);
  Dual f[3];
#pragma unroll
  for (int k = 0; k < NPB; ++k) {
    const int slot = b * kSlots + k;
    const int info = c.slot_info[slot];
    if (info < 0) continue;
    const int ps = info >> 1;
    const double sgn = (info & 1) ? 1.0 : -1.0;
    const double* sp = tp + (size_t)slot * kTanSlot;
    const double* pp = tp + (size_t)ps * kTanSlot;
    const BlockRec<Dual> p = tan_rec(S_in, D_in, ps >> 2);
    const Dual lx = tan_par(sp, 2), ly = tan_par(sp, 3);
    const Dual l0 = tsqrt(lx * lx + ly * ly);
    const Dual il0 = 1.0 / l0;
    BondGrad<Dual> g;
    bond_grad_p<MODEL, Dual, Dual>(o, p, tan_par(sp, 0), tan_par(sp, 1), tan_par(pp, 0), tan_par(pp, 1), lx, ly, l0, il0, tan_par(sp, 4),
                                   tan_par(sp, 5), tan_par(sp, 6), sgn, g);
    f[0] = f[0] + g.fx; f[1] = f[1] + g.fy; f[2] = f[2] + g.fth;
    const Dual am(mem[0], mem[3]), ac(mem[1], mem[4]), kc(mem[2], mem[5]);
    if (CONTACT == DFX_CONTACT_DISTANCE) {
      Dual ro[3][2], rp[3][2];
      tan_node_triple<NPB>(tp, slot, ro);
      tan_node_triple<NPB>(tp, ps, rp);
      const double* co = c.cen + (moff + b) * kTanCen;
      const double* cp = c.cen + (moff + (ps >> 2)) * kTanCen;
      DistContactGrad<Dual> dc;
      distance_contact_grad<Dual, Dual>(o, p, Dual(co[0], co[2]), Dual(co[1], co[3]), Dual(cp[0], cp[2]), Dual(cp[1], cp[3]), ro, rp, info & 1,
                                        am, ac, kc, dc);
      f[0] = f[0] + dc.fx; f[1] = f[1] + dc.fy; f[2] = f[2] + dc.fth;
    } else if (CONTACT == DFX_CONTACT_ANGLE) {
      ContactGrad<Dual> cg;
      const Dual kap = sgn * (o.th - p.th);
      contact_grad<Dual, Dual>(kap, tan_par(sp, 7), tan_par(sp, 8), am, ac, kc, cg);
      f[2] = f[2] + sgn * cg.dkap;
    }
  }
  // DOF part (fwd_dof of dfx_stage.h and its derivative)
  const double* tg = c.tgrid + (size_t)m * c.grid_stride + 2 * (size_t)st.n;
  const double t = tg[0], h = tg[1];
  const int i = st.i, r = i + 1;
  const double t_i = t + T.c[i] * h, t_next = t + T.c[r] * h;
  const int sidx = c.block_special[b];
  const double* bk = c.blk + (moff + b) * kTanBlk;
  const size_t nd = (size_t)c.nb * 3;
  double* A = st.A + (size_t)m * c.a_rows * nd;
  double* DA = st.DA + (size_t)m * c.a_rows * nd;
  const double* rin = S_in + (size_t)b * kRec;
  const double* din = D_in + (size_t)b * kRec;
  const double* yb = st.Y + (moff + b) * kRec;
  const double* dyb = st.DY + (moff + b) * kRec;
  double* ro = st.S_out + (moff + b) * kRec;
  double* dro = st.D_out + (moff + b) * kRec;
  for (int d = 0; d < 3; ++d) {
    const size_t dof = (size_t)b * 3 + d;
    bool constrained = false;
    double fload = 0.0, dfload = 0.0, cnext = 0.0, cdnext = 0.0, dcnext = 0.0;
    if (sidx >= 0) {
      const dfx_special& sp = c.special[sidx];
      constrained = (sp.con_mask >> d) & 1;
      double unused;
      if (constrained) tan_drive(c, m, sp.con_coef[d], t_next, cnext, cdnext, dcnext);
      else tan_drive(c, m, sp.load_coef[d], t_i, fload, unused, dfload);
    }
    const double v_i = rin[5 + d], dv_i = din[5 + d];
    const double inv_m = bk[d], dinv_m = bk[3 + d], damp = bk[6 + d], ddamp = bk[9 + d];
    const double a = constrained ? 0.0 : (fload - f[d].v - damp * v_i) * inv_m;
    // a = F / m: da = dF / m + F d(1/m)
    const double da = constrained ? 0.0 : (dfload - f[d].e - ddamp * v_i - damp * dv_i) * inv_m + (fload - f[d].v - damp * v_i) * dinv_m;
    A[(size_t)(i ? i : st.a0) * nd + dof] = a;
    DA[(size_t)(i ? i : st.a0) * nd + dof] = da;
    double sv = T.a[r][i] * a, sq = T.aa[r][i] * a, dsv = T.a[r][i] * da, dsq = T.aa[r][i] * da;
    for (int l = 0; l < i; ++l) {
      const size_t row = l ? l : st.a0;
      const double al = A[row * nd + dof], dal = DA[row * nd + dof];
      sv += T.a[r][l] * al; sq += T.aa[r][l] * al;
      dsv += T.a[r][l] * dal; dsq += T.aa[r][l] * dal;
    }
    double qnext = yb[d] + h * (T.c[r] * yb[5 + d] + h * sq);
    double vnext = yb[5 + d] + h * sv;
    double dqnext = dyb[d] + h * (T.c[r] * dyb[5 + d] + h * dsq);
    double dvnext = dyb[5 + d] + h * dsv;
    if (constrained) { qnext = cnext; vnext = cdnext; dqnext = dcnext; dvnext = 0.0; }
    ro[d] = qnext; ro[5 + d] = vnext;
    dro[d] = dqnext; dro[5 + d] = dvnext;
    if (d == 2) {
      double s, co;
      fast_sincos(0.5 * qnext, &s, &co);
      ro[3] = co; ro[4] = s;
      dro[3] = 0.0; dro[4] = 0.0;
    }
  }
}

// row k of fields and fields_dot (B, T, 2, nb, 3) from the step-base records
static __global__ void k_tan_snapshot(int B, int nb, int Tn, int k, const double* S, const double* D, double* fields, double* fields_dot) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)B * nb) return;
  const int m = (int)(gid / nb), b = (int)(gid % nb);
  const size_t nd = (size_t)nb * 3;
  const size_t row = ((size_t)m * Tn + k) * 2 * nd;
  const double* r = S + (size_t)gid * kRec;
  const double* d = D + (size_t)gid * kRec;
  for (int j = 0; j < 3; ++j) {
    fields[row + b * 3 + j] = r[j];
    fields[row + nd + b * 3 + j] = r[5 + j];
    fields_dot[row + b * 3 + j] = d[j];
    fields_dot[row + nd + b * 3 + j] = d[5 + j];
  }
}

// rows [out_ptr[n], out_ptr[n + 1]) of fields and fields_dot from the dense output of step n: the quartic of the adaptive pass (k_prepare
// of dfx_kernels.h, the same expressions in the same order) on (q_n, q_n+1, q_mid, v_n, v_n+1) and on (v_n, v_n+1, v_mid, A_0, A_6), and
// the same linear formula on their tangents -- its coefficients hold primal step data only (h, theta).  One lane per (member, block).
static __global__ void __launch_bounds__(256) k_tan_dense(TanCtx c, TanDense dn) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)c.B * c.nb) return;
  const int m = (int)(gid / c.nb), b = (int)(gid % c.nb);
  if (dn.n >= c.n_steps[m]) return;
  const int32_t* op = dn.out_ptr + (size_t)m * dn.op_stride;
  const int lo = op[dn.n], hi = op[dn.n + 1];
  if (hi <= lo) return;
  const double h = c.tgrid[(size_t)m * c.grid_stride + 2 * (size_t)dn.n + 1];
  const size_t nd = (size_t)c.nb * 3;
  const double* A = dn.A + (size_t)m * c.a_rows * nd;
  const double* DA = dn.DA + (size_t)m * c.a_rows * nd;
  const double* y0 = dn.Y0 + (size_t)gid * kRec;
  const double* dy0 = dn.DY0 + (size_t)gid * kRec;
  const double* y1 = dn.Y1 + (size_t)gid * kRec;
  const double* dy1 = dn.DY1 + (size_t)gid * kRec;
  const int sidx = c.block_special[b];
  for (int d = 0; d < 3; ++d) {
    const size_t dof = (size_t)b * 3 + d;
    const bool constrained = sidx >= 0 && ((c.special[sidx].con_mask >> d) & 1);
    const double qn = y0[d], vn = y0[5 + d], q1 = y1[d], v1 = y1[5 + d];
    const double dqn = dy0[d], dvn = dy0[5 + d], dq1 = dy1[d], dv1 = dy1[5 + d];
    const double a0 = A[(size_t)dn.a0 * nd + dof], a6 = A[(size_t)dn.a6 * nd + dof];
    const double da0 = DA[(size_t)dn.a0 * nd + dof], da6 = DA[(size_t)dn.a6 * nd + dof];
    double sm = dn.cm[0] * a0 + dn.cm[6] * a6, sma = dn.cma[0] * a0 + dn.cma[6] * a6;
    double dsm = dn.cm[0] * da0 + dn.cm[6] * da6, dsma = dn.cma[0] * da0 + dn.cma[6] * da6;
    for (int l = 1; l < 6; ++l) {
      const double al = A[(size_t)l * nd + dof], dal = DA[(size_t)l * nd + dof];
      sm += dn.cm[l] * al; sma += dn.cma[l] * al;
      dsm += dn.cm[l] * dal; dsma += dn.cma[l] * dal;
    }
    const double qmid = qn + h * (0.5 * vn + h * sma), vmid = vn + h * sm;
    const double dqmid = dqn + h * (0.5 * dvn + h * dsma), dvmid = dvn + h * dsm;
    for (int kk = lo; kk < hi; ++kk) {
      const double r = dn.theta[(size_t)m * dn.Tn + kk];
      double oq = dopri_dense(qn, q1, qmid, vn, v1, h, r), ov = dopri_dense(vn, v1, vmid, a0, a6, h, r);
      double doq = dopri_dense(dqn, dq1, dqmid, dvn, dv1, h, r), dov = dopri_dense(dvn, dv1, dvmid, da0, da6, h, r);
      if (constrained) { tan_drive(c, m, c.special[sidx].con_coef[d], dn.ts[kk], oq, ov, doq); dov = 0.0; }
      const size_t row = ((size_t)m * dn.Tn + kk) * 2 * nd;
      dn.fields[row + dof] = oq;
      dn.fields[row + nd + dof] = ov;
      dn.fields_dot[row + dof] = doq;
      dn.fields_dot[row + nd + dof] = dov;
    }
  }
}

}  // namespace dfx
