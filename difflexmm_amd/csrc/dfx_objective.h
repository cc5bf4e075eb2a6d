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
//
// The ligament strain-energy objective (dfx_strain_objective_value[_and_grad]) is a weighted sum over LIGAMENTS and output times,
//   J_m = sum_k tau_k sum_bonds w_mb [ c_stretch E_stretch + c_shear E_shear + c_bend E_bend + c_contact E_contact ](bond; u_k, params_m)
// The bond energy is linear in its three stiffnesses and the contact penalty in k_contact, so the weighted energy of a ligament is the plain
// energy evaluated with (c_stretch k_stretch, c_shear k_shear, c_bend k_rot) and c_contact k_contact, times w tau: ONE evaluation of
// bond_grad / contact_grad (dfx_physics.h) gives the value and every first derivative.  The host turns the bond weights into slot weights
// (both end slots of a ligament carry its weight) and lists the blocks that own a weighted end; an item is one (output time k, listed
// block j) pair of one member, its four slots on the four lanes of a DPP quad.
//   k_strain_objective           every lane whose slot carries a weighted ligament evaluates its OWN side of it in gather form (as the forward
//                                stage does: no atomics), the quad adds dE/d(x, y, theta) in the fixed order of quad_sum and lane 0 stores rows
//                                0..2 of G[(k, m, b)]; a ligament's energy is counted on its end-0 lane; partials / k_objective_finish as above
//   k_strain_objective_explicit  after the sweep: d J / d(own node vector) into g_r, the two void-angle terms into g_phi (phi1 on the end-0
//                                slot, phi2 on the end-1 slot, as the reverse stage), and on end-0 slots d J / d(reference vector, stiffnesses,
//                                contact constants) into g_b when the call collects them; one lane per (member, listed slot), output times in order
//
// The signal misfit (dfx_signal_values, dfx_signal_misfit_value[_and_grad]): a signal is a linear combination of displacement, velocity and
// elastic-force components of listed blocks, J_m = 1/2 sum_k tau_k sum_s omega_s (S_mks - Starget_mks)^2.  The per-ligament arithmetic is
// dfx_signal.h (host and device).  FORCE blocks are the blocks with a force term; the SET holds them and the blocks bonded to them.
//   k_signal_channels   items (output k, force block j), the four slots of an item on one DPP quad: each lane its own side of its ligament
//                       in gather form, quad_sum gives dE/d(x, y, theta) of the block, lane 0 stores the three channels
//   k_signal_residual   one lane per (member, output, signal): the signal's terms in list order (field terms straight from the history)
//                       give S; the residual cotangent c = tau omega (S - Starget) is stored beside it; value partials / k_objective_finish
//   k_signal_direction  one lane per (member, output, distinct (block, component)): sum coef c over the terms that name it, in list order --
//                       a field component goes to its own row of G, a force component into the direction w
//   k_signal_cotangent  items (output k, block j of the set): Dual records seeded with w on the own and the partner block, the quad-summed
//                       epsilon parts of dE/d(x, y, theta) are (K w) on the block: ADDED to rows 0..2 of G[(k, m, b)] by lane 0
//   k_signal_explicit   after the sweep: one lane per (member, slot of the set), output times in order: the epsilon parts of dE/d(node
//                       vector) into g_r, of dE/dphi1 (end-0 slot) / dE/dphi2 (end-1 slot) into g_phi, and on end-0 slots of dE/d(reference
//                       vector, stiffnesses, contact constants) into g_b when the call collects them
// HINGE channels (components 9 + 3 n + d): dE_h/d(x, y, theta)_b of ONE ligament, the one on node n of block b -- the summand that
// k_signal_channels adds over a block's four slots.  The listed hinges extend the channel space behind the block channels: a (member, output)
// row of chan and of w holds n_fb * 3 block entries, then n_hg * 3 hinge entries.  The set also holds the two end blocks of every listed hinge.
//   k_signal_hinge_channels  one lane per (output k, listed hinge): the own side of that ligament, nothing summed across lanes
//   the cotangent of a hinge direction w_h is Hess(E_h) w_h on both end blocks: in k_signal_cotangent / k_signal_explicit the lane on the
//   hinge's own slot adds w_h to its own-block seed and the lane on the partner slot adds it to its partner-block seed (signal_seed_hinge;
//   the seeds are linear) -- still one evaluation per lane, the quad sum and lane 0's store as before, so two hinges of a block never
//   meet in a row of G from two lanes.  A call without hinge terms takes none of these branches: the arithmetic of the parent, bit for bit.
//
// The signal projections (dfx_signal_projections, dfx_signal_projection_value[_and_grad]): the same signals projected on n_rows rows of a
// time basis B shared by the members, P_msj = sum_k B_jk S_mks, J_m = 1/2 sum_s sum_j W_sj (P_msj - Ptarget_msj)^2.  S comes from
// k_signal_channels + k_signal_residual run without targets; from the cotangent c on, k_signal_direction / _cotangent / _explicit as above.
//   k_signal_project           the time reduction, one wave per (member, signal, row): lane l adds B_jk S_mks for k = l, l + 64, ... in
//                              ascending order, then obj_wave_sum over the lanes -- the order is fixed by (T, lane) alone.  Lane 0 stores
//                              P and holds the pair's term of the value: every (s, j) is counted once; the waves of a workgroup are added
//                              in order into its partial, k_objective_finish adds the partials
//   k_signal_project_residual  one lane per (member, output, signal): c_mks = sum_j W_sj (P_msj - Ptarget_msj) B_jk, j ascending, into
//                              the residual-cotangent buffer
//
// The signal cross-correlation (dfx_signal_xcorr, dfx_signal_xcorr_value[_and_grad]): pairs (A_p, B_p) of those signals (B_p may be a
// column of a fixed template array) correlated over the lags d = -D .. D in output indices, R[d] = sum_p sum_k A_p[k] B_p[k + d],
// rho = R / N with N = EA = sum A^2 ("reference"), sqrt(EA EB) ("coefficient") or 1 ("none"); a reduction over the lags (the value at one
// lag, the maximum, a softmax) gives a peak M and a delay delta, J = w_peak M + 1/2 w_delay (delta - delta_target)^2.  S as for the
// projections; from the cotangent c on, k_signal_direction / _cotangent / _explicit as above.
//   k_signal_xcorr           one wave per (member, lag) and two more per member for EA and EB: lane l adds outputs l, l + 64, ... ascending
//                            with the pairs ascending inside, then obj_wave_sum
//   k_signal_xcorr_reduce    one wave per member: N, rho, the reduction in a fixed lane-strided order, J, M, delta and the cotangents
//                            Rbar = (dJ/d rho) / N on the lags and (eA, eB) on the energies.  Ties of the maximum: the lowest lag takes the
//                            whole gradient (the subgradient np.argmax implies; JAX's max splits a tie evenly -- ties are a set of
//                            measure zero).  A member with N == 0 gets NaN values and an all-zero cotangent
//   k_signal_xcorr_residual  one lane per (member, output, signal): c from Rbar, eA, eB, the signals and the templates, pairs and lags
//                            ascending, into the residual-cotangent buffer; lags whose Rbar is exactly 0 are skipped
//
// The signal spectral ratios (dfx_signal_spectrum, dfx_signal_spectrum_value[_and_grad]): a third occupant of that slot.  G groups of two
// non-negative forms of the projections, N_mg = n0_g + sum W^n_gsj P_msj^2 and D_mg likewise, a measure l = N / D or ln N - ln D per group,
// J = sum_g a_g l_g or its KS smooth maximum.  S and P as for the projections (k_signal_project with W == nullptr); from c on as above.
//   k_signal_spectrum_forms     one wave per (member, group, side): lane l adds W P^2 over the (signal, row) pairs l, l + 64, ... ascending,
//                               obj_wave_sum, lane 0 adds the offset
//   k_signal_spectrum_reduce    one wave per member, lane l holds groups l, l + 64, ...: the measures, the maximum (lowest group on a tie),
//                               the exponent sums with the maximum subtracted; J, l, lam dl/dN, lam dl/dD.  A member with some D <= 0 (LOG:
//                               or N <= 0; KS: or a non-finite l) gets J = NaN, NaN in the offending l and an all-zero cotangent
//   k_signal_spectrum_weights   one lane per (member, signal, row): Weff = 2 sum_g (lam dl/dN Wn + lam dl/dD Wd), g ascending
//   k_signal_spectrum_residual  k_signal_project_residual with per-member weights and no targets: c_mks = sum_j Weff_msj P_msj B_jk
//
// The peak ligament strain (dfx_strain_peak_value[_and_grad]): NOT a sum but a smooth maximum over (output time, ligament) pairs of
//   q_mkb = a_mb (l0 eps)^2 + s_mb (l0 gamma)^2 + r_mb kappa^2 = 2 E_bond with the coefficient triple in place of the stiffnesses,
// weighted W = tau_k omega_mb >= 0: KS  J = q_hat + log(sum W exp(beta (q - q_hat))) / beta, or PNORM  J = q_hat (sum W (q / q_hat)^p)^(1/p).
// Items and quads as for the strain energy.  The softmax weights pi need the global maximum and sum first, hence four passes:
//   k_strain_peak_measure    q of every counted pair (end-0 lane) into a scratch image by (member, output, bond), per-workgroup (maximum, key k * n_bonds + bond);
//                            k_strain_peak_finish reduces them to q_hat, k_hat, b_hat per member (ties: the lowest key)
//   k_strain_peak_sum        the terms from the stored q: wave sum, waves in order, one partial per workgroup; k_strain_peak_value adds the
//                            partials as k_objective_finish does and forms J (J, q_hat, k_hat, b_hat into pinned host memory)
//   k_strain_peak_cotangent  the ligament gradient again (nothing but q is stored; both ends of a ligament read the same q, hence the same
//                            pi), times 2 pi, quad-summed into rows 0..2 of G
//   k_strain_peak_explicit   after the sweep: 2 pi dE/d(node vector) into g_r and, on end-0 slots, 2 pi dE/d(reference vector) into g_b[0..1]
// No atomics anywhere: the same history gives the same bits.
#pragma once
#include "dfx_kernels.h"
#include "dfx_signal.h"

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

// ---- ligament strain energy ------------------------------------------------------------------------------------------------------
constexpr int kObjStrain = 2;              // ObjJob::kind of a strain call (not a DFX_OBJ_* kind: the entries of its own set it)
constexpr int kObjQuads = kObjThreads / 4;  // items per workgroup

// ObjArgs of a strain call: blocks = listed blocks, w = SLOT weights (w_members * n_slots: both end slots of a ligament carry its weight),
// lever = the four part coefficients (c_stretch, c_shear, c_bend, c_contact)
struct StrainLig {
  BondGrad<double> g;
  ContactGrad<double> cg;       // zeros unless CONTACT == 1 and c_contact != 0
  double sgn;
  bool end0;
};

// one side of the ligament on `slot` at output time k of member m, stiffnesses scaled by the part coefficients; parameters from the
// resident images as k_response reads them
template <int MODEL, int CONTACT>
__device__ __forceinline__ void strain_eval(const DevCtx& c, const MemberBases& B, const double* f, int slot, int info, const double* parts,
                                            StrainLig& S) {
  const int b = slot >> 2, ps = info >> 1, pb = ps >> 2;
  BlockRec<double> o, p;
  o.x = f[(size_t)b * 3]; o.y = f[(size_t)b * 3 + 1]; o.th = f[(size_t)b * 3 + 2];
  p.x = f[(size_t)pb * 3]; p.y = f[(size_t)pb * 3 + 1]; p.th = f[(size_t)pb * 3 + 2];
  fast_sincos(0.5 * o.th, &o.sh, &o.ch);
  fast_sincos(0.5 * p.th, &p.sh, &p.ch);
  const double2 ro = ldg<double2>(B.p_r, (u32)slot * 16), rp = ldg<double2>(B.p_r, (u32)ps * 16);
  double lx, ly, l0, il0, ks, ksh, kr;
  if (c.l_dict_on) {
    const int li = B.p_lidx[slot];
    lx = B.l_dict[li * 4]; ly = B.l_dict[li * 4 + 1]; l0 = B.l_dict[li * 4 + 2]; il0 = B.l_dict[li * 4 + 3];
  } else {
    lx = B.p_l[(size_t)slot * 2]; ly = B.p_l[(size_t)slot * 2 + 1]; l0 = sqrt(lx * lx + ly * ly); il0 = 1.0 / l0;
  }
  if (c.k_uniform) { ks = B.cst[3]; ksh = B.cst[4]; kr = B.cst[5]; }
  else { ks = B.p_k[(size_t)slot * 4]; ksh = B.p_k[(size_t)slot * 4 + 1]; kr = B.p_k[(size_t)slot * 4 + 2]; }
  S.sgn = (info & 1) ? 1.0 : -1.0;
  S.end0 = !(info & 1);
  bond_grad<MODEL, double>(o, p, ro.x, ro.y, rp.x, rp.y, lx, ly, l0, il0, parts[0] * ks, parts[1] * ksh, parts[2] * kr, S.sgn, S.g);
  S.cg.dkap = S.cg.p1 = S.cg.p2 = S.cg.am = S.cg.ac = S.cg.kc = S.cg.e = 0.0;
  if (CONTACT == 1 && parts[3] != 0.0) {
    const double2 ph = ldg<double2>(B.p_phi, (u32)slot * 16);
    contact_grad<double>(S.sgn * (o.th - p.th), ph.x, ph.y, B.cst[0], B.cst[1], parts[3] * B.cst[2], S.cg);
  }
}

// grid (chunks of kObjQuads items, members): a wave never spans two members, the four slots of an item sit in one DPP quad
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(kObjThreads) void k_strain_objective(DevCtx c, ObjArgs a, double* G, double* partial) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_act;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  const bool valid = item < total;
  double val = 0.0, fx = 0.0, fy = 0.0, fth = 0.0;
  int k = 0, b = 0;
  if (valid) {
    k = (int)(item / a.n_act);
    b = a.blocks[(int)(item % a.n_act)];
    const int slot = b * 4 + kk;
    const int info = c.slot_info[slot];
    const double tw = (a.tau ? a.tau[k] : 1.0) * a.w[(size_t)m * a.w_stride + slot];
    if (info >= 0 && tw != 0.0) {
      const MemberBases B = member_bases(c, m);
      const size_t nd = (size_t)c.n_blocks * 3;
      StrainLig S;
      strain_eval<MODEL, CONTACT>(c, B, a.fields + ((size_t)m * c.n_timepoints + k) * nd * 2, slot, info, a.lever, S);
      fx = tw * S.g.fx; fy = tw * S.g.fy; fth = tw * (S.g.fth + S.sgn * S.cg.dkap);
      if (S.end0) val = tw * (S.g.e + S.cg.e);
    }
  }
  // every lane of the quad takes part (lanes without a weighted ligament, and the lanes of a padded item, add zeros)
  fx = quad_sum(fx); fy = quad_sum(fy); fth = quad_sum(fth);
  if (valid && G && kk == 0) {
    double* g = G + ((size_t)k * c.batch + m) * ((size_t)c.n_blocks * 6) + (size_t)b * 6;
    g[0] = fx; g[1] = fy; g[2] = fth;
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

// grid (chunks of 64 listed slots, members); every accumulator entry touched belongs to one lane
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(64) void k_strain_objective_explicit(DevCtx c, ObjArgs a) {
  const int m = blockIdx.y;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= a.n_act * 4) return;
  const int slot = a.blocks[idx >> 2] * 4 + (idx & 3);
  const int info = c.slot_info[slot];
  const double w = a.w[(size_t)m * a.w_stride + slot];
  if (info < 0 || w == 0.0) return;
  const MemberBases B = member_bases(c, m);
  const size_t nd = (size_t)c.n_blocks * 3;
  const bool bonds = c.g_b && !(info & 1);
  double rx = 0.0, ry = 0.0, phi = 0.0, q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < c.n_timepoints; ++k) {
    const double tw = (a.tau ? a.tau[k] : 1.0) * w;
    if (tw == 0.0) continue;
    StrainLig S;
    strain_eval<MODEL, CONTACT>(c, B, a.fields + ((size_t)m * c.n_timepoints + k) * nd * 2, slot, info, a.lever, S);
    rx += tw * S.g.rx; ry += tw * S.g.ry;
    phi += tw * (S.end0 ? S.cg.p1 : S.cg.p2);
    if (bonds) {
      q[0] += tw * S.g.lx; q[1] += tw * S.g.ly;
      q[2] += tw * (a.lever[0] * S.g.ks); q[3] += tw * (a.lever[1] * S.g.ksh); q[4] += tw * (a.lever[2] * S.g.kr);
      q[5] += tw * S.cg.am; q[6] += tw * S.cg.ac; q[7] += tw * (a.lever[3] * S.cg.kc);
    }
  }
  const size_t ms = (size_t)m * c.n_slots + slot;
  c.g_r[ms * 2] += rx; c.g_r[ms * 2 + 1] += ry;
  if (CONTACT == 1 && phi != 0.0) { c.g_phi[ms] += phi; c.touch[0] = 1; }
  if (bonds) for (int i = 0; i < 8; ++i) c.g_b[ms * 8 + i] += q[i];
}

// ---- signal misfit ------------------------------------------------------------------------------------------------------------------
constexpr int kObjSignal = 3;              // ObjJob::kind of a signal-misfit call

struct SigArgs {
  const double* fields;       // batch * T * n_blocks*6
  const int32_t* fblocks;     // n_fb force blocks
  const int32_t* fmap;        // n_blocks: index of the block in fblocks, or -1
  const int32_t* set;         // n_set blocks: force blocks and the blocks bonded to them, and both end blocks of every listed hinge
  const int32_t* hslots;      // n_hg listed hinges: the slot block * 4 + node of each (null when n_hg == 0)
  const int32_t* hmap;        // n_slots: index of the slot in hslots, or -1 (null when n_hg == 0)
  const int32_t* sig_ptr;     // n_sig + 1: the terms of signal s, in list order
  const int32_t* term_src;    // >= 0: offset of a field component inside one output time of the history; < 0: -(1 + channel)
  const double* term_coef;
  const int32_t* uc_ptr;      // n_uc + 1: the terms that name distinct (block, component) number i, in list order
  const int32_t* uc_dst;      // >= 0: b*6 + row inside G of one (output, member); < 0: -(1 + channel) inside w
  const int32_t* uc_sig;      // signal of each such term
  const double* uc_coef;
  const double* target;       // (T, n_sig), members target_stride apart (0: shared); null: signal values only
  const double* omega;        // n_sig or null
  const double* tau;          // T or null
  double *chan, *S, *cres, *w;  // batch * T * (n_ch | n_sig | n_sig | n_ch)
  long long target_stride;
  int n_fb, n_set, n_sig, n_uc;
  int n_hg, n_ch;             // listed hinges; channels of one (member, output): (n_fb + n_hg) * 3
};

// what one side of the ligament on `slot` reads at one output time (f: the member's history at that time), as strain_eval
__device__ __forceinline__ void signal_load(const DevCtx& c, const MemberBases& B, const double* f, int slot, int info, int contact, SignalLigIn& in) {
  const int b = slot >> 2, ps = info >> 1, pb = ps >> 2;
  in.o.x = f[(size_t)b * 3]; in.o.y = f[(size_t)b * 3 + 1]; in.o.th = f[(size_t)b * 3 + 2];
  in.p.x = f[(size_t)pb * 3]; in.p.y = f[(size_t)pb * 3 + 1]; in.p.th = f[(size_t)pb * 3 + 2];
  fast_sincos(0.5 * in.o.th, &in.o.sh, &in.o.ch);
  fast_sincos(0.5 * in.p.th, &in.p.sh, &in.p.ch);
  const double2 ro = ldg<double2>(B.p_r, (u32)slot * 16), rp = ldg<double2>(B.p_r, (u32)ps * 16);
  in.rox = ro.x; in.roy = ro.y; in.rpx = rp.x; in.rpy = rp.y;
  if (c.l_dict_on) {
    const int li = B.p_lidx[slot];
    in.lx = B.l_dict[li * 4]; in.ly = B.l_dict[li * 4 + 1]; in.l0 = B.l_dict[li * 4 + 2]; in.il0 = B.l_dict[li * 4 + 3];
  } else {
    in.lx = B.p_l[(size_t)slot * 2]; in.ly = B.p_l[(size_t)slot * 2 + 1]; in.l0 = sqrt(in.lx * in.lx + in.ly * in.ly); in.il0 = 1.0 / in.l0;
  }
  if (c.k_uniform) { in.ks = B.cst[3]; in.ksh = B.cst[4]; in.kr = B.cst[5]; }
  else { in.ks = B.p_k[(size_t)slot * 4]; in.ksh = B.p_k[(size_t)slot * 4 + 1]; in.kr = B.p_k[(size_t)slot * 4 + 2]; }
  in.sgn = (info & 1) ? 1.0 : -1.0;
  in.phi1 = in.phi2 = in.am = in.ac = in.kc = 0.0;
  if (contact) {
    const double2 ph = ldg<double2>(B.p_phi, (u32)slot * 16);
    in.phi1 = ph.x; in.phi2 = ph.y; in.am = B.cst[0]; in.ac = B.cst[1]; in.kc = B.cst[2];
  }
}

// grid (chunks of kObjQuads items, members)
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(kObjThreads) void k_signal_channels(DevCtx c, SigArgs a) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_fb;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  const bool valid = item < total;
  double fx = 0.0, fy = 0.0, fth = 0.0;
  if (valid) {
    const int k = (int)(item / a.n_fb);
    const int slot = a.fblocks[(int)(item % a.n_fb)] * 4 + kk;
    const int info = c.slot_info[slot];
    if (info >= 0) {
      SignalLigIn in;
      signal_load(c, member_bases(c, m), a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info, CONTACT, in);
      signal_lig_force<MODEL, CONTACT>(in, fx, fy, fth);
    }
  }
  // every lane of the quad takes part (slots without a ligament and the lanes of a padded item add zeros)
  fx = quad_sum(fx); fy = quad_sum(fy); fth = quad_sum(fth);
  if (valid && kk == 0) {
    double* ch = a.chan + ((size_t)m * c.n_timepoints + (size_t)(item / a.n_fb)) * (size_t)a.n_ch + (size_t)(item % a.n_fb) * 3;
    ch[0] = fx; ch[1] = fy; ch[2] = fth;
  }
}

constexpr int kHingeThreads = 64;          // items per workgroup of k_signal_hinge_channels: one lane each

// grid (chunks of kHingeThreads (output, listed hinge) items, members): the own side of the hinge's ligament -- the summand of
// k_signal_channels, stored behind the block channels of its (member, output) row.  Every listed slot carries a ligament (the host refuses
// the others), so a lane needs no neighbour and nothing is summed.
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(kHingeThreads) void k_signal_hinge_channels(DevCtx c, SigArgs a) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_hg;
  const long long item = (long long)blockIdx.x * kHingeThreads + threadIdx.x;
  if (item >= total) return;
  const int k = (int)(item / a.n_hg), i = (int)(item % a.n_hg);
  const int slot = a.hslots[i];
  const int info = c.slot_info[slot];
  if (info < 0) return;
  SignalLigIn in;
  double fx, fy, fth;
  signal_load(c, member_bases(c, m), a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info, CONTACT, in);
  signal_lig_force<MODEL, CONTACT>(in, fx, fy, fth);
  double* ch = a.chan + ((size_t)m * c.n_timepoints + k) * (size_t)a.n_ch + (size_t)(a.n_fb + i) * 3;
  ch[0] = fx; ch[1] = fy; ch[2] = fth;
}

// grid (chunks of kObjThreads (output, signal) pairs, members)
__global__ __launch_bounds__(kObjThreads) void k_signal_residual(DevCtx c, SigArgs a, double* partial) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_sig;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  double val = 0.0;
  if (item < total) {
    const int k = (int)(item / a.n_sig), s = (int)(item % a.n_sig);
    const double* f = a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6);
    const double* ch = a.chan + ((size_t)m * c.n_timepoints + k) * (size_t)a.n_ch;
    double S = 0.0;
    for (int t = a.sig_ptr[s]; t < a.sig_ptr[s + 1]; ++t) {
      const int src = a.term_src[t];
      S += a.term_coef[t] * (src >= 0 ? f[src] : ch[-1 - src]);
    }
    const size_t at = (size_t)m * total + (size_t)item;
    a.S[at] = S;
    if (a.target) {
      const double r = S - a.target[(size_t)m * a.target_stride + (size_t)item];
      const double cr = (a.tau ? a.tau[k] : 1.0) * (a.omega ? a.omega[s] : 1.0) * r;
      a.cres[at] = cr;
      val = 0.5 * cr * r;
    }
  }
  if (!partial) return;
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

// grid (chunks of kObjThreads (output, distinct (block, component)) pairs, members); every entry of G / w written belongs to one lane
__global__ __launch_bounds__(kObjThreads) void k_signal_direction(DevCtx c, SigArgs a, double* G) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_uc;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  if (item >= total) return;
  const int k = (int)(item / a.n_uc), i = (int)(item % a.n_uc);
  const double* cr = a.cres + ((size_t)m * c.n_timepoints + k) * (size_t)a.n_sig;
  double v = 0.0;
  for (int t = a.uc_ptr[i]; t < a.uc_ptr[i + 1]; ++t) v += a.uc_coef[t] * cr[a.uc_sig[t]];
  const int dst = a.uc_dst[i];
  if (dst >= 0) G[((size_t)k * c.batch + m) * ((size_t)c.n_blocks * 6) + dst] = v;
  else a.w[((size_t)m * c.n_timepoints + k) * (size_t)a.n_ch + (-1 - dst)] = v;
}

// the direction on block b at one (member, output): w of a force block, zero elsewhere
__device__ __forceinline__ bool signal_seed(const SigArgs& a, const double* wk, int b, double* w3) {
  const int j = a.fmap[b];
  w3[0] = j >= 0 ? wk[j * 3] : 0.0; w3[1] = j >= 0 ? wk[j * 3 + 1] : 0.0; w3[2] = j >= 0 ? wk[j * 3 + 2] : 0.0;
  return w3[0] != 0.0 || w3[1] != 0.0 || w3[2] != 0.0;
}

// the direction of the listed hinge on `slot` (if any) added to w3 (the own-block seed of the lane on that slot, the partner-block seed of
// the lane on its partner slot); only called when the call lists hinges.  Returns whether w3 is non-zero now.
__device__ __forceinline__ bool signal_seed_hinge(const SigArgs& a, const double* wk, int slot, double* w3) {
  const int i = a.hmap[slot];
  if (i >= 0) {
    const double* wh = wk + (size_t)(a.n_fb + i) * 3;
    w3[0] += wh[0]; w3[1] += wh[1]; w3[2] += wh[2];
  }
  return w3[0] != 0.0 || w3[1] != 0.0 || w3[2] != 0.0;
}

// grid (chunks of kObjQuads items, members): runs behind k_signal_direction on the same stream (it adds to rows that kernel may have set)
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(kObjThreads) void k_signal_cotangent(DevCtx c, SigArgs a, double* G) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_set;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  const bool valid = item < total;
  double hx = 0.0, hy = 0.0, hth = 0.0;
  int k = 0, b = 0;
  if (valid) {
    k = (int)(item / a.n_set);
    b = a.set[(int)(item % a.n_set)];
    const int slot = b * 4 + kk;
    const int info = c.slot_info[slot];
    if (info >= 0) {
      const double* wk = a.w + ((size_t)m * c.n_timepoints + k) * (size_t)a.n_ch;
      double wo[3], wp[3];
      bool so = signal_seed(a, wk, b, wo), sp = signal_seed(a, wk, info >> 3, wp);
      if (a.n_hg) { so = signal_seed_hinge(a, wk, slot, wo); sp = signal_seed_hinge(a, wk, info >> 1, wp); }
      if (so || sp) {
        SignalLigIn in;
        SignalLigOut out;
        signal_load(c, member_bases(c, m), a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info, CONTACT, in);
        signal_lig_eps<MODEL, CONTACT>(in, wo, wp, out);
        hx = out.hx; hy = out.hy; hth = out.hth;
      }
    }
  }
  hx = quad_sum(hx); hy = quad_sum(hy); hth = quad_sum(hth);
  if (valid && kk == 0) {
    double* g = G + ((size_t)k * c.batch + m) * ((size_t)c.n_blocks * 6) + (size_t)b * 6;
    g[0] += hx; g[1] += hy; g[2] += hth;
  }
}

// grid (chunks of 64 slots of the set, members); every accumulator entry touched belongs to one lane
template <int MODEL, int CONTACT>
__global__ __launch_bounds__(64) void k_signal_explicit(DevCtx c, SigArgs a) {
  const int m = blockIdx.y;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= a.n_set * 4) return;
  const int b = a.set[idx >> 2], slot = b * 4 + (idx & 3);
  const int info = c.slot_info[slot];
  if (info < 0) return;
  const MemberBases B = member_bases(c, m);
  const bool end0 = !(info & 1), bonds = c.g_b && end0;
  double rx = 0.0, ry = 0.0, phi = 0.0, q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < c.n_timepoints; ++k) {
    const double* wk = a.w + ((size_t)m * c.n_timepoints + k) * (size_t)a.n_ch;
    double wo[3], wp[3];
    bool so = signal_seed(a, wk, b, wo), sp = signal_seed(a, wk, info >> 3, wp);
    if (a.n_hg) { so = signal_seed_hinge(a, wk, slot, wo); sp = signal_seed_hinge(a, wk, info >> 1, wp); }
    if (!so && !sp) continue;
    SignalLigIn in;
    SignalLigOut out;
    signal_load(c, B, a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info, CONTACT, in);
    signal_lig_eps<MODEL, CONTACT>(in, wo, wp, out);
    rx += out.rx; ry += out.ry;
    phi += end0 ? out.p1 : out.p2;
    if (bonds) for (int i = 0; i < 8; ++i) q[i] += out.q[i];
  }
  const size_t ms = (size_t)m * c.n_slots + slot;
  c.g_r[ms * 2] += rx; c.g_r[ms * 2 + 1] += ry;
  if (CONTACT == 1 && phi != 0.0) { c.g_phi[ms] += phi; c.touch[0] = 1; }
  if (bonds) for (int i = 0; i < 8; ++i) c.g_b[ms * 8 + i] += q[i];
}

// ---- signal projections ---------------------------------------------------------------------------------------------------------------
constexpr int kObjProject = 4;             // ObjJob::kind of a signal-projection call: a signal job behind the sweep (k_signal_explicit)

struct ProjArgs {
  const double* basis;        // n_rows * T, shared by the members
  const double* W;            // n_sig * n_rows, or null: projections only
  const double* target;       // (n_sig, n_rows), members target_stride apart (0: shared); null: zeros
  double* P;                  // batch * n_sig * n_rows
  long long target_stride;
  int n_rows;
};

// grid (chunks of kObjWaves (signal, row) pairs, members): wave `pair` of a member holds one (s, j).  Lane l adds B_jk S_mks over
// k = l, l + 64, ... ascending, obj_wave_sum adds the lanes; a wave past the last pair adds zeros and stores nothing (it stays for the
// barrier).  With `partial` the value term of the pair sits on lane 0 and the workgroup's waves are added in order.
__global__ __launch_bounds__(kObjThreads) void k_signal_project(DevCtx c, SigArgs a, ProjArgs p, double* partial) {
  const int m = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = c.n_timepoints;
  const int pair = blockIdx.x * kObjWaves + wv;
  const bool valid = pair < a.n_sig * p.n_rows;
  double v = 0.0, val = 0.0;
  size_t at = 0;
  if (valid) {
    const int s = pair / p.n_rows, j = pair % p.n_rows;
    const double* S = a.S + (size_t)m * T * a.n_sig + s;
    const double* b = p.basis + (size_t)j * T;
    for (int k = lane; k < T; k += 64) v += b[k] * S[(size_t)k * a.n_sig];
    at = (size_t)m * a.n_sig * p.n_rows + pair;
  }
  v = obj_wave_sum(v);
  if (valid && lane == 0) {
    p.P[at] = v;
    if (p.W) {
      const double r = v - (p.target ? p.target[(size_t)m * p.target_stride + pair] : 0.0);
      val = 0.5 * p.W[pair] * r * r;
    }
  }
  if (!partial) return;
  __shared__ double red[kObjWaves];
  if (lane == 0) red[wv] = val;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int w = 1; w < kObjWaves; ++w) s += red[w];
    partial[(size_t)m * gridDim.x + blockIdx.x] = s;
  }
}

// grid (chunks of kObjThreads (output, signal) pairs, members), behind k_signal_project on the same stream: the cotangent of the value on
// the signals, c_mks = sum_j W_sj (P_msj - Ptarget_msj) B_jk with j ascending, into cres -- where k_signal_residual puts tau omega (S - Starget)
__global__ __launch_bounds__(kObjThreads) void k_signal_project_residual(DevCtx c, SigArgs a, ProjArgs p) {
  const int m = blockIdx.y;
  const int T = c.n_timepoints;
  const long long total = (long long)T * a.n_sig;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  if (item >= total) return;
  const int k = (int)(item / a.n_sig), s = (int)(item % a.n_sig);
  const double* P = p.P + ((size_t)m * a.n_sig + s) * p.n_rows;
  const double* W = p.W + (size_t)s * p.n_rows;
  const double* tg = p.target ? p.target + (size_t)m * p.target_stride + (size_t)s * p.n_rows : nullptr;
  double cr = 0.0;
  for (int j = 0; j < p.n_rows; ++j) cr += W[j] * (P[j] - (tg ? tg[j] : 0.0)) * p.basis[(size_t)j * T + k];
  a.cres[(size_t)m * total + (size_t)item] = cr;
}

// ---- signal cross-correlation ---------------------------------------------------------------------------------------------------------
constexpr int kObjXcorr = 5;               // ObjJob::kind of a cross-correlation call: a signal job behind the sweep (k_signal_explicit)

struct XcorrArgs {
  const int32_t *pair_a, *pair_b;   // n_pairs: side A a signal; side B a signal (>= 0) or template column -1 - b
  const double* templ;              // (T, n_templ), members templ_stride apart (0: shared); null: no template column is named
  double *R, *rho, *Rbar;           // batch * (2 D + 1) each, lag d at index d + D
  double *E, *ebar;                 // batch * 2 each: (EA, EB) and their cotangents (eA, eB)
  double *peak, *delay;             // batch each
  long long templ_stride;
  int n_pairs, n_templ, D, norm, reduce, lag0;
  double beta, w_peak, w_delay, delay_target;
};

// side B of pair p of member m at output k (S: the member's signals, (T, n_sig))
__device__ __forceinline__ double xcorr_side_b(const XcorrArgs& x, const double* S, int n_sig, const double* G, int b, int k) {
  return b >= 0 ? S[(size_t)k * n_sig + b] : G[(size_t)k * x.n_templ + (-1 - b)];
}

// grid (chunks of kObjWaves rows, members): wave `row` of a member holds lag d = row - D for row <= 2 D, then EA (row 2 D + 1) and EB
// (row 2 D + 2).  Lane l adds outputs k = l, l + 64, ... ascending with the pairs ascending inside, products whose partner output k + d
// falls outside [0, T) left out; obj_wave_sum adds the lanes.  A wave past the last row stores nothing.
__global__ __launch_bounds__(kObjThreads) void k_signal_xcorr(DevCtx c, SigArgs a, XcorrArgs x) {
  const int m = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = c.n_timepoints, nl = 2 * x.D + 1;
  const int row = blockIdx.x * kObjWaves + wv;
  if (row >= nl + 2) return;                    // (no barrier in this kernel: a whole wave leaves)
  const double* S = a.S + (size_t)m * T * a.n_sig;
  const double* G = x.templ ? x.templ + (size_t)m * x.templ_stride : nullptr;
  double v = 0.0;
  if (row < nl) {
    const int d = row - x.D;
    for (int k = lane; k < T; k += 64) {
      const int kb = k + d;
      if (kb < 0 || kb >= T) continue;
      for (int p = 0; p < x.n_pairs; ++p) v += S[(size_t)k * a.n_sig + x.pair_a[p]] * xcorr_side_b(x, S, a.n_sig, G, x.pair_b[p], kb);
    }
  } else {
    const bool sideA = row == nl;
    for (int k = lane; k < T; k += 64)
      for (int p = 0; p < x.n_pairs; ++p) {
        const double s = sideA ? S[(size_t)k * a.n_sig + x.pair_a[p]] : xcorr_side_b(x, S, a.n_sig, G, x.pair_b[p], k);
        v += s * s;
      }
  }
  v = obj_wave_sum(v);
  if (lane == 0) {
    if (row < nl) x.R[(size_t)m * nl + row] = v;
    else x.E[(size_t)m * 2 + (row - nl)] = v;
  }
}

// the lanes' (value, index) candidates of a maximum: the larger value wins, on equal values the lower index; every lane ends with the result
__device__ __forceinline__ void xcorr_wave_argmax(double& v, int& i) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
  }
}

// grid (members), one wave each: N and rho = R / N, then the reduction over the lags in a fixed lane-strided order (lane l holds lags
// l, l + 64, ... ascending; the maximum first, then the exponent sums with the maximum subtracted, obj_wave_sum over the lanes), the value
// J = w_peak M + 1/2 w_delay (delta - delta_target)^2 into objective[m] (and pinned host memory when given), M and delta per member, the
// cotangents Rbar = g / N on the lags and (eA, eB) on the energies.  N == 0: J = M = delta = rho = NaN and every cotangent 0.
__global__ __launch_bounds__(64) void k_signal_xcorr_reduce(XcorrArgs x, double* objective, double* host3, int batch) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int nl = 2 * x.D + 1;
  const double* R = x.R + (size_t)m * nl;
  double* rho = x.rho + (size_t)m * nl;
  double* Rbar = x.Rbar + (size_t)m * nl;
  const double EA = x.E[(size_t)m * 2], EB = x.E[(size_t)m * 2 + 1];
  const double N = x.norm == DFX_XCORR_NORM_REFERENCE ? EA : x.norm == DFX_XCORR_NORM_COEFFICIENT ? sqrt(EA * EB) : 1.0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (N == 0.0) {
    for (int i = lane; i < nl; i += 64) { rho[i] = nan; Rbar[i] = 0.0; }
    if (lane == 0) {
      x.ebar[(size_t)m * 2] = x.ebar[(size_t)m * 2 + 1] = 0.0;
      x.peak[m] = x.delay[m] = nan;
      if (objective) objective[m] = nan;
      if (host3) { host3[m] = nan; host3[batch + m] = nan; host3[2 * batch + m] = nan; }
    }
    return;
  }
  // the maximum and the lowest lag that reaches it
  double best = 0.0;
  int at = -1;
  for (int i = lane; i < nl; i += 64) {
    const double r = R[i] / N;
    rho[i] = r;
    if (at < 0 || r > best) { best = r; at = i; }
  }
  xcorr_wave_argmax(best, at);
  double M, delta, Z = 1.0;
  if (x.reduce == DFX_XCORR_SOFTMAX) {
    double z = 0.0, zd = 0.0;
    for (int i = lane; i < nl; i += 64) {
      const double e = exp(x.beta * (R[i] / N - best));
      z += e; zd += (double)(i - x.D) * e;
    }
    z = obj_wave_sum(z); zd = obj_wave_sum(zd);
    Z = __shfl(z, 0, 64);
    M = best + log(Z) / x.beta;
    delta = __shfl(zd, 0, 64) / Z;
  } else if (x.reduce == DFX_XCORR_MAX) {
    M = best; delta = (double)(at - x.D);
  } else {
    M = R[x.lag0 + x.D] / N; delta = (double)x.lag0;
    at = x.lag0 + x.D;
  }
  // g = dJ / d rho on the lags, Rbar = g / N, Nbar = - sum g rho / N
  const double dd = x.w_delay * (delta - x.delay_target);
  double gr = 0.0;
  for (int i = lane; i < nl; i += 64) {
    const double r = R[i] / N;
    double g;
    if (x.reduce == DFX_XCORR_SOFTMAX) {
      const double pi = exp(x.beta * (r - best)) / Z;
      g = x.w_peak * pi + dd * x.beta * pi * ((double)(i - x.D) - delta);
    } else {
      g = i == at ? x.w_peak : 0.0;
    }
    Rbar[i] = g / N;
    gr += g * r;
  }
  gr = obj_wave_sum(gr);
  if (lane == 0) {
    const double Nbar = -gr / N;
    double eA = 0.0, eB = 0.0;
    if (x.norm == DFX_XCORR_NORM_REFERENCE) eA = Nbar;
    else if (x.norm == DFX_XCORR_NORM_COEFFICIENT) { eA = Nbar * N / (2.0 * EA); eB = Nbar * N / (2.0 * EB); }
    x.ebar[(size_t)m * 2] = eA; x.ebar[(size_t)m * 2 + 1] = eB;
    const double J = x.w_peak * M + 0.5 * dd * (delta - x.delay_target);
    x.peak[m] = M; x.delay[m] = delta;
    if (objective) objective[m] = J;
    if (host3) { host3[m] = J; host3[batch + m] = M; host3[2 * batch + m] = delta; }     // pinned host memory, as k_objective_finish
  }
}

// grid (chunks of kObjThreads (output, signal) items, members), behind k_signal_xcorr_reduce on the same stream: the cotangent of J on the
// signals into cres, where k_signal_project_residual puts its own --
//   c_ks = sum over pairs with a_p = s: ( sum_d Rbar[d] B_p[k + d] + 2 eA A_p[k] ) + sum over pairs with b_p = s: ( sum_d Rbar[d] A_p[k - d] + 2 eB B_p[k] )
// the A-side pairs first, each group with p ascending and d ascending inside; lags whose Rbar is exactly 0 are skipped (under "at" and
// "max" all but one), partner outputs outside [0, T) contribute nothing
__global__ __launch_bounds__(kObjThreads) void k_signal_xcorr_residual(DevCtx c, SigArgs a, XcorrArgs x) {
  const int m = blockIdx.y;
  const int T = c.n_timepoints, nl = 2 * x.D + 1;
  const long long total = (long long)T * a.n_sig;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  if (item >= total) return;
  const int k = (int)(item / a.n_sig), s = (int)(item % a.n_sig);
  const double* S = a.S + (size_t)m * T * a.n_sig;
  const double* G = x.templ ? x.templ + (size_t)m * x.templ_stride : nullptr;
  const double* Rbar = x.Rbar + (size_t)m * nl;
  const double eA = x.ebar[(size_t)m * 2], eB = x.ebar[(size_t)m * 2 + 1];
  double cr = 0.0;
  for (int p = 0; p < x.n_pairs; ++p) {
    if (x.pair_a[p] != s) continue;
    const int b = x.pair_b[p];
    double acc = 0.0;
    for (int i = 0; i < nl; ++i) {
      const int kb = k + i - x.D;
      if (Rbar[i] == 0.0 || kb < 0 || kb >= T) continue;
      acc += Rbar[i] * xcorr_side_b(x, S, a.n_sig, G, b, kb);
    }
    cr += acc + 2.0 * eA * S[(size_t)k * a.n_sig + s];
  }
  for (int p = 0; p < x.n_pairs; ++p) {
    if (x.pair_b[p] != s) continue;
    const int sa = x.pair_a[p];
    double acc = 0.0;
    for (int i = 0; i < nl; ++i) {
      const int ka = k - (i - x.D);
      if (Rbar[i] == 0.0 || ka < 0 || ka >= T) continue;
      acc += Rbar[i] * S[(size_t)ka * a.n_sig + sa];
    }
    cr += acc + 2.0 * eB * S[(size_t)k * a.n_sig + s];
  }
  a.cres[(size_t)m * total + (size_t)item] = cr;
}

// ---- signal spectral ratios -----------------------------------------------------------------------------------------------------------
constexpr int kObjSpectrum = 7;            // ObjJob::kind of a spectral-ratio call: a signal job behind the sweep (k_signal_explicit)

struct SpecArgs {
  const double *Wn, *Wd;            // (G, n_sig * n_rows) each, shared by the members, entries >= 0
  const double *n0, *d0;            // (G,), members off_stride apart (0: shared)
  const double* a;                  // (G,) group coefficients
  double* forms;                    // batch * G * 2: N | D per group
  double* l;                        // batch * G: the measures
  double* lam;                      // batch * G * 2: lam_g dl_g/dN | lam_g dl_g/dD
  double* Weff;                     // batch * n_sig * n_rows
  long long off_stride;
  int G, measure, aggregate;
  double beta;
};

// grid (chunks of kObjWaves (group, side) rows, members), behind k_signal_project on the same stream: wave `row` of a member holds group
// row / 2, side row % 2 (0: numerator, 1: denominator).  Lane l adds W P^2 over the flattened (signal, row) pairs l, l + 64, ... ascending
// (a weight that is exactly 0 adds nothing, whatever P holds), obj_wave_sum adds the lanes, lane 0 adds the offset and stores.  A wave past
// the last row stores nothing (no barrier in this kernel: a whole wave leaves).
__global__ __launch_bounds__(kObjThreads) void k_signal_spectrum_forms(SigArgs a, ProjArgs p, SpecArgs x) {
  const int m = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * kObjWaves + wv;
  if (row >= 2 * x.G) return;
  const int g = row >> 1, side = row & 1;
  const int np = a.n_sig * p.n_rows;
  const double* W = (side ? x.Wd : x.Wn) + (size_t)g * np;
  const double* P = p.P + (size_t)m * np;
  double v = 0.0;
  for (int i = lane; i < np; i += 64) {
    const double w = W[i];
    if (w != 0.0) v += w * P[i] * P[i];
  }
  v = obj_wave_sum(v);
  if (lane == 0) x.forms[((size_t)m * x.G + g) * 2 + side] = (side ? x.d0 : x.n0)[(size_t)m * x.off_stride + g] + v;
}

// grid (members), one wave each, behind k_signal_spectrum_forms: lane l holds groups l, l + 64, ... ascending.  The measures first
// (l = N / D or ln N - ln D), then -- DFX_SPECTRUM_KS -- the maximum of z = a l (lowest group on a tie), then the exponent sums with the
// maximum subtracted; obj_wave_sum over the lanes.  J into objective[m] and, when given, J | l into pinned host memory (J at host[m], l at
// host[batch + m * G + g]); lam_g dl_g/dN and lam_g dl_g/dD per group.  A member with some D <= 0 (DFX_SPECTRUM_LOG: or some N <= 0;
// DFX_SPECTRUM_KS: or some non-finite l) gets J = NaN, NaN in the offending l and zeros in lam: no division by zero reaches the sweep.
__global__ __launch_bounds__(64) void k_signal_spectrum_reduce(SpecArgs x, double* objective, double* host, int batch) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int G = x.G;
  const double* F = x.forms + (size_t)m * G * 2;
  double* L = x.l + (size_t)m * G;
  double* lam = x.lam + (size_t)m * G * 2;
  double* hl = host ? host + batch + (size_t)m * G : nullptr;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool log_m = x.measure == DFX_SPECTRUM_LOG, ks = x.aggregate == DFX_SPECTRUM_KS;
  // the measures
  int bad = 0;
  for (int g = lane; g < G; g += 64) {
    const double N = F[g * 2], D = F[g * 2 + 1];
    double l = nan;
    if (D > 0.0 && (!log_m || N > 0.0)) {
      l = log_m ? log(N) - log(D) : N / D;
      if (ks && !isfinite(l)) l = nan;
    }
    if (l != l) bad = 1;
    L[g] = l;
    if (hl) hl[g] = l;
  }
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if (bad) {
    for (int g = lane; g < G; g += 64) lam[g * 2] = lam[g * 2 + 1] = 0.0;
    if (lane == 0) {
      if (objective) objective[m] = nan;
      if (host) host[m] = nan;
    }
    return;
  }
  double J, M = 0.0, Z = 1.0;
  if (ks) {
    double best = 0.0;
    int at = -1;
    for (int g = lane; g < G; g += 64) {
      const double z = x.a[g] * L[g];
      if (at < 0 || z > best) { best = z; at = g; }
    }
    xcorr_wave_argmax(best, at);
    M = best;
    double e = 0.0;
    for (int g = lane; g < G; g += 64) e += exp(x.beta * (x.a[g] * L[g] - M));
    e = obj_wave_sum(e);
    Z = __shfl(e, 0, 64);
    J = M + log(Z) / x.beta;
  } else {
    double s = 0.0;
    for (int g = lane; g < G; g += 64) s += x.a[g] * L[g];
    J = obj_wave_sum(s);
  }
  for (int g = lane; g < G; g += 64) {
    const double N = F[g * 2], D = F[g * 2 + 1];
    const double lg = ks ? x.a[g] * (exp(x.beta * (x.a[g] * L[g] - M)) / Z) : x.a[g];
    lam[g * 2] = lg * (log_m ? 1.0 / N : 1.0 / D);
    lam[g * 2 + 1] = lg * (log_m ? -1.0 / D : -N / (D * D));
  }
  if (lane == 0) {
    if (objective) objective[m] = J;
    if (host) host[m] = J;                              // pinned host memory, as k_objective_finish
  }
}

// grid (chunks of kObjThreads (signal, row) pairs, members), behind k_signal_spectrum_reduce: the effective row weights of the member,
// Weff_msj = 2 sum_g (lam_g dl_g/dN Wn_gsj + lam_g dl_g/dD Wd_gsj) with g ascending
__global__ __launch_bounds__(kObjThreads) void k_signal_spectrum_weights(SigArgs a, ProjArgs p, SpecArgs x) {
  const int m = blockIdx.y;
  const int np = a.n_sig * p.n_rows;
  const int i = blockIdx.x * kObjThreads + threadIdx.x;
  if (i >= np) return;
  const double* lam = x.lam + (size_t)m * x.G * 2;
  double acc = 0.0;
  for (int g = 0; g < x.G; ++g) acc += lam[g * 2] * x.Wn[(size_t)g * np + i] + lam[g * 2 + 1] * x.Wd[(size_t)g * np + i];
  x.Weff[(size_t)m * np + i] = 2.0 * acc;
}

// grid (chunks of kObjThreads (output, signal) pairs, members), behind k_signal_spectrum_weights: the twin of k_signal_project_residual
// with per-member row weights and no targets, c_mks = sum_j Weff_msj P_msj B_jk with j ascending, into cres
__global__ __launch_bounds__(kObjThreads) void k_signal_spectrum_residual(DevCtx c, SigArgs a, ProjArgs p, SpecArgs x) {
  const int m = blockIdx.y;
  const int T = c.n_timepoints;
  const long long total = (long long)T * a.n_sig;
  const long long item = (long long)blockIdx.x * kObjThreads + threadIdx.x;
  if (item >= total) return;
  const int k = (int)(item / a.n_sig), s = (int)(item % a.n_sig);
  const double* P = p.P + ((size_t)m * a.n_sig + s) * p.n_rows;
  const double* W = x.Weff + ((size_t)m * a.n_sig + s) * p.n_rows;
  double cr = 0.0;
  for (int j = 0; j < p.n_rows; ++j) cr += W[j] * P[j] * p.basis[(size_t)j * T + k];
  a.cres[(size_t)m * total + (size_t)item] = cr;
}

// ---- peak ligament strain ------------------------------------------------------------------------------------------------------------
constexpr int kObjPeak = 6;                // ObjJob::kind of a peak-strain call

// ObjArgs of a peak call: blocks = listed blocks, w = SLOT weights omega (as a strain call), tau, lever unused.  Beside it:
struct PeakArgs {
  const double* coef;          // coef_members * n_slots * 3: (a, s, r) of the slot's ligament (both end slots carry them)
  const int32_t* slot_bond;    // n_slots: bond id of the slot's ligament
  double* Q;                   // batch * T * n_bonds: q of every counted (output, ligament) pair; other entries are never read
  double* pmax;                // batch * chunks: the maximum of each workgroup ...
  long long* pkey;             // ... and its key k * n_bonds + bond (the lowest key among equal maxima)
  double* res;                 // batch * 4: q_hat, S (the sum of pass 2), J
  int32_t* at;                 // batch * 2: k_hat, b_hat
  long long coef_stride;       // 0 when one array serves all members
  int n_bonds, aggregate;
  double sharp;                // beta (KS) or p (PNORM)
};

constexpr long long kPeakNoKey = 0x7fffffffffffffffLL;

__device__ __forceinline__ double peak_neg_inf() { return -__longlong_as_double(0x7ff0000000000000LL); }

// (value, key) candidates of a maximum: the larger value wins, on equal values the lower key; the identity is (-inf, kPeakNoKey)
__device__ __forceinline__ void peak_take(double& v, long long& key, double ov, long long okey) {
  if (ov > v || (ov == v && okey < key)) { v = ov; key = okey; }
}
__device__ __forceinline__ void peak_wave_argmax(double& v, long long& key) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const long long okey = __shfl_xor(key, off, 64);
    peak_take(v, key, ov, okey);
  }
}

// one side of the ligament on `slot` with the coefficient triple in place of the stiffnesses: g.e = q / 2 and every first derivative of it
// (the loads of strain_eval, repeated here because no existing kernel may change: a change to how slots, the reference-vector dictionary
// or the fields are laid out has to be made in both; the stiffness image is not read)
template <int MODEL>
__device__ __forceinline__ void peak_eval(const DevCtx& c, const MemberBases& B, const double* f, int slot, int info, const double* coef,
                                          BondGrad<double>& g) {
  const int b = slot >> 2, ps = info >> 1, pb = ps >> 2;
  BlockRec<double> o, p;
  o.x = f[(size_t)b * 3]; o.y = f[(size_t)b * 3 + 1]; o.th = f[(size_t)b * 3 + 2];
  p.x = f[(size_t)pb * 3]; p.y = f[(size_t)pb * 3 + 1]; p.th = f[(size_t)pb * 3 + 2];
  fast_sincos(0.5 * o.th, &o.sh, &o.ch);
  fast_sincos(0.5 * p.th, &p.sh, &p.ch);
  const double2 ro = ldg<double2>(B.p_r, (u32)slot * 16), rp = ldg<double2>(B.p_r, (u32)ps * 16);
  double lx, ly, l0, il0;
  if (c.l_dict_on) {
    const int li = B.p_lidx[slot];
    lx = B.l_dict[li * 4]; ly = B.l_dict[li * 4 + 1]; l0 = B.l_dict[li * 4 + 2]; il0 = B.l_dict[li * 4 + 3];
  } else {
    lx = B.p_l[(size_t)slot * 2]; ly = B.p_l[(size_t)slot * 2 + 1]; l0 = sqrt(lx * lx + ly * ly); il0 = 1.0 / l0;
  }
  const double* cf = coef + (size_t)slot * 3;
  bond_grad<MODEL, double>(o, p, ro.x, ro.y, rp.x, rp.y, lx, ly, l0, il0, cf[0], cf[1], cf[2], (info & 1) ? 1.0 : -1.0, g);
}

// the weight W = tau_k omega of the pair on this lane; 0: the lane contributes the identity
__device__ __forceinline__ double peak_weight(const DevCtx& c, const ObjArgs& a, int m, int k, int slot, int& info) {
  info = c.slot_info[slot];
  if (info < 0) return 0.0;
  return (a.tau ? a.tau[k] : 1.0) * a.w[(size_t)m * a.w_stride + slot];
}

// pass 1, grid (chunks of kObjQuads items, members): q of every counted pair (a ligament is counted on its end-0 lane) into Q and the
// workgroup's maximum with its key into pmax / pkey
template <int MODEL>
__global__ __launch_bounds__(kObjThreads) void k_strain_peak_measure(DevCtx c, ObjArgs a, PeakArgs p) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_act;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  double best = peak_neg_inf();
  long long key = kPeakNoKey;
  if (item < total) {
    const int k = (int)(item / a.n_act);
    const int slot = a.blocks[(int)(item % a.n_act)] * 4 + kk;
    int info;
    const double W = peak_weight(c, a, m, k, slot, info);
    if (W != 0.0 && !(info & 1)) {
      BondGrad<double> g;
      peak_eval<MODEL>(c, member_bases(c, m), a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info,
                       p.coef + (size_t)m * p.coef_stride, g);
      const int bond = p.slot_bond[slot];
      best = 2.0 * g.e;
      key = (long long)k * p.n_bonds + bond;
      p.Q[((size_t)m * c.n_timepoints + k) * p.n_bonds + bond] = best;
    }
  }
  __shared__ double red[kObjWaves];
  __shared__ long long redk[kObjWaves];
  peak_wave_argmax(best, key);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = best; redk[threadIdx.x >> 6] = key; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < kObjWaves; ++wv) peak_take(best, key, red[wv], redk[wv]);
    p.pmax[(size_t)m * gridDim.x + blockIdx.x] = best;
    p.pkey[(size_t)m * gridDim.x + blockIdx.x] = key;
  }
}

// grid (members): the member's workgroup maxima, strided over the lanes, to q_hat, k_hat, b_hat (a maximum with the lowest-key tie rule does
// not depend on the order it is taken in)
__global__ __launch_bounds__(kObjThreads) void k_strain_peak_finish(PeakArgs p, int n_partial) {
  const int m = blockIdx.x;
  double best = peak_neg_inf();
  long long key = kPeakNoKey;
  for (int i = threadIdx.x; i < n_partial; i += kObjThreads) peak_take(best, key, p.pmax[(size_t)m * n_partial + i], p.pkey[(size_t)m * n_partial + i]);
  __shared__ double red[kObjWaves];
  __shared__ long long redk[kObjWaves];
  peak_wave_argmax(best, key);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = best; redk[threadIdx.x >> 6] = key; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < kObjWaves; ++wv) peak_take(best, key, red[wv], redk[wv]);
    p.res[(size_t)m * 4] = best;
    // no candidate won (every q of the member is NaN: a non-finite history): peak = -inf, J = NaN and peak_at = (-1, -1)
    p.at[(size_t)m * 2] = key == kPeakNoKey ? -1 : (int32_t)(key / p.n_bonds);
    p.at[(size_t)m * 2 + 1] = key == kPeakNoKey ? -1 : (int32_t)(key % p.n_bonds);
  }
}

// the term of a counted pair in the sum of pass 2: W exp(beta (q - q_hat)) or W (q / q_hat)^p (q_hat == 0: every q is 0 and so is the term)
__device__ __forceinline__ double peak_term(const PeakArgs& p, double W, double q, double qhat) {
  if (p.aggregate == DFX_PEAK_KS) return W * exp(p.sharp * (q - qhat));
  return qhat > 0.0 ? W * pow(q / qhat, p.sharp) : 0.0;
}

// pi of a pair from the member's q_hat and S: KS  W exp(beta (q - q_hat)) / S  (= W exp(beta (q - J)));
// PNORM  W (q / q_hat)^(p - 1) S^((1 - p) / p)  (= W q^(p-1) J^(1-p)), 0 when q_hat == 0
__device__ __forceinline__ double peak_pi(const PeakArgs& p, double W, double q, double qhat, double S) {
  if (p.aggregate == DFX_PEAK_KS) return W * exp(p.sharp * (q - qhat)) / S;
  return qhat > 0.0 ? W * pow(q / qhat, p.sharp - 1.0) * pow(S, (1.0 - p.sharp) / p.sharp) : 0.0;
}

// pass 2, grid as pass 1: the terms from the stored q, wave sum, the waves of a workgroup in order into its partial
__global__ __launch_bounds__(kObjThreads) void k_strain_peak_sum(DevCtx c, ObjArgs a, PeakArgs p, double* partial) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_act;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  double val = 0.0;
  if (item < total) {
    const int k = (int)(item / a.n_act);
    const int slot = a.blocks[(int)(item % a.n_act)] * 4 + kk;
    int info;
    const double W = peak_weight(c, a, m, k, slot, info);
    if (W != 0.0 && !(info & 1)) val = peak_term(p, W, p.Q[((size_t)m * c.n_timepoints + k) * p.n_bonds + p.slot_bond[slot]], p.res[(size_t)m * 4]);
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

// grid (members): the second level of k_objective_finish on the partials of pass 2, then J; S and J beside q_hat in res, J into objective[m],
// and J | q_hat (doubles) and (k_hat, b_hat) (int32) into pinned host memory when given
__global__ __launch_bounds__(kObjThreads) void k_strain_peak_value(PeakArgs p, const double* partial, int n_partial, double* objective,
                                                                    double* host2, int32_t* host_at, int batch) {
  const int m = blockIdx.x;
  double v = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kObjThreads) v += partial[(size_t)m * n_partial + i];
  __shared__ double red[kObjWaves];
  v = obj_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = red[0];
    for (int wv = 1; wv < kObjWaves; ++wv) S += red[wv];
    const double qhat = p.res[(size_t)m * 4];
    const double J = p.aggregate == DFX_PEAK_KS ? qhat + log(S) / p.sharp : (qhat > 0.0 ? qhat * pow(S, 1.0 / p.sharp) : 0.0);
    p.res[(size_t)m * 4 + 1] = S; p.res[(size_t)m * 4 + 2] = J;
    if (objective) objective[m] = J;
    if (host2) { host2[m] = J; host2[batch + m] = qhat; }          // pinned host memory, as k_objective_finish
    if (host_at) { host_at[m * 2] = p.at[(size_t)m * 2]; host_at[m * 2 + 1] = p.at[(size_t)m * 2 + 1]; }
  }
}

// pass 3, grid as pass 1: every lane whose slot carries a weighted ligament evaluates its own side again, pi dq/d(x, y, theta) = 2 pi dE/d(..)
// is added over the quad and lane 0 stores rows 0..2 of G[(k, m, b)], as k_strain_objective does
template <int MODEL>
__global__ __launch_bounds__(kObjThreads) void k_strain_peak_cotangent(DevCtx c, ObjArgs a, PeakArgs p, double* G) {
  const int m = blockIdx.y;
  const long long total = (long long)c.n_timepoints * a.n_act;
  const long long item = (long long)blockIdx.x * kObjQuads + (threadIdx.x >> 2);
  const int kk = threadIdx.x & 3;
  const bool valid = item < total;
  double fx = 0.0, fy = 0.0, fth = 0.0;
  int k = 0, b = 0;
  if (valid) {
    k = (int)(item / a.n_act);
    b = a.blocks[(int)(item % a.n_act)];
    const int slot = b * 4 + kk;
    int info;
    const double W = peak_weight(c, a, m, k, slot, info);
    if (W != 0.0) {
      BondGrad<double> g;
      peak_eval<MODEL>(c, member_bases(c, m), a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info,
                       p.coef + (size_t)m * p.coef_stride, g);
      const double q = p.Q[((size_t)m * c.n_timepoints + k) * p.n_bonds + p.slot_bond[slot]];      // both ends of a ligament: the same pi
      const double s = 2.0 * peak_pi(p, W, q, p.res[(size_t)m * 4], p.res[(size_t)m * 4 + 1]);
      fx = s * g.fx; fy = s * g.fy; fth = s * g.fth;
    }
  }
  fx = quad_sum(fx); fy = quad_sum(fy); fth = quad_sum(fth);
  if (valid && kk == 0) {
    double* g = G + ((size_t)k * c.batch + m) * ((size_t)c.n_blocks * 6) + (size_t)b * 6;
    g[0] = fx; g[1] = fy; g[2] = fth;
  }
}

// pass 4, after the sweep, grid (chunks of 64 listed slots, members): pi dq/d(own node vector) into g_r and, on end-0 slots when the call
// collects them, pi dq/d(reference vector) into g_b[0..1] (the coefficients are constants of the call: nothing reaches the stiffnesses, the
// contact constants or the void angles); output times in order, every accumulator entry touched belongs to one lane
template <int MODEL>
__global__ __launch_bounds__(64) void k_strain_peak_explicit(DevCtx c, ObjArgs a, PeakArgs p) {
  const int m = blockIdx.y;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= a.n_act * 4) return;
  const int slot = a.blocks[idx >> 2] * 4 + (idx & 3);
  const int info = c.slot_info[slot];
  const double w = a.w[(size_t)m * a.w_stride + slot];
  if (info < 0 || w == 0.0) return;
  const MemberBases B = member_bases(c, m);
  const bool bonds = c.g_b && !(info & 1);
  const int bond = p.slot_bond[slot];
  const double qhat = p.res[(size_t)m * 4], S = p.res[(size_t)m * 4 + 1];
  double rx = 0.0, ry = 0.0, lx = 0.0, ly = 0.0;
  for (int k = 0; k < c.n_timepoints; ++k) {
    const double W = (a.tau ? a.tau[k] : 1.0) * w;
    if (W == 0.0) continue;
    BondGrad<double> g;
    peak_eval<MODEL>(c, B, a.fields + ((size_t)m * c.n_timepoints + k) * ((size_t)c.n_blocks * 6), slot, info, p.coef + (size_t)m * p.coef_stride, g);
    const double s = 2.0 * peak_pi(p, W, p.Q[((size_t)m * c.n_timepoints + k) * p.n_bonds + bond], qhat, S);
    rx += s * g.rx; ry += s * g.ry;
    if (bonds) { lx += s * g.lx; ly += s * g.ly; }
  }
  const size_t ms = (size_t)m * c.n_slots + slot;
  c.g_r[ms * 2] += rx; c.g_r[ms * 2 + 1] += ry;
  if (bonds) { c.g_b[ms * 8] += lx; c.g_b[ms * 8 + 1] += ly; }
}

}  // namespace
