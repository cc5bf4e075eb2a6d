// engine_objective.hip -- libdfx host side: weighted kinetic-energy and angular-momentum objectives evaluated and differentiated on the
// device-resident history (dfx_objective_value, dfx_objective_value_and_grad).  "Fill the cotangent buffer G, reduce the value" before the
// reverse sweep, "add the explicit d objective / d parameters" after it: the sweep itself is run_adjoint, unchanged.
// The ligament strain-energy objective (dfx_strain_objective_value[_and_grad]) takes the same route with kernels of its own: its cotangent
// on the fields is the weighted ligament force, its explicit terms reach node vectors, void angles and the per-ligament parameters.
// The signal misfit (dfx_signal_values, dfx_signal_misfit_value[_and_grad]) likewise: force channels, signals and residual cotangents on the
// device, the Hessian-vector product K w of its force terms added to the cotangent, mixed second derivatives behind the sweep.
// The signal projections (dfx_signal_projections, dfx_signal_projection_value[_and_grad]) put a time reduction between the signals and
// their cotangent: P = B S, the value a weighted quadratic form of P, c = B^T (W (P - Ptarget)); from c on the signal misfit's launches.
// The signal cross-correlation (dfx_signal_xcorr, dfx_signal_xcorr_value[_and_grad]) is a second, nonlinear occupant of that slot: R over the
// lags and the two energies, a reduction to a peak and a delay, and the cotangent c of J = w_peak M + 1/2 w_delay (delta - delta_target)^2.
// The peak ligament strain (dfx_strain_peak_value[_and_grad]) is a smooth maximum, not a sum: its cotangent is the ligament force weighted
// by a softmax over all (output, ligament) pairs, so a maximum and a sum are reduced before the first cotangent is written.
// Every family is a prepare_* (the checks of the call, return 1 with h->err; then its uploads) and a launch_* (the value and, with G, the
// cotangent).  A value entry runs them between need_fields and download; a gradient entry between need_trajectory and objective_sweep, the
// one place that sets what the sweep consults on the handle for the call in flight and takes it back on every way out.
// (shared declarations in dfx_engine.h, the kernels in dfx_objective.h)
#include "dfx_engine.h"
#include "dfx_objective.h"

#include <cmath>

namespace {

struct ObjHost {               // the validated arguments of a call, compacted
  ObjJob job;
  std::vector<int32_t> blocks; // blocks whose weight is non-zero in any member
};

unsigned chunks_of(long long items, int per) { return (unsigned)std::max<long long>(1, (items + per - 1) / per); }

// v[0..n) (null: nothing to check) is finite and, with nonneg, not negative -- or h->err says that `what` is not
bool all_finite(dfx_handle* h, const char* who, const char* what, const double* v, size_t n, bool nonneg = false) {
  for (size_t i = 0; v && i < n; ++i)
    if (!std::isfinite(v[i]) || (nonneg && v[i] < 0.0)) {
      h->err = std::string(who) + (nonneg ? ": non-finite or negative " : ": non-finite ") + what;
      return false;
    }
  return true;
}

// what the weighted jobs share: the job of the listed blocks, then the uploads of listed blocks, weights (nw of them, w_stride apart per
// member) and output-time weights; the value buffer
int upload_job(dfx_handle* h, int kind, const double* w, size_t nw, int w_stride, const double* tau, ObjHost& out) {
  const int Tn = (int)h->ts.size();
  out.job = ObjJob{kind, (int)out.blocks.size(), w_stride, 0, tau != nullptr};
  HIP_OK(h->d_obj_blocks.ensure(std::max<size_t>(1, out.blocks.size())));
  HIP_OK(h->d_obj_w.ensure(nw));
  HIP_OK(h->d_obj.ensure(h->pl.batch));
  if (!out.blocks.empty())
    HIP_OK(hipMemcpyAsync(h->d_obj_blocks.p, out.blocks.data(), sizeof(int32_t) * out.blocks.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(h->d_obj_w.p, w, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
  if (tau) {
    HIP_OK(h->d_obj_tau.ensure(Tn));
    HIP_OK(hipMemcpyAsync(h->d_obj_tau.p, tau, sizeof(double) * Tn, hipMemcpyHostToDevice, h->stream));
  }
  return 0;
}

// bond weights (null: ones) of wm members -> slot weights (both end slots of a ligament carry its weight); listed blocks = the blocks that
// own a weighted end; member_any, when given: which members have a non-zero weight at all
void slot_weights(const Plan& pl, const double* bw, size_t wm, std::vector<double>& sw, std::vector<int32_t>& blocks, std::vector<char>* member_any) {
  const size_t nb = pl.n_blocks, NS = pl.n_slots, nbd = pl.n_bonds;
  sw.assign(wm * NS, 0.0);
  std::vector<char> listed(nb, 0);
  for (size_t sl = 0; sl < NS; ++sl) {
    if (pl.slot_info[sl] < 0) continue;
    const size_t bond = (size_t)pl.slot_bond[sl];
    for (size_t m = 0; m < wm; ++m) {
      const double v = bw ? bw[m * nbd + bond] : 1.0;
      sw[m * NS + sl] = v;
      if (v != 0.0) { listed[sl >> 2] = 1; if (member_any) (*member_any)[m] = 1; }
    }
  }
  blocks.clear();
  for (size_t b = 0; b < nb; ++b) if (listed[b]) blocks.push_back((int32_t)b);
}

// argument checks shared by the two entries (return 1 with h->err), then the uploads: listed blocks, weights, output-time weights, levers
int prepare_objective(dfx_handle* h, const char* who, int32_t kind, const double* w, int32_t w_per_member, const double* tau, const double* lever,
                      int32_t lever_per_member, ObjHost& out) {
  const Plan& pl = h->pl;
  const size_t B = pl.batch, nb = pl.n_blocks;
  if (kind != DFX_OBJ_KINETIC && kind != DFX_OBJ_ANGULAR_MOMENTUM) {
    h->err = std::string(who) + ": unknown objective kind " + std::to_string(kind) + " (DFX_OBJ_KINETIC = 0, DFX_OBJ_ANGULAR_MOMENTUM = 1)";
    return 1;
  }
  if (!w) { h->err = std::string(who) + ": block_weights is NULL"; return 1; }
  if (kind == DFX_OBJ_ANGULAR_MOMENTUM && !lever) {
    h->err = std::string(who) + ": the angular-momentum objective needs lever0 (block centroid - spin centre of every block)";
    return 1;
  }
  const size_t nw = (w_per_member ? B : 1) * nb, nl = kind == DFX_OBJ_ANGULAR_MOMENTUM ? (lever_per_member ? B : 1) * nb * 2 : 0;
  if (!all_finite(h, who, "block weight", w, nw) || !all_finite(h, who, "time weight", tau, h->ts.size()) || !all_finite(h, who, "lever0", lever, nl)) return 1;
  out.blocks.clear();
  for (size_t b = 0; b < nb; ++b) {
    bool any = false;
    for (size_t m = 0; m < (w_per_member ? B : 1) && !any; ++m) any = w[m * nb + b] != 0.0;
    if (any) out.blocks.push_back((int32_t)b);
  }
  if (int rc = upload_job(h, kind, w, nw, w_per_member ? (int)nb : 0, tau, out)) return rc;
  out.job.lever_stride = lever_per_member ? (int)nb * 2 : 0;
  if (nl) {
    HIP_OK(h->d_obj_lever.ensure(nl));
    HIP_OK(hipMemcpyAsync(h->d_obj_lever.p, lever, sizeof(double) * nl, hipMemcpyHostToDevice, h->stream));
  }
  return 0;
}

// the kernel arguments of a weighted job; the lever buffer carries the levers (angular kind) or the part coefficients (strain)
ObjArgs obj_args(const dfx_handle* h, const ObjJob& j) {
  ObjArgs a;
  a.fields = h->d_fields.p; a.blocks = h->d_obj_blocks.p; a.w = h->d_obj_w.p;
  a.tau = j.has_tau ? h->d_obj_tau.p : nullptr;
  a.lever = j.kind == DFX_OBJ_KINETIC ? nullptr : h->d_obj_lever.p;
  a.n_act = j.n_act; a.w_stride = j.w_stride; a.lever_stride = j.lever_stride;
  return a;
}

// cotangents into G (may be null: value only), the value into d_obj and, when given, into pinned host memory
int launch_objective(dfx_handle* h, const ObjJob& j, double* G, double* objective_host) {
  const size_t B = h->pl.batch;
  const unsigned chunks = chunks_of((long long)h->ts.size() * j.n_act, kObjThreads);
  HIP_OK(h->d_obj_part.ensure(B * chunks));
  DevCtx c = make_ctx(h);
  const ObjArgs a = obj_args(h, j);
  const dim3 grid(chunks, (unsigned)B);
  if (j.kind == DFX_OBJ_KINETIC) hipLaunchKernelGGL(k_objective<DFX_OBJ_KINETIC>, grid, dim3(kObjThreads), 0, h->stream, c, a, G, h->d_obj_part.p);
  else hipLaunchKernelGGL(k_objective<DFX_OBJ_ANGULAR_MOMENTUM>, grid, dim3(kObjThreads), 0, h->stream, c, a, G, h->d_obj_part.p);
  hipLaunchKernelGGL(k_objective_finish, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, (const double*)h->d_obj_part.p, (int)chunks, h->d_obj.p,
                     objective_host);
  return 0;
}

// ---- ligament strain energy: slot weights and listed blocks of the bond weights; the part coefficients travel in the lever buffer
int prepare_strain(dfx_handle* h, const char* who, const double* bw, int32_t w_per_member, const double* tau, const double* parts, ObjHost& out) {
  const Plan& pl = h->pl;
  if (!bw) { h->err = std::string(who) + ": bond_weights is NULL"; return 1; }
  if (!parts) { h->err = std::string(who) + ": parts4 is NULL"; return 1; }
  if (pl.n_ovf) {
    h->err = std::string(who) + ": nodes with more than one ligament (a general bond list with extra ligaments) are not supported by the strain-energy objective";
    return 1;
  }
  const size_t wm = w_per_member ? pl.batch : 1;
  if (!all_finite(h, who, "bond weight", bw, wm * pl.n_bonds) || !all_finite(h, who, "time weight", tau, h->ts.size()) ||
      !all_finite(h, who, "part coefficient", parts, 4))
    return 1;
  if (parts[3] != 0.0 && pl.contact != DFX_CONTACT_ANGLE) {
    h->err = std::string(who) + ": c_contact != 0 needs a lattice with the angle contact (the distance-based contact energy is not part of this objective)";
    return 1;
  }
  std::vector<double> sw;
  slot_weights(pl, bw, wm, sw, out.blocks, nullptr);
  if (int rc = upload_job(h, kObjStrain, sw.data(), sw.size(), w_per_member ? (int)pl.n_slots : 0, tau, out)) return rc;
  HIP_OK(h->d_obj_lever.ensure(4));
  HIP_OK(hipMemcpyAsync(h->d_obj_lever.p, parts, sizeof(double) * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the slot weights are a local of this function
  return 0;
}

// the build of a strain kernel for the handle's bond model; the angle contact only where the lattice has it (c_contact != 0 is refused
// elsewhere), so the distance-based contact takes the CONTACT = 0 build
template <class F> void with_strain_physics(const dfx_handle* h, F&& f) {
  with_physics<all_physics>(h->pl.model, h->pl.contact == DFX_CONTACT_ANGLE ? 1 : 0, [&](auto M, auto C) { if constexpr (C() != DFX_CONTACT_DISTANCE) f(M, C); });
}

// ligament forces into G (may be null: value only), the value into d_obj and, when given, into pinned host memory
int launch_strain(dfx_handle* h, const ObjJob& j, double* G, double* objective_host) {
  const size_t B = h->pl.batch;
  const unsigned chunks = chunks_of((long long)h->ts.size() * j.n_act, kObjQuads);
  HIP_OK(h->d_obj_part.ensure(B * chunks));
  DevCtx c = make_ctx(h);
  const ObjArgs a = obj_args(h, j);
  const dim3 grid(chunks, (unsigned)B);
  with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_strain_objective<M(), C()>), grid, dim3(kObjThreads), 0, h->stream, c, a, G, h->d_obj_part.p); });
  hipLaunchKernelGGL(k_objective_finish, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, (const double*)h->d_obj_part.p, (int)chunks, h->d_obj.p,
                     objective_host);
  return 0;
}

// ---- peak ligament strain: the checks of a call (return 1 with h->err), then slot weights and listed blocks of the bond weights and bond
// coefficients -> slot coefficients (both end slots of a ligament carry them)
int prepare_peak(dfx_handle* h, const char* who, const double* coef, int32_t coef_per_member, const double* bw, int32_t w_per_member,
                 const double* tau, int32_t aggregate, double sharp, ObjHost& out) {
  const Plan& pl = h->pl;
  const size_t B = pl.batch, NS = pl.n_slots, nbd = pl.n_bonds, Tn = h->ts.size();
  const std::string w(who);
  if (!coef) { h->err = w + ": bond_coef is NULL"; return 1; }
  if (pl.n_ovf) {
    h->err = w + ": nodes with more than one ligament (a general bond list with extra ligaments) are not supported by the peak-strain objective";
    return 1;
  }
  if (aggregate != DFX_PEAK_KS && aggregate != DFX_PEAK_PNORM) {
    h->err = w + ": unknown aggregate " + std::to_string(aggregate) + " (DFX_PEAK_KS = 0, DFX_PEAK_PNORM = 1)";
    return 1;
  }
  if (!std::isfinite(sharp)) { h->err = w + ": sharpness is not finite"; return 1; }
  if (aggregate == DFX_PEAK_KS && !(sharp > 0.0)) { h->err = w + ": sharpness beta must be positive with the KS aggregate"; return 1; }
  if (aggregate == DFX_PEAK_PNORM && !(sharp >= 1.0)) { h->err = w + ": sharpness p must be at least 1 with the p-norm aggregate"; return 1; }
  const size_t cm = coef_per_member ? B : 1, wm = bw && w_per_member ? B : 1;
  if (!all_finite(h, who, "bond coefficient", coef, cm * nbd * 3, true) || !all_finite(h, who, "bond weight", bw, wm * nbd, true) ||
      !all_finite(h, who, "time weight", tau, Tn, true))
    return 1;
  const bool any_tau = !tau || std::any_of(tau, tau + Tn, [](double t) { return t > 0.0; });
  std::vector<double> sw, sc(cm * NS * 3, 0.0);
  std::vector<char> member_any(wm, 0);
  slot_weights(pl, bw, wm, sw, out.blocks, &member_any);
  for (size_t sl = 0; sl < NS; ++sl) {
    if (pl.slot_info[sl] < 0) continue;
    const size_t bond = (size_t)pl.slot_bond[sl];
    for (size_t m = 0; m < cm; ++m)
      for (int i = 0; i < 3; ++i) sc[(m * NS + sl) * 3 + i] = coef[(m * nbd + bond) * 3 + i];
  }
  for (size_t m = 0; m < wm; ++m)
    if (!member_any[m] || !any_tau) {
      h->err = w + ": all weights are zero for member " + std::to_string(m) + " (a peak needs one (output, ligament) pair with tau * omega > 0)";
      return 1;
    }
  h->pk.aggregate = aggregate; h->pk.sharp = sharp; h->pk.coef_stride = coef_per_member ? (long long)(NS * 3) : 0;
  if (int rc = upload_job(h, kObjPeak, sw.data(), sw.size(), wm > 1 || (bw && w_per_member) ? (int)NS : 0, tau, out)) return rc;
  HIP_OK(h->d_pk_coef.ensure(sc.size()));
  HIP_OK(h->d_pk_res.ensure(B * 4));
  HIP_OK(h->d_pk_at.ensure(B * 2));
  HIP_OK(hipMemcpyAsync(h->d_pk_coef.p, sc.data(), sizeof(double) * sc.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the slot arrays are locals of this function
  return 0;
}

PeakArgs peak_args(const dfx_handle* h) {
  PeakArgs p;
  p.coef = h->d_pk_coef.p; p.slot_bond = h->d_slot_bond.p;
  p.Q = h->d_pk_q.p; p.pmax = h->d_pk_max.p; p.pkey = h->d_pk_key.p; p.res = h->d_pk_res.p; p.at = h->d_pk_at.p;
  p.coef_stride = h->pk.coef_stride;
  p.n_bonds = (int)h->pl.n_bonds; p.aggregate = h->pk.aggregate; p.sharp = h->pk.sharp;
  return p;
}

// the peak kernels are built per bond model only (no contact part in q)
template <class F> void with_peak_physics(const dfx_handle* h, F&& f) {
  with_physics<all_physics>(h->pl.model, 0, [&](auto M, auto C) { if constexpr (C() == 0) f(M); });
}

// the four reductions of the value (J into d_obj; J | q_hat as doubles and (k_hat, b_hat) as int32 behind them into pinned host memory when
// given), then -- with G -- the cotangent of the sweep
int launch_peak(dfx_handle* h, const ObjJob& j, double* G, double* host) {
  const size_t B = h->pl.batch;
  const unsigned chunks = chunks_of((long long)h->ts.size() * j.n_act, kObjQuads);
  HIP_OK(h->d_pk_q.ensure(B * h->ts.size() * (size_t)h->pl.n_bonds));
  HIP_OK(h->d_pk_max.ensure(B * chunks));
  HIP_OK(h->d_pk_key.ensure(B * chunks));
  HIP_OK(h->d_obj_part.ensure(B * chunks));
  DevCtx c = make_ctx(h);
  const ObjArgs a = obj_args(h, j);
  const PeakArgs p = peak_args(h);
  const dim3 grid(chunks, (unsigned)B);
  int32_t* host_at = host ? reinterpret_cast<int32_t*>(host + 2 * B) : nullptr;
  with_peak_physics(h, [&](auto M) { hipLaunchKernelGGL((k_strain_peak_measure<M()>), grid, dim3(kObjThreads), 0, h->stream, c, a, p); });
  hipLaunchKernelGGL(k_strain_peak_finish, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, p, (int)chunks);
  hipLaunchKernelGGL(k_strain_peak_sum, grid, dim3(kObjThreads), 0, h->stream, c, a, p, h->d_obj_part.p);
  hipLaunchKernelGGL(k_strain_peak_value, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, p, (const double*)h->d_obj_part.p, (int)chunks, h->d_obj.p,
                     host, host_at, (int)B);
  if (G) with_peak_physics(h, [&](auto M) { hipLaunchKernelGGL((k_strain_peak_cotangent<M()>), grid, dim3(kObjThreads), 0, h->stream, c, a, p, G); });
  return 0;
}

// ---- signal misfit: the term list compacted into index tables.  FORCE blocks: the blocks with a force term (components 6..8); the SET: those
// and the blocks bonded to them (every ligament with an end on a force block is evaluated from both of its ends).  HINGES: the (block, node)
// slots with a hinge term (components 9 + 3 node + dof), their channels behind the block channels; both end blocks of each join the set
}  // namespace

// (SigTerms / SigTables: dfx_engine.h -- the forward-mode signal entries of engine_tangent.hip build the same tables)
// The checks of a term list (return 1 with h->err) and its tables: force blocks, the set, the terms by signal in list order.
int signal_term_tables(dfx_handle* h, const char* who, const SigTerms& t, SigTables& out) {
  const Plan& pl = h->pl;
  const size_t nb = pl.n_blocks;
  const int ns = t.n_signals;
  const std::string w(who);
  if (ns <= 0) { h->err = w + ": n_signals must be positive"; return 1; }
  if (t.n <= 0 || !t.signal || !t.block || !t.comp || !t.coef) { h->err = w + ": an empty term list (a NULL term array, or n_terms <= 0)"; return 1; }
  std::vector<int> count(ns, 0);
  bool force = false;
  for (int i = 0; i < t.n; ++i) {
    if (t.signal[i] < 0 || t.signal[i] >= ns) { h->err = w + ": term " + std::to_string(i) + " names signal " + std::to_string(t.signal[i]) + " out of range (n_signals = " + std::to_string(ns) + ")"; return 1; }
    if (t.block[i] < 0 || (size_t)t.block[i] >= nb) { h->err = w + ": term " + std::to_string(i) + " names block " + std::to_string(t.block[i]) + " out of range (n_blocks = " + std::to_string(nb) + ")"; return 1; }
    if (t.comp[i] < 0 || t.comp[i] > (h->sig_hinges ? 20 : 8)) {
      h->err = w + ": term " + std::to_string(i) + " names component " + std::to_string(t.comp[i]) + " out of range (0..2 displacement, 3..5 velocity, 6..8 elastic force" +
               (h->sig_hinges ? ", 9 + 3 node + dof hinge force)" : "; the hinge forces 9 + 3 node + dof are off: dfx_signal_hinge_channels)");
      return 1;
    }
    if (t.comp[i] >= 9) {
      const int node = (t.comp[i] - 9) / 3;
      if (node >= pl.n_npb) { h->err = w + ": term " + std::to_string(i) + " names the hinge on node " + std::to_string(node) + " but a block of this lattice has " + std::to_string(pl.n_npb) + " nodes"; return 1; }
      if (pl.slot_info[(size_t)t.block[i] * 4 + node] < 0) { h->err = w + ": term " + std::to_string(i) + " names the hinge on node " + std::to_string(node) + " of block " + std::to_string(t.block[i]) + ", which carries no ligament"; return 1; }
    }
    if (!std::isfinite(t.coef[i])) { h->err = w + ": non-finite coefficient"; return 1; }
    ++count[t.signal[i]];
    force = force || t.comp[i] >= 6;
  }
  for (int s = 0; s < ns; ++s)
    if (!count[s]) { h->err = w + ": signal " + std::to_string(s) + " is empty (no term names it)"; return 1; }
  if (force && pl.contact == DFX_CONTACT_DISTANCE) {
    h->err = w + ": force components need the ligament and angle-contact energy (the distance-based contact energy is not part of the signal channels)";
    return 1;
  }
  if (force && pl.n_ovf) {
    h->err = w + ": nodes with more than one ligament (a general bond list with extra ligaments) are not supported by the force components of a signal";
    return 1;
  }
  // force blocks, listed hinges and the set
  std::vector<int32_t>&fmap = out.fmap, &fblocks = out.fblocks, &set = out.set, &hslots = out.hslots, &hmap = out.hmap;
  fmap.assign(nb, -1); fblocks.clear(); set.clear(); hslots.clear(); hmap.clear();
  std::vector<char> in_f(nb, 0), in_set(nb, 0);
  for (int i = 0; i < t.n; ++i) if (t.comp[i] >= 6 && t.comp[i] < 9) in_f[t.block[i]] = 1;
  if (std::any_of(t.comp, t.comp + t.n, [](int32_t c) { return c >= 9; })) {
    hmap.assign(pl.n_slots, -1);
    for (int i = 0; i < t.n; ++i) if (t.comp[i] >= 9) hmap[(size_t)t.block[i] * 4 + (t.comp[i] - 9) / 3] = 0;
    for (size_t sl = 0; sl < (size_t)pl.n_slots; ++sl) {
      if (hmap[sl] < 0) continue;
      hmap[sl] = (int32_t)hslots.size();
      hslots.push_back((int32_t)sl);
      in_set[sl >> 2] = 1;
      in_set[pl.slot_info[sl] >> 3] = 1;
    }
  }
  for (size_t b = 0; b < nb; ++b) {
    if (!in_f[b]) continue;
    fmap[b] = (int32_t)fblocks.size();
    fblocks.push_back((int32_t)b);
    in_set[b] = 1;
    for (int kk = 0; kk < 4; ++kk) {
      const int info = pl.slot_info[b * 4 + kk];
      if (info >= 0) in_set[info >> 3] = 1;
    }
  }
  for (size_t b = 0; b < nb; ++b) if (in_set[b]) set.push_back((int32_t)b);
  // the terms by signal, list order kept
  std::vector<int32_t>&sig_ptr = out.sig_ptr, &term_src = out.term_src;
  std::vector<double>& term_coef = out.term_coef;
  sig_ptr.assign(ns + 1, 0); term_src.assign(t.n, 0); term_coef.assign(t.n, 0.0);
  for (int s = 0; s < ns; ++s) sig_ptr[s + 1] = sig_ptr[s] + count[s];
  {
    std::vector<int32_t> at(sig_ptr.begin(), sig_ptr.end() - 1);
    for (int i = 0; i < t.n; ++i) {
      const int c = t.comp[i], b = t.block[i], o = at[t.signal[i]]++;
      term_src[o] = c < 3 ? b * 3 + c : c < 6 ? (int)nb * 3 + b * 3 + (c - 3) : c < 9 ? -1 - (fmap[b] * 3 + (c - 6))
                                                                              : -1 - (((int)fblocks.size() + hmap[(size_t)b * 4 + (c - 9) / 3]) * 3 + (c - 9) % 3);
      term_coef[o] = t.coef[i];
    }
  }
  return 0;
}

namespace {

int prepare_signal(dfx_handle* h, const char* who, const SigTerms& t, const double* targets, int32_t targets_per_member, const double* omega,
                   const double* tau, bool want_target) {
  const Plan& pl = h->pl;
  const size_t B = pl.batch;
  const int Tn = (int)h->ts.size(), ns = t.n_signals;
  const std::string w(who);
  // (signal_term_tables makes these two checks again: here they come before the check of the targets, there before the checks of the terms,
  // and a call that is wrong in both ways reports the same error as ever)
  if (ns <= 0) { h->err = w + ": n_signals must be positive"; return 1; }
  if (t.n <= 0 || !t.signal || !t.block || !t.comp || !t.coef) { h->err = w + ": an empty term list (a NULL term array, or n_terms <= 0)"; return 1; }
  if (want_target && !targets) { h->err = w + ": targets is NULL"; return 1; }
  SigTables tb;
  if (int rc = signal_term_tables(h, who, t, tb)) return rc;
  const size_t n_tg = want_target ? (targets_per_member ? B : 1) * (size_t)Tn * ns : 0;
  if (!all_finite(h, who, "target", targets, n_tg)) return 1;
  if (want_target && (!all_finite(h, who, "signal weight", omega, ns) || !all_finite(h, who, "time weight", tau, Tn))) return 1;
  const std::vector<int32_t>&fmap = tb.fmap, &fblocks = tb.fblocks, &set = tb.set, &sig_ptr = tb.sig_ptr, &term_src = tb.term_src, &hslots = tb.hslots, &hmap = tb.hmap;
  const std::vector<double>& term_coef = tb.term_coef;
  const size_t nb = pl.n_blocks;
  // the terms by distinct (block, component), list order kept; all three components of a force block and of a listed hinge are listed
  // (w is written whole)
  const int n_fb = (int)fblocks.size();
  std::map<std::pair<int, int>, std::vector<int>> by_dof;
  for (int32_t b : fblocks) for (int c = 6; c < 9; ++c) by_dof[{b, c}];
  for (int32_t sl : hslots) for (int d = 0; d < 3; ++d) by_dof[{sl >> 2, 9 + 3 * (sl & 3) + d}];
  for (int i = 0; i < t.n; ++i) by_dof[{t.block[i], t.comp[i]}].push_back(i);
  std::vector<int32_t> uc_ptr(1, 0), uc_dst, uc_sig;
  std::vector<double> uc_coef;
  for (const auto& e : by_dof) {
    const int b = e.first.first, c = e.first.second;
    uc_dst.push_back(c < 6 ? b * 6 + c : c < 9 ? -1 - (fmap[b] * 3 + (c - 6)) : -1 - ((n_fb + hmap[(size_t)b * 4 + (c - 9) / 3]) * 3 + (c - 9) % 3));
    for (int i : e.second) { uc_sig.push_back(t.signal[i]); uc_coef.push_back(t.coef[i]); }
    uc_ptr.push_back((int32_t)uc_sig.size());
  }
  dfx_handle::SigJob& J = h->sig;
  J.n_fb = n_fb; J.n_set = (int)set.size(); J.n_sig = ns; J.n_uc = (int)uc_dst.size(); J.n_terms = t.n; J.n_blocks = (int)nb;
  J.n_hg = (int)hslots.size();
  const size_t n_ch = (size_t)(J.n_fb + J.n_hg) * 3;
  J.has_target = want_target; J.has_omega = want_target && omega; J.has_tau = want_target && tau;
  J.target_stride = targets_per_member ? (long long)Tn * ns : 0;
  // one int table and one double table, in the order sig_args reads them
  std::vector<int32_t> tab;
  for (const std::vector<int32_t>* v : std::initializer_list<const std::vector<int32_t>*>{&fblocks, &fmap, &set, &sig_ptr, &term_src, &uc_ptr, &uc_dst, &uc_sig, &hslots, &hmap}) tab.insert(tab.end(), v->begin(), v->end());
  std::vector<double> dbl(term_coef);
  dbl.insert(dbl.end(), uc_coef.begin(), uc_coef.end());
  if (J.has_omega) dbl.insert(dbl.end(), omega, omega + ns);
  if (J.has_tau) dbl.insert(dbl.end(), tau, tau + Tn);
  if (want_target) dbl.insert(dbl.end(), targets, targets + n_tg);
  HIP_OK(h->d_sig_tab.ensure(tab.size()));
  HIP_OK(h->d_sig_coef.ensure(dbl.size()));
  HIP_OK(h->d_sig_chan.ensure(B * Tn * n_ch));
  HIP_OK(h->d_sig_w.ensure(B * Tn * n_ch));
  HIP_OK(h->d_sig_S.ensure(B * Tn * (size_t)ns));
  HIP_OK(h->d_sig_c.ensure(B * Tn * (size_t)ns));
  HIP_OK(h->d_obj.ensure(B));
  HIP_OK(hipMemcpyAsync(h->d_sig_tab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(h->d_sig_coef.p, dbl.data(), sizeof(double) * dbl.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the tables are locals of this function
  return 0;
}

SigArgs sig_args(const dfx_handle* h) {
  const dfx_handle::SigJob& J = h->sig;
  const int Tn = (int)h->ts.size();
  SigArgs a;
  a.fields = h->d_fields.p;
  const int32_t* ip = h->d_sig_tab.p;
  a.fblocks = ip; ip += J.n_fb;
  a.fmap = ip; ip += J.n_blocks;
  a.set = ip; ip += J.n_set;
  a.sig_ptr = ip; ip += J.n_sig + 1;
  a.term_src = ip; ip += J.n_terms;
  a.uc_ptr = ip; ip += J.n_uc + 1;
  a.uc_dst = ip; ip += J.n_uc;
  a.uc_sig = ip; ip += J.n_terms;
  a.hslots = J.n_hg ? ip : nullptr; ip += J.n_hg;
  a.hmap = J.n_hg ? ip : nullptr;
  const double* dp = h->d_sig_coef.p;
  a.term_coef = dp; dp += J.n_terms;
  a.uc_coef = dp; dp += J.n_terms;
  a.omega = J.has_omega ? dp : nullptr; dp += J.has_omega ? J.n_sig : 0;
  a.tau = J.has_tau ? dp : nullptr; dp += J.has_tau ? Tn : 0;
  a.target = J.has_target ? dp : nullptr;
  a.chan = h->d_sig_chan.p; a.S = h->d_sig_S.p; a.cres = h->d_sig_c.p; a.w = h->d_sig_w.p;
  a.target_stride = J.target_stride;
  a.n_fb = J.n_fb; a.n_set = J.n_set; a.n_sig = J.n_sig; a.n_uc = J.n_uc;
  a.n_hg = J.n_hg; a.n_ch = (J.n_fb + J.n_hg) * 3;
  return a;
}

// from the residual cotangents in d_sig_c to the cotangent G of the sweep: the field rows and the direction w, then K w of the force terms
void launch_signal_reverse(dfx_handle* h, const DevCtx& c, const SigArgs& a, double* G) {
  const dfx_handle::SigJob& J = h->sig;
  const size_t B = h->pl.batch;
  const long long Tn = (long long)h->ts.size();
  hipLaunchKernelGGL(k_signal_direction, dim3(chunks_of(Tn * J.n_uc, kObjThreads), (unsigned)B), dim3(kObjThreads), 0, h->stream, c, a, G);
  if (J.n_set) {
    const dim3 grid(chunks_of(Tn * J.n_set, kObjQuads), (unsigned)B);
    with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_signal_cotangent<M(), C()>), grid, dim3(kObjThreads), 0, h->stream, c, a, G); });
  }
}

// channels, signals and (with targets) residual cotangents and the value into d_obj / pinned host memory; with G the cotangent of the sweep
int launch_signal(dfx_handle* h, double* G, double* objective_host) {
  const dfx_handle::SigJob& J = h->sig;
  const size_t B = h->pl.batch;
  const long long Tn = (long long)h->ts.size();
  DevCtx c = make_ctx(h);
  const SigArgs a = sig_args(h);
  if (J.n_fb) {
    const dim3 grid(chunks_of(Tn * J.n_fb, kObjQuads), (unsigned)B);
    with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_signal_channels<M(), C()>), grid, dim3(kObjThreads), 0, h->stream, c, a); });
  }
  if (J.n_hg) {
    const dim3 grid(chunks_of(Tn * J.n_hg, kHingeThreads), (unsigned)B);
    with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_signal_hinge_channels<M(), C()>), grid, dim3(kHingeThreads), 0, h->stream, c, a); });
  }
  const unsigned chunks = chunks_of(Tn * J.n_sig, kObjThreads);
  if (J.has_target) HIP_OK(h->d_obj_part.ensure(B * chunks));
  hipLaunchKernelGGL(k_signal_residual, dim3(chunks, (unsigned)B), dim3(kObjThreads), 0, h->stream, c, a, J.has_target ? h->d_obj_part.p : nullptr);
  if (J.has_target)
    hipLaunchKernelGGL(k_objective_finish, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, (const double*)h->d_obj_part.p, (int)chunks, h->d_obj.p,
                       objective_host);
  if (G) launch_signal_reverse(h, c, a, G);
  return 0;
}

// ---- signal projections: the checks of the basis, the row weights and the targets (return 1 with h->err), prepare_signal without targets
// for the terms, then basis | row weights | targets into one buffer.  want_w: the call forms a value (row weights required)
int prepare_projection(dfx_handle* h, const char* who, const SigTerms& t, const double* basis, int32_t n_rows, const double* row_weights,
                       const double* targets, int32_t targets_per_member, bool want_w) {
  const size_t B = h->pl.batch;
  const size_t Tn = h->ts.size();
  const std::string w(who);
  if (n_rows < 1) { h->err = w + ": n_rows must be at least 1, got " + std::to_string(n_rows); return 1; }
  if (!basis) { h->err = w + ": basis is NULL"; return 1; }
  if (want_w && !row_weights) { h->err = w + ": row_weights is NULL"; return 1; }
  const size_t ns = t.n_signals > 0 ? (size_t)t.n_signals : 0, n_w = want_w ? ns * n_rows : 0;
  const size_t n_tg = want_w && targets ? (targets_per_member ? B : 1) * ns * n_rows : 0;
  if (!all_finite(h, who, "basis entry", basis, (size_t)n_rows * Tn) || !all_finite(h, who, "row weight", row_weights, n_w) ||
      !all_finite(h, who, "target", targets, n_tg))
    return 1;
  if (int rc = prepare_signal(h, who, t, nullptr, 0, nullptr, nullptr, false)) return rc;
  dfx_handle::ProjJob& J = h->proj;
  J.n_rows = n_rows; J.has_w = want_w; J.has_target = n_tg != 0;
  J.target_stride = targets_per_member ? (long long)(ns * n_rows) : 0;
  std::vector<double> dbl(basis, basis + (size_t)n_rows * Tn);
  if (n_w) dbl.insert(dbl.end(), row_weights, row_weights + n_w);
  if (n_tg) dbl.insert(dbl.end(), targets, targets + n_tg);
  HIP_OK(h->d_proj_coef.ensure(dbl.size()));
  HIP_OK(h->d_proj_P.ensure(B * ns * n_rows));
  HIP_OK(hipMemcpyAsync(h->d_proj_coef.p, dbl.data(), sizeof(double) * dbl.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the table is a local of this function
  return 0;
}

ProjArgs proj_args(const dfx_handle* h) {
  const dfx_handle::ProjJob& J = h->proj;
  ProjArgs p;
  const double* dp = h->d_proj_coef.p;
  p.basis = dp; dp += (size_t)J.n_rows * h->ts.size();
  p.W = J.has_w ? dp : nullptr; dp += J.has_w ? (size_t)h->sig.n_sig * J.n_rows : 0;
  p.target = J.has_target ? dp : nullptr;
  p.P = h->d_proj_P.p;
  p.target_stride = J.target_stride;
  p.n_rows = J.n_rows;
  return p;
}

// channels and signals (launch_signal without targets), the projections and (with row weights) the value into d_obj / pinned host memory;
// with G the cotangent c on the signals and from it the cotangent of the sweep
int launch_projection(dfx_handle* h, double* G, double* objective_host) {
  const dfx_handle::ProjJob& J = h->proj;
  const size_t B = h->pl.batch;
  if (int rc = launch_signal(h, nullptr, nullptr)) return rc;
  DevCtx c = make_ctx(h);
  const SigArgs a = sig_args(h);
  const ProjArgs p = proj_args(h);
  const unsigned chunks = chunks_of((long long)h->sig.n_sig * J.n_rows, kObjWaves);
  if (J.has_w) HIP_OK(h->d_obj_part.ensure(B * chunks));
  hipLaunchKernelGGL(k_signal_project, dim3(chunks, (unsigned)B), dim3(kObjThreads), 0, h->stream, c, a, p, J.has_w ? h->d_obj_part.p : nullptr);
  if (J.has_w)
    hipLaunchKernelGGL(k_objective_finish, dim3((unsigned)B), dim3(kObjThreads), 0, h->stream, (const double*)h->d_obj_part.p, (int)chunks, h->d_obj.p,
                       objective_host);
  if (G) {
    hipLaunchKernelGGL(k_signal_project_residual, dim3(chunks_of((long long)h->ts.size() * h->sig.n_sig, kObjThreads), (unsigned)B), dim3(kObjThreads), 0,
                       h->stream, c, a, p);
    launch_signal_reverse(h, c, a, G);
  }
  return 0;
}

// ---- signal cross-correlation: the checks of the pairs, the templates, the lags and the reduction (return 1 with h->err), prepare_signal
// without targets for the terms, then pairs | templates into one buffer.  value: the call forms J (the reduction and its weights are checked)
struct XcorrCall {
  int32_t n_pairs; const int32_t *pair_a, *pair_b; const double* templ; int32_t n_templ, templ_per_member, max_lag, norm;
  bool value; int32_t reduce, lag0; double beta, w_peak, w_delay, delay_target;
};

int prepare_xcorr(dfx_handle* h, const char* who, const SigTerms& t, const XcorrCall& q) {
  const size_t B = h->pl.batch;
  const size_t Tn = h->ts.size();
  const std::string w(who);
  const int ns = t.n_signals;
  if (q.n_pairs < 1) { h->err = w + ": n_pairs must be at least 1, got " + std::to_string(q.n_pairs); return 1; }
  if (!q.pair_a || !q.pair_b) { h->err = w + ": pair_a or pair_b is NULL"; return 1; }
  if (q.templ && q.n_templ < 1) { h->err = w + ": templates given with n_templates = " + std::to_string(q.n_templ); return 1; }
  bool named = false;
  for (int p = 0; p < q.n_pairs; ++p) {
    const int a = q.pair_a[p], b = q.pair_b[p];
    if (a < 0 || a >= ns) { h->err = w + ": pair " + std::to_string(p) + " names signal " + std::to_string(a) + " out of range (n_signals = " + std::to_string(ns) + ")"; return 1; }
    if (b >= ns) { h->err = w + ": pair " + std::to_string(p) + " names signal " + std::to_string(b) + " out of range (n_signals = " + std::to_string(ns) + ")"; return 1; }
    if (b < 0 && !q.templ) { h->err = w + ": pair " + std::to_string(p) + " names template column " + std::to_string(-1 - (long long)b) + " but templates is NULL"; return 1; }
    if (b < 0 && -1 - (long long)b >= q.n_templ) { h->err = w + ": pair " + std::to_string(p) + " names template column " + std::to_string(-1 - (long long)b) + " out of range (n_templates = " + std::to_string(q.n_templ) + ")"; return 1; }
    named = named || b < 0;
  }
  if (q.max_lag < 0 || (size_t)q.max_lag + 1 > Tn) { h->err = w + ": max_lag " + std::to_string(q.max_lag) + " outside [0, T - 1] (T = " + std::to_string(Tn) + ")"; return 1; }
  if (q.norm != DFX_XCORR_NORM_REFERENCE && q.norm != DFX_XCORR_NORM_COEFFICIENT && q.norm != DFX_XCORR_NORM_NONE) {
    h->err = w + ": unknown normalisation " + std::to_string(q.norm) + " (DFX_XCORR_NORM_REFERENCE = 0, _COEFFICIENT = 1, _NONE = 2)";
    return 1;
  }
  if (q.value) {
    if (q.reduce != DFX_XCORR_AT && q.reduce != DFX_XCORR_MAX && q.reduce != DFX_XCORR_SOFTMAX) {
      h->err = w + ": unknown reduction " + std::to_string(q.reduce) + " (DFX_XCORR_AT = 0, DFX_XCORR_MAX = 1, DFX_XCORR_SOFTMAX = 2)";
      return 1;
    }
    if (q.reduce == DFX_XCORR_AT && (q.lag0 < -q.max_lag || q.lag0 > q.max_lag)) {
      h->err = w + ": lag0 " + std::to_string(q.lag0) + " outside [-max_lag, max_lag] (max_lag = " + std::to_string(q.max_lag) + ")";
      return 1;
    }
    if (q.reduce == DFX_XCORR_SOFTMAX && !(std::isfinite(q.beta) && q.beta > 0.0)) { h->err = w + ": beta must be positive and finite with the softmax reduction"; return 1; }
    if (!std::isfinite(q.w_peak) || !std::isfinite(q.w_delay)) { h->err = w + ": non-finite weight"; return 1; }
    if (!std::isfinite(q.delay_target)) { h->err = w + ": non-finite delay_target"; return 1; }
    if (q.w_delay != 0.0 && q.reduce != DFX_XCORR_SOFTMAX) { h->err = w + ": w_delay != 0 needs the softmax reduction (the delay of a maximum has no derivative)"; return 1; }
  }
  const size_t n_tp = q.templ ? (q.templ_per_member ? B : 1) * Tn * (size_t)q.n_templ : 0;
  if (!all_finite(h, who, "template", q.templ, n_tp)) return 1;
  if (int rc = prepare_signal(h, who, t, nullptr, 0, nullptr, nullptr, false)) return rc;
  dfx_handle::XcorrJob& J = h->xc;
  J.n_pairs = q.n_pairs; J.n_templ = q.templ ? q.n_templ : 0; J.D = q.max_lag; J.norm = q.norm;
  J.has_templ = named; J.templ_stride = q.templ_per_member ? (long long)(Tn * (size_t)q.n_templ) : 0;
  J.reduce = q.value ? q.reduce : DFX_XCORR_AT; J.lag0 = q.value ? q.lag0 : 0; J.beta = q.value ? q.beta : 1.0;
  J.w_peak = q.value ? q.w_peak : 1.0; J.w_delay = q.value ? q.w_delay : 0.0; J.delay_target = q.value ? q.delay_target : 0.0;
  std::vector<double> dbl((size_t)q.n_pairs, 0.0);                 // 2 n_pairs int32: pair_a | pair_b
  memcpy(dbl.data(), q.pair_a, sizeof(int32_t) * q.n_pairs);
  memcpy(reinterpret_cast<char*>(dbl.data()) + sizeof(int32_t) * q.n_pairs, q.pair_b, sizeof(int32_t) * q.n_pairs);
  if (named) dbl.insert(dbl.end(), q.templ, q.templ + n_tp);
  const size_t nl = 2 * (size_t)q.max_lag + 1;
  HIP_OK(h->d_xc_coef.ensure(dbl.size()));
  HIP_OK(h->d_xc_R.ensure(B * nl * 3));
  HIP_OK(h->d_xc_s.ensure(B * 6));
  HIP_OK(hipMemcpyAsync(h->d_xc_coef.p, dbl.data(), sizeof(double) * dbl.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the table is a local of this function
  return 0;
}

XcorrArgs xcorr_args(const dfx_handle* h) {
  const dfx_handle::XcorrJob& J = h->xc;
  const size_t B = h->pl.batch, nl = 2 * (size_t)J.D + 1;
  XcorrArgs x;
  x.pair_a = reinterpret_cast<const int32_t*>(h->d_xc_coef.p);
  x.pair_b = x.pair_a + J.n_pairs;
  x.templ = J.has_templ ? h->d_xc_coef.p + J.n_pairs : nullptr;
  x.R = h->d_xc_R.p; x.rho = x.R + B * nl; x.Rbar = x.rho + B * nl;
  x.E = h->d_xc_s.p; x.ebar = x.E + B * 2; x.peak = x.ebar + B * 2; x.delay = x.peak + B;
  x.templ_stride = J.templ_stride;
  x.n_pairs = J.n_pairs; x.n_templ = J.n_templ; x.D = J.D; x.norm = J.norm; x.reduce = J.reduce; x.lag0 = J.lag0;
  x.beta = J.beta; x.w_peak = J.w_peak; x.w_delay = J.w_delay; x.delay_target = J.delay_target;
  return x;
}

// channels and signals (launch_signal without targets), R, EA, EB over the lags, the reduction (J into d_obj and, when given, J | M | delta
// into pinned host memory); with G the cotangent c on the signals and from it the cotangent of the sweep
int launch_xcorr(dfx_handle* h, double* G, double* host3) {
  const dfx_handle::XcorrJob& J = h->xc;
  const size_t B = h->pl.batch;
  if (int rc = launch_signal(h, nullptr, nullptr)) return rc;
  DevCtx c = make_ctx(h);
  const SigArgs a = sig_args(h);
  const XcorrArgs x = xcorr_args(h);
  hipLaunchKernelGGL(k_signal_xcorr, dim3(chunks_of(2LL * J.D + 3, kObjWaves), (unsigned)B), dim3(kObjThreads), 0, h->stream, c, a, x);
  hipLaunchKernelGGL(k_signal_xcorr_reduce, dim3((unsigned)B), dim3(64), 0, h->stream, x, h->d_obj.p, host3, (int)B);
  if (G) {
    hipLaunchKernelGGL(k_signal_xcorr_residual, dim3(chunks_of((long long)h->ts.size() * h->sig.n_sig, kObjThreads), (unsigned)B), dim3(kObjThreads), 0,
                       h->stream, c, a, x);
    launch_signal_reverse(h, c, a, G);
  }
  return 0;
}

// ---- signal spectral ratios: the checks of the basis, the group weights, the offsets and the reduction (return 1 with h->err),
// prepare_signal without targets for the terms, then basis | Wn | Wd | n0 | d0 | a into one buffer.  value: the call forms J (aggregate,
// beta and the group coefficients are checked); without, only the measures are asked for and a is zeros
struct SpectrumCall {
  const double* basis; int32_t n_rows, G; const double *Wn, *Wd, *n0, *d0; int32_t off_per_member;
  bool value; int32_t measure, aggregate; double beta; const double* a;
};

int prepare_spectrum(dfx_handle* h, const char* who, const SigTerms& t, const SpectrumCall& q) {
  const size_t B = h->pl.batch;
  const size_t Tn = h->ts.size();
  const std::string w(who);
  if (q.n_rows < 1) { h->err = w + ": n_rows must be at least 1, got " + std::to_string(q.n_rows); return 1; }
  if (!q.basis) { h->err = w + ": basis is NULL"; return 1; }
  if (q.G < 1) { h->err = w + ": n_groups must be at least 1, got " + std::to_string(q.G); return 1; }
  if (!q.Wn || !q.Wd) { h->err = w + ": num_weights or den_weights is NULL"; return 1; }
  if (q.measure != DFX_SPECTRUM_RATIO && q.measure != DFX_SPECTRUM_LOG) {
    h->err = w + ": unknown measure " + std::to_string(q.measure) + " (DFX_SPECTRUM_RATIO = 0, DFX_SPECTRUM_LOG = 1)";
    return 1;
  }
  if (q.value) {
    if (q.aggregate != DFX_SPECTRUM_SUM && q.aggregate != DFX_SPECTRUM_KS) {
      h->err = w + ": unknown aggregate " + std::to_string(q.aggregate) + " (DFX_SPECTRUM_SUM = 0, DFX_SPECTRUM_KS = 1)";
      return 1;
    }
    if (q.aggregate == DFX_SPECTRUM_KS && !(std::isfinite(q.beta) && q.beta > 0.0)) { h->err = w + ": beta must be positive and finite with the KS aggregate"; return 1; }
    if (!q.a) { h->err = w + ": group_coef is NULL"; return 1; }
  }
  const size_t G = (size_t)q.G, ns = t.n_signals > 0 ? (size_t)t.n_signals : 0, np = ns * q.n_rows, om = q.off_per_member ? B : 1;
  if (!all_finite(h, who, "basis entry", q.basis, (size_t)q.n_rows * Tn) || !all_finite(h, who, "group weight", q.Wn, G * np, true) ||
      !all_finite(h, who, "group weight", q.Wd, G * np, true) || !all_finite(h, who, "offset", q.n0, om * G, true) ||
      !all_finite(h, who, "offset", q.d0, om * G, true) || !all_finite(h, who, "group coefficient", q.value ? q.a : nullptr, G))
    return 1;
  for (size_t g = 0; g < G && ns; ++g) {
    if (std::any_of(q.Wn + g * np, q.Wn + (g + 1) * np, [](double v) { return v > 0.0; })) continue;
    for (size_t m = 0; m < om; ++m)
      if (!q.n0 || q.n0[m * G + g] == 0.0) {
        h->err = w + ": the numerator of group " + std::to_string(g) + " is empty (no weight and a zero offset)";
        return 1;
      }
  }
  if (int rc = prepare_signal(h, who, t, nullptr, 0, nullptr, nullptr, false)) return rc;
  dfx_handle::SpecJob& J = h->sp;
  J.n_rows = q.n_rows; J.G = q.G; J.off_stride = q.off_per_member ? (long long)G : 0;
  J.measure = q.measure; J.aggregate = q.value ? q.aggregate : DFX_SPECTRUM_SUM; J.beta = q.value ? q.beta : 1.0;
  std::vector<double> dbl(q.basis, q.basis + (size_t)q.n_rows * Tn);
  dbl.insert(dbl.end(), q.Wn, q.Wn + G * np);
  dbl.insert(dbl.end(), q.Wd, q.Wd + G * np);
  for (const double* off : {q.n0, q.d0}) {
    if (off) dbl.insert(dbl.end(), off, off + om * G);
    else dbl.insert(dbl.end(), om * G, 0.0);
  }
  if (q.value) dbl.insert(dbl.end(), q.a, q.a + G);
  else dbl.insert(dbl.end(), G, 0.0);
  HIP_OK(h->d_sp_coef.ensure(dbl.size()));
  HIP_OK(h->d_proj_P.ensure(B * np));
  HIP_OK(h->d_sp_forms.ensure(B * G * 2));
  HIP_OK(h->d_sp_l.ensure(B * G));
  HIP_OK(h->d_sp_lam.ensure(B * G * 2));
  HIP_OK(h->d_sp_weff.ensure(B * np));
  HIP_OK(hipMemcpyAsync(h->d_sp_coef.p, dbl.data(), sizeof(double) * dbl.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));       // the table is a local of this function
  return 0;
}

// the projections of a spectrum call (basis in its own buffer, no row weights, no targets) and the spectrum arguments
void spectrum_args(const dfx_handle* h, ProjArgs& p, SpecArgs& x) {
  const dfx_handle::SpecJob& J = h->sp;
  const size_t B = h->pl.batch, G = (size_t)J.G, np = (size_t)h->sig.n_sig * J.n_rows, om = J.off_stride ? B : 1;
  const double* dp = h->d_sp_coef.p;
  p.basis = dp; dp += (size_t)J.n_rows * h->ts.size();
  p.W = nullptr; p.target = nullptr; p.P = h->d_proj_P.p; p.target_stride = 0; p.n_rows = J.n_rows;
  x.Wn = dp; dp += G * np;
  x.Wd = dp; dp += G * np;
  x.n0 = dp; dp += om * G;
  x.d0 = dp; dp += om * G;
  x.a = dp;
  x.forms = h->d_sp_forms.p; x.l = h->d_sp_l.p; x.lam = h->d_sp_lam.p; x.Weff = h->d_sp_weff.p;
  x.off_stride = J.off_stride;
  x.G = J.G; x.measure = J.measure; x.aggregate = J.aggregate; x.beta = J.beta;
}

// channels and signals (launch_signal without targets), the projections, the forms N, D of every group, the reduction (J into d_obj and, when
// given, J | l into pinned host memory); with G the effective row weights, the cotangent c on the signals and from it the cotangent of the sweep
int launch_spectrum(dfx_handle* h, double* G, double* host) {
  const dfx_handle::SpecJob& J = h->sp;
  const size_t B = h->pl.batch;
  if (int rc = launch_signal(h, nullptr, nullptr)) return rc;
  DevCtx c = make_ctx(h);
  const SigArgs a = sig_args(h);
  ProjArgs p;
  SpecArgs x;
  spectrum_args(h, p, x);
  const long long np = (long long)h->sig.n_sig * J.n_rows;
  hipLaunchKernelGGL(k_signal_project, dim3(chunks_of(np, kObjWaves), (unsigned)B), dim3(kObjThreads), 0, h->stream, c, a, p, (double*)nullptr);
  hipLaunchKernelGGL(k_signal_spectrum_forms, dim3(chunks_of(2LL * J.G, kObjWaves), (unsigned)B), dim3(kObjThreads), 0, h->stream, a, p, x);
  hipLaunchKernelGGL(k_signal_spectrum_reduce, dim3((unsigned)B), dim3(64), 0, h->stream, x, h->d_obj.p, host, (int)B);
  if (G) {
    hipLaunchKernelGGL(k_signal_spectrum_weights, dim3(chunks_of(np, kObjThreads), (unsigned)B), dim3(kObjThreads), 0, h->stream, a, p, x);
    hipLaunchKernelGGL(k_signal_spectrum_residual, dim3(chunks_of((long long)h->ts.size() * h->sig.n_sig, kObjThreads), (unsigned)B), dim3(kObjThreads), 0,
                       h->stream, c, a, p, x);
    launch_signal_reverse(h, c, a, G);
  }
  return 0;
}

// ---- what the entries share
// A value entry needs the fields of a forward pass (and, all but dfx_objective_value, its parameters) and somewhere to put its result
int need_fields(dfx_handle* h, const char* who, const void* out, const char* out_name, bool params = true) {
  if (!h->have_fields || (params && !h->have_params)) { h->err = std::string(who) + ": run forward first"; return 1; }
  if (!out) { h->err = std::string(who) + ": " + out_name + " is NULL"; return 1; }
  return 0;
}

// A gradient entry needs the kept trajectory of a forward pass whose checkpoint is still this handle's
int need_trajectory(dfx_handle* h, const char* who) {
  if (!h->have_traj || !h->have_fields) { h->err = std::string(who) + ": run forward with keep_trajectory=1 first"; return 1; }
  if (h->ck->writer != h) { h->err = std::string(who) + ": " + kStaleCheckpoint; return 1; }
  return 0;
}

// The end of a value entry: the results (dst null: not asked for) down, then the one wait of the call
struct Download { void* dst; const void* src; size_t bytes; };
int download(dfx_handle* h, std::initializer_list<Download> list) {
  for (const Download& d : list)
    if (d.dst) HIP_OK(hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  HIP_OK(hipGetLastError());
  return 0;
}

// How every gradient entry runs behind its own prepare_*: the buffers of the sweep, `job` behind it (launch_objective_explicit; centroids: the
// block-centroid accumulator exists for this call on every lattice), `launch(G, host)` for the value and the cotangent (host: stage_bytes of
// pinned memory the launch may fill, null when stage_bytes == 0; the caller reads h->obj_stage after a return of 0), then the sweep itself --
// want / views / device_views / stats, every sweep form and checkpoint level, the kept steps of an adaptive solve.
template <class Launch>
int objective_sweep(dfx_handle* h, const ObjJob& job, bool centroids, size_t stage_bytes, Launch&& launch, const dfx_grads* want, dfx_grads* views,
                    int32_t device_views, dfx_stats* stats) {
  const Plan& pl = h->pl;
  const size_t B = pl.batch, nb = pl.n_blocks, n_G = B * h->ts.size() * nb * 6;
  if (ensure_adjoint_buffers(h)) return 2;
  HIP_OK(h->d_G.ensure(n_G));
  // (on a lattice without distance contact the buffer stays on the handle afterwards: the stage kernels touch g_c with distance contact only,
  // and the other entries neither zero nor collect it)
  if (centroids) HIP_OK(h->d_g_c.ensure(B * nb * 2));
  if (stage_bytes) HIP_OK(h->obj_stage.ensure(stage_bytes));
  // what the sweep consults on the handle for this call (explicit terms behind it, the centroid accumulator, device views) is taken back on
  // EVERY way out of this function, a failed launch or allocation included: the next call on the handle must not inherit it
  struct Scope {
    dfx_handle* h;
    ~Scope() { h->obj_job = nullptr; h->obj_centroids = false; h->device_views = false; }
  } scope{h};
  h->obj_centroids = centroids;
  h->obj_job = &job;
  h->device_views = device_views != 0;
  set_grad_wishes(h, want);
  // one launch: accumulators and cotangents cleared, cursors at the last segment (as the kinetic entries)
  if (zero_grad_accumulators(h, h->d_G.p, n_G, (int)h->segs.size())) return 2;
  if (int rc = launch(h->d_G.p, stage_bytes ? reinterpret_cast<double*>(h->obj_stage.p) : nullptr)) return rc;
  return run_adjoint(h, want, nullptr, views, stats, false, 0, true);
}

// the job of a signal family behind the sweep (k_signal_explicit): the set of the term list in flight
ObjJob signal_job(const dfx_handle* h, int kind, bool has_tau) { return ObjJob{kind, h->sig.n_set, 0, 0, has_tau}; }

}  // namespace

void launch_objective_explicit(dfx_handle* h, const DevCtx& c) {
  const ObjJob& j = *h->obj_job;
  if (j.n_act == 0) return;
  if (j.kind == kObjSignal || j.kind == kObjProject || j.kind == kObjXcorr || j.kind == kObjSpectrum) {       // the same direction w, whichever residual it came from
    const SigArgs a = sig_args(h);
    const dim3 grid((unsigned)((a.n_set * 4 + 63) / 64), (unsigned)h->pl.batch);
    with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_signal_explicit<M(), C()>), grid, dim3(64), 0, h->stream, c, a); });
    return;
  }
  if (j.kind == kObjPeak) {
    const ObjArgs a = obj_args(h, j);
    const PeakArgs p = peak_args(h);
    const dim3 grid((unsigned)((j.n_act * 4 + 63) / 64), (unsigned)h->pl.batch);
    with_peak_physics(h, [&](auto M) { hipLaunchKernelGGL((k_strain_peak_explicit<M()>), grid, dim3(64), 0, h->stream, c, a, p); });
    return;
  }
  if (j.kind == kObjStrain) {
    const ObjArgs a = obj_args(h, j);
    const dim3 grid((unsigned)((j.n_act * 4 + 63) / 64), (unsigned)h->pl.batch);
    with_strain_physics(h, [&](auto M, auto C) { hipLaunchKernelGGL((k_strain_objective_explicit<M(), C()>), grid, dim3(64), 0, h->stream, c, a); });
    return;
  }
  const ObjArgs a = obj_args(h, j);
  const dim3 grid((unsigned)((j.n_act + 63) / 64), (unsigned)h->pl.batch);
  if (j.kind == DFX_OBJ_KINETIC) hipLaunchKernelGGL(k_objective_explicit<DFX_OBJ_KINETIC>, grid, dim3(64), 0, h->stream, c, a);
  else hipLaunchKernelGGL(k_objective_explicit<DFX_OBJ_ANGULAR_MOMENTUM>, grid, dim3(64), 0, h->stream, c, a);
}

int dfx_objective_value(dfx_handle* h, int32_t kind, const double* block_weights, int32_t weights_per_member, const double* time_weights,
                        const double* lever0, int32_t lever_per_member, double* objective) {
  const char* who = "objective_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective", false)) return rc;
  ObjHost oh;
  if (int rc = prepare_objective(h, who, kind, block_weights, weights_per_member, time_weights, lever0, lever_per_member, oh)) return rc;
  if (int rc = launch_objective(h, oh.job, nullptr, nullptr)) return rc;
  return download(h, {{objective, h->d_obj.p, sizeof(double) * h->pl.batch}});
}

int dfx_objective_value_and_grad(dfx_handle* h, int32_t kind, const double* block_weights, int32_t weights_per_member,
                                 const double* time_weights, const double* lever0, int32_t lever_per_member, double* objective,
                                 const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats) {
  const char* who = "objective_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  ObjHost oh;
  if (int rc = prepare_objective(h, who, kind, block_weights, weights_per_member, time_weights, lever0, lever_per_member, oh)) return rc;
  // the angular kind depends on the block centroids through its levers
  if (int rc = objective_sweep(h, oh.job, kind == DFX_OBJ_ANGULAR_MOMENTUM, objective ? sizeof(double) * B : 0,
                               [&](double* G, double* host) { return launch_objective(h, oh.job, G, host); }, want, views, device_views, stats))
    return rc;
  if (objective) memcpy(objective, h->obj_stage.p, sizeof(double) * B);
  return 0;
}

int dfx_strain_objective_value(dfx_handle* h, const double* bond_weights, int32_t weights_per_member, const double* time_weights,
                               const double* parts4, double* objective) {
  const char* who = "strain_objective_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  ObjHost oh;
  if (int rc = prepare_strain(h, who, bond_weights, weights_per_member, time_weights, parts4, oh)) return rc;
  if (int rc = launch_strain(h, oh.job, nullptr, nullptr)) return rc;
  return download(h, {{objective, h->d_obj.p, sizeof(double) * h->pl.batch}});
}

int dfx_strain_objective_value_and_grad(dfx_handle* h, const double* bond_weights, int32_t weights_per_member, const double* time_weights,
                                        const double* parts4, double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views,
                                        dfx_stats* stats) {
  const char* who = "strain_objective_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  ObjHost oh;
  if (int rc = prepare_strain(h, who, bond_weights, weights_per_member, time_weights, parts4, oh)) return rc;
  if (int rc = objective_sweep(h, oh.job, false, objective ? sizeof(double) * B : 0,
                               [&](double* G, double* host) { return launch_strain(h, oh.job, G, host); }, want, views, device_views, stats))
    return rc;
  if (objective) memcpy(objective, h->obj_stage.p, sizeof(double) * B);
  return 0;
}

int dfx_strain_peak_value(dfx_handle* h, const double* bond_coef, int32_t coef_per_member, const double* bond_weights,
                          int32_t weights_per_member, const double* time_weights, int32_t aggregate, double sharpness, double* objective,
                          double* peak, int32_t* peak_at) {
  const char* who = "strain_peak_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  ObjHost oh;
  if (int rc = prepare_peak(h, who, bond_coef, coef_per_member, bond_weights, weights_per_member, time_weights, aggregate, sharpness, oh)) return rc;
  if (int rc = launch_peak(h, oh.job, nullptr, nullptr)) return rc;
  const size_t B = h->pl.batch;
  std::vector<double> res(B * 4);
  if (int rc = download(h, {{res.data(), h->d_pk_res.p, sizeof(double) * B * 4}, {peak_at, h->d_pk_at.p, sizeof(int32_t) * B * 2}})) return rc;
  for (size_t m = 0; m < B; ++m) {
    objective[m] = res[m * 4 + 2];
    if (peak) peak[m] = res[m * 4];
  }
  return 0;
}

int dfx_strain_peak_value_and_grad(dfx_handle* h, const double* bond_coef, int32_t coef_per_member, const double* bond_weights,
                                   int32_t weights_per_member, const double* time_weights, int32_t aggregate, double sharpness,
                                   double* objective, double* peak, int32_t* peak_at, const dfx_grads* want, dfx_grads* views,
                                   int32_t device_views, dfx_stats* stats) {
  const char* who = "strain_peak_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  ObjHost oh;
  if (int rc = prepare_peak(h, who, bond_coef, coef_per_member, bond_weights, weights_per_member, time_weights, aggregate, sharpness, oh)) return rc;
  const bool any = objective || peak || peak_at;
  if (int rc = objective_sweep(h, oh.job, false, any ? (sizeof(double) + sizeof(int32_t)) * 2 * B : 0,
                               [&](double* G, double* host) { return launch_peak(h, oh.job, G, host); }, want, views, device_views, stats))
    return rc;
  const double* st = reinterpret_cast<const double*>(h->obj_stage.p);      // J | q_hat | (k_hat, b_hat) as int32
  if (objective) memcpy(objective, st, sizeof(double) * B);
  if (peak) memcpy(peak, st + B, sizeof(double) * B);
  if (peak_at) memcpy(peak_at, st + 2 * B, sizeof(int32_t) * 2 * B);
  return 0;
}

int dfx_signal_hinge_channels(dfx_handle* h, int32_t enable) {
  h->sig_hinges = enable != 0;
  return 0;
}

int dfx_signal_values(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                      const double* term_coef, int32_t n_signals, double* values) {
  const char* who = "signal_values";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, values, "values")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_signal(h, who, t, nullptr, 0, nullptr, nullptr, false)) return rc;
  if (int rc = launch_signal(h, nullptr, nullptr)) return rc;
  return download(h, {{values, h->d_sig_S.p, sizeof(double) * h->pl.batch * h->ts.size() * (size_t)n_signals}});
}

int dfx_signal_misfit_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                            const double* term_coef, int32_t n_signals, const double* targets, int32_t targets_per_member,
                            const double* signal_weights, const double* time_weights, double* objective) {
  const char* who = "signal_misfit_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_signal(h, who, t, targets, targets_per_member, signal_weights, time_weights, true)) return rc;
  if (int rc = launch_signal(h, nullptr, nullptr)) return rc;
  return download(h, {{objective, h->d_obj.p, sizeof(double) * h->pl.batch}});
}

int dfx_signal_misfit_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                     const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* targets,
                                     int32_t targets_per_member, const double* signal_weights, const double* time_weights, double* objective,
                                     const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats) {
  const char* who = "signal_misfit_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_signal(h, who, t, targets, targets_per_member, signal_weights, time_weights, true)) return rc;
  if (int rc = objective_sweep(h, signal_job(h, kObjSignal, h->sig.has_tau), false, objective ? sizeof(double) * B : 0,
                               [&](double* G, double* host) { return launch_signal(h, G, host); }, want, views, device_views, stats))
    return rc;
  if (objective) memcpy(objective, h->obj_stage.p, sizeof(double) * B);
  return 0;
}

int dfx_signal_projections(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                           const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows, double* values) {
  const char* who = "signal_projections";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, values, "values")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_projection(h, who, t, basis, n_rows, nullptr, nullptr, 0, false)) return rc;
  if (int rc = launch_projection(h, nullptr, nullptr)) return rc;
  return download(h, {{values, h->d_proj_P.p, sizeof(double) * h->pl.batch * (size_t)n_signals * (size_t)n_rows}});
}

int dfx_signal_projection_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows,
                                const double* row_weights, const double* targets, int32_t targets_per_member, double* objective) {
  const char* who = "signal_projection_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_projection(h, who, t, basis, n_rows, row_weights, targets, targets_per_member, true)) return rc;
  if (int rc = launch_projection(h, nullptr, nullptr)) return rc;
  return download(h, {{objective, h->d_obj.p, sizeof(double) * h->pl.batch}});
}

int dfx_signal_projection_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                         const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis,
                                         int32_t n_rows, const double* row_weights, const double* targets, int32_t targets_per_member,
                                         double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats) {
  const char* who = "signal_projection_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  if (int rc = prepare_projection(h, who, t, basis, n_rows, row_weights, targets, targets_per_member, true)) return rc;
  if (int rc = objective_sweep(h, signal_job(h, kObjProject, false), false, objective ? sizeof(double) * B : 0,
                               [&](double* G, double* host) { return launch_projection(h, G, host); }, want, views, device_views, stats))
    return rc;
  if (objective) memcpy(objective, h->obj_stage.p, sizeof(double) * B);
  return 0;
}

int dfx_signal_xcorr(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                     const double* term_coef, int32_t n_signals, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b,
                     const double* templates, int32_t n_templates, int32_t templates_per_member, int32_t max_lag, int32_t normalisation,
                     double* values) {
  const char* who = "signal_xcorr";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, values, "values")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const XcorrCall q{n_pairs, pair_a, pair_b, templates, n_templates, templates_per_member, max_lag, normalisation, false, 0, 0, 1.0, 1.0, 0.0, 0.0};
  if (int rc = prepare_xcorr(h, who, t, q)) return rc;
  if (int rc = launch_xcorr(h, nullptr, nullptr)) return rc;
  return download(h, {{values, xcorr_args(h).rho, sizeof(double) * h->pl.batch * (2 * (size_t)max_lag + 1)}});
}

int dfx_signal_xcorr_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                           const int32_t* term_component, const double* term_coef, int32_t n_signals, int32_t n_pairs, const int32_t* pair_a,
                           const int32_t* pair_b, const double* templates, int32_t n_templates, int32_t templates_per_member, int32_t max_lag,
                           int32_t normalisation, int32_t reduce, int32_t lag0, double beta, double w_peak, double w_delay,
                           double delay_target, double* objective, double* peak, double* delay) {
  const char* who = "signal_xcorr_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const XcorrCall q{n_pairs, pair_a, pair_b, templates, n_templates, templates_per_member, max_lag, normalisation, true, reduce, lag0, beta, w_peak,
                    w_delay, delay_target};
  if (int rc = prepare_xcorr(h, who, t, q)) return rc;
  if (int rc = launch_xcorr(h, nullptr, nullptr)) return rc;
  const size_t bytes = sizeof(double) * h->pl.batch;
  const XcorrArgs x = xcorr_args(h);
  return download(h, {{objective, h->d_obj.p, bytes}, {peak, x.peak, bytes}, {delay, x.delay, bytes}});
}

int dfx_signal_xcorr_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                    const int32_t* term_component, const double* term_coef, int32_t n_signals, int32_t n_pairs,
                                    const int32_t* pair_a, const int32_t* pair_b, const double* templates, int32_t n_templates,
                                    int32_t templates_per_member, int32_t max_lag, int32_t normalisation, int32_t reduce, int32_t lag0,
                                    double beta, double w_peak, double w_delay, double delay_target, double* objective, double* peak,
                                    double* delay, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats) {
  const char* who = "signal_xcorr_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const XcorrCall q{n_pairs, pair_a, pair_b, templates, n_templates, templates_per_member, max_lag, normalisation, true, reduce, lag0, beta, w_peak,
                    w_delay, delay_target};
  if (int rc = prepare_xcorr(h, who, t, q)) return rc;
  const bool any = objective || peak || delay;
  if (int rc = objective_sweep(h, signal_job(h, kObjXcorr, false), false, any ? sizeof(double) * 3 * B : 0,
                               [&](double* G, double* host) { return launch_xcorr(h, G, host); }, want, views, device_views, stats))
    return rc;
  const double* st = reinterpret_cast<const double*>(h->obj_stage.p);      // J | M | delta
  if (objective) memcpy(objective, st, sizeof(double) * B);
  if (peak) memcpy(peak, st + B, sizeof(double) * B);
  if (delay) memcpy(delay, st + 2 * B, sizeof(double) * B);
  return 0;
}

int dfx_signal_spectrum(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                        const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows, int32_t n_groups,
                        const double* num_weights, const double* den_weights, const double* num_offset, const double* den_offset,
                        int32_t offsets_per_member, int32_t measure, double* values) {
  const char* who = "signal_spectrum";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, values, "values")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const SpectrumCall q{basis, n_rows, n_groups, num_weights, den_weights, num_offset, den_offset, offsets_per_member, false, measure, DFX_SPECTRUM_SUM, 1.0, nullptr};
  if (int rc = prepare_spectrum(h, who, t, q)) return rc;
  if (int rc = launch_spectrum(h, nullptr, nullptr)) return rc;
  const size_t n = h->pl.batch * (size_t)n_groups;
  std::vector<double> forms(n * 2), l(n);
  if (int rc = download(h, {{forms.data(), h->d_sp_forms.p, sizeof(double) * n * 2}, {l.data(), h->d_sp_l.p, sizeof(double) * n}})) return rc;
  for (size_t i = 0; i < n; ++i) { values[i * 3] = forms[i * 2]; values[i * 3 + 1] = forms[i * 2 + 1]; values[i * 3 + 2] = l[i]; }
  return 0;
}

int dfx_signal_spectrum_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                              const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows,
                              int32_t n_groups, const double* num_weights, const double* den_weights, const double* num_offset,
                              const double* den_offset, int32_t offsets_per_member, int32_t measure, int32_t aggregate, double beta,
                              const double* group_coef, double* objective, double* measures) {
  const char* who = "signal_spectrum_value";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_fields(h, who, objective, "objective")) return rc;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const SpectrumCall q{basis, n_rows, n_groups, num_weights, den_weights, num_offset, den_offset, offsets_per_member, true, measure, aggregate, beta,
                       group_coef};
  if (int rc = prepare_spectrum(h, who, t, q)) return rc;
  if (int rc = launch_spectrum(h, nullptr, nullptr)) return rc;
  const size_t B = h->pl.batch;
  return download(h, {{objective, h->d_obj.p, sizeof(double) * B}, {measures, h->d_sp_l.p, sizeof(double) * B * (size_t)n_groups}});
}

int dfx_signal_spectrum_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                       const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis,
                                       int32_t n_rows, int32_t n_groups, const double* num_weights, const double* den_weights,
                                       const double* num_offset, const double* den_offset, int32_t offsets_per_member, int32_t measure,
                                       int32_t aggregate, double beta, const double* group_coef, double* objective, double* measures,
                                       const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats) {
  const char* who = "signal_spectrum_value_and_grad";
  HIP_OK(hipSetDevice(h->device));
  if (int rc = need_trajectory(h, who)) return rc;
  const size_t B = h->pl.batch;
  const SigTerms t{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  const SpectrumCall q{basis, n_rows, n_groups, num_weights, den_weights, num_offset, den_offset, offsets_per_member, true, measure, aggregate, beta,
                       group_coef};
  if (int rc = prepare_spectrum(h, who, t, q)) return rc;
  const bool any = objective || measures;
  if (int rc = objective_sweep(h, signal_job(h, kObjSpectrum, false), false, any ? sizeof(double) * B * (1 + (size_t)n_groups) : 0,
                               [&](double* G, double* host) { return launch_spectrum(h, G, host); }, want, views, device_views, stats))
    return rc;
  const double* st = reinterpret_cast<const double*>(h->obj_stage.p);      // J | l
  if (objective) memcpy(objective, st, sizeof(double) * B);
  if (measures) memcpy(measures, st + B, sizeof(double) * B * (size_t)n_groups);
  return 0;
}
