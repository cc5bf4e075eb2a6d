// engine_tangent.hip -- forward mode (kernels in dfx_tangent.h): dfx_forward_tangent[_multi], the derivative of the fixed-grid solve along
// K directions per member, dfx_forward_tangent_dense[_multi], the derivative of the adaptive solve's dense output on every member's own
// frozen accepted steps, and dfx_rhs_jvp, one right-hand-side evaluation with K tangents (the forward-mode twin of dfx_rhs_vjp).
//
// One stage launch per Runge-Kutta stage on the handle's stream, one lane per (member, block), primal evaluated once.  The K directions
// are served in passes of a compile-time chunk width (kWidths; the tail takes the narrowest shipped width that holds it, its spare
// directions zero); fields comes from the first pass.  The buffers are the call's own and are sized for ONE pass, so the device footprint
// does not grow with K, and the trajectory checkpoint and the resident history of the last dfx_forward are left as they were (a later
// dfx_adjoint still reverses that solve).  Host side: the parameter image of the tangent kernels (plain per-slot layout, value and
// tangents) is built from the packed primal image dfx_set_params left on the handle and from params_dots.
//
// Small problems take the other form (plan_passes): where batch x blocks x K lanes do not even give every SIMD of the chip one wave, a stage
// is bound by the latency of one lane's instruction stream, and the K-wide lane is the longer stream -- there the directions are spread
// over lanes instead, one slice of width 1 per direction along grid.y in ONE pass (the replicated-members form, measured the cheaper one on
// the paper lattice: profiles/r09_tangent_multi.txt).  DFX_TANGENT_MULTI_FORM=chunked|spread forces either form (tests, measurements).
//
// dfx_forward_tangent and dfx_forward_tangent_dense are the _multi entries with n_dirs = 1 -- (batch, 1, ...) is (batch, ...) -- under
// their own names in h->err.  One direction is one pass of width 1 with one slice in BOTH forms, so DFX_TANGENT_MULTI_FORM cannot change
// a single-direction call.
//
// dfx_forward_tangent_signals_multi / _dense_multi are the same two solves with another end of a pass (SignalSink): instead of the download
// of fields / fields_dot, the force channels and their tangents, the signals and their tangents and a finiteness flag per workgroup are
// formed on the pass's own buffers (k_tan_signal_channels, k_tan_signal_combine, k_tan_finite_flags) and (batch, KT, T, n_signals) comes
// back -- the columns of a least-squares Jacobian without the history crossing PCIe.
#include "dfx_engine.h"
#include "dfx_tangent.h"

using namespace dfx;

namespace {

// the shipped chunk widths, widest first (profiles/r09_tangent_multi.txt: the widest whose ligament + contact evaluation has no scratch traffic)
constexpr int kWidths[] = {4, 2, 1};
static_assert(kWidths[0] == kTanMaxWidth, "kTanMaxWidth");

struct MultiBufs {
  DevBuf<double> tp, blk, mem, cen, tgrid, t0, s0, s0d, Y[2], DY[2], S[2], DS[2], A, DA, fields, fields_dot;
  ~MultiBufs() {
    DevBuf<double>* all[] = {&tp, &blk, &mem, &cen, &tgrid, &t0, &s0, &s0d, &Y[0], &Y[1], &DY[0], &DY[1], &S[0], &S[1], &DS[0], &DS[1],
                             &A, &DA, &fields, &fields_dot};
    for (auto* b : all) b->release();
  }
};

struct MultiKernels {
  void (*stage)(dim3, hipStream_t, const TanCtx&, const Tableau&, const TanStageM&);
  void (*init)(dim3, hipStream_t, const TanCtx&, const double*, const double*, double*, double*, const TanSlices&);
  void (*snapshot)(dim3, hipStream_t, int, int, int, int, const double*, const double*, const TanSlices&, double*, double*);
  void (*dense)(dim3, hipStream_t, const TanCtx&, const TanDenseM&);
  void (*rhs_out)(dim3, hipStream_t, const TanCtx&, const MultiBufs&, const TanSlices&);
};

template <int MODEL, int CONTACT, int NPB, int KC>
void launch_stage(dim3 grid, hipStream_t s, const TanCtx& c, const Tableau& T, const TanStageM& st) {
  hipLaunchKernelGGL((k_tan_stage_multi<MODEL, CONTACT, NPB, KC>), grid, dim3(256), 0, s, c, T, st);
}
template <int KC>
void launch_init(dim3 grid, hipStream_t s, const TanCtx& c, const double* s0, const double* s0d, double* S, double* D, const TanSlices& sl) {
  hipLaunchKernelGGL(k_tan_init_multi<KC>, grid, dim3(256), 0, s, c, s0, s0d, S, D, sl);
}
template <int KC>
void launch_snapshot(dim3 grid, hipStream_t s, int B, int nb, int Tn, int j, const double* S, const double* D, const TanSlices& sl, double* f, double* fd) {
  hipLaunchKernelGGL(k_tan_snapshot_multi<KC>, grid, dim3(256), 0, s, B, nb, Tn, j, S, D, sl, f, fd);
}
template <int KC>
void launch_dense(dim3 grid, hipStream_t s, const TanCtx& c, const TanDenseM& dn) {
  hipLaunchKernelGGL(k_tan_dense_multi<KC>, grid, dim3(256), 0, s, c, dn);
}
template <int KC>
void launch_rhs_out(dim3 grid, hipStream_t s, const TanCtx& c, const MultiBufs& d, const TanSlices& sl) {
  hipLaunchKernelGGL(k_tan_rhs_out_multi<KC>, grid, dim3(256), 0, s, c, (const double*)d.Y[0].p, (const double*)d.DY[0].p, (const double*)d.A.p,
                     (const double*)d.DA.p, sl, d.fields.p, d.fields_dot.p);
}

template <int KC>
MultiKernels pick_physics(int model, int contact, int npb) {
  MultiKernels k = {};
  with_physics<all_physics>(model, contact, [&](auto M, auto C) {
    k = {npb == 3 ? launch_stage<M(), C(), 3, KC> : launch_stage<M(), C(), 4, KC>, launch_init<KC>, launch_snapshot<KC>, launch_dense<KC>, launch_rhs_out<KC>};
  });
  return k;
}
MultiKernels pick_kernels(int model, int contact, int npb, int kc) {
  switch (kc) {
    case 4: return pick_physics<4>(model, contact, npb);
    case 2: return pick_physics<2>(model, contact, npb);
    default: return pick_physics<1>(model, contact, npb);
  }
}

struct Pass {
  int k0, n, kc, slices;              // directions [k0, k0 + n) in `slices` chunks of width kc, slices * kc >= n
  int kt() const { return kc * slices; }
};

// lanes that give every SIMD of the chip one wave (256 CUs x 4 SIMDs x 64 lanes): below it a stage is latency-bound
constexpr long long kFillLanes = 256LL * 4 * 64;

std::vector<Pass> plan_passes(int K, long long units) {
  std::vector<Pass> out;
  const char* form = getenv("DFX_TANGENT_MULTI_FORM");
  const bool spread = form && !strcmp(form, "spread") ? true : form && !strcmp(form, "chunked") ? false : units * K <= kFillLanes;
  if (spread) { out.push_back({0, K, 1, K}); return out; }
  int k0 = 0;
  while (k0 < K) {
    const int rem = K - k0;
    int kc = kWidths[0];
    for (int w : kWidths) if (w >= rem) kc = w;        // the narrowest shipped width that holds the tail
    const int n = std::min(rem, kc);
    out.push_back({k0, n, kc, 1});
    k0 += n;
  }
  return out;
}

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

// The parameter image of one pass (layouts: dfx_tangent.h): primal values from the packed image, tangents of directions
// [p.k0, p.k0 + p.n) from params_dots (NULL array: zero tangent); the spare directions of the chunk stay zero.
struct MultiImage { std::vector<double> tp, blk, mem, cen; };

void multi_image(const dfx_handle* h, const dfx_params* params_dots, const Pass& p, MultiImage& img);

// the images of all slices of a pass, one after the other
void pass_image(const dfx_handle* h, const dfx_params* params_dots, const Pass& p, MultiImage& img) {
  if (p.slices == 1) { multi_image(h, params_dots, p, img); return; }
  img.tp.clear(); img.blk.clear(); img.mem.clear(); img.cen.clear();
  for (int j = 0; j < p.slices; ++j) {
    MultiImage one;
    const int k0 = p.k0 + j * p.kc;
    multi_image(h, params_dots, Pass{k0, std::max(0, std::min(p.kc, p.k0 + p.n - k0)), p.kc, 1}, one);
    img.tp.insert(img.tp.end(), one.tp.begin(), one.tp.end()); img.blk.insert(img.blk.end(), one.blk.begin(), one.blk.end());
    img.mem.insert(img.mem.end(), one.mem.begin(), one.mem.end()); img.cen.insert(img.cen.end(), one.cen.begin(), one.cen.end());
  }
}

void multi_image(const dfx_handle* h, const dfx_params* params_dots, const Pass& p, MultiImage& img) {
  const Plan& pl = h->pl;
  const PackedParams& pp = h->pp;
  const int B = pl.batch, nb = pl.n_blocks, NS = pl.n_slots, npb = pl.n_npb, kc = p.kc;
  const int SN = tan_slot_n(kc), BN = tan_blk_n(kc), MN = tan_mem_n(kc), CN = tan_cen_n(kc);
  std::vector<double>&tp = img.tp, &blk = img.blk, &mem = img.mem, &cen = img.cen;
  tp.assign((size_t)B * NS * SN, 0.0); blk.assign((size_t)B * nb * BN, 0.0); mem.assign((size_t)B * MN, 0.0);
  cen.clear();
  const bool dist = pl.contact == DFX_CONTACT_DISTANCE;
  if (dist) cen.assign((size_t)B * nb * CN, 0.0);
  dfx_params zero_dot;
  memset(&zero_dot, 0, sizeof(zero_dot));
  for (int m = 0; m < B; ++m) {
    for (int s = 0; s < NS; ++s) {
      double* o = tp.data() + ((size_t)m * NS + s) * SN;
      const size_t ms = (size_t)m * NS + s;
      const int b = s / kSlots, k = s % kSlots;
      if (k >= npb) continue;
      o[0] = pp.p_r[ms * 2]; o[1] = pp.p_r[ms * 2 + 1];
      for (int j = 0; j < p.n; ++j) {
        const dfx_params& q = params_dots ? params_dots[p.k0 + j] : zero_dot;
        if (!q.centroid_node_vectors) continue;
        const double* r = q.centroid_node_vectors + (((size_t)m * nb + b) * npb + k) * 2;
        o[kTanSlotVals * (1 + j)] = r[0]; o[kTanSlotVals * (1 + j) + 1] = r[1];
      }
      const int bond = pl.slot_bond[s];
      if (pl.slot_info[s] < 0 || bond < 0) continue;
      if (pp.l_dict_ok) {
        const double* d = pp.l_dict.data() + (size_t)m * 1024 + 4 * pp.l_idx[ms];
        o[2] = d[0]; o[3] = d[1];
      } else { o[2] = pp.p_l[ms * 2]; o[3] = pp.p_l[ms * 2 + 1]; }
      for (int j = 0; j < 3; ++j) o[4 + j] = pp.k_uniform ? pp.cst[(size_t)m * 16 + 3 + j] : pp.p_k[ms * 4 + j];
      o[7] = pp.p_phi[ms * 2]; o[8] = pp.p_phi[ms * 2 + 1];
      const size_t mb = (size_t)m * pl.n_bonds + bond;
      for (int j = 0; j < p.n; ++j) {
        const dfx_params& q = params_dots ? params_dots[p.k0 + j] : zero_dot;
        double* t = o + kTanSlotVals * (1 + j);
        if (q.reference_vector) { t[2] = q.reference_vector[mb * 2]; t[3] = q.reference_vector[mb * 2 + 1]; }
        if (q.k_bond) for (int i = 0; i < 3; ++i) t[4 + i] = q.k_bond[mb * 3 + i];
        if (q.void_angle0 && pl.contact == DFX_CONTACT_ANGLE) { t[7] = q.void_angle0[mb * 2]; t[8] = q.void_angle0[mb * 2 + 1]; }
      }
    }
    for (int b = 0; b < nb; ++b) {
      double* o = blk.data() + ((size_t)m * nb + b) * BN;
      const size_t mb = (size_t)m * nb + b;
      for (int d = 0; d < 3; ++d) {
        const size_t i = mb * 3 + d;
        const double im = pp.inv_m[i];
        o[d] = im;
        o[3 + d] = pp.damping[i];
        for (int j = 0; j < p.n; ++j) {
          const dfx_params& q = params_dots ? params_dots[p.k0 + j] : zero_dot;
          double* t = o + kTanBlkVals * (1 + j);
          t[d] = q.inertia ? -q.inertia[i] * im * im : 0.0;        // d(1/m) = -dm / m^2
          t[3 + d] = q.damping ? q.damping[i] : 0.0;
        }
      }
      if (dist) {
        double* c = cen.data() + mb * CN;
        c[0] = pp.centroid[mb * 2]; c[1] = pp.centroid[mb * 2 + 1];
        for (int j = 0; j < p.n; ++j) {
          const dfx_params& q = params_dots ? params_dots[p.k0 + j] : zero_dot;
          if (q.block_centroids) { c[2 + 2 * j] = q.block_centroids[mb * 2]; c[3 + 2 * j] = q.block_centroids[mb * 2 + 1]; }
        }
      }
    }
    double* o = mem.data() + (size_t)m * MN;
    for (int j = 0; j < 3; ++j) o[j] = pp.contact[(size_t)m * 3 + j];
    for (int j = 0; j < p.n; ++j) {
      const dfx_params& q = params_dots ? params_dots[p.k0 + j] : zero_dot;
      double* t = o + 3 + kTanMemDir * j;
      for (int i = 0; i < 3; ++i) t[i] = (q.contact && pl.contact) ? q.contact[(size_t)m * 3 + i] : 0.0;
      if (q.fn_params)
        for (int f = 0; f < pl.n_fns; ++f)
          for (int i = 0; i < DFX_FN_PARAMS; ++i) t[3 + f * DFX_FN_PARAMS + i] = q.fn_params[((size_t)m * pl.n_fns + f) * DFX_FN_PARAMS + i];
    }
  }
}

int fail(dfx_handle* h, const char* who, const std::string& what, int rc = 1);

// What a call needs on the device, sized for its widest pass: the image, the time grid, the initial state, the work buffers.  Everything is
// allocated here, before any pass is paid for; a failure releases all of it (MultiBufs) and is an ordinary error return.
int multi_alloc(dfx_handle* h, const Pass& widest, const std::vector<double>& tgrid, const std::vector<double>& t0, const double* state0, bool have_s0d,
                int a_rows, int Tn, MultiBufs& d, TanCtx& c) {
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks, NS = pl.n_slots;
  const bool dist = pl.contact == DFX_CONTACT_DISTANCE;
  const size_t rec = (size_t)B * nb * kRec, nfield = (size_t)B * Tn * nb * 6, nstate = (size_t)B * nb * 6;
  const size_t kc_max = widest.kt(), ns = widest.slices;      // (later passes are no wider and hold one slice)
  HIP_OK(d.tp.ensure(ns * B * NS * tan_slot_n(widest.kc))); HIP_OK(d.blk.ensure(ns * B * nb * tan_blk_n(widest.kc)));
  HIP_OK(d.mem.ensure(ns * B * tan_mem_n(widest.kc)));
  if (dist) HIP_OK(d.cen.ensure(ns * B * nb * tan_cen_n(widest.kc)));
  HIP_OK(d.tgrid.ensure(tgrid.size())); HIP_OK(d.t0.ensure(t0.size()));
  for (int j = 0; j < 2; ++j) {
    HIP_OK(d.Y[j].ensure(rec)); HIP_OK(d.S[j].ensure(rec));
    HIP_OK(d.DY[j].ensure(rec * kc_max)); HIP_OK(d.DS[j].ensure(rec * kc_max));
  }
  HIP_OK(d.A.ensure((size_t)B * a_rows * nb * 3)); HIP_OK(d.DA.ensure((size_t)B * a_rows * nb * 3 * kc_max));
  HIP_OK(d.fields.ensure(nfield)); HIP_OK(d.fields_dot.ensure(nfield * kc_max));
  if (state0) HIP_OK(d.s0.ensure(nstate));
  if (have_s0d) HIP_OK(d.s0d.ensure(nstate * kc_max));
  hipStream_t st = h->stream;
  HIP_OK(hipMemcpyAsync(d.tgrid.p, tgrid.data(), sizeof(double) * tgrid.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.t0.p, t0.data(), sizeof(double) * t0.size(), hipMemcpyHostToDevice, st));
  if (state0) HIP_OK(hipMemcpyAsync(d.s0.p, state0, sizeof(double) * nstate, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));
  c.B = B; c.nb = nb; c.n_fns = pl.n_fns; c.n_stages = pl.tab.s;
  c.slot_info = h->d_slot_info.p; c.block_special = h->d_block_special.p; c.special = h->d_special.p; c.fns = h->d_fns.p;
  c.tp = d.tp.p; c.blk = d.blk.p; c.mem = d.mem.p; c.cen = dist ? d.cen.p : nullptr;
  c.tgrid = d.tgrid.p; c.t0 = d.t0.p;
  c.grid_stride = 0; c.t0_stride = 0;
  c.a_rows = a_rows; c.n_steps = nullptr;
  for (int f = 0; f < DFX_MAX_FNS; ++f) c.tabdot[f] = nullptr;
  c.tab_k0 = 0; c.tab_dirs = 0;
  return 0;
}

// the sample tangents of table drives the handle holds (dfx_fn_table_tangents) for a call of n_dirs directions
int table_tangents(dfx_handle* h, const char* who, int n_dirs, TanCtx& c) {
  for (int f = 0; f < h->pl.n_fns; ++f) {
    if (!h->tab_dots_n[f]) continue;
    if (h->tab_dots_n[f] != n_dirs)
      return fail(h, who, "the sample tangents of table function " + std::to_string(f) + " were set for " + std::to_string(h->tab_dots_n[f]) +
                              " directions, this call has " + std::to_string(n_dirs) + " (dfx_fn_table_tangents)");
    c.tabdot[f] = h->d_tab_dots[f].p;
    c.tab_dirs = n_dirs;
  }
  return 0;
}

// the image and the initial tangents of one pass: state0_dots (batch, n_dirs, 2, nb, 3) -> (kc, batch, 2, nb, 3), spare directions zero
int multi_upload_pass(dfx_handle* h, const dfx_params* params_dots, const double* state0_dots, int n_dirs, const Pass& p, MultiBufs& d) {
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks;
  MultiImage img;
  pass_image(h, params_dots, p, img);
  hipStream_t st = h->stream;
  HIP_OK(hipMemcpyAsync(d.tp.p, img.tp.data(), sizeof(double) * img.tp.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.blk.p, img.blk.data(), sizeof(double) * img.blk.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.mem.p, img.mem.data(), sizeof(double) * img.mem.size(), hipMemcpyHostToDevice, st));
  if (!img.cen.empty()) HIP_OK(hipMemcpyAsync(d.cen.p, img.cen.data(), sizeof(double) * img.cen.size(), hipMemcpyHostToDevice, st));
  std::vector<double> s0d;
  if (state0_dots) {
    const size_t ns = (size_t)nb * 6;
    s0d.assign((size_t)p.kt() * B * ns, 0.0);
    for (int j = 0; j < p.n; ++j)
      for (int m = 0; m < B; ++m)
        memcpy(s0d.data() + ((size_t)j * B + m) * ns, state0_dots + ((size_t)m * n_dirs + p.k0 + j) * ns, sizeof(double) * ns);
    HIP_OK(hipMemcpyAsync(d.s0d.p, s0d.data(), sizeof(double) * s0d.size(), hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipStreamSynchronize(st));      // (the image and s0d are this function's own)
  return 0;
}

// fields (first pass) and the pass's columns of fields_dots (batch, n_dirs, T, 2, nb, 3) back to the caller; 3 when something is not finite
int multi_download_pass(dfx_handle* h, const Pass& p, int n_dirs, int Tn, MultiBufs& d, double* fields, double* fields_dots, const char* who) {
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks;
  const size_t nrow = (size_t)Tn * nb * 6, nfield = (size_t)B * nrow;
  hipStream_t st = h->stream;
  std::vector<double> f_host(p.k0 == 0 ? nfield : 0), fd_host(nfield * p.kt());
  if (p.k0 == 0) HIP_OK(hipMemcpyAsync(f_host.data(), d.fields.p, sizeof(double) * nfield, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(fd_host.data(), d.fields_dot.p, sizeof(double) * fd_host.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (p.k0 == 0 && fields) memcpy(fields, f_host.data(), sizeof(double) * nfield);
  bool finite = all_finite(f_host.data(), f_host.size());
  for (int m = 0; m < B; ++m)
    for (int j = 0; j < p.n; ++j) {
      const double* src = fd_host.data() + ((size_t)m * p.kt() + j) * nrow;
      finite = finite && all_finite(src, nrow);
      if (fields_dots) memcpy(fields_dots + ((size_t)m * n_dirs + p.k0 + j) * nrow, src, sizeof(double) * nrow);
    }
  if (!finite) { h->err = std::string(who) + ": non-finite state or tangent"; return 3; }
  return 0;
}

// ---- the signal sink: what a pass of dfx_forward_tangent_signals[_dense]_multi ends in instead of multi_download_pass ---------------------
constexpr int kFlagGroups = 1024;          // workgroups of k_tan_finite_flags at the most (each strides over the rest)

struct SignalSink {
  SigTerms terms;
  double *signals, *signals_dots;          // the caller's (batch, T, n_signals) and (batch, n_dirs, T, n_signals)
  SigTables tb;
  DevBuf<double> chan, chan_dot, S, S_dot, coef;
  DevBuf<int32_t> tab, flags;
  ~SignalSink() {
    chan.release(); chan_dot.release(); S.release(); S_dot.release(); coef.release(); tab.release(); flags.release();
  }
};

unsigned chunks_of(long long items, int per) { return (unsigned)std::max<long long>(1, (items + per - 1) / per); }

// the channel launches of one pass: the force blocks on quads, then the listed hinges one lane each (either may be absent); returns how many
template <int MODEL, int CONTACT, int KC>
int launch_sig_channels(unsigned members, unsigned slices, hipStream_t s, const TanCtx& c, const TanSlices& sl, const TanSigArgs& a) {
  if (a.n_fb)
    hipLaunchKernelGGL((k_tan_signal_channels<MODEL, CONTACT, KC>), dim3(chunks_of((long long)a.Tn * a.n_fb, kTanSigQuads), members, slices), dim3(kTanSigThreads),
                       0, s, c, sl, a);
  if (a.n_hg)
    hipLaunchKernelGGL((k_tan_hinge_channels<MODEL, CONTACT, KC>), dim3(chunks_of((long long)a.Tn * a.n_hg, kTanHingeThreads), members, slices),
                       dim3(kTanHingeThreads), 0, s, c, sl, a);
  return (a.n_fb != 0) + (a.n_hg != 0);
}
using SigChannelsFn = int (*)(unsigned, unsigned, hipStream_t, const TanCtx&, const TanSlices&, const TanSigArgs&);
template <int KC>
SigChannelsFn pick_sig_physics(int model, bool angle) {
  SigChannelsFn f = nullptr;
  with_physics<all_physics>(model, angle ? 1 : 0, [&](auto M, auto C) { if constexpr (C() != DFX_CONTACT_DISTANCE) f = launch_sig_channels<M(), C(), KC>; });
  return f;
}
// the build for the handle's bond model and the pass's width; the angle contact only where the lattice has it (force terms with the
// distance-based contact are refused, so that lattice never gets here with a force block)
SigChannelsFn pick_sig_channels(const Plan& pl, int kc) {
  const bool angle = pl.contact == DFX_CONTACT_ANGLE;
  switch (kc) {
    case 4: return pick_sig_physics<4>(pl.model, angle);
    case 2: return pick_sig_physics<2>(pl.model, angle);
    default: return pick_sig_physics<1>(pl.model, angle);
  }
}

// The sink's device side, sized for the widest pass and allocated with the call's other buffers, before any pass is paid for; a failure
// releases all of it (SignalSink) and is an ordinary error return.  The term tables go up here: fblocks | sig_ptr | term_src | hslots, and term_coef.
int sink_alloc(dfx_handle* h, SignalSink& k, const Pass& widest, int Tn) {
  const size_t B = h->pl.batch, kt = widest.kt(), T = Tn, n_ch = (k.tb.fblocks.size() + k.tb.hslots.size()) * 3, ns = k.terms.n_signals;
  HIP_OK(k.chan.ensure(B * T * n_ch)); HIP_OK(k.chan_dot.ensure(B * kt * T * n_ch));
  HIP_OK(k.S.ensure(B * T * ns)); HIP_OK(k.S_dot.ensure(B * kt * T * ns));
  HIP_OK(k.flags.ensure(kFlagGroups));
  std::vector<int32_t> tab;
  for (const std::vector<int32_t>* v : {&k.tb.fblocks, &k.tb.sig_ptr, &k.tb.term_src, &k.tb.hslots}) tab.insert(tab.end(), v->begin(), v->end());
  HIP_OK(k.tab.ensure(tab.size())); HIP_OK(k.coef.ensure(k.tb.term_coef.size()));
  HIP_OK(hipMemcpyAsync(k.tab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(k.coef.p, k.tb.term_coef.data(), sizeof(double) * k.tb.term_coef.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));      // (tab is this function's own)
  return 0;
}

// the three launches behind a pass, on its fields / fields_dot; returns how many workgroups wrote a flag
int sink_launch(dfx_handle* h, SignalSink& k, const Pass& p, int Tn, const MultiBufs& d, const TanCtx& c, const TanSlices& sl, long long& launches) {
  const Plan& pl = h->pl;
  const size_t B = pl.batch, nfield = B * (size_t)Tn * pl.n_blocks * 6;
  TanSigArgs a;
  a.fields = d.fields.p; a.fields_dot = d.fields_dot.p;
  a.n_fb = (int)k.tb.fblocks.size(); a.n_sig = k.terms.n_signals; a.Tn = Tn;
  a.n_hg = (int)k.tb.hslots.size(); a.n_ch = (a.n_fb + a.n_hg) * 3;
  a.fblocks = k.tab.p; a.sig_ptr = k.tab.p + a.n_fb; a.term_src = a.sig_ptr + a.n_sig + 1; a.hslots = a.term_src + k.terms.n;
  a.term_coef = k.coef.p;
  a.chan = k.chan.p; a.chan_dot = k.chan_dot.p; a.S = k.S.p; a.S_dot = k.S_dot.p;
  hipStream_t st = h->stream;
  if (a.n_ch) launches += pick_sig_channels(pl, p.kc)((unsigned)B, (unsigned)p.slices, st, c, sl, a);
  hipLaunchKernelGGL(k_tan_signal_combine, dim3(chunks_of((long long)Tn * a.n_sig, kTanSigThreads), (unsigned)B, (unsigned)p.kt()), dim3(kTanSigThreads), 0, st,
                     a, pl.n_blocks, p.kt());
  const size_t nx = p.k0 == 0 ? nfield : 0, ny = nfield * p.kt();       // (fields: the first pass vouches for them, later passes store the same)
  const int groups = (int)std::min<size_t>(kFlagGroups, (nx + ny + kTanSigThreads - 1) / kTanSigThreads);
  hipLaunchKernelGGL(k_tan_finite_flags, dim3((unsigned)groups), dim3(kTanSigThreads), 0, st, (const double*)d.fields.p, nx, (const double*)d.fields_dot.p, ny,
                     k.flags.p);
  launches += 2;
  return groups;
}

// signals (first pass) and the pass's columns of signals_dots (batch, n_dirs, T, n_signals) back to the caller; 3 when a flag is set
int sink_download(dfx_handle* h, SignalSink& k, const Pass& p, int n_dirs, int Tn, int groups, const char* who) {
  const size_t B = h->pl.batch, nrow = (size_t)Tn * k.terms.n_signals;
  hipStream_t st = h->stream;
  std::vector<double> sd_host(B * p.kt() * nrow);
  std::vector<int32_t> flags(groups);
  HIP_OK(hipMemcpyAsync(sd_host.data(), k.S_dot.p, sizeof(double) * sd_host.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(flags.data(), k.flags.p, sizeof(int32_t) * groups, hipMemcpyDeviceToHost, st));
  if (p.k0 == 0) HIP_OK(hipMemcpyAsync(k.signals, k.S.p, sizeof(double) * B * nrow, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (size_t m = 0; m < B; ++m)
    for (int j = 0; j < p.n; ++j)
      memcpy(k.signals_dots + (m * n_dirs + p.k0 + j) * nrow, sd_host.data() + (m * p.kt() + j) * nrow, sizeof(double) * nrow);
  int32_t bad = 0;
  for (int32_t f : flags) bad |= f;
  if (bad) { h->err = std::string(who) + ": non-finite state or tangent"; return 3; }
  return 0;
}

// what a signal call checks before anything is allocated: the outputs and the term list (the refusals of dfx_signal_values)
int sink_prepare(dfx_handle* h, const char* who, SignalSink& k) {
  if (!k.signals || !k.signals_dots) { h->err = std::string(who) + ": signals / signals_dots is NULL"; return 1; }
  return signal_term_tables(h, who, k.terms, k.tb);
}

TanSlices pass_slices(const dfx_handle* h, const Pass& p, int a_rows) {
  const Plan& pl = h->pl;
  const long long B = pl.batch, nb = pl.n_blocks;
  TanSlices sl;
  sl.d_plane = B * nb * kRec; sl.da_plane = B * a_rows * nb * 3;
  sl.tp_plane = B * pl.n_slots * tan_slot_n(p.kc); sl.blk_plane = B * nb * tan_blk_n(p.kc);
  sl.mem_plane = B * tan_mem_n(p.kc); sl.cen_plane = B * nb * tan_cen_n(p.kc);
  sl.kt = p.kt();
  return sl;
}

// stage i of step n: the two step-base buffers alternate (y holds this step's), the stage records ping-pong between S[0] and S[1]
TanStageM stage_args(const MultiBufs& d, int y, int i, int S, long long n, int a0, const TanSlices& sl) {
  TanStageM tm;
  TanStage& ts = tm.s;
  ts.S_in = i == 0 ? d.Y[y].p : d.S[i & 1].p;
  ts.D_in = i == 0 ? d.DY[y].p : d.DS[i & 1].p;
  ts.Y = d.Y[y].p; ts.DY = d.DY[y].p;
  ts.S_out = i == S - 1 ? d.Y[y ^ 1].p : d.S[(i + 1) & 1].p;
  ts.D_out = i == S - 1 ? d.DY[y ^ 1].p : d.DS[(i + 1) & 1].p;
  ts.A = d.A.p; ts.DA = d.DA.p;
  ts.n = n; ts.i = i; ts.a0 = a0;
  tm.sl = sl;
  return tm;
}

int fail(dfx_handle* h, const char* who, const std::string& what, int rc) {
  h->err = std::string(who) + ": " + what;
  return rc;
}

// The fixed grid: checks steps_per_interval / step_times and forms (t, h) of every step, exactly as the fixed-grid forward solve does
// (one grid, or one per member), with the first output time(s) t0 and the step count N.
int fixed_grid(dfx_handle* h, const char* who, const double* timepoints, int Tn, const int32_t* steps_per_interval, const double* step_times,
               bool per_member_times, std::vector<double>& tgrid, std::vector<double>& t0, long long& N) {
  if (Tn < 1 || !timepoints || (Tn > 1 && !steps_per_interval)) return fail(h, who, "need >= 1 timepoint and >= 1 step per interval");
  if (per_member_times && !step_times) return fail(h, who, "per-member time grids need step_times (batch, n_steps + 1)");
  std::vector<long long> step0(Tn, 0);
  for (int k = 0; k + 1 < Tn; ++k) {
    if (steps_per_interval[k] < 1) return fail(h, who, "need >= 1 timepoint and >= 1 step per interval");
    step0[k + 1] = step0[k] + steps_per_interval[k];
  }
  N = step0[Tn - 1];
  const int n_grids = per_member_times ? h->pl.batch : 1;
  tgrid.assign((size_t)n_grids * std::max<long long>(N, 1) * 2, 0.0);
  t0.assign(n_grids, 0.0);
  for (int g = 0; g < n_grids; ++g) {
    const double* tp = timepoints + (size_t)g * Tn;
    const double* tsg = step_times ? step_times + (size_t)g * (N + 1) : nullptr;
    t0[g] = tp[0];
    if (tsg) {
      for (long long n = 0; n < N; ++n)
        if (!(tsg[n + 1] > tsg[n])) return fail(h, who, "step_times must be strictly increasing");
      for (int k = 0; k < Tn; ++k)
        if (tsg[step0[k]] != tp[k]) return fail(h, who, "step_times must contain every timepoint at the start of its interval");
    }
    double* out = tgrid.data() + (size_t)g * N * 2;
    for (int k = 0; k + 1 < Tn; ++k) {
      const int spi = steps_per_interval[k];
      const double heq = (tp[k + 1] - tp[k]) / spi;
      for (int j = 0; j < spi; ++j) {
        const long long n = step0[k] + j;
        out[2 * n] = tsg ? tsg[n] : tp[k] + j * heq;
        out[2 * n + 1] = tsg ? tsg[n + 1] - tsg[n] : heq;
      }
    }
  }
  return 0;
}

// The dense pass's grid: (t, h) of every step of every member (entry N_m is the step of size zero at the member's final state), which
// steps hold an output of some member, and on the device the step counts, out_ptr / theta of dfx_dense_output_map and the output times.
struct DenseGrid {
  std::vector<double> tgrid;
  std::vector<char> has_out;
  long long Nmax = 0, gs = 0;
  DevBuf<long long> nst;
  DevBuf<int32_t> out_ptr;
  DevBuf<double> theta, ts;
  ~DenseGrid() { nst.release(); out_ptr.release(); theta.release(); ts.release(); }
};

int dense_grid(dfx_handle* h, const char* who, const double* timepoints, int Tn, const double* step_times, const int64_t* n_steps, int64_t stride,
               DenseGrid& g) {
  if (Tn < 1 || !timepoints || !step_times || !n_steps || stride < 1)
    return fail(h, who, "need >= 1 timepoint, step_times (batch, stride) and n_steps (batch)");
  const int B = h->pl.batch;
  std::vector<int32_t> out_ptr((size_t)B * stride);
  std::vector<double> theta((size_t)B * Tn);
  switch (dfx_dense_output_map(step_times, n_steps, stride, B, timepoints, Tn, out_ptr.data(), theta.data())) {
    case 0: break;
    case 1: return fail(h, who, "step_times must be strictly increasing");
    case 2: return fail(h, who, "every member's t_0 must be timepoints[0]");
    case 3: return fail(h, who, "every member's last step must end at or beyond the last timepoint (and the timepoints must not decrease)");
    default: return fail(h, who, "n_steps[m] must lie in [0, stride - 1]");
  }
  long long Nmax = 0;
  for (int m = 0; m < B; ++m) Nmax = std::max<long long>(Nmax, n_steps[m]);
  // a member the last forward pass flagged has no accepted steps to run on (a call without any step claims none: the initial state alone)
  for (int m = 0; Nmax > 0 && m < B && m < (int)h->member_status.size(); ++m)
    if (h->member_status[m])
      return fail(h, who, "member " + std::to_string(m) + " was flagged by the last forward pass (dfx_member_status): its steps are not a solve", 3);
  g.Nmax = Nmax; g.gs = 2 * (Nmax + 1);
  g.tgrid.assign((size_t)B * g.gs, 0.0);
  g.has_out.assign(Nmax + 1, 0);
  std::vector<long long> nst(B);
  for (int m = 0; m < B; ++m) {
    const double* t = step_times + (size_t)m * stride;
    const int32_t* op = out_ptr.data() + (size_t)m * stride;
    double* out = g.tgrid.data() + (size_t)m * g.gs;
    nst[m] = n_steps[m];
    for (long long n = 0; n < nst[m]; ++n) {
      out[2 * n] = t[n]; out[2 * n + 1] = t[n + 1] - t[n];
      if (op[n + 1] > op[n]) g.has_out[n] = 1;
    }
    for (long long n = nst[m]; n <= Nmax; ++n) { out[2 * n] = t[nst[m]]; out[2 * n + 1] = 0.0; }
  }
  hipStream_t st = h->stream;
  HIP_OK(g.nst.ensure(B)); HIP_OK(g.out_ptr.ensure(out_ptr.size())); HIP_OK(g.theta.ensure(theta.size())); HIP_OK(g.ts.ensure(Tn));
  HIP_OK(hipMemcpyAsync(g.nst.p, nst.data(), sizeof(long long) * B, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(g.out_ptr.p, out_ptr.data(), sizeof(int32_t) * out_ptr.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(g.theta.p, theta.data(), sizeof(double) * theta.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(g.ts.p, timepoints, sizeof(double) * Tn, hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));      // (nst, out_ptr and theta are this function's own)
  return 0;
}

// what every entry refuses; who: the entry's name in h->err
int check_handle(dfx_handle* h, const char* who) {
  if (!h->have_params) return fail(h, who, "set_params first");
  if (h->pl.n_ovf) return fail(h, who, "nodes that carry more than one ligament (extra ligaments of a general bond list) are not supported");
  return 0;
}

void fill_stats(dfx_stats* stats, long long steps, long long evals, long long launches, double ms) {
  if (!stats) return;
  memset(stats, 0, sizeof(*stats));
  stats->steps = steps; stats->rhs_evals = evals; stats->launches = launches; stats->kernel_ms = ms;
  stats->stage_kernel_us = steps ? 1e3 * ms / (double)evals : 0.0;
  stats->streams = 1;
}

int forward_tangent(dfx_handle* h, const char* who, const double* state0, const double* state0_dots, const dfx_params* params_dots, int n_dirs,
                    const double* timepoints, int Tn, const int32_t* steps_per_interval, const double* step_times, bool per_member_times,
                    double* fields, double* fields_dots, dfx_stats* stats, SignalSink* sink = nullptr) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = check_handle(h, who)) return rc;
  if (n_dirs < 1) return fail(h, who, "need >= 1 direction");
  if (sink) if (int rc = sink_prepare(h, who, *sink)) return rc;
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks, S = pl.tab.s;
  std::vector<double> tgrid, t0;
  long long N = 0;
  if (int rc = fixed_grid(h, who, timepoints, Tn, steps_per_interval, step_times, per_member_times, tgrid, t0, N)) return rc;
  const std::vector<Pass> passes = plan_passes(n_dirs, (long long)B * nb);
  MultiBufs d;
  TanCtx c;
  if (int rc = multi_alloc(h, passes[0], tgrid, t0, state0, state0_dots != nullptr, S, Tn, d, c)) return rc;
  if (int rc = table_tangents(h, who, n_dirs, c)) return rc;
  if (sink) if (int rc = sink_alloc(h, *sink, passes[0], Tn)) return rc;
  hipStream_t st = h->stream;
  c.grid_stride = per_member_times ? 2 * N : 0;
  c.t0_stride = per_member_times ? 1 : 0;
  const long long evals = N * S * (long long)passes.size();
  long long launches = 0;
  double ms_all = 0.0;
  for (const Pass& p : passes) {
    if (int rc = multi_upload_pass(h, params_dots, state0_dots, n_dirs, p, d)) return rc;
    c.tab_k0 = p.k0;
    const MultiKernels kn = pick_kernels(pl.model, pl.contact, pl.n_npb, p.kc);
    const dim3 grid((unsigned)(((size_t)B * nb + 255) / 256), (unsigned)p.slices);
    const TanSlices sl = pass_slices(h, p, S);
    HIP_OK(hipEventRecord(h->ev0, st));
    kn.init(grid, st, c, state0 ? d.s0.p : nullptr, state0_dots ? d.s0d.p : nullptr, d.Y[0].p, d.DY[0].p, sl);
    kn.snapshot(grid, st, B, nb, Tn, 0, d.Y[0].p, d.DY[0].p, sl, d.fields.p, d.fields_dot.p);
    launches += 2;
    int y = 0;          // which of the two step-base buffers holds the current step
    long long n = 0;
    for (int k = 0; k + 1 < Tn; ++k) {
      for (int j = 0; j < steps_per_interval[k]; ++j, ++n) {
        for (int i = 0; i < S; ++i) kn.stage(grid, st, c, pl.tab, stage_args(d, y, i, S, n, 0, sl));
        launches += S;
        y ^= 1;
      }
      kn.snapshot(grid, st, B, nb, Tn, k + 1, d.Y[y].p, d.DY[y].p, sl, d.fields.p, d.fields_dot.p);
      ++launches;
    }
    const int groups = sink ? sink_launch(h, *sink, p, Tn, d, c, sl, launches) : 0;
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(h->ev1, st));
    const int rc = sink ? sink_download(h, *sink, p, n_dirs, Tn, groups, who) : multi_download_pass(h, p, n_dirs, Tn, d, fields, fields_dots, who);
    if (rc == 2) return rc;
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ms_all += ms;
    fill_stats(stats, N, evals, launches, ms_all);
    if (rc) return rc;
  }
  return 0;
}

int forward_tangent_dense(dfx_handle* h, const char* who, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                          int n_dirs, const double* timepoints, int Tn, const double* step_times, const int64_t* n_steps, int64_t stride,
                          double* fields, double* fields_dots, dfx_stats* stats, SignalSink* sink = nullptr) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = check_handle(h, who)) return rc;
  const Plan& pl = h->pl;
  if (pl.tab.s != 6) return fail(h, who, "the dense output is defined for the dopri5 tableau");
  if (n_dirs < 1) return fail(h, who, "need >= 1 direction");
  if (sink) if (int rc = sink_prepare(h, who, *sink)) return rc;
  const int B = pl.batch, nb = pl.n_blocks, S = pl.tab.s;
  DenseGrid g;
  if (int rc = dense_grid(h, who, timepoints, Tn, step_times, n_steps, stride, g)) return rc;
  const long long Nmax = g.Nmax;
  const std::vector<double> t0(1, timepoints[0]);
  const std::vector<Pass> passes = plan_passes(n_dirs, (long long)B * nb);
  MultiBufs d;
  TanCtx c;
  if (int rc = multi_alloc(h, passes[0], g.tgrid, t0, state0, state0_dots != nullptr, 7, Tn, d, c)) return rc;
  if (int rc = table_tangents(h, who, n_dirs, c)) return rc;
  if (sink) if (int rc = sink_alloc(h, *sink, passes[0], Tn)) return rc;
  hipStream_t st = h->stream;
  c.grid_stride = g.gs; c.t0_stride = 0;
  c.n_steps = g.nst.p;
  const Dopri D = make_dopri();
  TanDenseM dm;
  TanDense& dn = dm.d;
  dn.A = d.A.p; dn.DA = d.DA.p;
  dn.out_ptr = g.out_ptr.p; dn.theta = g.theta.p; dn.ts = g.ts.p;
  dn.fields = d.fields.p; dn.fields_dot = d.fields_dot.p;
  dn.op_stride = stride; dn.Tn = Tn;
  for (int l = 0; l < 7; ++l) { dn.cm[l] = D.cm[l]; dn.cma[l] = D.cma[l]; }
  const long long evals = (Nmax * S + 1) * (long long)passes.size();
  long long launches = 0;
  double ms_all = 0.0;
  for (const Pass& p : passes) {
    if (int rc = multi_upload_pass(h, params_dots, state0_dots, n_dirs, p, d)) return rc;
    c.tab_k0 = p.k0;
    const MultiKernels kn = pick_kernels(pl.model, pl.contact, pl.n_npb, p.kc);
    const dim3 grid((unsigned)(((size_t)B * nb + 255) / 256), (unsigned)p.slices);
    const TanSlices sl = pass_slices(h, p, 7);
    dm.sl = sl;
    HIP_OK(hipEventRecord(h->ev0, st));
    kn.init(grid, st, c, state0 ? d.s0.p : nullptr, state0_dots ? d.s0d.p : nullptr, d.Y[0].p, d.DY[0].p, sl);
    kn.snapshot(grid, st, B, nb, Tn, 0, d.Y[0].p, d.DY[0].p, sl, d.fields.p, d.fields_dot.p);
    launches += 2;
    int y = 0;          // which of the two step-base buffers holds step n
    for (long long n = 0; Nmax > 0 && n <= Nmax; ++n) {
      const int a0 = (n & 1) ? 6 : 0;           // A_0 of step n = A_6 of step n - 1: the two places alternate
      for (int i = 0; i < (n == Nmax ? 1 : S); ++i) {
        kn.stage(grid, st, c, pl.tab, stage_args(d, y, i, S, n, a0, sl));
        ++launches;
        if (i == 0 && n > 0 && g.has_out[n - 1]) {
          // the outputs inside step n - 1: its step base is still in the other buffer (stage 5 of step n overwrites it), A_6 has just arrived
          dn.Y0 = d.Y[y ^ 1].p; dn.DY0 = d.DY[y ^ 1].p; dn.Y1 = d.Y[y].p; dn.DY1 = d.DY[y].p;
          dn.n = n - 1; dn.a0 = a0 ^ 6; dn.a6 = a0;
          kn.dense(grid, st, c, dm);
          ++launches;
        }
      }
      y ^= 1;
    }
    const int groups = sink ? sink_launch(h, *sink, p, Tn, d, c, sl, launches) : 0;
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(h->ev1, st));
    const int rc = sink ? sink_download(h, *sink, p, n_dirs, Tn, groups, who) : multi_download_pass(h, p, n_dirs, Tn, d, fields, fields_dots, who);
    if (rc == 2) return rc;
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ms_all += ms;
    fill_stats(stats, Nmax, evals, launches, ms_all);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace

extern "C" int dfx_forward_tangent(dfx_handle* h, const double* state0, const double* state0_dot, const dfx_params* params_dot,
                                   const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval, const double* step_times,
                                   int32_t per_member_times, double* fields, double* fields_dot, dfx_stats* stats) {
  return forward_tangent(h, "forward_tangent", state0, state0_dot, params_dot, 1, timepoints, n_timepoints, steps_per_interval, step_times,
                         per_member_times != 0, fields, fields_dot, stats);
}

extern "C" int dfx_forward_tangent_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                         int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval,
                                         const double* step_times, int32_t per_member_times, double* fields, double* fields_dots,
                                         dfx_stats* stats) {
  return forward_tangent(h, "forward_tangent_multi", state0, state0_dots, params_dots, n_dirs, timepoints, n_timepoints, steps_per_interval,
                         step_times, per_member_times != 0, fields, fields_dots, stats);
}

// ---- forward mode through the adaptive solve's dense output ---------------------------------------------------------------------------
// Which outputs every frozen step holds, and where: the rule of k_control (dfx_kernels.h) -- an output belongs to the first accepted step
// with ts[k] <= t_{n+1} -- and its two IEEE operations for theta, so that out_ptr / theta carry the bits of the arrays the adaptive pass
// recorded for the reverse sweep (AdaptRec).  Entries of out_ptr beyond N_m repeat the last one.
extern "C" int dfx_dense_output_map(const double* step_times, const int64_t* n_steps, int64_t stride, int32_t batch, const double* timepoints,
                                    int32_t n_timepoints, int32_t* out_ptr, double* theta) {
  if (!step_times || !n_steps || !timepoints || !out_ptr || !theta || batch < 1 || n_timepoints < 1 || stride < 1) return 4;
  const int Tn = n_timepoints;
  for (int m = 0; m < batch; ++m) {
    const long long N = n_steps[m];
    if (N < 0 || N + 1 > stride) return 4;
    const double* t = step_times + (size_t)m * stride;
    int32_t* op = out_ptr + (size_t)m * stride;
    double* th = theta + (size_t)m * Tn;
    for (long long n = 0; n < N; ++n) if (!(t[n + 1] > t[n])) return 1;
    if (t[0] != timepoints[0]) return 2;
    if (!(t[N] >= timepoints[Tn - 1])) return 3;
    int k = 1;
    op[0] = 1; th[0] = 0.0;
    for (long long n = 0; n < N; ++n) {
      for (; k < Tn && timepoints[k] <= t[n + 1]; ++k) th[k] = (timepoints[k] - t[n]) / (t[n + 1] - t[n]);
      op[n + 1] = k;
    }
    if (k != Tn) return 3;
    for (long long n = N + 1; n < stride; ++n) op[n] = k;
  }
  return 0;
}

extern "C" int dfx_forward_tangent_dense(dfx_handle* h, const double* state0, const double* state0_dot, const dfx_params* params_dot,
                                         const double* timepoints, int32_t n_timepoints, const double* step_times, const int64_t* n_steps,
                                         int64_t stride, double* fields, double* fields_dot, dfx_stats* stats) {
  return forward_tangent_dense(h, "forward_tangent_dense", state0, state0_dot, params_dot, 1, timepoints, n_timepoints, step_times, n_steps, stride,
                               fields, fields_dot, stats);
}

extern "C" int dfx_forward_tangent_dense_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                               int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const double* step_times,
                                               const int64_t* n_steps, int64_t stride, double* fields, double* fields_dots, dfx_stats* stats) {
  return forward_tangent_dense(h, "forward_tangent_dense_multi", state0, state0_dots, params_dots, n_dirs, timepoints, n_timepoints, step_times,
                               n_steps, stride, fields, fields_dots, stats);
}

// ---- forward-mode signals: the two solves above with the signal sink at the end of every pass ----------------------------------------------
extern "C" int dfx_forward_tangent_signals_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                                 int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval,
                                                 const double* step_times, int32_t per_member_times, int32_t n_terms, const int32_t* term_signal,
                                                 const int32_t* term_block, const int32_t* term_component, const double* term_coef,
                                                 int32_t n_signals, double* signals, double* signals_dots, dfx_stats* stats) {
  SignalSink sink;
  sink.terms = SigTerms{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  sink.signals = signals; sink.signals_dots = signals_dots;
  return forward_tangent(h, "forward_tangent_signals_multi", state0, state0_dots, params_dots, n_dirs, timepoints, n_timepoints, steps_per_interval,
                         step_times, per_member_times != 0, nullptr, nullptr, stats, &sink);
}

extern "C" int dfx_forward_tangent_signals_dense_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                                       int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const double* step_times,
                                                       const int64_t* n_steps, int64_t stride, int32_t n_terms, const int32_t* term_signal,
                                                       const int32_t* term_block, const int32_t* term_component, const double* term_coef,
                                                       int32_t n_signals, double* signals, double* signals_dots, dfx_stats* stats) {
  SignalSink sink;
  sink.terms = SigTerms{n_terms, term_signal, term_block, term_component, term_coef, n_signals};
  sink.signals = signals; sink.signals_dots = signals_dots;
  return forward_tangent_dense(h, "forward_tangent_signals_dense_multi", state0, state0_dots, params_dots, n_dirs, timepoints, n_timepoints, step_times,
                               n_steps, stride, nullptr, nullptr, stats, &sink);
}

// One evaluation is the tangent solve's own machinery on a step of size zero at t: k_tan_init_multi builds the records (prescribed DOFs and
// their tangents from c(t)), stage 0 of the unchanged k_tan_stage_multi leaves a and da in row 0 of A / DA (the dense pass ends every
// member with exactly this evaluation), and k_tan_rhs_out_multi writes the two results in the layout of one output row, so the pass forms,
// the images and the download are those of dfx_forward_tangent_multi.  The stage kernel itself is not touched: its ligament walk shares no
// code with a second kernel, so the shipped builds keep their registers (profiles/r09_tangent_multi_resources.txt).
extern "C" int dfx_rhs_jvp(dfx_handle* h, const double* y, double t, const double* y_dots, const dfx_params* params_dots, int32_t n_dirs,
                           double* dy, double* dy_dots) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = check_handle(h, "rhs_jvp")) return rc;
  if (n_dirs < 1) return fail(h, "rhs_jvp", "need >= 1 direction");
  if (!y) return fail(h, "rhs_jvp", "need y (batch, 2, n_blocks, 3)");
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks;
  const std::vector<double> tgrid{t, 0.0}, t0{t};          // one step of size zero at t
  const std::vector<Pass> passes = plan_passes(n_dirs, (long long)B * nb);
  MultiBufs d;
  TanCtx c;
  if (int rc = multi_alloc(h, passes[0], tgrid, t0, y, y_dots != nullptr, 1, 1, d, c)) return rc;
  if (int rc = table_tangents(h, "rhs_jvp", n_dirs, c)) return rc;
  hipStream_t st = h->stream;
  for (const Pass& p : passes) {
    if (int rc = multi_upload_pass(h, params_dots, y_dots, n_dirs, p, d)) return rc;
    c.tab_k0 = p.k0;
    const MultiKernels kn = pick_kernels(pl.model, pl.contact, pl.n_npb, p.kc);
    const dim3 grid((unsigned)(((size_t)B * nb + 255) / 256), (unsigned)p.slices);
    const TanSlices sl = pass_slices(h, p, 1);
    kn.init(grid, st, c, d.s0.p, y_dots ? d.s0d.p : nullptr, d.Y[0].p, d.DY[0].p, sl);
    kn.stage(grid, st, c, pl.tab, stage_args(d, 0, 0, pl.tab.s, 0, 0, sl));          // (S_out: the records of a next stage nobody runs)
    kn.rhs_out(grid, st, c, d, sl);
    HIP_OK(hipGetLastError());
    if (int rc = multi_download_pass(h, p, n_dirs, 1, d, dy, dy_dots, "rhs_jvp")) return rc;
  }
  return 0;
}
