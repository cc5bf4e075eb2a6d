// engine_tangent.hip -- forward mode (kernels in dfx_tangent.h): dfx_forward_tangent, the derivative of the fixed-grid solve, and
// dfx_forward_tangent_dense, the derivative of the adaptive solve's dense output on every member's own frozen accepted steps.
//
// One stage launch per Runge-Kutta stage on the handle's stream, one lane per (member, block); the buffers are the call's own, so the
// trajectory checkpoint and the resident history of the last dfx_forward are left as they were (a later dfx_adjoint still reverses that
// solve).  Host side: the parameter image of the tangent kernels (plain per-slot layout, value and tangent) is built from the packed
// primal image dfx_set_params left on the handle and from params_dot.
#include "dfx_engine.h"
#include "dfx_tangent.h"

using namespace dfx;

namespace {

struct TanBufs {
  DevBuf<double> tp, blk, mem, cen, tgrid, t0, s0, s0d, Y[2], DY[2], S[2], DS[2], A, DA, fields, fields_dot;
  ~TanBufs() {
    DevBuf<double>* all[] = {&tp, &blk, &mem, &cen, &tgrid, &t0, &s0, &s0d, &Y[0], &Y[1], &DY[0], &DY[1], &S[0], &S[1], &DS[0], &DS[1],
                             &A, &DA, &fields, &fields_dot};
    for (auto* b : all) b->release();
  }
};

using StageLaunch = void (*)(dim3, hipStream_t, const TanCtx&, const Tableau&, const TanStage&);

template <int MODEL, int CONTACT, int NPB>
void launch_tan_stage(dim3 grid, hipStream_t s, const TanCtx& c, const Tableau& T, const TanStage& st) {
  hipLaunchKernelGGL((k_tan_stage<MODEL, CONTACT, NPB>), grid, dim3(256), 0, s, c, T, st);
}

template <int MODEL, int CONTACT>
StageLaunch pick_npb(int npb) { return npb == 3 ? launch_tan_stage<MODEL, CONTACT, 3> : launch_tan_stage<MODEL, CONTACT, 4>; }

template <int MODEL>
StageLaunch pick_contact(int contact, int npb) {
  if (contact == DFX_CONTACT_DISTANCE) return pick_npb<MODEL, DFX_CONTACT_DISTANCE>(npb);
  if (contact == DFX_CONTACT_ANGLE) return pick_npb<MODEL, DFX_CONTACT_ANGLE>(npb);
  return pick_npb<MODEL, DFX_CONTACT_NONE>(npb);
}

StageLaunch pick_stage(int model, int contact, int npb) {
  switch (model) {
    case kNonlinear: return pick_contact<kNonlinear>(contact, npb);
    case kLinearized: return pick_contact<kLinearized>(contact, npb);
    case kSimpleSpring: return pick_contact<kSimpleSpring>(contact, npb);
    default: return pick_contact<kStretchTorsion>(contact, npb);
  }
}

bool all_finite(const std::vector<double>& v) {
  for (double x : v) if (!std::isfinite(x)) return false;
  return true;
}

// The parameter image of the tangent kernels: primal values from the packed image, tangents from params_dot (NULL array: zero tangent)
struct TanImage { std::vector<double> tp, blk, mem, cen; };

void tangent_image(const dfx_handle* h, const dfx_params* params_dot, TanImage& img) {
  const Plan& pl = h->pl;
  const PackedParams& pp = h->pp;
  const int B = pl.batch, nb = pl.n_blocks, NS = pl.n_slots, npb = pl.n_npb;
  std::vector<double>&tp = img.tp, &blk = img.blk, &mem = img.mem, &cen = img.cen;
  dfx_params zero_dot;
  memset(&zero_dot, 0, sizeof(zero_dot));
  const dfx_params& q = params_dot ? *params_dot : zero_dot;
  tp.assign((size_t)B * NS * kTanSlot, 0.0); blk.assign((size_t)B * nb * kTanBlk, 0.0); mem.assign((size_t)B * kTanMem, 0.0);
  cen.clear();
  const bool dist = pl.contact == DFX_CONTACT_DISTANCE;
  if (dist) cen.assign((size_t)B * nb * kTanCen, 0.0);
  for (int m = 0; m < B; ++m) {
    for (int s = 0; s < NS; ++s) {
      double* o = tp.data() + ((size_t)m * NS + s) * kTanSlot;
      const size_t ms = (size_t)m * NS + s;
      const int b = s / kSlots, k = s % kSlots;
      if (k >= npb) continue;
      o[0] = pp.p_r[ms * 2]; o[1] = pp.p_r[ms * 2 + 1];
      if (q.centroid_node_vectors) {
        const double* r = q.centroid_node_vectors + (((size_t)m * nb + b) * npb + k) * 2;
        o[9] = r[0]; o[10] = r[1];
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
      if (q.reference_vector) { o[11] = q.reference_vector[mb * 2]; o[12] = q.reference_vector[mb * 2 + 1]; }
      if (q.k_bond) for (int j = 0; j < 3; ++j) o[13 + j] = q.k_bond[mb * 3 + j];
      if (q.void_angle0 && pl.contact == DFX_CONTACT_ANGLE) { o[16] = q.void_angle0[mb * 2]; o[17] = q.void_angle0[mb * 2 + 1]; }
    }
    for (int b = 0; b < nb; ++b) {
      double* o = blk.data() + ((size_t)m * nb + b) * kTanBlk;
      for (int d = 0; d < 3; ++d) {
        const size_t i = ((size_t)m * nb + b) * 3 + d;
        const double im = pp.inv_m[i];
        o[d] = im;
        o[3 + d] = q.inertia ? -q.inertia[i] * im * im : 0.0;     // d(1/m) = -dm / m^2
        o[6 + d] = pp.damping[i];
        o[9 + d] = q.damping ? q.damping[i] : 0.0;
      }
      if (dist) {
        double* c = cen.data() + ((size_t)m * nb + b) * kTanCen;
        c[0] = pp.centroid[((size_t)m * nb + b) * 2]; c[1] = pp.centroid[((size_t)m * nb + b) * 2 + 1];
        if (q.block_centroids) { c[2] = q.block_centroids[((size_t)m * nb + b) * 2]; c[3] = q.block_centroids[((size_t)m * nb + b) * 2 + 1]; }
      }
    }
    double* o = mem.data() + (size_t)m * kTanMem;
    for (int j = 0; j < 3; ++j) {
      o[j] = pp.contact[(size_t)m * 3 + j];
      o[3 + j] = (q.contact && pl.contact) ? q.contact[(size_t)m * 3 + j] : 0.0;
    }
    if (q.fn_params)
      for (int f = 0; f < pl.n_fns; ++f)
        for (int j = 0; j < DFX_FN_PARAMS; ++j) o[6 + f * DFX_FN_PARAMS + j] = q.fn_params[((size_t)m * pl.n_fns + f) * DFX_FN_PARAMS + j];
  }
}

// device buffers of one call (the image, the time grid, the initial state and tangent, the work buffers) and the kernels' context
int tangent_upload(dfx_handle* h, const dfx_params* params_dot, const std::vector<double>& tgrid, const std::vector<double>& t0, const double* state0,
                   const double* state0_dot, int a_rows, int Tn, TanBufs& d, TanCtx& c) {
  const Plan& pl = h->pl;
  const int B = pl.batch, nb = pl.n_blocks;
  TanImage img;
  tangent_image(h, params_dot, img);
  const std::vector<double>&tp = img.tp, &blk = img.blk, &mem = img.mem, &cen = img.cen;
  const bool dist = pl.contact == DFX_CONTACT_DISTANCE;
  const size_t rec = (size_t)B * nb * kRec, nfield = (size_t)B * Tn * nb * 6;
  HIP_OK(d.tp.ensure(tp.size())); HIP_OK(d.blk.ensure(blk.size())); HIP_OK(d.mem.ensure(mem.size()));
  HIP_OK(d.tgrid.ensure(tgrid.size())); HIP_OK(d.t0.ensure(t0.size()));
  for (int j = 0; j < 2; ++j) {
    HIP_OK(d.Y[j].ensure(rec)); HIP_OK(d.DY[j].ensure(rec)); HIP_OK(d.S[j].ensure(rec)); HIP_OK(d.DS[j].ensure(rec));
  }
  HIP_OK(d.A.ensure((size_t)B * a_rows * nb * 3)); HIP_OK(d.DA.ensure((size_t)B * a_rows * nb * 3));
  HIP_OK(d.fields.ensure(nfield)); HIP_OK(d.fields_dot.ensure(nfield));
  hipStream_t st = h->stream;
  HIP_OK(hipMemcpyAsync(d.tp.p, tp.data(), sizeof(double) * tp.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.blk.p, blk.data(), sizeof(double) * blk.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.mem.p, mem.data(), sizeof(double) * mem.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.tgrid.p, tgrid.data(), sizeof(double) * tgrid.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d.t0.p, t0.data(), sizeof(double) * t0.size(), hipMemcpyHostToDevice, st));
  if (dist) {
    HIP_OK(d.cen.ensure(cen.size()));
    HIP_OK(hipMemcpyAsync(d.cen.p, cen.data(), sizeof(double) * cen.size(), hipMemcpyHostToDevice, st));
  }
  const size_t nstate = (size_t)B * nb * 6;
  if (state0) { HIP_OK(d.s0.ensure(nstate)); HIP_OK(hipMemcpyAsync(d.s0.p, state0, sizeof(double) * nstate, hipMemcpyHostToDevice, st)); }
  if (state0_dot) { HIP_OK(d.s0d.ensure(nstate)); HIP_OK(hipMemcpyAsync(d.s0d.p, state0_dot, sizeof(double) * nstate, hipMemcpyHostToDevice, st)); }
  HIP_OK(hipStreamSynchronize(st));      // (the image is this function's own)
  c.B = B; c.nb = nb; c.n_fns = pl.n_fns; c.n_stages = pl.tab.s;
  c.slot_info = h->d_slot_info.p; c.block_special = h->d_block_special.p; c.special = h->d_special.p; c.fns = h->d_fns.p;
  c.tp = d.tp.p; c.blk = d.blk.p; c.mem = d.mem.p; c.cen = dist ? d.cen.p : nullptr;
  c.tgrid = d.tgrid.p; c.t0 = d.t0.p;
  c.grid_stride = 0; c.t0_stride = 0;
  c.a_rows = a_rows; c.n_steps = nullptr;
  return 0;
}

}  // namespace

extern "C" int dfx_forward_tangent(dfx_handle* h, const double* state0, const double* state0_dot, const dfx_params* params_dot,
                                   const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval, const double* step_times,
                                   int32_t per_member_times, double* fields, double* fields_dot, dfx_stats* stats) {
  HIP_OK(hipSetDevice(h->device));
  if (!h->have_params) { h->err = "forward_tangent: set_params first"; return 1; }
  const Plan& pl = h->pl;
  if (pl.n_ovf) {
    h->err = "forward_tangent: nodes that carry more than one ligament (extra ligaments of a general bond list) are not supported";
    return 1;
  }
  if (n_timepoints < 1 || !timepoints || (n_timepoints > 1 && !steps_per_interval)) {
    h->err = "forward_tangent: need >= 1 timepoint and >= 1 step per interval"; return 1;
  }
  if (per_member_times && !step_times) { h->err = "forward_tangent: per-member time grids need step_times (batch, n_steps + 1)"; return 1; }
  const int B = pl.batch, nb = pl.n_blocks, Tn = n_timepoints, npb = pl.n_npb;
  std::vector<long long> step0(Tn, 0);
  for (int k = 0; k + 1 < Tn; ++k) {
    if (steps_per_interval[k] < 1) { h->err = "forward_tangent: need >= 1 timepoint and >= 1 step per interval"; return 1; }
    step0[k + 1] = step0[k] + steps_per_interval[k];
  }
  const long long N = step0[Tn - 1];
  const int n_grids = per_member_times ? B : 1;
  // (t, h) of every step, exactly as the fixed-grid forward solve forms them
  std::vector<double> tgrid((size_t)n_grids * std::max<long long>(N, 1) * 2), t0(n_grids);
  for (int g = 0; g < n_grids; ++g) {
    const double* tp = timepoints + (size_t)g * Tn;
    const double* tsg = step_times ? step_times + (size_t)g * (N + 1) : nullptr;
    t0[g] = tp[0];
    if (tsg) {
      for (long long n = 0; n < N; ++n)
        if (!(tsg[n + 1] > tsg[n])) { h->err = "forward_tangent: step_times must be strictly increasing"; return 1; }
      for (int k = 0; k < Tn; ++k)
        if (tsg[step0[k]] != tp[k]) { h->err = "forward_tangent: step_times must contain every timepoint at the start of its interval"; return 1; }
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
  const int S = pl.tab.s;
  const size_t nfield = (size_t)B * Tn * nb * 6;
  TanBufs d;
  TanCtx c;
  if (int rc = tangent_upload(h, params_dot, tgrid, t0, state0, state0_dot, S, Tn, d, c)) return rc;
  hipStream_t st = h->stream;
  c.grid_stride = per_member_times ? 2 * N : 0;
  c.t0_stride = per_member_times ? 1 : 0;
  const dim3 grid((unsigned)(((size_t)B * nb + 255) / 256));
  const StageLaunch stage = pick_stage(pl.model, pl.contact, npb);
  long long launches = 0;
  HIP_OK(hipEventRecord(h->ev0, st));
  hipLaunchKernelGGL(k_tan_init, grid, dim3(256), 0, st, c, state0 ? d.s0.p : nullptr, state0_dot ? d.s0d.p : nullptr, d.Y[0].p, d.DY[0].p);
  hipLaunchKernelGGL(k_tan_snapshot, grid, dim3(256), 0, st, B, nb, Tn, 0, d.Y[0].p, d.DY[0].p, d.fields.p, d.fields_dot.p);
  launches += 2;
  int y = 0;          // which of the two step-base buffers holds the current step
  long long n = 0;
  for (int k = 0; k + 1 < Tn; ++k) {
    for (int j = 0; j < steps_per_interval[k]; ++j, ++n) {
      for (int i = 0; i < S; ++i) {
        TanStage ts;
        ts.S_in = i == 0 ? d.Y[y].p : d.S[i & 1].p;
        ts.D_in = i == 0 ? d.DY[y].p : d.DS[i & 1].p;
        ts.Y = d.Y[y].p; ts.DY = d.DY[y].p;
        ts.S_out = i == S - 1 ? d.Y[y ^ 1].p : d.S[(i + 1) & 1].p;
        ts.D_out = i == S - 1 ? d.DY[y ^ 1].p : d.DS[(i + 1) & 1].p;
        ts.A = d.A.p; ts.DA = d.DA.p;
        ts.n = n; ts.i = i; ts.a0 = 0;
        stage(grid, st, c, pl.tab, ts);
        ++launches;
      }
      y ^= 1;
    }
    hipLaunchKernelGGL(k_tan_snapshot, grid, dim3(256), 0, st, B, nb, Tn, k + 1, d.Y[y].p, d.DY[y].p, d.fields.p, d.fields_dot.p);
    ++launches;
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(h->ev1, st));
  std::vector<double> f_host(nfield), fd_host(nfield);
  HIP_OK(hipMemcpyAsync(f_host.data(), d.fields.p, sizeof(double) * nfield, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(fd_host.data(), d.fields_dot.p, sizeof(double) * nfield, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  float ms = 0.0f;
  HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (fields) memcpy(fields, f_host.data(), sizeof(double) * nfield);
  if (fields_dot) memcpy(fields_dot, fd_host.data(), sizeof(double) * nfield);
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->steps = N; stats->rhs_evals = N * S; stats->launches = launches; stats->kernel_ms = ms;
    stats->stage_kernel_us = N ? 1e3 * ms / (double)(N * S) : 0.0;
    stats->streams = 1;
  }
  if (!all_finite(f_host) || !all_finite(fd_host)) { h->err = "forward_tangent: non-finite state or tangent"; return 3; }
  return 0;
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
  HIP_OK(hipSetDevice(h->device));
  if (!h->have_params) { h->err = "forward_tangent_dense: set_params first"; return 1; }
  const Plan& pl = h->pl;
  if (pl.n_ovf) {
    h->err = "forward_tangent_dense: nodes that carry more than one ligament (extra ligaments of a general bond list) are not supported";
    return 1;
  }
  if (pl.tab.s != 6) { h->err = "forward_tangent_dense: the dense output is defined for the dopri5 tableau"; return 1; }
  if (n_timepoints < 1 || !timepoints || !step_times || !n_steps || stride < 1) {
    h->err = "forward_tangent_dense: need >= 1 timepoint, step_times (batch, stride) and n_steps (batch)"; return 1;
  }
  const int B = pl.batch, nb = pl.n_blocks, Tn = n_timepoints, npb = pl.n_npb;
  std::vector<int32_t> out_ptr((size_t)B * stride);
  std::vector<double> theta((size_t)B * Tn);
  switch (dfx_dense_output_map(step_times, n_steps, stride, B, timepoints, Tn, out_ptr.data(), theta.data())) {
    case 0: break;
    case 1: h->err = "forward_tangent_dense: step_times must be strictly increasing"; return 1;
    case 2: h->err = "forward_tangent_dense: every member's t_0 must be timepoints[0]"; return 1;
    case 3: h->err = "forward_tangent_dense: every member's last step must end at or beyond the last timepoint (and the timepoints must not decrease)"; return 1;
    default: h->err = "forward_tangent_dense: n_steps[m] must lie in [0, stride - 1]"; return 1;
  }
  long long Nmax = 0;
  for (int m = 0; m < B; ++m) Nmax = std::max<long long>(Nmax, n_steps[m]);
  // a member the last forward pass flagged has no accepted steps to run on (a call without any step claims none: the initial state alone)
  for (int m = 0; Nmax > 0 && m < B && m < (int)h->member_status.size(); ++m)
    if (h->member_status[m]) {
      h->err = "forward_tangent_dense: member " + std::to_string(m) + " was flagged by the last forward pass (dfx_member_status): its steps are not a solve";
      return 3;
    }
  // (t, h) of every step of every member; entry N_m is the step of size zero at the member's final state
  const long long gs = 2 * (Nmax + 1);
  std::vector<double> tgrid((size_t)B * gs, 0.0), t0(1, timepoints[0]);
  std::vector<long long> nst(B);
  std::vector<char> has_out(Nmax + 1, 0);          // does some member have an output inside step n
  for (int m = 0; m < B; ++m) {
    const double* t = step_times + (size_t)m * stride;
    const int32_t* op = out_ptr.data() + (size_t)m * stride;
    double* out = tgrid.data() + (size_t)m * gs;
    nst[m] = n_steps[m];
    for (long long n = 0; n < nst[m]; ++n) {
      out[2 * n] = t[n]; out[2 * n + 1] = t[n + 1] - t[n];
      if (op[n + 1] > op[n]) has_out[n] = 1;
    }
    for (long long n = nst[m]; n <= Nmax; ++n) { out[2 * n] = t[nst[m]]; out[2 * n + 1] = 0.0; }
  }
  const int S = pl.tab.s;
  const size_t nfield = (size_t)B * Tn * nb * 6;
  TanBufs d;
  TanCtx c;
  if (int rc = tangent_upload(h, params_dot, tgrid, t0, state0, state0_dot, 7, Tn, d, c)) return rc;
  hipStream_t st = h->stream;
  DevBuf<long long> d_nst;
  DevBuf<int32_t> d_op;
  DevBuf<double> d_theta, d_ts;
  struct Release {
    DevBuf<long long>& a; DevBuf<int32_t>& b; DevBuf<double>&c, &e;
    ~Release() { a.release(); b.release(); c.release(); e.release(); }
  } release{d_nst, d_op, d_theta, d_ts};
  HIP_OK(d_nst.ensure(B)); HIP_OK(d_op.ensure(out_ptr.size())); HIP_OK(d_theta.ensure(theta.size())); HIP_OK(d_ts.ensure(Tn));
  HIP_OK(hipMemcpyAsync(d_nst.p, nst.data(), sizeof(long long) * B, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_op.p, out_ptr.data(), sizeof(int32_t) * out_ptr.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_theta.p, theta.data(), sizeof(double) * theta.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_ts.p, timepoints, sizeof(double) * Tn, hipMemcpyHostToDevice, st));
  c.grid_stride = gs; c.t0_stride = 0;
  c.n_steps = d_nst.p;
  const Dopri D = make_dopri();
  TanDense dn;
  dn.A = d.A.p; dn.DA = d.DA.p;
  dn.out_ptr = d_op.p; dn.theta = d_theta.p; dn.ts = d_ts.p;
  dn.fields = d.fields.p; dn.fields_dot = d.fields_dot.p;
  dn.op_stride = stride; dn.Tn = Tn;
  for (int l = 0; l < 7; ++l) { dn.cm[l] = D.cm[l]; dn.cma[l] = D.cma[l]; }
  const dim3 grid((unsigned)(((size_t)B * nb + 255) / 256));
  const StageLaunch stage = pick_stage(pl.model, pl.contact, npb);
  long long launches = 0;
  HIP_OK(hipEventRecord(h->ev0, st));
  hipLaunchKernelGGL(k_tan_init, grid, dim3(256), 0, st, c, state0 ? d.s0.p : nullptr, state0_dot ? d.s0d.p : nullptr, d.Y[0].p, d.DY[0].p);
  hipLaunchKernelGGL(k_tan_snapshot, grid, dim3(256), 0, st, B, nb, Tn, 0, d.Y[0].p, d.DY[0].p, d.fields.p, d.fields_dot.p);
  launches += 2;
  int y = 0;          // which of the two step-base buffers holds step n
  for (long long n = 0; Nmax > 0 && n <= Nmax; ++n) {
    const int a0 = (n & 1) ? 6 : 0;           // A_0 of step n = A_6 of step n - 1: the two places alternate
    for (int i = 0; i < (n == Nmax ? 1 : S); ++i) {
      TanStage ts;
      ts.S_in = i == 0 ? d.Y[y].p : d.S[i & 1].p;
      ts.D_in = i == 0 ? d.DY[y].p : d.DS[i & 1].p;
      ts.Y = d.Y[y].p; ts.DY = d.DY[y].p;
      ts.S_out = i == S - 1 ? d.Y[y ^ 1].p : d.S[(i + 1) & 1].p;
      ts.D_out = i == S - 1 ? d.DY[y ^ 1].p : d.DS[(i + 1) & 1].p;
      ts.A = d.A.p; ts.DA = d.DA.p;
      ts.n = n; ts.i = i; ts.a0 = a0;
      stage(grid, st, c, pl.tab, ts);
      ++launches;
      if (i == 0 && n > 0 && has_out[n - 1]) {
        // the outputs inside step n - 1: its step base is still in the other buffer (stage 5 of step n overwrites it), A_6 has just arrived
        dn.Y0 = d.Y[y ^ 1].p; dn.DY0 = d.DY[y ^ 1].p; dn.Y1 = d.Y[y].p; dn.DY1 = d.DY[y].p;
        dn.n = n - 1; dn.a0 = a0 ^ 6; dn.a6 = a0;
        hipLaunchKernelGGL(k_tan_dense, grid, dim3(256), 0, st, c, dn);
        ++launches;
      }
    }
    y ^= 1;
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(h->ev1, st));
  std::vector<double> f_host(nfield), fd_host(nfield);
  HIP_OK(hipMemcpyAsync(f_host.data(), d.fields.p, sizeof(double) * nfield, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(fd_host.data(), d.fields_dot.p, sizeof(double) * nfield, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  float ms = 0.0f;
  HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (fields) memcpy(fields, f_host.data(), sizeof(double) * nfield);
  if (fields_dot) memcpy(fields_dot, fd_host.data(), sizeof(double) * nfield);
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->steps = Nmax; stats->rhs_evals = Nmax * S + 1; stats->launches = launches; stats->kernel_ms = ms;
    stats->stage_kernel_us = Nmax ? 1e3 * ms / (double)(Nmax * S + 1) : 0.0;
    stats->streams = 1;
  }
  if (!all_finite(f_host) || !all_finite(fd_host)) { h->err = "forward_tangent_dense: non-finite state or tangent"; return 3; }
  return 0;
}
