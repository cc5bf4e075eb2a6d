// engine_drive.hip -- libdfx host side: the samples of a table drive as a differentiable leaf -- per-member table values, the drive-cotangent
// trace around a reverse sweep and its reduction onto the samples (kernels: dfx_drive.h), per-direction sample tangents for forward mode
// (one of the translation units of dfx_engine.h; the design in DESIGN.md section 4)
#include "dfx_engine.h"
#include "dfx_drive.h"

static int table_fn(dfx_handle* h, const char* who, int32_t fn) {
  if (fn < 0 || fn >= h->pl.n_fns || h->pl.fn_type[fn] != DFX_FN_TABLE) {
    h->err = std::string(who) + ": time function " + std::to_string(fn) + " is not a table (DFX_FN_TABLE)";
    return 1;
  }
  return 0;
}

// TimeFn::tab of every member of the packed image: its own copy of the tables that have one (after pack_params, before the upload)
void patch_member_tables(dfx_handle* h) {
  const Plan& pl = h->pl;
  if (h->pp.fns.size() < (size_t)pl.batch * DFX_MAX_FNS) return;
  for (int f = 0; f < pl.n_fns; ++f) {
    if (!h->fn_table_member[f]) continue;
    const size_t n2 = pl.fn_table[f].size();
    for (int m = 0; m < pl.batch; ++m) h->pp.fns[(size_t)m * DFX_MAX_FNS + f].tab = h->d_fn_table_m[f].p + (size_t)m * n2;
  }
}

void release_drive_buffers(dfx_handle* h) {
  if (h->ev_red0) (void)hipEventDestroy(h->ev_red0);
  if (h->ev_red1) (void)hipEventDestroy(h->ev_red1);
  h->ev_red0 = h->ev_red1 = nullptr;
  h->d_gbar.release(); h->d_gtimes.release();
  for (int f = 0; f < DFX_MAX_FNS; ++f) { h->d_fn_table_m[f].release(); h->d_tab_grad[f].release(); h->d_tab_dots[f].release(); }
}

int dfx_fn_table_values(dfx_handle* h, int32_t fn, const double* values, int32_t per_member) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = table_fn(h, "fn_table_values", fn)) return rc;
  if (!values) { h->err = "fn_table_values: values is NULL"; return 1; }
  const Plan& pl = h->pl;
  const size_t B = pl.batch, n = pl.fn_table[fn].size() / 2;
  std::vector<double> img(B * 2 * n);
  for (size_t m = 0; m < B; ++m) {
    const double* y = values + (per_member ? m * n : 0);
    for (size_t j = 0; j < n; ++j) {
      if (!std::isfinite(y[j])) { h->err = "fn_table_values: a value is not finite"; return 1; }
      img[m * 2 * n + j] = pl.fn_table[fn][j];
      img[m * 2 * n + n + j] = y[j];
    }
  }
  HIP_OK(hipStreamSynchronize(h->stream));        // (nothing queued may still read the old values)
  HIP_OK(h->d_fn_table_m[fn].ensure(img.size()));
  HIP_OK(hipMemcpy(h->d_fn_table_m[fn].p, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
  h->fn_table_member[fn] = true;
  if (h->have_params) {
    patch_member_tables(h);
    HIP_OK(hipMemcpy(h->d_fns.p, h->pp.fns.data(), sizeof(TimeFn) * h->pp.fns.size(), hipMemcpyHostToDevice));
  }
  h->have_traj = false;
  h->have_fields = false;
  h->have_trace = false;
  return 0;
}

int dfx_fn_table_grads(dfx_handle* h, int32_t enable) {
  HIP_OK(hipSetDevice(h->device));
  if (enable) {       // what no sweep could serve is refused here, not at the next gradient call
    if (h->pl.n_fns == 0) { h->err = "fn_table_grads: the problem has no time function"; return 1; }
    if (h->pl.n_ovf) {
      h->err = "fn_table_grads: the drive-cotangent trace is not available on lattices whose nodes carry more than one ligament";
      return 1;
    }
  }
  h->table_grads = enable != 0;
  if (!h->table_grads) h->have_trace = false;
  return 0;
}

TraceCtx trace_ctx(const dfx_handle* h) { return TraceCtx{h->d_gbar.p, h->trace_rows}; }

int trace_begin(dfx_handle* h, long long rows) {
  h->have_trace = false;
  if (!h->table_grads) return 0;
  const Plan& pl = h->pl;
  if (pl.n_ovf) {
    h->err = "fn_table_grads: the drive-cotangent trace is not available on lattices whose nodes carry more than one ligament "
             "(dfx_fn_table_grads(h, 0) switches the request off)";
    return 1;
  }
  if (pl.n_fns == 0) { h->err = "fn_table_grads: the problem has no time function"; return 1; }
  const size_t n = (size_t)pl.batch * pl.n_fns * (size_t)rows * pl.tab.s;
  HIP_OK(h->d_gbar.ensure(n));
  HIP_OK(hipMemsetAsync(h->d_gbar.p, 0, sizeof(double) * n, h->stream));
  h->trace_rows = rows;
  return 0;
}

int trace_finish(dfx_handle* h, const DevCtx& c, const int* n_acc) {
  if (!h->table_grads) return 0;
  const Plan& pl = h->pl;
  const size_t B = pl.batch;
  const long long rows = h->trace_rows, n_stage = rows * pl.tab.s;
  HIP_OK(h->d_gtimes.ensure(B * (size_t)n_stage));
  // DFX_TIMING: the reduction's own device time (events around it, reported by trace_report once the sweep has been waited for)
  h->trace_timed = false;
  if (getenv("DFX_TIMING")) {
    if (!h->ev_red0) (void)hipEventCreate(&h->ev_red0);
    if (!h->ev_red1) (void)hipEventCreate(&h->ev_red1);
    h->trace_timed = h->ev_red0 && h->ev_red1 && hipEventRecord(h->ev_red0, h->stream) == hipSuccess;
  }
  if (!c.t_steps && h->segs.empty()) HIP_OK(hipMemsetAsync(h->d_gtimes.p, 0, sizeof(double) * B * (size_t)n_stage, h->stream));   // (no step at all)
  else {
    StageTimes tms;
    for (int r = 0; r < kFnRows; ++r) tms.c[r] = r <= pl.tab.s ? pl.tab.c[r] : 0.0;
    DevCtx ca = c;
    ca.m0 = 0;
    hipLaunchKernelGGL(k_stage_times, dim3((unsigned)((rows + 63) / 64), (unsigned)B), dim3(64), 0, h->stream, ca, tms, (const Seg*)h->d_segs.p,
                       (int)h->segs.size(), rows, (long long)(rows - 1), n_acc, h->d_gtimes.p);
    h->launches++;
  }
  for (int f = 0; f < pl.n_fns; ++f) {
    if (pl.fn_type[f] != DFX_FN_TABLE) continue;
    const size_t n = pl.fn_table[f].size() / 2;
    HIP_OK(h->d_tab_grad[f].ensure(B * n));
    hipLaunchKernelGGL(k_table_grad, dim3((unsigned)n, (unsigned)B), dim3(64), 0, h->stream, (const TimeFn*)h->d_fns.p, f, pl.n_fns,
                       (const double*)h->d_gbar.p, (const double*)h->d_gtimes.p, n_stage, h->d_tab_grad[f].p);
    h->launches++;
  }
  if (h->trace_timed) h->trace_timed = hipEventRecord(h->ev_red1, h->stream) == hipSuccess;
  h->have_trace = true;
  return 0;
}

void trace_report(dfx_handle* h) {
  if (!h->trace_timed) return;
  h->trace_timed = false;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev_red0, h->ev_red1) != hipSuccess) { (void)hipGetLastError(); return; }
  fprintf(stderr, "[dfx] table gradients: stage times + reduction of the drive cotangent onto the samples: %.1f us on the device\n", 1e3 * ms);
}

int dfx_fn_table_grad(dfx_handle* h, int32_t fn, double* grad) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = table_fn(h, "fn_table_grad", fn)) return rc;
  if (!h->have_trace) { h->err = "fn_table_grad: no reverse sweep has kept the drive cotangent (dfx_fn_table_grads(h, 1), then a gradient call)"; return 1; }
  if (!grad) { h->err = "fn_table_grad: grad is NULL"; return 1; }
  const size_t n = h->pl.fn_table[fn].size() / 2;
  HIP_OK(hipMemcpyAsync(grad, h->d_tab_grad[fn].p, sizeof(double) * h->pl.batch * n, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int dfx_drive_cotangent(dfx_handle* h, int32_t member, double* times, double* gbar, int64_t capacity, int64_t* n) {
  HIP_OK(hipSetDevice(h->device));
  if (!h->have_trace) { h->err = "drive_cotangent: no reverse sweep has kept the drive cotangent (dfx_fn_table_grads(h, 1), then a gradient call)"; return 1; }
  if (member < 0 || member >= h->pl.batch) { h->err = "drive_cotangent: no such member"; return 1; }
  if (!n || capacity < 0) { h->err = "drive_cotangent: bad arguments"; return 1; }
  const Plan& pl = h->pl;
  // the stage evaluations of the member's own sweep: every step of a fixed grid; its accepted steps and the evaluation at the final state
  long long steps = h->trace_rows - 1;
  if (h->adaptive_records && member < (int)h->accepted_per_member.size()) steps = std::min<long long>(steps, h->accepted_per_member[member] + 1);
  const long long n_stage = h->trace_rows * pl.tab.s, mine = steps * pl.tab.s;
  *n = mine;
  const long long cnt = std::min<long long>(mine, capacity);
  if (cnt > 0) {
    if (times) HIP_OK(hipMemcpyAsync(times, h->d_gtimes.p + (size_t)member * n_stage, sizeof(double) * cnt, hipMemcpyDeviceToHost, h->stream));
    if (gbar)
      for (int f = 0; f < pl.n_fns; ++f)
        HIP_OK(hipMemcpyAsync(gbar + (size_t)f * capacity, h->d_gbar.p + ((size_t)member * pl.n_fns + f) * n_stage, sizeof(double) * cnt,
                              hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int dfx_fn_table_tangents(dfx_handle* h, int32_t fn, const double* values_dots, int32_t n_dirs) {
  HIP_OK(hipSetDevice(h->device));
  if (int rc = table_fn(h, "fn_table_tangents", fn)) return rc;
  if (!values_dots) { h->tab_dots_n[fn] = 0; return 0; }
  if (n_dirs < 1) { h->err = "fn_table_tangents: need >= 1 direction"; return 1; }
  const size_t cnt = (size_t)n_dirs * h->pl.batch * (h->pl.fn_table[fn].size() / 2);
  for (size_t i = 0; i < cnt; ++i)
    if (!std::isfinite(values_dots[i])) { h->err = "fn_table_tangents: a tangent is not finite"; return 1; }
  HIP_OK(hipStreamSynchronize(h->stream));
  HIP_OK(h->d_tab_dots[fn].ensure(cnt));
  HIP_OK(hipMemcpy(h->d_tab_dots[fn].p, values_dots, sizeof(double) * cnt, hipMemcpyHostToDevice));
  h->tab_dots_n[fn] = n_dirs;
  return 0;
}
