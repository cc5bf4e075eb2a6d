// stage_builds_adj.hip -- the per-stage builds of the reverse stage kernel (k_adj_stage<..., ISTAGE>: the launches that fill the chip, 2/3 of
// a C3 step), a translation unit of their own so that they can be compiled for what they are: kernels bound by the ISSUE of their ~300 fp64
// instructions per lane at four waves per SIMD.  Makefile: -mllvm -amdgpu-sched-strategy=max-ilp and DFX_ADJ_OCC = waves_per_eu(4) for this
// file only -- together 3 % on the launch (profiles/r05_reverse_stage_schedule.txt); the same strategy costs the forward kernel 6 %, and alone
// (without the occupancy pin) it costs this one 5 %.  It also takes these kernels out of a lottery: in the big translation unit their schedule
// depended on which OTHER kernels were compiled next to them (round 5's library split lost 3 % on them without touching a line of theirs).
// No host logic beyond the launch switch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "dfx_builds.h"
#include "dfx_kernels.h"

namespace dfx_hot {

// the launch switch: the caller has selected a per-stage build (select_adj_build, dfx_builds.h), so the build exists
void launch_adj_stage_build(int model, int contact, int npb, hipStream_t st, dim3 grid, const DevCtx& c, const AdjCoef& acf, int i, int j, int in_buf, int wbuf,
                            int local_only, const StageCoef& rc, int rb) {
  auto go = [&](auto* k) { hipLaunchKernelGGL(k, grid, dim3(kThreads), 0, st, c, acf, i, j, in_buf, wbuf, local_only, rc, rb); };
  with_physics<loop_physics>(model, contact, [&](auto M, auto C) {
    auto stage_build = [&](auto NPB) { with_index<kStageBuilds>(i, [&](auto I) { go(k_adj_stage<M(), C(), 0, 0, NPB(), 1, 0, 1, I()>); }); };
    npb == 3 ? stage_build(int_c<3>{}) : stage_build(int_c<4>{});
  });
}

}  // namespace dfx_hot
