// dfx_builds.h -- which build of the two stage kernels (k_fwd_stage, k_adj_stage: dfx_kernels.h) a stage launch takes: the rule, as pure
// functions of a BuildQuery.  No HIP, no handle: plain C++17, so a host program can print the table (tests/test_stage_build_select.py).
// engine_launch.hip fills the query (build_query), selects, and instantiates what was selected; what dfx_stats.tile_kernels reports
// (build_code) is derived from the same selection.
#pragma once
#include "dfx_dispatch.h"

namespace dfx {
struct BuildQuery {
  int model, contact;           // Plan::model, Plan::contact
  int n_npb, n_ovf, s;          // nodes per block, ligaments beyond one per node (general bond lists), stages of the tableau
  bool pack3;                   // 3-node blocks take the packed mapping: five triangles per 16 lanes (pack3(), engine_launch.hip)
  bool wt, stage_builds;        // dfx_handle::wt (write-through table builds), dfx_handle::stage_builds
  // the common parameter shape the per-stage builds compile in: uniform stiffnesses and damping, the reference-vector dictionary in LDS,
  // equal steps, no stage checkpoint, no adaptive clock
  bool k_uniform, l_dict_on, l_dict_lds, damping_uniform, t_steps, AD, clock;
  bool records;                 // the stage records live in the trajectory checkpoint (DevCtx::rps > 1)
  bool fn_tab, g_b;             // the segment's time-function table is there; per-ligament gradients are wanted
  bool trace = false;           // the drive cotangent is kept per stage (dfx_fn_table_grads)
};
constexpr int kStageBuilds = 6;       // per-stage builds exist for the stages 0 .. 5

// npb == 0: nothing is launched (general bond lists have no distance-based contact)
struct FwdBuild {
  int npb, tab, ovf, wt;        // template arguments NPB, TAB, OVF, WT of k_fwd_stage
  int istage, recs;             // ISTAGE (-1: the generic build) and, for a per-stage build, RECS
  bool packed_grid;             // the grid of the packed mapping (DevCtx::n_wg3), else the slot grid
};
enum AdjKind { kAdjGeneric, kAdjBondGrads, kAdjRebuild, kAdjOvf, kAdjTrace };
struct AdjBuild {
  AdjKind kind;       // generic: k_adj_stage<M, C, 0, 0, NPB, TAB, 0, WT, ISTAGE>; bond_grads: <M, C, 1, 1>; rebuild: k_adj_stage_rb; ovf: <M, C, 1, 1, 4, 0, 1>;
                      // trace: k_adj_stage_trace<M, C> (the bond_grads build + the drive-cotangent trace)
  int npb, tab, wt, istage;
  bool packed_grid;
};

// the per-stage builds (stage index, common parameter shape and -- forward, where the records live in the checkpoint -- the buffer
// arguments as compile-time constants) of the write-through table kernels
inline bool stage_build_ok(const BuildQuery& q, int i) {
  const bool shape = q.k_uniform && q.l_dict_on && q.l_dict_lds && q.damping_uniform && !q.t_steps;
  return loop_physics(q.model, q.contact) && q.wt && q.stage_builds && shape && i >= 0 && i < kStageBuilds;
}

inline FwdBuild select_fwd_build(const BuildQuery& q, int i, int in_buf, int out_buf, int y_buf, int mode) {
  // general bond lists: the build that walks a node's extra ligaments (quad mapping, in-kernel time functions)
  if (q.n_ovf) return {q.contact != 2 ? 4 : 0, 0, 1, 0, -1, 1, false};
  const bool tab = q.fn_tab && !q.clock;          // the segment's time-function table is there: the build that reads it
  const bool packed = q.contact != 2 && q.pack3 && !(mode & 2);
  if (tab && (packed || q.wt)) {
    if (stage_build_ok(q, i) && !q.AD) {        // (a table means no adaptive clock)
      const bool recs = q.records && in_buf == -1 - i && out_buf == -2 - i && y_buf == -1 && mode == 0;
      return {packed ? 3 : 4, 1, 0, 1, i, recs ? 1 : 0, packed};
    }
    if (!packed) return {4, 1, 0, 1, -1, 1, false};
  }
  return {packed ? 3 : 4, tab ? 1 : 0, 0, 0, -1, 1, packed};
}

inline AdjBuild select_adj_build(const BuildQuery& q, int i, int local_only) {
  if (q.n_ovf) return {kAdjOvf, q.contact != 2 ? 4 : 0, 0, 0, -1, false};      // general bond lists: one build for every checkpoint level
  // sample gradients of a table drive: like per-ligament gradients, one build for every checkpoint level, off the per-stage builds (the
  // engine refuses the request on general bond lists before it launches; the single-stage hook keeps its build)
  if (q.trace && !local_only) return {kAdjTrace, 4, 0, 0, -1, false};
  if (q.g_b) return {kAdjBondGrads, 4, 0, 0, -1, false};
  if (q.AD) return {kAdjRebuild, 4, 0, 0, -1, false};
  const bool tab = q.fn_tab && !local_only;
  const bool packed = q.contact != 2 && q.pack3;
  if (tab && (packed || q.wt)) {
    if (stage_build_ok(q, i)) return {kAdjGeneric, packed ? 3 : 4, 1, 1, i, packed};      // (no stage checkpoint here, and no clock where there is a table)
    if (!packed) return {kAdjGeneric, 4, 1, 1, -1, false};
  }
  return {kAdjGeneric, packed ? 3 : 4, tab ? 1 : 0, 0, -1, packed};
}

// what dfx_stats.tile_kernels reports of the stage launches of a sweep: 2 if every stage of a step takes a per-stage build, else 0
inline int build_code(const BuildQuery& q, bool reverse) {
  for (int i = 0; i < q.s; ++i) {
    if (reverse) { const AdjBuild b = select_adj_build(q, i, 0); if (b.kind != kAdjGeneric || b.istage < 0) return 0; }
    else if (select_fwd_build(q, i, 0, 0, 0, 0).istage < 0) return 0;
  }
  return 2;
}

}  // namespace dfx
