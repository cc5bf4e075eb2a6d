// dfx_persist_api.h -- what the engine's host code and the persistent kernels' translation unit (dfx_persist.hip) share.
// The persistent kernels are compiled on their own because they need one compiler switch the stage kernels must not get:
// -mllvm -disable-machine-licm.  Their stage loop is the first long loop around the ligament arithmetic, and the machine-level
// loop-invariant code motion hoists every fp64 literal of that arithmetic (the polynomial coefficients of atan2 / sincos, ~80
// registers of v_mov) out of it: 203 VGPRs and two waves per SIMD instead of 108 and four (profiles/r05_persistent_kernels.txt).
// (Included behind dfx_kernels.h: PersistCtx names dfx::Seg and dfx_special.)
#pragma once
#include <hip/hip_runtime.h>
#include "dfx_persist_prio.h"

namespace dfx_persist {

constexpr int kPRing = 8;      // places in the hand-off ring
constexpr int kPAhead = 4;     // a place is re-poisoned this many stage ordinals before its record is due
constexpr int kPersistThreads = 256;
constexpr unsigned kPoisonWord = 0xFFFFFFFFu;
constexpr int kPersistStages = 6;   // fixed-grid tableaus of the library: 4 (RK4) and 6 (Dormand-Prince)
constexpr int kSpinLimit = 1 << 23; // polls (>= 0.5 us each) before a wave gives up: seconds
// what the hand-off protocol leans on (dfx_persist.h): a place is re-poisoned kPAhead ordinals ahead of its record -- at least two, so that
// the store is complete (the owner's next poll waits for it) before a neighbour can ask -- and the ring is longer than that look-ahead
static_assert(kPAhead >= 2 && kPRing >= kPAhead + 1, "hand-off ring: re-poison at least two ordinals ahead, ring longer than the look-ahead");

struct PersistCoef {            // the whole tableau in acceleration form (host side: persist_fwd_tab cuts the loop's rows out of it)
  double cv[kPersistStages][kPersistStages];
  double cq[kPersistStages][kPersistStages];
  double c[kPersistStages + 1];
};
struct PersistArgs {
  double* ring;                 // kPRing * batch * n_blocks * kPos
  int* give_up;                 // pinned host word: != 0 once a wave gave up (1 + the stage ordinal it waited for)
  int n_steps, nm, waves_per_member;
  int spin_limit;               // polls before a wave gives up (kSpinLimit; the test hook dfx_test_set_spin_limit makes it tiny)
  int xcd_wg;                   // > 0: workgroups per member, every member on ONE XCD (workgroup b sits on XCD b % 8: persist_wave); 0: waves packed densely
  int prio;                     // member-ranked issue priority (dfx_persist_prio.h): 0: off, else the launch's workgroups per compute unit
#ifdef DFX_PERSIST_TIMING
  unsigned* dbg;                // diagnostic build: 8 words per wave (six phase sums, total ticks, stages)
#endif
};


// The reverse loop's coefficients as it consumes them: ONE row of 16 doubles per stage, fetched by one group of scalar loads at the top of
// the stage.  The structure of the sums is baked into the numbers: a later stage jj that does not enter stage i's sums (jj <= i, jj >= s)
// has coefficient 0 -- the loop reads every Ybar place (zeroed at the start of a launch, finite ever after) and multiplies, no selects;
// stage 0 takes the later stages' Ybar with weight 1 (the sum that enters lambda).
//   row[i] = { cf[1..5] | cur[1..5] | col[s] | cur[s] | col[i] | 0 0 0 },   cf[jj] = jj > i && jj < s ? (i > 0 ? col[i][jj] : 1) : 0
constexpr int kAdjRow = 16;
struct PersistAdjTab { double row[kPersistStages][kAdjRow]; };
// the forward loop's, likewise: an earlier stage l >= i has weight 0 (its acceleration's place holds a finite number from the start)
//   row[i] = { cv[i][0..4] | cq[i][0..4] | cv[i][i] | cq[i][i] | c[i+1] | 0 0 0 },   cv[i][l], cq[i][l] = 0 for l >= i
struct PersistFwdTab { double row[kPersistStages][kAdjRow]; };
static_assert((kPRing & (kPRing - 1)) == 0, "the ring place of a stage ordinal is taken with a mask");

// What the persistent loops (forward and reverse) read of the engine's context, built by the host per launch (engine_launch.hip, persist_ctx): every
// per-member array already points at the launch's first member, so the kernel indexes with the member's number inside the launch.
// DevCtx by value is ~80 fields; what the stage loop needs of it did not fit the scalar registers and was spilled to vector lanes and
// re-read, or re-loaded from the argument segment, at every stage (profiles/r14_persist_lean.txt).
struct PersistCtx {
  int n_blocks, n_slots, n_fns, batch, s, rps, n_special, m0;
  int k_uniform, damping_uniform, l_dict_on, nbuf;
  const int32_t* slot_info;
  const int32_t* block_special;
  const dfx_special* special;
  const double *p_r, *p_l, *p_k, *p_phi, *l_dict, *cst, *inv_m, *damping;
  const uint8_t* p_lidx;
  const double* fn_tab;
  const dfx::Seg* cur;
  const double* t_steps;
  long long ts_stride;
  double* traj;
  double *POS, *VEL, *AD;       // forward: stage buffers (buffer 0 = the step state), stage checkpoint or null
  long long ad_stride;
  double *LAM, *W;
  const double* G;
  double *g_r, *g_phi, *blk_m, *blk_c, *fn_g;
  int* touch;
};

// kernels by (bond model, contact, lanes per block); nullptr: no such build
const void* fwd_kernel(int model, int contact, int npb);
const void* adj_kernel(int model, int contact, int npb);
// the adaptive controller inside the stage loop and the reverse sweep of the steps it keeps (dfx_persist_dense.hip)
const void* adaptive_fwd_kernel(int model, int contact);
const void* adj_dense_kernel(int model, int contact, int npb);
// places 0 .. kPAhead-1 of the ring, members [m0, m0 + nm), poisoned on `st`
void launch_ring_poison(hipStream_t st, double* ring, int batch, int n_blocks, int m0, int nm, int width);

}  // namespace dfx_persist
