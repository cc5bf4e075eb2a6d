// dfx_persist_prio.h -- the issue priority (s_setprio, 0 .. 3) a wave of the persistent stage loops computes at: the rule, as one pure
// function.  No HIP, no handle: plain C++ (constexpr, so the kernels call it too), and a host program can print the table
// (tests/test_persist_prio_host.py).
//
// Why.  Where a launch puts two or three workgroups on a compute unit, the waves that share a SIMD belong to different members, and the
// members do not depend on each other.  At equal priority the SIMD issues for the oldest of its waves, and which member is the oldest
// differs from SIMD to SIMD; a member needs its neighbours' records at every stage, so it runs at the pace of its slowest wave and every
// member is paced as if it lost the arbitration everywhere.  A rank that is the same for every wave of a member, on every SIMD, gives
// the first member its solo pace chip-wide and the others the issue slots it leaves: they take turns instead of computing and
// waiting together.  The rank holds only while a wave computes; a wave that polls the ring is at priority 0 (dfx_persist.h), so a
// spinning wave never outranks a computing one.
//   mode      0: off (DFX_PERSIST_PRIO=0, engine_launch.hip); otherwise on
//   ml        the member's number inside the launch
//   per_cu    workgroups of the launch a compute unit holds (persist_shape)
//   xcd_wg    > 0: one member per XCD -- member 8 * mi + x sits on XCD x (persist_wave), so the members that can share a SIMD differ in mi
// A launch with one workgroup per compute unit has one wave per SIMD and nothing to arbitrate: 0.
#pragma once

namespace dfx_persist {

constexpr int persist_prio(int mode, int ml, int per_cu, int xcd_wg) {
  if (mode == 0 || per_cu < 2) return 0;
  const int ranks = per_cu < 4 ? per_cu : 4;
  const int r = xcd_wg > 0 ? (ml >> 3) : ml;
  return 3 - r % ranks;
}

}  // namespace dfx_persist
