// dfx_dispatch.h -- from the run-time bond model and contact model (Plan::model, Plan::contact) to the template arguments of a kernel: the one
// place where that switch is written out.  Host only, plain C++17.
//   with_physics<loop_physics>(model, contact, [&](auto M, auto C) { launch(k<M(), C()>); });
// calls the function with the pair as two std::integral_constant values and returns true; a pair the predicate excludes is neither
// instantiated nor called, and the call returns false.
#pragma once
#include <type_traits>

#include "dfx_physics.h"

namespace dfx {

template <int V>
using int_c = std::integral_constant<int, V>;

// which (model, contact) pairs a site serves.  contact: 0 none, 1 angle-based, 2 distance-based (DFX_CONTACT_*, include/dfx.h)
constexpr bool all_physics(int, int) { return true; }
// what the per-stage builds, the persistent loops and the kept adaptive solve exist for: the two ligament models, no distance contact
constexpr bool loop_physics(int model, int contact) { return (model == kNonlinear || model == kLinearized) && contact != 2; }

template <bool (*Served)(int, int), int M, int C = 0, class F>
bool with_contact(int contact, F& f) {
  if constexpr (C <= 2) {
    if (contact != C) return with_contact<Served, M, C + 1>(contact, f);
    if constexpr (Served(M, C)) { f(int_c<M>{}, int_c<C>{}); return true; }
  }
  return false;
}
template <bool (*Served)(int, int), class F>
bool with_physics(int model, int contact, F&& f) {
  switch (model) {
    case kNonlinear: return with_contact<Served, kNonlinear>(contact, f);
    case kLinearized: return with_contact<Served, kLinearized>(contact, f);
    case kSimpleSpring: return with_contact<Served, kSimpleSpring>(contact, f);
    case kStretchTorsion: return with_contact<Served, kStretchTorsion>(contact, f);
  }
  return false;
}

// the same for an index 0 <= i < N (the stage index of the per-stage builds): f(int_c<i>{}); false: out of range
template <int N, int I = 0, class F>
bool with_index(int i, F&& f) {
  if constexpr (I < N) {
    if (i == I) { f(int_c<I>{}); return true; }
    return with_index<N, I + 1>(i, f);
  }
  return false;
}

}  // namespace dfx
