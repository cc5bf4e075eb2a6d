// dfx_persist_dense.hip -- the adaptive controller inside the persistent stage loop and the reverse sweep of the steps it keeps
// (dfx_persist_dense.h), a translation unit of their own, compiled like dfx_persist.hip (no machine-level loop-invariant code motion:
// dfx_persist_api.h says why).  No host logic here beyond handing out kernel addresses.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "dfx_dispatch.h"
#include "dfx_kernels.h"
#include "dfx_persist_dense.h"

namespace dfx_persist {

const void* adaptive_fwd_kernel(int model, int contact) {
  const void* fn = nullptr;
  with_physics<loop_physics>(model, contact, [&](auto M, auto C) { fn = (const void*)k_adaptive_fwd_loop<M(), C()>; });
  return fn;
}
const void* adj_dense_kernel(int model, int contact, int npb) {
  const void* fn = nullptr;
  with_physics<loop_physics>(model, contact, [&](auto M, auto C) { fn = npb == 3 ? (const void*)k_adj_dense_loop<M(), C(), 3> : (const void*)k_adj_dense_loop<M(), C(), 4>; });
  return fn;
}

}  // namespace dfx_persist
