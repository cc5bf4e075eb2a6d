// dfx_persist.hip -- the persistent stage-loop kernels of libdfx (dfx_persist.h), a translation unit of their own: see
// dfx_persist_api.h for why.  No host logic here beyond handing out kernel addresses.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "dfx_dispatch.h"
#include "dfx_kernels.h"
#include "dfx_persist.h"

namespace dfx_persist {

const void* fwd_kernel(int model, int contact, int npb) {
  const void* fn = nullptr;
  with_physics<loop_physics>(model, contact, [&](auto M, auto C) { fn = npb == 3 ? (const void*)k_fwd_persist<M(), C(), 3> : (const void*)k_fwd_persist<M(), C(), 4>; });
  return fn;
}
const void* adj_kernel(int model, int contact, int npb) {
  const void* fn = nullptr;
  with_physics<loop_physics>(model, contact, [&](auto M, auto C) { fn = npb == 3 ? (const void*)k_adj_persist<M(), C(), 3> : (const void*)k_adj_persist<M(), C(), 4>; });
  return fn;
}
void launch_ring_poison(hipStream_t st, double* ring, int batch, int n_blocks, int m0, int nm, int width) {
  const int per_member = n_blocks * width;
  hipLaunchKernelGGL(k_ring_poison, dim3((per_member + kThreads - 1) / kThreads, nm), dim3(kThreads), 0, st, ring, batch, n_blocks, m0, width, kPAhead);
}

}  // namespace dfx_persist
