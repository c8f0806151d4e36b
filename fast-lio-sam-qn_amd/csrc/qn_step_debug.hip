// qn_step_debug.hip - routine 1 of qn_debug_step_math: the pivoted 6 x 6 LDL' solve d_ldlt_solve6 (qn_step_math.cuh) called directly, one problem per lane.  The
// other routines' kernels are in qn_selftest.cuh, in the engine's translation unit; this one cannot be.  d_ldlt_solve6 is `inline`, not forced, and in that unit
// d_propose is its only caller: the compiler inlines it there as the last call of a local function.  A second direct caller in the same unit takes that away -
// the controller kernels (k_solve, k_accumulate, k_far_reduce and their k_lanes forms) then CALL the routine, 1100 instructions shorter each and no longer the
// code the registration results are pinned to.  Here it has one caller again.  Test infrastructure: nothing on the registration path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qn_step_math.cuh"

namespace qn {

#define QN_STEP_DEBUG_BLOCK 64
// in: A (36, full symmetric, row major), lambda, b (6) per problem -> out: x (6) of (A + lambda I) x = -b.  SolveWork per lane in LDS: 512 B x 64 = 32 KiB a block.
static __global__ void __launch_bounds__(QN_STEP_DEBUG_BLOCK) k_debug_ldlt_solve6(const double* __restrict__ in, uint32_t n, double* __restrict__ out) {
  __shared__ SolveWork work[QN_STEP_DEBUG_BLOCK];
  const uint32_t i = blockIdx.x * QN_STEP_DEBUG_BLOCK + threadIdx.x;
  if (i >= n) return;
  SolveWork* w = &work[threadIdx.x];
  const double* r = in + 43 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 6; k++) w->rhs[k] = -r[37 + k];
  d_ldlt_solve6(r, r[36], out + 6 * (size_t)i, w);
}

// launched for qn_debug_step_math (qn_engine.hip) on its stream; in / out are device pointers
hipError_t debug_launch_ldlt_solve6(const double* in, uint32_t n, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_debug_ldlt_solve6, dim3((n + QN_STEP_DEBUG_BLOCK - 1) / QN_STEP_DEBUG_BLOCK), dim3(QN_STEP_DEBUG_BLOCK), 0, stream, in, n, out);
  return hipGetLastError();
}

}  // namespace qn
