// qn_linearize_debug.hip - the kernels of qn_debug_linearize (include/qn_engine.h): what stands between a correspondence and the 6 x 6 system the solver gets,
// called directly on the caller's inputs.  accumulate_point_n (qn_linearize.cuh) one correspondence per lane; emit_point with pose_gram and fold7 (qn_tick.cuh) in a
// block shaped like AccumulateK::run's - the poses, G = R R^T, the transpose buffers and the wave rows in LDS of the sizes that kernel gives them, `first` true on
// the first trip only, the waves summed in wave order; reduce_rows (qn_gicp_kernels.cuh) in all four instantiations.  A translation unit of its own: the product
// kernels are compiled without a line of this.  Test infrastructure (tests/test_gpu_linearize.py): nothing on the registration path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qn_tick.cuh"

namespace qn {

#define QN_LIN_POINT 37                                              // which 0, per correspondence: Rx (12), Tx (12), pa (3), pb (3), na (3), nb (3), lin
#define QN_LIN_HEAD 25                                               // which 1, per block: Rx (12), Tx (12), lin
#define QN_LIN_LANE 13                                               // which 1, per trip and lane: have, pa (3), pb (3), na (3), nb (3)

static __global__ void __launch_bounds__(QN_BLOCK) k_debug_accumulate_point(const double* __restrict__ in, uint32_t n, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * QN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double* r = in + QN_LIN_POINT * (size_t)i;
  double Rx[3][4], Tx[3][4];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) { Rx[a][b] = r[4 * a + b]; Tx[a][b] = r[12 + 4 * a + b]; }
  const float4 pa = make_float4((float)r[24], (float)r[25], (float)r[26], 1.f), pb = make_float4((float)r[27], (float)r[28], (float)r[29], 0.f);
  const double na[3] = {r[30], r[31], r[32]}, nb[3] = {r[33], r[34], r[35]};
  double acc[QN_NPART];
#pragma unroll
  for (int u = 0; u < QN_NPART; u++) acc[u] = 0;
  accumulate_point_n(Rx, Tx, pa, pb, na, nb, r[36] != 0.0, acc);
#pragma unroll
  for (int u = 0; u < QN_NPART; u++) out[QN_NPART * (size_t)i + u] = acc[u];
}

// one block of the grid per caller block; out per block: the four wave rows as emit_point left them, then their sum in wave order
static __global__ void __launch_bounds__(QN_BLOCK) k_debug_emit_point(const double* __restrict__ in, int trips, double* __restrict__ out) {
  __shared__ double red[QN_BLOCK / 64][7 * 64];                      // (AccumulateK::run's sizes)
  __shared__ double wsum[QN_BLOCK / 64][QN_NPART];
  __shared__ double sRx[12], sTx[12], sG[9];
  const int tid = threadIdx.x;
  const double* blk = in + (size_t)blockIdx.x * (QN_LIN_HEAD + (size_t)trips * QN_BLOCK * QN_LIN_LANE);
  if (tid < 12) { sRx[tid] = blk[tid]; sTx[tid] = blk[12 + tid]; }
  __syncthreads();
  pose_gram(sRx, sG, tid);
  __syncthreads();
  const bool lin = blk[24] != 0.0;
  bool first = true;
  for (int t = 0; t < trips; t++, first = false) {                   // (block-uniform trip count)
    const double* r = blk + QN_LIN_HEAD + ((size_t)t * QN_BLOCK + tid) * QN_LIN_LANE;
    const bool have = r[0] != 0.0;
    const float4 pa = make_float4((float)r[1], (float)r[2], (float)r[3], 1.f), pb = make_float4((float)r[4], (float)r[5], (float)r[6], 0.f);
    const double na[3] = {r[7], r[8], r[9]}, nb[3] = {r[10], r[11], r[12]};      // handed over as they are: a lane without a correspondence may hold anything
    wave_lds_fence();
    emit_point(have, lin, first, sRx, sTx, sG, pa, pb, na, nb, red[tid >> 6], wsum[tid >> 6]);
  }
  __syncthreads();
  double* o = out + (size_t)blockIdx.x * 5 * QN_NPART;
  if (tid < (QN_BLOCK / 64) * QN_NPART) o[tid] = (&wsum[0][0])[tid];
  if (tid < QN_NPART) { double v = 0;
#pragma unroll
    for (int w = 0; w < QN_BLOCK / 64; w++) v += wsum[w][tid];
    o[(QN_BLOCK / 64) * QN_NPART + tid] = v; }
}

// one block.  The rows were copied in by the host before the launch: a launch makes them visible to every load of the kernel, the agent-scope ones of
// COHERENT included (those exist for rows that other blocks of the SAME launch wrote).
template <int NT, bool COHERENT>
static __global__ void __launch_bounds__(NT) k_debug_reduce_rows(const double* __restrict__ rows, int n, double* __restrict__ out) {
  __shared__ double part[QN_NPART][QN_ROW_SEGS + 1];
  __shared__ double sums[QN_NPART];
  reduce_rows<NT, COHERENT>(rows, n, part, sums);
  if (threadIdx.x < QN_NPART) out[threadIdx.x] = sums[threadIdx.x];
}

// launched for qn_debug_linearize (qn_engine.hip, which has validated which, n and arg) on its stream; in / out are device pointers
hipError_t debug_launch_linearize(int which, const double* in, uint32_t n, uint32_t arg, double* out, hipStream_t stream) {
  if (which == 0) hipLaunchKernelGGL(k_debug_accumulate_point, dim3((n + QN_BLOCK - 1) / QN_BLOCK), dim3(QN_BLOCK), 0, stream, in, n, out);
  else if (which == 1) hipLaunchKernelGGL(k_debug_emit_point, dim3(n), dim3(QN_BLOCK), 0, stream, in, (int)arg, out);
  else if (arg == 256) hipLaunchKernelGGL((k_debug_reduce_rows<256, false>), dim3(1), dim3(256), 0, stream, in, (int)n, out);
  else if (arg == 257) hipLaunchKernelGGL((k_debug_reduce_rows<256, true>), dim3(1), dim3(256), 0, stream, in, (int)n, out);
  else if (arg == 512) hipLaunchKernelGGL((k_debug_reduce_rows<512, false>), dim3(1), dim3(512), 0, stream, in, (int)n, out);
  else hipLaunchKernelGGL((k_debug_reduce_rows<512, true>), dim3(1), dim3(512), 0, stream, in, (int)n, out);
  return hipGetLastError();
}

}  // namespace qn
