// qn_map_compact.cuh - what the units around the map slot share on the device besides the cell walk (qn_mapoutliers.hip, qn_mapground.hip):
//   counts    block_count: the lanes of a block for which each of up to five predicates holds, by ballot and popcount, one word per wave in LDS, into the
//             block's own slot; k_slot_fold (one block) adds the slots up.  No atomics: integer sums, the same on every run.
//   compact   the order-preserving compaction of the slot's records: a unit's own flag kernel writes one removed byte per record and the kept count of every
//             MO_BLOCK records (block_count); k_mo_scan (one block) turns the counts into offsets, the last one the number kept; k_mo_compact moves a block's
//             kept records to its offset, in order, by ballot / popcount ranks and the waves' counts through LDS - the static map's scheme: stable and the
//             same on every run; qn_kf_map_compact_shrink makes the kept records the slot.
// A unit that counts but never filters the map slot (qn_mapoccupancy.inc in qn_staticmap.hip) defines QN_MAP_COUNTS_ONLY first and gets the counts alone, so it
// carries no copy of the compaction kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "qn_kf_buf.h"

#define MO_BLOCK 256
#define MO_WAVES (MO_BLOCK / 64)
#define MO_SCAN_BLOCK 1024

namespace {

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                              // (lane 0 holds the wave's sum)
}

// dst[j] = the number of lanes of this block (MO_BLOCK threads, all of them here) whose j-th predicate holds
template <typename... B> __device__ __forceinline__ void block_count(uint32_t* __restrict__ dst, B... preds) {
  constexpr int K = sizeof...(B);
  static_assert(K >= 1 && K <= 5, "one to five counts");
  __shared__ uint32_t wk[K][MO_WAVES];
  const bool pred[K] = {preds...};
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint32_t c = (uint32_t)__popcll(__ballot(pred[j]));
    if ((threadIdx.x & 63) == 0) wk[j][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    uint32_t acc = 0;
    for (int w = 0; w < MO_WAVES; w++) acc += wk[threadIdx.x][w];
    dst[threadIdx.x] = acc;
  }
}

// one block: out[j] = the sum over the nb blocks of slots[K b + j], j < K
template <typename W, int K>
__global__ void __launch_bounds__(MO_SCAN_BLOCK) k_slot_fold(const W* __restrict__ slots, uint32_t nb, W* __restrict__ out) {
  __shared__ W ws[K][MO_SCAN_BLOCK / 64];
  W a[K];
#pragma unroll
  for (int j = 0; j < K; j++) a[j] = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += MO_SCAN_BLOCK) {
#pragma unroll
    for (int j = 0; j < K; j++) a[j] += slots[K * (size_t)b + j];
  }
#pragma unroll
  for (int j = 0; j < K; j++) {
    const W v = wave_sum(a[j]);
    if ((threadIdx.x & 63) == 0) ws[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    W acc = 0;
    for (int w = 0; w < MO_SCAN_BLOCK / 64; w++) acc += ws[threadIdx.x][w];
    out[threadIdx.x] = acc;
  }
}

#ifndef QN_MAP_COUNTS_ONLY
// one block: off[b] = the kept records of the blocks before b, off[nb] = all of them (k_static_scan's scheme: thread i scans the blocks
// [i chunk, (i + 1) chunk), the threads' sums through a wave scan and the waves in order)
__global__ void __launch_bounds__(MO_SCAN_BLOCK) k_mo_scan(const uint32_t* __restrict__ cnt, uint32_t nb, uint32_t* __restrict__ off) {
  __shared__ uint32_t ws[MO_SCAN_BLOCK / 64];
  const uint32_t chunk = (nb + MO_SCAN_BLOCK - 1) / MO_SCAN_BLOCK;
  const uint32_t a = min(threadIdx.x * chunk, nb), b = min(a + chunk, nb);
  uint32_t sum = 0;
  for (uint32_t t = a; t < b; t++) sum += cnt[t];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t v = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(v, o); if ((int)lane >= o) v += u; }
  if (lane == 63) ws[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int w = 0; w < MO_SCAN_BLOCK / 64; w++) { const uint32_t u = ws[w]; ws[w] = acc; acc += u; }
  }
  __syncthreads();
  uint32_t run = ws[wv] + v - sum;
  for (uint32_t t = a; t < b; t++) { off[t] = run; run += cnt[t]; }
  if (threadIdx.x == MO_SCAN_BLOCK - 1) off[nb] = run;              // the last thread's range ends at nb
}

// the block's kept records, in order, to kept[off[block] ..]
__global__ void __launch_bounds__(MO_BLOCK) k_mo_compact(uint32_t n, const float4* __restrict__ map, const uint8_t* __restrict__ removed, const uint32_t* __restrict__ off,
                                                         float4* __restrict__ kept) {
  __shared__ uint32_t wk[MO_WAVES];
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool keep = i < n && removed[i] == 0;
  const float4 p = keep ? map[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wk[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = off[blockIdx.x];
#pragma unroll
  for (int w = 0; w < MO_WAVES; w++) if ((uint32_t)w < wave) before += wk[w];
  if (keep) kept[before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = p;
}

// The common end of the calls that filter the map slot: the `kept` records whose removed byte is 0, compacted by the offsets of k_mo_scan into d_kept (scratch),
// become the slot.  From the shrink on the slot has changed: its generation advances, so every result computed from it - normals, an outlier classification,
// the ground - is stale.
inline int qn_kf_map_compact_shrink(qn_kf_store* s, const float4* map, uint32_t n, const uint8_t* d_removed, const uint32_t* d_off, float4* d_kept, uint32_t kept,
                                    const float** d_xyzi_out, uint32_t* n_out) {
  hipStream_t stream = qn_kf_int_stream(s);
  hipLaunchKernelGGL(k_mo_compact, dim3((n + MO_BLOCK - 1) / MO_BLOCK), dim3(MO_BLOCK), 0, stream, n, map, d_removed, d_off, d_kept);
  QN_KFCHK(s, hipGetLastError());
  const int rc = qn_kf_int_map_shrink(s, d_kept, kept);
  if (rc != QN_OK) return rc;
  QN_KFCHK(s, hipStreamSynchronize(stream));
  uint64_t gen = 0;
  *d_xyzi_out = (const float*)qn_kf_int_map(s, n_out, &gen);
  return QN_OK;
}
#endif  // QN_MAP_COUNTS_ONLY

}  // namespace
