// qn_map_compact.cuh - the order-preserving compaction of the map slot's records that the units filtering it share (qn_mapoutliers.hip,
// qn_mapground.hip): a unit's own flag kernel writes one removed byte per record and the kept count of every MO_BLOCK records; k_mo_scan (one block) turns
// the counts into offsets, the last one the number kept; k_mo_compact moves a block's kept records to its offset, in order, by ballot / popcount ranks and
// the waves' counts through LDS - the static map's scheme: stable and the same on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define MO_BLOCK 256
#define MO_WAVES (MO_BLOCK / 64)
#define MO_SCAN_BLOCK 1024

namespace {

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

}  // namespace
