// qn_map_compact.cuh - what the units around the map slot share on the device besides the cell walk (qn_mapoutliers.hip with qn_mapclusters.inc, qn_mapground.hip,
// qn_staticmap.hip with qn_mapoccupancy.inc, qn_mapdistance.inc, qn_maproute.inc and qn_mapfrontier.inc, qn_verify.hip with qn_maplocalize.inc); the lock-free
// union-find of the clusters and the frontiers is qn_union_find.cuh, what the fields over the dense occupancy grid share - geometry, tile, lists - qn_dense_grid.cuh:
//   waves     wave_sum, wave_min, wave_max: a value folded over the 64 lanes by shuffles, lane 0 holds the result (int, u32, u64; f32 by fminf / fmaxf);
//             wave_each_key: a callable run once per distinct key the lanes of a wave hold - the key, its first lane and the ballot of the lanes that share it -
//             so that a wave folds its lanes of one key first and issues one set of atomics for them (k_mf_flatten, k_mf_relabel, k_mf_costs).
//   counts    block_count: the lanes of a block for which each of up to five predicates holds, by ballot and popcount; block_sum, block_max: up to three values
//             a lane folded over the block.  Each has one word per wave in LDS and a barrier of its own and writes the block's own slot; k_slot_fold (one
//             block) adds the slots up, k_slot_max takes the largest.  No atomics: integer sums and extremes, the same on every run.  Three kernels whose calls
//             measured slower with a fold's own barrier (k_md_axis<true> and k_mr_stats through dg_block_stats of qn_dense_grid.cuh, k_mg_extent) keep their wave
//             results in words of their own behind block_count's barrier, and say so where they do (profiles/EXPERIMENTS.md has the figures).
//   scan      scan_row: the exclusive scan of a row of per-block counts in one block; k_scan_rows, a block per row, is the kernel over it (one row: a filter's
//             or a list's counts, the last word the total; a row per centre, in place: the crop), k_static_scan (qn_staticmap.hip) the one with a tail of its own.
//   rank      lane_rank: a lane's place among the lanes of its wave for which a predicate holds, by ballot and popcount; block_rank: its place in the block, the
//             waves' counts through LDS, on top of the block's offset from the scan - where a stable compaction puts the lane's record: the same on every run.
//             The kernels with one predicate call block_rank and write their own payload there (k_mo_compact, k_mc_pick, k_mc_root_label, k_mf_pick,
//             k_dg_list_pick of qn_dense_grid.cuh for the two voxel lists);
//             those with a table of their own (k_static_compact: rounds, k_ml_compact: centres) take lane_rank for the last term.
//   compact   the order-preserving compaction of the slot's records: a unit's own flag kernel writes one removed byte per record and the kept count of every
//             MO_BLOCK records (block_count), k_scan_rows turns the counts into offsets, k_mo_compact moves a block's kept records to its offset, in order;
//             qn_kf_map_compact_shrink makes the kept records the slot.  Templates on the record type: instantiated only in the units that filter the slot, so a
//             unit that only counts, scans or lists carries no copy of the compaction kernel.
// Tested directly: tests/test_gpu_map_prims.py runs the folds, the key walk, the slot folds, the scan and the rank on inputs no unit can produce, through
// qn_kf_debug_map_prims (qn_map_selftest.hip), against the serial references of tests/map_prims_cases.py; tests/test_gpu_compact_seams.py has the seams of the
// scan and the rank through the units.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "qn_kf_buf.h"

#define MO_BLOCK 256
#define MO_WAVES (MO_BLOCK / 64)
#define MO_SCAN_BLOCK 1024

namespace {

struct op_sum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct op_min {
  template <typename T> __device__ T operator()(T a, T b) const { return min(a, b); }
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct op_max {
  template <typename T> __device__ T operator()(T a, T b) const { return max(a, b); }
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// v folded over the wave (all 64 lanes here): lane 0 holds the result
template <typename T, typename F> __device__ __forceinline__ T wave_fold(T v, F f) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_down(v, o));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_fold(v, op_sum()); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_fold(v, op_min()); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_fold(v, op_max()); }

// f(key, lead, same) once per distinct key among the lanes of the wave (all 64 here) for which has holds: lead the first lane that holds the key, same the
// ballot of the lanes that do.  The loop is uniform over the wave, so f may shuffle and ballot
template <typename K, typename F> __device__ __forceinline__ void wave_each_key(bool has, K key, F f) {
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const K k0 = __shfl(key, lead);
    const unsigned long long same = __ballot(has && key == k0);
    f(k0, lead, same);
    todo &= ~same;
  }
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

// dst[j] = the j-th value (one to three of type T) folded by f over the lanes of this block (MO_BLOCK threads, all of them here), behind a barrier of its own.
// The words belong to the instantiation (F, T, the number of values), like block_count's: a kernel that calls the same one twice puts a __syncthreads() between
// the calls, as k_mc_number does for block_count - the second call's writes would otherwise race with the first one's reads
template <typename F, typename T, typename... V> __device__ __forceinline__ void block_fold(F f, T* __restrict__ dst, V... vals) {
  constexpr int K = sizeof...(V);
  static_assert(K >= 1 && K <= 3, "one to three values");
  __shared__ T wk[K][MO_WAVES];
  const T val[K] = {(T)vals...};
#pragma unroll
  for (int j = 0; j < K; j++) {
    const T v = wave_fold(val[j], f);
    if ((threadIdx.x & 63) == 0) wk[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    T acc = wk[threadIdx.x][0];
    for (int w = 1; w < MO_WAVES; w++) acc = f(acc, wk[threadIdx.x][w]);
    dst[threadIdx.x] = acc;
  }
}
template <typename T, typename... V> __device__ __forceinline__ void block_sum(T* __restrict__ dst, V... vals) { block_fold(op_sum(), dst, vals...); }
template <typename T, typename... V> __device__ __forceinline__ void block_max(T* __restrict__ dst, V... vals) { block_fold(op_max(), dst, vals...); }

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

// one block: out[0] = the largest of the nb slots (0 without one); a template, like k_slot_fold, so that only a unit that launches it carries it
template <typename W> __global__ void __launch_bounds__(MO_SCAN_BLOCK) k_slot_max(const W* __restrict__ slots, uint32_t nb, W* __restrict__ out) {
  __shared__ W ws[MO_SCAN_BLOCK / 64];
  W m = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += MO_SCAN_BLOCK) m = max(m, slots[b]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    W top = 0;
    for (int w = 0; w < MO_SCAN_BLOCK / 64; w++) top = max(top, ws[w]);
    out[0] = top;
  }
}

// the set ballot bits below the calling lane: its rank among the lanes of its wave for which the predicate holds
__device__ __forceinline__ uint32_t lane_rank(unsigned long long bal) {
  const uint32_t lane = threadIdx.x & 63;
  return (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

// base + the lanes of this block (MO_BLOCK threads, all of them here) before the calling one for which keep holds: where a stable compaction puts the lane's record
__device__ __forceinline__ uint32_t block_rank(bool keep, uint32_t base) {
  __shared__ uint32_t wk[MO_WAVES];
  const uint32_t wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wk[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
#pragma unroll
  for (int w = 0; w < MO_WAVES; w++) if ((uint32_t)w < wave) base += wk[w];
  return base + lane_rank(bal);
}

// One block (MO_SCAN_BLOCK threads, all of them here): off[t] = the sum of cnt[0 .. t), t < nb.  Thread i scans the range [i chunk, (i + 1) chunk), the threads'
// sums go through a wave scan and the waves in order.  cnt == off is allowed: a thread rewrites only the entries it summed.  Returns the sum up to the end of the
// calling thread's range: in the last thread - its range ends at nb, empty or not - the sum of the row.
__device__ __forceinline__ uint32_t scan_row(const uint32_t* cnt, uint32_t nb, uint32_t* off) {
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
  for (uint32_t t = a; t < b; t++) { const uint32_t u = cnt[t]; off[t] = run; run += u; }
  return run;
}

// block r: row r of cnt (the rows nb apart) to its exclusive offsets in off, tot[r] = the row's sum.  One row with tot = off + nb: off[nb] is the total
__global__ void __launch_bounds__(MO_SCAN_BLOCK) k_scan_rows(const uint32_t* cnt, uint32_t nb, uint32_t* off, uint32_t* tot) {
  const uint32_t run = scan_row(cnt + (size_t)blockIdx.x * nb, nb, off + (size_t)blockIdx.x * nb);
  if (threadIdx.x == MO_SCAN_BLOCK - 1) tot[blockIdx.x] = run;
}

// the block's kept records, in order, to kept[off[block] ..].  A template, like the call below, so that only a unit that filters the slot carries the kernel.
template <typename R>
__global__ void __launch_bounds__(MO_BLOCK) k_mo_compact(uint32_t n, const R* __restrict__ map, const uint8_t* __restrict__ removed, const uint32_t* __restrict__ off,
                                                         R* __restrict__ kept) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool keep = i < n && removed[i] == 0;
  const R p = keep ? map[i] : R();
  const uint32_t j = block_rank(keep, off[blockIdx.x]);
  if (keep) kept[j] = p;
}

// The common end of the calls that filter the map slot: the `kept` records whose removed byte is 0, compacted by the offsets of k_scan_rows into d_kept (scratch),
// become the slot.  From the shrink on the slot has changed: its generation advances, so every result computed from it - normals, an outlier classification,
// the ground - is stale.
template <typename R>
int qn_kf_map_compact_shrink(qn_kf_store* s, const R* map, uint32_t n, const uint8_t* d_removed, const uint32_t* d_off, R* d_kept, uint32_t kept,
                             const float** d_xyzi_out, uint32_t* n_out) {
  hipStream_t stream = qn_kf_int_stream(s);
  hipLaunchKernelGGL(k_mo_compact<R>, dim3((n + MO_BLOCK - 1) / MO_BLOCK), dim3(MO_BLOCK), 0, stream, n, map, d_removed, d_off, d_kept);
  QN_KFCHK(s, hipGetLastError());
  const int rc = qn_kf_int_map_shrink(s, d_kept, kept);
  if (rc != QN_OK) return rc;
  QN_KFCHK(s, hipStreamSynchronize(stream));
  uint64_t gen = 0;
  *d_xyzi_out = (const float*)qn_kf_int_map(s, n_out, &gen);
  return QN_OK;
}

}  // namespace
