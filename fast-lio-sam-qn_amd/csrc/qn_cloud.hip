// qn_cloud.hip - the feeder of the hot path, on the GPU.  Own translation unit.
//   LoopClosure::setSrcAndDstCloud (fast_lio_sam_qn/src/loop_closure.cpp:58-108): per keyframe transformPcd
//   (include/utilities.hpp:164-175), concatenation, voxelizePcd = pcl::VoxelGrid (utilities.hpp:38-51);
//   LoopClosure::fetchClosestKeyframeIdx (loop_closure.cpp:34-56).
// Keyframe clouds (PosePcd::pcd_, sensor frame, immutable: include/pose_pcd.hpp:7-19) are uploaded ONCE into a store
// and stay resident in HBM; a loop attempt then assembles its source / target clouds on the device and hands the
// device pointers to qn_icp_alignment_device / the batch API - no point cloud crosses PCIe per attempt.
// VoxelGrid: 64-bit keys (leaf index << 32 | point index) are sorted by leaf index with a hand-written STABLE LSD radix
// sort (8-bit digits, only as many passes as the leaf grid has bits; the input is in ascending point order and stability
// keeps it so inside every leaf), leaf heads are compacted with the engine's own scan kernels and one thread per leaf sums
// its points in ascending point order in f32 - the order the oracle fixes (PCL's own order inside a leaf is unspecified).
// The corrected global map (qn_kf_build_map, fast_lio_sam_qn.cpp:302-316, 398-411, 435-448) reuses the store: every keyframe in one
// transform launch, intensity carried in .w, a radix sort with 4096-key tiles, its own output slot.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include <algorithm>
#include "../../include/qn_engine.h"
#include "qn_util_kernels.cuh"
#include "qn_kf_internal.h"

namespace qn {

__global__ void k_kf_transform(const float4* __restrict__ in, uint32_t n, const double* __restrict__ T, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i]; const double x = p.x, y = p.y, z = p.z;
  out[i] = make_float4((float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]), (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]),
                       (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]), 1.0f);
}
// pcl::VoxelGrid on a cloud that is not dense (utilities.hpp:38-51 -> pcl::VoxelGrid::applyFilter: `if (!input_->is_dense) if (!isXYZFinite(p)) continue;`,
// getMinMax3D skips them as well): non-finite points take no part - they are dropped by a stable compaction (flag, exclusive scan, scatter).
__global__ void k_finite_flags(const float4* __restrict__ pts, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  flag[i] = (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) ? 1u : 0u;
}
__global__ void k_compact_finite(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) out[pos[i]] = pts[i];
}
struct VoxelDims { float inv; int minb[3]; int div0, div01; };
__global__ void k_voxel_keys(const float4* __restrict__ pts, uint32_t n, VoxelDims d, unsigned long long* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const int i0 = (int)(floorf(p.x * d.inv) - (float)d.minb[0]);
  const int i1 = (int)(floorf(p.y * d.inv) - (float)d.minb[1]);
  const int i2 = (int)(floorf(p.z * d.inv) - (float)d.minb[2]);
  keys[i] = ((unsigned long long)(uint32_t)(i0 + i1 * d.div0 + i2 * d.div01) << 32) | i;
}
// ---- stable LSD radix sort pass over bits [shift, shift + 8) of the 64-bit key; tile = one 256-thread block, one key per thread
__global__ void __launch_bounds__(QN_BLOCK) k_radix_hist(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * QN_BLOCK + threadIdx.x;
  if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];             // digit-major: the scan yields global offsets directly
}
__global__ void __launch_bounds__(QN_BLOCK) k_radix_scatter(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks,
                                                            const uint32_t* __restrict__ offs, unsigned long long* __restrict__ out) {
  __shared__ uint32_t wcount[QN_BLOCK / 64][256];
  for (int t = threadIdx.x; t < (QN_BLOCK / 64) * 256; t += QN_BLOCK) (&wcount[0][0])[t] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * QN_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool valid = i < n;
  const unsigned long long key = valid ? keys[i] : 0ull;
  const uint32_t d = (uint32_t)(key >> shift) & 255u;
  unsigned long long same = __ballot(valid);                            // lanes of this wave holding the same digit
#pragma unroll
  for (int b = 0; b < 8; b++) { const unsigned long long m = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? m : ~m; }
  const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
  if (valid && rank == 0) wcount[wid][d] = (uint32_t)__popcll(same);
  __syncthreads();
  if (!valid) return;
  uint32_t before = 0;
  for (int w = 0; w < wid; w++) before += wcount[w][d];
  out[offs[d * nblocks + blockIdx.x] + before + rank] = key;
}

__global__ void k_leaf_flags(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1u : 0u;
}
__global__ void k_leaf_heads(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t n, uint32_t* __restrict__ heads) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) heads[pos[i]] = i;
  if (i == n - 1) heads[pos[n]] = n;          // pos[n] = number of leaves (exclusive scan total)
}
__global__ void k_leaf_centroids(const float4* __restrict__ pts, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ heads,
                                 const uint32_t* __restrict__ nleaf_ptr, float4* __restrict__ out) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= *nleaf_ptr) return;
  const uint32_t a = heads[m], b = heads[m + 1];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (uint32_t t = a; t < b; t++) { const float4 p = pts[(uint32_t)keys[t]]; sx = sx + p.x; sy = sy + p.y; sz = sz + p.z; }
  const float cnt = (float)(b - a);
  out[m] = make_float4(sx / cnt, sy / cnt, sz / cnt, 1.0f);
}

// ---- corrected global map (fast_lio_sam_qn.cpp:302-316, 398-411, 435-448): transformPcd of EVERY keyframe with its corrected
// pose, concatenation, voxelizePcd at save_voxel_resolution - xyz AND intensity (PointXYZI; VoxelGrid averages all fields).
// Sized for 10^3 keyframes / 3e7 points: one transform launch for all keyframes, radix tiles of QN_MAP_TILE keys per block.
#define QN_MAP_TILE 4096
#define QN_MAP_ITEMS (QN_MAP_TILE / QN_BLOCK)
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
struct MapKf { const float4* src; uint32_t off, n, blk0, has_i; };     // one listed keyframe: its concatenation offset, first tile, pose = its list position
// transformPcd of every listed keyframe in ONE launch: tile b belongs to keyframe blk_kf[b] (the same f64 arithmetic and order as
// k_kf_transform, so xyz is bit-identical to qn_kf_assemble's); intensity = the resident .w for qn_kf_add_xyzi keyframes, 0 for
// qn_kf_add ones.  Fused: the tile's bounding box of the finite points and its count of non-finite ones -> part[b].
__global__ void __launch_bounds__(QN_BLOCK) k_map_transform(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const double* __restrict__ poses,
                                                            float4* __restrict__ out, BBoxOut* __restrict__ part) {
  __shared__ int smn[QN_BLOCK / 64][3], smx[QN_BLOCK / 64][3], sbad[QN_BLOCK / 64];
  const uint32_t k = blk_kf[blockIdx.x];
  const MapKf f = kfs[k];
  const double* T = poses + 16 * (size_t)k;
  const uint32_t base = (blockIdx.x - f.blk0) * QN_MAP_TILE;
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int bad = 0;
#pragma unroll 4
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const uint32_t i = base + j * QN_BLOCK + threadIdx.x;
    if (i >= f.n) break;
    const float4 p = f.src[i]; const double x = p.x, y = p.y, z = p.z;
    const float4 q = make_float4((float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]), (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]),
                                 (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]), f.has_i ? p.w : 0.0f);
    out[f.off + i] = q;
    if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z))) { bad++; continue; }
    const int ox = f2ord(q.x), oy = f2ord(q.y), oz = f2ord(q.z);
    mn[0] = min(mn[0], ox); mn[1] = min(mn[1], oy); mn[2] = min(mn[2], oz);
    mx[0] = max(mx[0], ox); mx[1] = max(mx[1], oy); mx[2] = max(mx[2], oz);
  }
#pragma unroll
  for (int d = 0; d < 3; d++) { mn[d] = wave_min_i(mn[d]); mx[d] = wave_max_i(mx[d]); }
  bad = wave_sum_i(bad);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { for (int d = 0; d < 3; d++) { smn[wid][d] = mn[d]; smx[wid][d] = mx[d]; } sbad[wid] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QN_BLOCK / 64; w++) { for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], smn[w][d]); mx[d] = max(mx[d], smx[w][d]); } bad += sbad[w]; }
    BBoxOut r; for (int d = 0; d < 3; d++) { r.mn[d] = mn[d]; r.mx[d] = mx[d]; } r.nonfinite = (uint32_t)bad;
    part[blockIdx.x] = r;
  }
}
// the per-tile partials -> one box and the total number of non-finite points (one block; deterministic, no atomics)
__global__ void __launch_bounds__(QN_BLOCK) k_map_bbox_reduce(const BBoxOut* __restrict__ part, uint32_t nb, BBoxOut* __restrict__ out) {
  __shared__ int smn[QN_BLOCK / 64][3], smx[QN_BLOCK / 64][3], sbad[QN_BLOCK / 64];
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int bad = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += QN_BLOCK) {
    const BBoxOut r = part[b];
    for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], r.mn[d]); mx[d] = max(mx[d], r.mx[d]); }
    bad += (int)r.nonfinite;
  }
#pragma unroll
  for (int d = 0; d < 3; d++) { mn[d] = wave_min_i(mn[d]); mx[d] = wave_max_i(mx[d]); }
  bad = wave_sum_i(bad);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { for (int d = 0; d < 3; d++) { smn[wid][d] = mn[d]; smx[wid][d] = mx[d]; } sbad[wid] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QN_BLOCK / 64; w++) { for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], smn[w][d]); mx[d] = max(mx[d], smx[w][d]); } bad += sbad[w]; }
    BBoxOut r; for (int d = 0; d < 3; d++) { r.mn[d] = mn[d]; r.mx[d] = mx[d]; } r.nonfinite = (uint32_t)bad;
    *out = r;
  }
}
// leaf keys as k_voxel_keys computes them; a non-finite point gets the leaf `sentinel` (= number of cells, past every real leaf), so the
// stable sort moves it behind all finite points in its original order and the leaf pass simply stops before it (no compaction pass)
__global__ void k_map_keys(const float4* __restrict__ pts, uint32_t n, VoxelDims d, uint32_t sentinel, unsigned long long* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  uint32_t leaf = sentinel;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const int i0 = (int)(floorf(p.x * d.inv) - (float)d.minb[0]);
    const int i1 = (int)(floorf(p.y * d.inv) - (float)d.minb[1]);
    const int i2 = (int)(floorf(p.z * d.inv) - (float)d.minb[2]);
    leaf = (uint32_t)(i0 + i1 * d.div0 + i2 * d.div01);
  }
  keys[i] = ((unsigned long long)leaf << 32) | i;
}
// lanes of this wave whose digit equals mine (8 ballots), restricted to `valid` lanes
__device__ __forceinline__ unsigned long long match_digit8(uint32_t d, bool valid) {
  unsigned long long same = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) { const unsigned long long m = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? m : ~m; }
  return same;
}
// ---- stable LSD radix pass over bits [shift, shift + 8), QN_MAP_TILE keys per block: digit histogram in LDS (one LDS add per distinct
// digit of a wave, so a tile whose keys share their high digits does not serialise on one bank) ...
__global__ void __launch_bounds__(QN_BLOCK) k_map_radix_hist(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * QN_MAP_TILE + threadIdx.x;
  const int lane = threadIdx.x & 63;
#pragma unroll 4
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const uint32_t i = base + j * QN_BLOCK;
    const bool valid = i < n;
    const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
    const unsigned long long same = match_digit8(d, valid);
    if (valid && (uint32_t)__popcll(same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&h[d], (uint32_t)__popcll(same));
  }
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];             // digit-major: the scan yields global offsets directly
}
// ... and the scatter: the tile is ranked in QN_MAP_ITEMS rounds of QN_BLOCK consecutive keys (round order = key order, wave order
// inside a round, lane order inside a wave: stable), each digit's running output position kept in LDS across the rounds.
__global__ void __launch_bounds__(QN_BLOCK) k_map_radix_scatter(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks,
                                                                const uint32_t* __restrict__ offs, unsigned long long* __restrict__ out) {
  __shared__ uint32_t wcount[QN_BLOCK / 64][256];
  __shared__ uint32_t run[256];
  for (int w = 0; w < QN_BLOCK / 64; w++) wcount[w][threadIdx.x] = 0;
  run[threadIdx.x] = offs[threadIdx.x * nblocks + blockIdx.x];
  const uint32_t base = blockIdx.x * QN_MAP_TILE + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long kv[QN_MAP_ITEMS];
#pragma unroll
  for (int j = 0; j < QN_MAP_ITEMS; j++) { const uint32_t i = base + j * QN_BLOCK; kv[j] = i < n ? keys[i] : 0ull; }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const bool valid = base + j * QN_BLOCK < n;
    const uint32_t d = (uint32_t)(kv[j] >> shift) & 255u;
    const unsigned long long same = match_digit8(d, valid);
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcount[wid][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (valid) {
      uint32_t before = run[d];
      for (int w = 0; w < wid; w++) before += wcount[w][d];
      out[before + rank] = kv[j];
    }
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < QN_BLOCK / 64; w++) { t += wcount[w][threadIdx.x]; wcount[w][threadIdx.x] = 0; }
    run[threadIdx.x] += t;
    __syncthreads();
  }
}
// one thread per leaf: f32 sums of x, y, z, intensity in ascending concatenation order, each / (float)count (a NaN intensity poisons its leaf's)
__global__ void k_map_centroids(const float4* __restrict__ pts, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ heads,
                                const uint32_t* __restrict__ nleaf_ptr, float4* __restrict__ out) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= *nleaf_ptr) return;
  const uint32_t a = heads[m], b = heads[m + 1];
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  for (uint32_t t = a; t < b; t++) { const float4 p = pts[(uint32_t)keys[t]]; sx = sx + p.x; sy = sy + p.y; sz = sz + p.z; si = si + p.w; }
  const float cnt = (float)(b - a);
  out[m] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
}
// pack a strided PointXYZI-like host layout into float4 (x, y, z, intensity)
__global__ void k_pack_xyzi(const char* __restrict__ in, uint32_t stride, uint32_t ioff, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* r = in + (size_t)i * stride;
  const float* p = (const float*)r;
  out[i] = make_float4(p[0], p[1], p[2], *(const float*)(r + ioff));
}

// ---- many loop-closure submaps in one pass (qn_kf_assemble_batch): the qn_kf_build_map structure with the submap as one more key field.
// The listed keyframes of all submaps are transformed by k_map_transform (one launch; tiles never straddle keyframes, so a submap owns
// a contiguous tile range and a contiguous point range [p0, p1)).  Keys are ((seg << L | leaf) << 32 | point index): one stable sort
// orders every submap's points by leaf, finite points of a submap first (its non-finite ones carry the sentinel leaf).
struct BatchSeg { VoxelDims vd; uint32_t p0, p1, nvox, sentinel, prefix, tripped; };  // nvox: finite points that are voxelized (0 if tripped / empty)
// one block per submap over its tile range: the box of its finite points and its non-finite count, in a fixed order (no atomics)
__global__ void __launch_bounds__(QN_BLOCK) k_seg_bbox_reduce(const BBoxOut* __restrict__ part, const uint32_t* __restrict__ tile_off, BBoxOut* __restrict__ out) {
  __shared__ int smn[QN_BLOCK / 64][3], smx[QN_BLOCK / 64][3], sbad[QN_BLOCK / 64];
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int bad = 0;
  const uint32_t b1 = tile_off[blockIdx.x + 1];
  for (uint32_t b = tile_off[blockIdx.x] + threadIdx.x; b < b1; b += QN_BLOCK) {
    const BBoxOut r = part[b];
    for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], r.mn[d]); mx[d] = max(mx[d], r.mx[d]); }
    bad += (int)r.nonfinite;
  }
#pragma unroll
  for (int d = 0; d < 3; d++) { mn[d] = wave_min_i(mn[d]); mx[d] = wave_max_i(mx[d]); }
  bad = wave_sum_i(bad);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { for (int d = 0; d < 3; d++) { smn[wid][d] = mn[d]; smx[wid][d] = mx[d]; } sbad[wid] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QN_BLOCK / 64; w++) { for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], smn[w][d]); mx[d] = max(mx[d], smx[w][d]); } bad += sbad[w]; }
    BBoxOut r; for (int d = 0; d < 3; d++) { r.mn[d] = mn[d]; r.mx[d] = mx[d]; } r.nonfinite = (uint32_t)bad;
    out[blockIdx.x] = r;
  }
}
// keys, one block per tile: leaf as k_voxel_keys computes it; the submap's sentinel for a non-finite point; leaf 0 for every finite point of a
// submap whose guard tripped (the stable sort then keeps them in concatenation order for the pass-through gather)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_keys(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                         const BatchSeg* __restrict__ segs, const float4* __restrict__ pts, unsigned long long* __restrict__ keys) {
  const uint32_t k = blk_kf[blockIdx.x];
  const MapKf f = kfs[k];
  const BatchSeg sg = segs[kf_seg[k]];
  const uint32_t base = (blockIdx.x - f.blk0) * QN_MAP_TILE;
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const uint32_t i = base + j * QN_BLOCK + threadIdx.x;
    if (i >= f.n) break;
    const uint32_t g = f.off + i;
    const float4 p = pts[g];
    uint32_t leaf = sg.sentinel;
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
      leaf = 0;
      if (!sg.tripped) {
        const int i0 = (int)(floorf(p.x * sg.vd.inv) - (float)sg.vd.minb[0]);
        const int i1 = (int)(floorf(p.y * sg.vd.inv) - (float)sg.vd.minb[1]);
        const int i2 = (int)(floorf(p.z * sg.vd.inv) - (float)sg.vd.minb[2]);
        leaf = (uint32_t)(i0 + i1 * sg.vd.div0 + i2 * sg.vd.div01);
      }
    }
    keys[g] = ((unsigned long long)(sg.prefix | leaf) << 32) | g;
  }
}
// leaf heads over the sorted keys, one block per tile of positions: a head is a voxelized position whose leaf differs from its predecessor's
// or that opens its submap (the submap field alone would not separate two submaps of different sort groups)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_leaf_flags(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                               const BatchSeg* __restrict__ segs, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ flag) {
  const uint32_t k = blk_kf[blockIdx.x];
  const MapKf f = kfs[k];
  const BatchSeg sg = segs[kf_seg[k]];
  const uint32_t base = (blockIdx.x - f.blk0) * QN_MAP_TILE, fe = sg.p0 + sg.nvox;
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const uint32_t i = base + j * QN_BLOCK + threadIdx.x;
    if (i >= f.n) break;
    const uint32_t g = f.off + i;
    flag[g] = (g < fe && (g == sg.p0 || (keys[g] >> 32) != (keys[g - 1] >> 32))) ? 1u : 0u;
  }
}
// after the exclusive scan pos of the flags: leaf m = [heads[m], ends[m]) (its position in the output = its rank over all submaps)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_leaf_bounds(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                                const BatchSeg* __restrict__ segs, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                                uint32_t* __restrict__ heads, uint32_t* __restrict__ ends) {
  const uint32_t k = blk_kf[blockIdx.x];
  const MapKf f = kfs[k];
  const BatchSeg sg = segs[kf_seg[k]];
  const uint32_t base = (blockIdx.x - f.blk0) * QN_MAP_TILE, fe = sg.p0 + sg.nvox;
  for (int j = 0; j < QN_MAP_ITEMS; j++) {
    const uint32_t i = base + j * QN_BLOCK + threadIdx.x;
    if (i >= f.n) break;
    const uint32_t g = f.off + i;
    if (g >= fe) continue;
    const uint32_t fl = flag[g], m = pos[g] + fl - 1;
    if (fl) heads[m] = g;
    if (g + 1 == fe || flag[g + 1]) ends[m] = g + 1;
  }
}
// one thread per leaf: k_leaf_centroids' arithmetic (f32 sums in ascending concatenation order, / (float)count, w = 1)
__global__ void k_batch_centroids(const float4* __restrict__ pts, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ heads,
                                  const uint32_t* __restrict__ ends, const uint32_t* __restrict__ nleaf_ptr, float4* __restrict__ out) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= *nleaf_ptr) return;
  const uint32_t a = heads[m], b = ends[m];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (uint32_t t = a; t < b; t++) { const float4 p = pts[(uint32_t)keys[t]]; sx = sx + p.x; sy = sy + p.y; sz = sz + p.z; }
  const float cnt = (float)(b - a);
  out[m] = make_float4(sx / cnt, sy / cnt, sz / cnt, 1.0f);
}
// each submap's first leaf and leaf count: res[2 s] = first, res[2 s + 1] = count
__global__ void k_batch_counts(const BatchSeg* __restrict__ segs, uint32_t nseg, const uint32_t* __restrict__ pos, uint32_t* __restrict__ res) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t a = pos[segs[s].p0];
  res[2 * s] = a; res[2 * s + 1] = pos[segs[s].p1] - a;
}
// a tripped submap: its finite points (the first n of its sorted range, in concatenation order), unfiltered, w = 1 as qn_kf_assemble copies them
__global__ void k_batch_gather(const unsigned long long* __restrict__ keys, uint32_t n, const float4* __restrict__ pts, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[(uint32_t)keys[i]];
  out[i] = make_float4(p.x, p.y, p.z, 1.0f);
}

}  // namespace qn

struct qn_kf_store {
  int device = 0; hipStream_t stream = nullptr;
  std::vector<float4*> clouds; std::vector<uint32_t> sizes; std::vector<uint8_t> has_i;   // has_i: added by qn_kf_add_xyzi (.w = intensity)
  float4* concat = nullptr; unsigned long long* keys = nullptr; unsigned long long* keys_alt = nullptr;
  uint32_t* flag = nullptr; uint32_t* pos = nullptr; uint32_t* heads = nullptr; uint32_t* sums = nullptr; size_t cap = 0;
  uint32_t* hist = nullptr; uint32_t* hist_sums = nullptr;
  float4* out[2] = {nullptr, nullptr}; size_t out_cap[2] = {0, 0}; uint32_t out_n[2] = {0, 0};
  double* poses = nullptr; size_t poses_cap = 0;
  qn::BBoxOut* bbox = nullptr; qn::BBoxOut* bbox_host = nullptr; uint32_t* count_host = nullptr; char* staging = nullptr; size_t staging_cap = 0;
  float4* map = nullptr; size_t map_cap = 0; uint32_t map_n = 0;                          // the corrected global map: its own slot
  qn::MapKf* map_kfs = nullptr; size_t map_kfs_cap = 0; uint32_t* map_blk = nullptr; size_t map_blk_cap = 0; qn::BBoxOut* map_part = nullptr; size_t map_part_cap = 0;
  // qn_kf_assemble_batch: its own output slot (all submaps in one buffer) and tables
  float4* bt_out = nullptr; size_t bt_out_cap = 0; std::vector<const float4*> bt_ptr; std::vector<uint32_t> bt_n;
  uint32_t* bt_ends = nullptr; size_t bt_ends_cap = 0; uint32_t* bt_kf_seg = nullptr; size_t bt_kf_seg_cap = 0; uint32_t* bt_tile_off = nullptr; size_t bt_tile_off_cap = 0;
  qn::BatchSeg* bt_segs = nullptr; size_t bt_segs_cap = 0; qn::BBoxOut* bt_bbox = nullptr; size_t bt_bbox_cap = 0; uint32_t* bt_res = nullptr; size_t bt_res_cap = 0;
  qn::BBoxOut* bt_bbox_host = nullptr; size_t bt_bbox_host_cap = 0; uint32_t* bt_res_host = nullptr; size_t bt_res_host_cap = 0;
  // scratch of other translation units (the ray-caster, qn_sim.hip): see qn_kf_internal.h
  void* int_scratch[QN_KF_INT_SCRATCH] = {}; size_t int_scratch_cap[QN_KF_INT_SCRATCH] = {}; void* int_pinned = nullptr; size_t int_pinned_cap = 0;
  void* ext[QN_KF_INT_EXT] = {}; qn_kf_int_release_fn ext_release[QN_KF_INT_EXT] = {};      // state of other translation units (qn_sc.hip)
  std::string last_error;
};
#define KFCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (s)->last_error = std::string(#call) + " -> " + hipGetErrorString(e_); return QN_ERR_HIP; } } while (0)

extern "C" int qn_kf_store_create(int device, qn_kf_store** out) {
  if (!out) return QN_ERR_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return QN_ERR_NO_DEVICE;
  qn_kf_store* s = new qn_kf_store(); s->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&s->bbox, sizeof(qn::BBoxOut)) != hipSuccess || hipHostMalloc(&s->bbox_host, sizeof(qn::BBoxOut), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&s->count_host, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { delete s; return QN_ERR_HIP; }
  *out = s;
  return QN_OK;
}
extern "C" void qn_kf_store_destroy(qn_kf_store* s) {
  if (!s) return;
  (void)hipSetDevice(s->device); if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (float4* p : s->clouds) (void)hipFree(p);
  (void)hipFree(s->concat); (void)hipFree(s->keys); (void)hipFree(s->keys_alt); (void)hipFree(s->flag); (void)hipFree(s->pos); (void)hipFree(s->heads); (void)hipFree(s->sums);
  (void)hipFree(s->hist); (void)hipFree(s->hist_sums); (void)hipFree(s->out[0]); (void)hipFree(s->out[1]); (void)hipFree(s->poses); (void)hipFree(s->bbox); (void)hipFree(s->staging);
  (void)hipFree(s->map); (void)hipFree(s->map_kfs); (void)hipFree(s->map_blk); (void)hipFree(s->map_part);
  (void)hipFree(s->bt_out); (void)hipFree(s->bt_ends); (void)hipFree(s->bt_kf_seg); (void)hipFree(s->bt_tile_off); (void)hipFree(s->bt_segs); (void)hipFree(s->bt_bbox); (void)hipFree(s->bt_res);
  for (int k = 0; k < QN_KF_INT_EXT; k++) if (s->ext[k] && s->ext_release[k]) s->ext_release[k](s->ext[k]);
  for (void* p : s->int_scratch) (void)hipFree(p);
  if (s->int_pinned) (void)hipHostFree(s->int_pinned);
  if (s->bt_bbox_host) (void)hipHostFree(s->bt_bbox_host); if (s->bt_res_host) (void)hipHostFree(s->bt_res_host);
  if (s->bbox_host) (void)hipHostFree(s->bbox_host); if (s->count_host) (void)hipHostFree(s->count_host);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}
extern "C" const char* qn_kf_last_error(const qn_kf_store* s) { return s ? s->last_error.c_str() : "null store"; }

// upload one keyframe cloud (sensor frame) - PosePcd::pcd_ - and keep it resident; ioff < 0: xyz only (.w = 1), else the intensity's byte offset
static int kf_add(qn_kf_store* s, const float* xyz, uint32_t n, uint32_t stride, int ioff, int32_t* id_out) {
  KFCHK(s, hipSetDevice(s->device));
  float4* d = nullptr;
  if (n) {
    const size_t bytes = (size_t)(n - 1) * stride + (ioff < 0 ? 12 : std::max(12, ioff + 4));
    if (bytes > s->staging_cap) { (void)hipFree(s->staging); s->staging = nullptr; s->staging_cap = 0; KFCHK(s, hipMalloc(&s->staging, bytes + bytes / 2)); s->staging_cap = bytes + bytes / 2; }
    KFCHK(s, hipMalloc(&d, sizeof(float4) * n));
    KFCHK(s, hipMemcpyAsync(s->staging, xyz, bytes, hipMemcpyHostToDevice, s->stream));
    if (ioff < 0) hipLaunchKernelGGL(qn::k_pack_points, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->staging, stride, n, d);
    else hipLaunchKernelGGL(qn::k_pack_xyzi, dim3((n + 255) / 256), dim3(256), 0, s->stream, (const char*)s->staging, stride, (uint32_t)ioff, n, d);
    const hipError_t e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) { (void)hipFree(d); s->last_error = std::string("kf_add -> ") + hipGetErrorString(e); return QN_ERR_HIP; }
  }
  s->clouds.push_back(d); s->sizes.push_back(n); s->has_i.push_back(ioff >= 0);
  *id_out = (int32_t)s->clouds.size() - 1;
  return QN_OK;
}
extern "C" int qn_kf_add(qn_kf_store* s, const float* xyz, uint32_t n, uint32_t stride, int32_t* id_out) {
  if (!s || !id_out || (n && !xyz) || stride < 12 || (stride & 3)) return QN_ERR_INVALID_ARG;
  return kf_add(s, xyz, n, stride, -1, id_out);
}
// PointXYZI records: xyz at 0, intensity at `ioff` (pcl::PointXYZI: stride 32, offset 16)
static bool xyzi_layout_ok(uint32_t stride, uint32_t ioff) { return !(stride & 3) && ioff >= 12 && !(ioff & 3) && (size_t)ioff + 4 <= stride; }
extern "C" int qn_kf_add_xyzi(qn_kf_store* s, const float* pts, uint32_t n, uint32_t stride, uint32_t ioff, int32_t* id_out) {
  if (!s || !id_out || (n && !pts) || !xyzi_layout_ok(stride, ioff)) return QN_ERR_INVALID_ARG;
  return kf_add(s, pts, n, stride, (int)ioff, id_out);
}

// ---- keyframes from device memory (qn_kf_add_device) and read-back of one keyframe (qn_kf_download_keyframe)
// The record layout rules of qn_kf_add / qn_kf_add_xyzi, and the same pack kernels: the resident bytes are identical for the same input bytes.
static bool device_layout_ok(uint32_t stride, int32_t ioff) { return ioff < 0 ? (stride >= 12 && !(stride & 3)) : xyzi_layout_ok(stride, (uint32_t)ioff); }
int qn_kf_int_copy_async(qn_kf_store* s, const void* d_pts, uint32_t n, uint32_t stride, int32_t ioff, float4** out) {
  *out = nullptr;
  if (!n) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  float4* d = nullptr;
  KFCHK(s, hipMalloc(&d, sizeof(float4) * n));
  if (ioff < 0) hipLaunchKernelGGL(qn::k_pack_points, dim3((n + 255) / 256), dim3(256), 0, s->stream, (const char*)d_pts, stride, n, d);
  else hipLaunchKernelGGL(qn::k_pack_xyzi, dim3((n + 255) / 256), dim3(256), 0, s->stream, (const char*)d_pts, stride, (uint32_t)ioff, n, d);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { (void)hipFree(d); s->last_error = std::string("kf_add_device -> ") + hipGetErrorString(e); return QN_ERR_HIP; }
  *out = d;
  return QN_OK;
}
void qn_kf_int_append(qn_kf_store* s, float4* const* bufs, const uint32_t* n, uint32_t count, bool has_i, int32_t* ids_out) {
  for (uint32_t k = 0; k < count; k++) {
    s->clouds.push_back(bufs[k]); s->sizes.push_back(n[k]); s->has_i.push_back(has_i);
    ids_out[k] = (int32_t)s->clouds.size() - 1;
  }
}
int qn_kf_int_device(const qn_kf_store* s) { return s->device; }
hipStream_t qn_kf_int_stream(const qn_kf_store* s) { return s->stream; }
size_t qn_kf_int_count(const qn_kf_store* s) { return s->clouds.size(); }
void qn_kf_int_set_error(qn_kf_store* s, const char* msg) { s->last_error = msg; }
void* qn_kf_int_scratch(qn_kf_store* s, int which, size_t bytes) {
  if (which < 0 || which >= QN_KF_INT_SCRATCH) return nullptr;
  if (bytes > s->int_scratch_cap[which]) {
    (void)hipFree(s->int_scratch[which]); s->int_scratch[which] = nullptr; s->int_scratch_cap[which] = 0;
    if (hipMalloc(&s->int_scratch[which], bytes) != hipSuccess) { s->int_scratch[which] = nullptr; return nullptr; }
    s->int_scratch_cap[which] = bytes;
  }
  return s->int_scratch[which];
}
const float4* qn_kf_int_keyframe(const qn_kf_store* s, int32_t id, uint32_t* n) { *n = s->sizes[id]; return s->clouds[id]; }
void* qn_kf_int_ext(const qn_kf_store* s, int which) { return which >= 0 && which < QN_KF_INT_EXT ? s->ext[which] : nullptr; }
void qn_kf_int_set_ext(qn_kf_store* s, int which, void* p, qn_kf_int_release_fn release) {
  if (which < 0 || which >= QN_KF_INT_EXT) return;
  if (s->ext[which] && s->ext_release[which] && s->ext[which] != p) s->ext_release[which](s->ext[which]);
  s->ext[which] = p; s->ext_release[which] = release;
}
void* qn_kf_int_pinned(qn_kf_store* s, size_t bytes) {
  if (bytes > s->int_pinned_cap) {
    if (s->int_pinned) (void)hipHostFree(s->int_pinned);
    s->int_pinned = nullptr; s->int_pinned_cap = 0;
    if (hipHostMalloc(&s->int_pinned, bytes, hipHostMallocDefault) != hipSuccess) { s->int_pinned = nullptr; return nullptr; }
    s->int_pinned_cap = bytes;
  }
  return s->int_pinned;
}
extern "C" int qn_kf_add_device(qn_kf_store* s, const float* d_pts, uint32_t n, uint32_t stride, int32_t ioff, int32_t* id_out) {
  if (!s || !id_out || (n && !d_pts) || !device_layout_ok(stride, ioff) || ((uintptr_t)d_pts & 3)) return QN_ERR_INVALID_ARG;
  if (n) {        // the records must lie inside one device allocation of this store's device: a host pointer here would fault the GPU
    KFCHK(s, hipSetDevice(s->device));
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, d_pts) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != s->device) { (void)hipGetLastError(); return QN_ERR_INVALID_ARG; }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_pts) != hipSuccess) { (void)hipGetLastError(); return QN_ERR_INVALID_ARG; }
    const size_t need = (size_t)(n - 1) * stride + (ioff < 0 ? 12 : std::max<size_t>(12, (size_t)ioff + 4));
    if ((const char*)d_pts < (const char*)base || (size_t)((const char*)d_pts - (const char*)base) + need > size) return QN_ERR_INVALID_ARG;
  }
  float4* d = nullptr;
  const int st = qn_kf_int_copy_async(s, d_pts, n, stride, ioff, &d);
  if (st != QN_OK) return st;
  if (n) {
    const hipError_t e = hipStreamSynchronize(s->stream);      // the caller may reuse its buffer when this returns
    if (e != hipSuccess) { (void)hipFree(d); s->last_error = std::string("kf_add_device -> ") + hipGetErrorString(e); return QN_ERR_HIP; }
  }
  qn_kf_int_append(s, &d, &n, 1, ioff >= 0, id_out);
  return QN_OK;
}
extern "C" int qn_kf_download_keyframe(qn_kf_store* s, int32_t id, float* xyzi_out) {
  if (!s || id < 0 || (size_t)id >= s->clouds.size() || (s->sizes[id] && !xyzi_out)) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->sizes[id];
  if (!n) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  KFCHK(s, hipMemcpy(xyzi_out, s->clouds[id], sizeof(float4) * n, hipMemcpyDeviceToHost));
  return QN_OK;
}

static int kf_reserve(qn_kf_store* s, size_t n) {
  if (n <= s->cap) return QN_OK;
  (void)hipFree(s->concat); (void)hipFree(s->keys); (void)hipFree(s->keys_alt); (void)hipFree(s->flag); (void)hipFree(s->pos); (void)hipFree(s->heads); (void)hipFree(s->sums); (void)hipFree(s->hist); (void)hipFree(s->hist_sums);
  s->concat = nullptr; s->keys = s->keys_alt = nullptr; s->flag = s->pos = s->heads = s->sums = nullptr; s->hist = s->hist_sums = nullptr; s->cap = 0;
  const size_t c = n + n / 2 + 1024;
  KFCHK(s, hipMalloc(&s->concat, sizeof(float4) * c)); KFCHK(s, hipMalloc(&s->keys, 8 * c)); KFCHK(s, hipMalloc(&s->keys_alt, 8 * c));
  KFCHK(s, hipMalloc(&s->flag, 4 * (c + 1))); KFCHK(s, hipMalloc(&s->pos, 4 * (c + 1))); KFCHK(s, hipMalloc(&s->heads, 4 * (c + 2)));
  KFCHK(s, hipMalloc(&s->sums, 4 * (c / (QN_BLOCK * QN_SCAN_ITEMS) + 2)));
  const size_t hb = (c + QN_BLOCK - 1) / QN_BLOCK * 256;                   // digit-major block histograms of one radix pass
  KFCHK(s, hipMalloc(&s->hist, 4 * (hb + 1))); KFCHK(s, hipMalloc(&s->hist_sums, 4 * (hb / (QN_BLOCK * QN_SCAN_ITEMS) + 2)));
  s->cap = c;
  return QN_OK;
}

// pcl::VoxelGrid::applyFilter's grid from the bounding box of the finite points: leaf-index origin and divisions, number of cells;
// returns false when PCL's overflow guard trips (its own arithmetic: f32 product, int64 cast; it warns and sets output = *input_)
static bool voxel_dims(const qn::BBoxOut& bb, double leaf, qn::VoxelDims* vd, long long* cells_out) {
  vd->inv = 1.0f / (float)leaf;
  long long cells = 1; int divb[3];
  for (int d = 0; d < 3; d++) {
    const float mn = qn::ord2f(bb.mn[d]), mx = qn::ord2f(bb.mx[d]);
    vd->minb[d] = (int)std::floor(mn * vd->inv); const int maxb = (int)std::floor(mx * vd->inv);
    divb[d] = maxb - vd->minb[d] + 1; cells *= divb[d];
  }
  long long pd = 1;
  for (int d = 0; d < 3; d++) { const float mn = qn::ord2f(bb.mn[d]), mx = qn::ord2f(bb.mx[d]); pd *= (long long)((mx - mn) * vd->inv) + 1; }
  *cells_out = cells;
  if (pd > (long long)INT32_MAX || cells > (long long)INT32_MAX) return false;
  vd->div0 = divb[0]; vd->div01 = divb[0] * divb[1];
  return true;
}
static const char* kOverflowWarning = "warning: leaf size is too small for the input dataset, integer indices would overflow: cloud passed through unfiltered (as pcl::VoxelGrid does)";

// transform + concatenate `count` resident keyframes with their poses (row-major 4x4 f64) and voxel-grid them into
// output slot 0 (source) or 1 (target); returns the device pointer (float4, stride 16) and the point count.
extern "C" int qn_kf_assemble(qn_kf_store* s, const int32_t* ids, const double* poses, uint32_t count, double leaf, int slot,
                              const float** d_xyz_out, uint32_t* n_out) {
  if (!s || !ids || !poses || !d_xyz_out || !n_out || (slot != 0 && slot != 1) || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  *d_xyz_out = nullptr; *n_out = 0;
  KFCHK(s, hipSetDevice(s->device));
  size_t total = 0;
  for (uint32_t k = 0; k < count; k++) { if (ids[k] < 0 || (size_t)ids[k] >= s->clouds.size()) return QN_ERR_INVALID_ARG; total += s->sizes[ids[k]]; }
  if (total == 0) return QN_ERR_EMPTY_CLOUD;
  if (total >= 0xffffffffull) return QN_ERR_CAPACITY;
  int rc = kf_reserve(s, total); if (rc != QN_OK) return rc;
  if ((size_t)count * 16 > s->poses_cap) { (void)hipFree(s->poses); s->poses = nullptr; s->poses_cap = 0; KFCHK(s, hipMalloc(&s->poses, sizeof(double) * 16 * (count + 8))); s->poses_cap = (size_t)16 * (count + 8); }
  hipStream_t st = s->stream;
  KFCHK(s, hipMemcpyAsync(s->poses, poses, sizeof(double) * 16 * count, hipMemcpyHostToDevice, st));
  size_t off = 0;
  for (uint32_t k = 0; k < count; k++) {                       // transformPcd + operator+= (loop_closure.cpp:76,83,89,92,102)
    const uint32_t n = s->sizes[ids[k]];
    if (n) hipLaunchKernelGGL(qn::k_kf_transform, dim3((n + 255) / 256), dim3(256), 0, st, s->clouds[ids[k]], n, s->poses + 16 * k, s->concat + off);
    off += n;
  }
  uint32_t n = (uint32_t)total;
  // pcl::VoxelGrid::applyFilter: bounds, leaf indices
  qn::BBoxOut init; for (int d = 0; d < 3; d++) { init.mn[d] = 0x7fffffff; init.mx[d] = (int)0x80000000; } init.nonfinite = 0;
  *s->bbox_host = init;
  KFCHK(s, hipMemcpyAsync(s->bbox, s->bbox_host, sizeof(qn::BBoxOut), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(qn::k_bbox, dim3(std::min<uint32_t>((n + QN_BLOCK - 1) / QN_BLOCK, 128)), dim3(QN_BLOCK), 0, st, s->concat, n, s->bbox);
  KFCHK(s, hipMemcpyAsync(s->bbox_host, s->bbox, sizeof(qn::BBoxOut), hipMemcpyDeviceToHost, st));
  KFCHK(s, hipStreamSynchronize(st));
  if (s->bbox_host->nonfinite) {                                  // rare path: drop the non-finite points like pcl::VoxelGrid does for a non-dense cloud (order of the others kept)
    const uint32_t nbf = (n + 255) / 256, sbf = (n + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
    hipLaunchKernelGGL(qn::k_finite_flags, dim3(nbf), dim3(256), 0, st, s->concat, n, s->flag);
    hipLaunchKernelGGL(qn::k_scan_block, dim3(sbf), dim3(QN_BLOCK), 0, st, s->flag, n, s->pos, s->sums);
    hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->sums, sbf);
    hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sbf), dim3(QN_BLOCK), 0, st, s->pos, n, s->sums, s->flag);
    if (n > s->out_cap[slot]) { (void)hipFree(s->out[slot]); s->out[slot] = nullptr; s->out_cap[slot] = 0; KFCHK(s, hipMalloc(&s->out[slot], sizeof(float4) * (n + n / 2))); s->out_cap[slot] = n + n / 2; }
    hipLaunchKernelGGL(qn::k_compact_finite, dim3(nbf), dim3(256), 0, st, (const float4*)s->concat, n, (const uint32_t*)s->flag, (const uint32_t*)s->pos, s->out[slot]);      // (the output slot as scratch)
    uint32_t kept = 0;
    KFCHK(s, hipMemcpyAsync(&kept, s->pos + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KFCHK(s, hipStreamSynchronize(st));
    if (kept == 0) return QN_ERR_EMPTY_CLOUD;
    KFCHK(s, hipMemcpyAsync(s->concat, s->out[slot], sizeof(float4) * kept, hipMemcpyDeviceToDevice, st));
    n = kept;
    s->last_error = "note: non-finite points dropped (pcl::VoxelGrid on a non-dense cloud)";
  }
  qn::VoxelDims vd; long long cells = 1;
  if (!voxel_dims(*s->bbox_host, leaf, &vd, &cells)) {
    s->last_error = kOverflowWarning;
    if (n > s->out_cap[slot]) { (void)hipFree(s->out[slot]); s->out[slot] = nullptr; s->out_cap[slot] = 0; KFCHK(s, hipMalloc(&s->out[slot], sizeof(float4) * (n + n / 2))); s->out_cap[slot] = n + n / 2; }
    KFCHK(s, hipMemcpyAsync(s->out[slot], s->concat, sizeof(float4) * n, hipMemcpyDeviceToDevice, st));
    KFCHK(s, hipStreamSynchronize(st));
    s->out_n[slot] = n; *d_xyz_out = (const float*)s->out[slot]; *n_out = n;
    return QN_OK;
  }
  const uint32_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(qn::k_voxel_keys, dim3(nb), dim3(256), 0, st, s->concat, n, vd, s->keys);
  unsigned long long* sorted = s->keys; unsigned long long* other = s->keys_alt;
  int bits = 1; while ((1ll << bits) < cells) bits++;
  const uint32_t rb = (n + QN_BLOCK - 1) / QN_BLOCK, hn = rb * 256, hsb = (hn + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
  for (int shift = 32; shift < 32 + bits; shift += 8) {                  // stable LSD passes over the leaf-index bits only
    hipLaunchKernelGGL(qn::k_radix_hist, dim3(rb), dim3(QN_BLOCK), 0, st, sorted, n, shift, rb, s->hist);
    hipLaunchKernelGGL(qn::k_scan_block, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist, s->hist_sums);
    hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->hist_sums, hsb);
    hipLaunchKernelGGL(qn::k_scan_add, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist_sums, n);
    hipLaunchKernelGGL(qn::k_radix_scatter, dim3(rb), dim3(QN_BLOCK), 0, st, sorted, n, shift, rb, s->hist, other);
    std::swap(sorted, other);
  }
  hipLaunchKernelGGL(qn::k_leaf_flags, dim3(nb), dim3(256), 0, st, sorted, n, s->flag);
  const uint32_t sb = (n + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
  hipLaunchKernelGGL(qn::k_scan_block, dim3(sb), dim3(QN_BLOCK), 0, st, s->flag, n, s->pos, s->sums);
  hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->sums, sb);
  hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sb), dim3(QN_BLOCK), 0, st, s->pos, n, s->sums, s->flag);
  hipLaunchKernelGGL(qn::k_leaf_heads, dim3(nb), dim3(256), 0, st, s->flag, s->pos, n, s->heads);
  if (n > s->out_cap[slot]) { (void)hipFree(s->out[slot]); s->out[slot] = nullptr; s->out_cap[slot] = 0; KFCHK(s, hipMalloc(&s->out[slot], sizeof(float4) * (n + n / 2))); s->out_cap[slot] = n + n / 2; }
  hipLaunchKernelGGL(qn::k_leaf_centroids, dim3(nb), dim3(256), 0, st, s->concat, sorted, s->heads, s->pos + n, s->out[slot]);
  KFCHK(s, hipMemcpyAsync(s->count_host, s->pos + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  KFCHK(s, hipGetLastError());
  KFCHK(s, hipStreamSynchronize(st));
  s->out_n[slot] = *s->count_host;
  *d_xyz_out = (const float*)s->out[slot]; *n_out = s->out_n[slot];
  return QN_OK;
}

extern "C" int qn_kf_download(qn_kf_store* s, int slot, float* xyz_out) {        // packed n x 3, for tests / visualisation
  if (!s || !xyz_out || (slot != 0 && slot != 1)) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->out_n[slot];
  if (!n) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  KFCHK(s, hipMemcpy2D(xyz_out, 12, s->out[slot], 16, 12, n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// the corrected global map (fast_lio_sam_qn.cpp:302-316, 398-411, 435-448): every listed keyframe transformed with its corrected pose,
// concatenated in list order, voxel-grid at `leaf` with intensity; into the store's own map slot (never assemble slots 0 / 1).
// Unlike qn_kf_assemble, a tripped overflow guard passes the WHOLE concatenation through, non-finite points included (output = *input_).
static int map_grow(qn_kf_store* s, void** p, size_t* cap, size_t need, size_t elem) {
  if (need <= *cap) return QN_OK;
  (void)hipFree(*p); *p = nullptr; *cap = 0;
  KFCHK(s, hipMalloc(p, elem * (need + need / 2)));
  *cap = need + need / 2;
  return QN_OK;
}
extern "C" int qn_kf_build_map(qn_kf_store* s, const int32_t* ids, const double* poses, uint32_t count, double leaf,
                               const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || (count && (!ids || !poses)) || !d_xyzi_out || !n_out || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  *d_xyzi_out = nullptr; *n_out = 0;
  s->map_n = 0; s->last_error.clear();
  if (count == 0) return QN_ERR_EMPTY_CLOUD;
  size_t total = 0, tiles = 0;
  for (uint32_t k = 0; k < count; k++) {
    if (ids[k] < 0 || (size_t)ids[k] >= s->clouds.size()) return QN_ERR_INVALID_ARG;
    total += s->sizes[ids[k]]; tiles += (s->sizes[ids[k]] + QN_MAP_TILE - 1) / QN_MAP_TILE;
  }
  if (total == 0) return QN_ERR_EMPTY_CLOUD;
  if (total >= 0xffffffffull) return QN_ERR_CAPACITY;
  KFCHK(s, hipSetDevice(s->device));
  int rc = kf_reserve(s, total); if (rc != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->map_kfs, &s->map_kfs_cap, count, sizeof(qn::MapKf))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->map_blk, &s->map_blk_cap, tiles, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->map_part, &s->map_part_cap, tiles, sizeof(qn::BBoxOut))) != QN_OK) return rc;
  if ((size_t)count * 16 > s->poses_cap) { (void)hipFree(s->poses); s->poses = nullptr; s->poses_cap = 0; KFCHK(s, hipMalloc(&s->poses, sizeof(double) * 16 * (count + 8))); s->poses_cap = (size_t)16 * (count + 8); }
  if ((rc = map_grow(s, (void**)&s->map, &s->map_cap, total, sizeof(float4))) != QN_OK) return rc;
  // the keyframe table and the tile -> keyframe table (host, O(count + tiles))
  std::vector<qn::MapKf> kfs(count); std::vector<uint32_t> blk(tiles);
  uint32_t off = 0, b0 = 0;
  for (uint32_t k = 0; k < count; k++) {
    const uint32_t n = s->sizes[ids[k]], nt = (n + QN_MAP_TILE - 1) / QN_MAP_TILE;
    kfs[k] = qn::MapKf{s->clouds[ids[k]], off, n, b0, s->has_i[ids[k]]};
    for (uint32_t t = 0; t < nt; t++) blk[b0 + t] = k;
    off += n; b0 += nt;
  }
  hipStream_t st = s->stream;
  const uint32_t n = (uint32_t)total, nt = (uint32_t)tiles;
  KFCHK(s, hipMemcpyAsync(s->poses, poses, sizeof(double) * 16 * count, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->map_kfs, kfs.data(), sizeof(qn::MapKf) * count, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->map_blk, blk.data(), sizeof(uint32_t) * tiles, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(qn::k_map_transform, dim3(nt), dim3(QN_BLOCK), 0, st, (const qn::MapKf*)s->map_kfs, (const uint32_t*)s->map_blk, (const double*)s->poses, s->concat, s->map_part);
  hipLaunchKernelGGL(qn::k_map_bbox_reduce, dim3(1), dim3(QN_BLOCK), 0, st, (const qn::BBoxOut*)s->map_part, nt, s->bbox);
  KFCHK(s, hipMemcpyAsync(s->bbox_host, s->bbox, sizeof(qn::BBoxOut), hipMemcpyDeviceToHost, st));
  KFCHK(s, hipStreamSynchronize(st));                               // sync 1 of 2: the bounding box sizes the grid
  const qn::BBoxOut bb = *s->bbox_host;
  const uint32_t n_fin = n - bb.nonfinite;
  if (n_fin == 0) return QN_ERR_EMPTY_CLOUD;
  qn::VoxelDims vd; long long cells = 1;
  if (!voxel_dims(bb, leaf, &vd, &cells)) {
    s->last_error = kOverflowWarning;
    KFCHK(s, hipMemcpyAsync(s->map, s->concat, sizeof(float4) * n, hipMemcpyDeviceToDevice, st));
    KFCHK(s, hipStreamSynchronize(st));
    s->map_n = n; *d_xyzi_out = (const float*)s->map; *n_out = n;
    return QN_OK;
  }
  const uint32_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(qn::k_map_keys, dim3(nb), dim3(256), 0, st, (const float4*)s->concat, n, vd, (uint32_t)cells, s->keys);
  unsigned long long* sorted = s->keys; unsigned long long* other = s->keys_alt;
  const long long maxleaf = bb.nonfinite ? cells : cells - 1;        // the sentinel leaf of the non-finite points is `cells`
  int bits = 1; while ((1ll << bits) <= maxleaf) bits++;
  const uint32_t rb = (n + QN_MAP_TILE - 1) / QN_MAP_TILE, hn = rb * 256, hsb = (hn + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
  for (int shift = 32; shift < 32 + bits; shift += 8) {                  // stable LSD passes over the leaf-index bits only
    hipLaunchKernelGGL(qn::k_map_radix_hist, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, n, shift, rb, s->hist);
    hipLaunchKernelGGL(qn::k_scan_block, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist, s->hist_sums);
    hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->hist_sums, hsb);
    hipLaunchKernelGGL(qn::k_scan_add, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist_sums, n);
    hipLaunchKernelGGL(qn::k_map_radix_scatter, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, n, shift, rb, (const uint32_t*)s->hist, other);
    std::swap(sorted, other);
  }
  // leaf heads over the finite prefix of the sorted keys (the engine's scans), then one thread per leaf
  const uint32_t nbf = (n_fin + 255) / 256, sb = (n_fin + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
  hipLaunchKernelGGL(qn::k_leaf_flags, dim3(nbf), dim3(256), 0, st, sorted, n_fin, s->flag);
  hipLaunchKernelGGL(qn::k_scan_block, dim3(sb), dim3(QN_BLOCK), 0, st, s->flag, n_fin, s->pos, s->sums);
  hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->sums, sb);
  hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sb), dim3(QN_BLOCK), 0, st, s->pos, n_fin, s->sums, s->flag);
  hipLaunchKernelGGL(qn::k_leaf_heads, dim3(nbf), dim3(256), 0, st, s->flag, s->pos, n_fin, s->heads);
  hipLaunchKernelGGL(qn::k_map_centroids, dim3(nbf), dim3(256), 0, st, (const float4*)s->concat, (const unsigned long long*)sorted, (const uint32_t*)s->heads, (const uint32_t*)(s->pos + n_fin), s->map);
  KFCHK(s, hipMemcpyAsync(s->count_host, s->pos + n_fin, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  KFCHK(s, hipGetLastError());
  KFCHK(s, hipStreamSynchronize(st));                               // sync 2 of 2: the leaf count
  s->map_n = *s->count_host;
  *d_xyzi_out = (const float*)s->map; *n_out = s->map_n;
  return QN_OK;
}

// the map into host records: only the 12 xyz bytes (offset 0) and the 4 intensity bytes (offset ioff) of each are written
extern "C" int qn_kf_download_map(qn_kf_store* s, void* out, uint32_t stride, uint32_t ioff) {
  if (!s || !out || !xyzi_layout_ok(stride, ioff)) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->map_n;
  if (!n) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  KFCHK(s, hipMemcpy2D(out, stride, s->map, 16, 12, n, hipMemcpyDeviceToHost));
  KFCHK(s, hipMemcpy2D((char*)out + ioff, stride, (const char*)s->map + 12, 16, 4, n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// S loop-closure submaps in one pass (LoopClosure::setSrcAndDstCloud for one query and its candidates, loop_closure.cpp:58-108): submap t =
// ids[seg_off[t] .. seg_off[t + 1]) with the poses of the same entries; each equals qn_kf_assemble of its list in all 16 bytes of every record.
// Into the store's batch slot (never slots 0 / 1 or the map slot).  Two host synchronisations: the per-submap boxes (grid sizes, sort
// bits), then the per-submap leaf counts.  Submaps are sorted in groups whose keys fit 32 bits - normally one group.
static int pin_grow(qn_kf_store* s, void** p, size_t* cap, size_t need, size_t elem) {
  if (need <= *cap) return QN_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *cap = 0;
  KFCHK(s, hipHostMalloc(p, elem * (need + need / 2), hipHostMallocDefault));
  *cap = need + need / 2;
  return QN_OK;
}
static int bits_for(unsigned long long v) { int b = 0; while (b < 64 && (1ull << b) <= v) b++; return b; }      // smallest b with v < 2^b
extern "C" int qn_kf_assemble_batch(qn_kf_store* s, const int32_t* ids, const double* poses, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                                    const float** d_xyz_out, uint32_t* n_out, int* status) {
  if (!s || !seg_off || n_seg == 0 || !d_xyz_out || !n_out || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  for (uint32_t t = 0; t < n_seg; t++) if (seg_off[t + 1] < seg_off[t]) return QN_ERR_INVALID_ARG;
  const uint32_t e0 = seg_off[0], count = seg_off[n_seg] - e0;
  if (count && (!ids || !poses)) return QN_ERR_INVALID_ARG;
  size_t total = 0, tiles = 0;
  for (uint32_t j = e0; j < e0 + count; j++) {
    if (ids[j] < 0 || (size_t)ids[j] >= s->clouds.size()) return QN_ERR_INVALID_ARG;
    total += s->sizes[ids[j]]; tiles += (s->sizes[ids[j]] + QN_MAP_TILE - 1) / QN_MAP_TILE;
  }
  for (uint32_t t = 0; t < n_seg; t++) { d_xyz_out[t] = nullptr; n_out[t] = 0; status[t] = QN_ERR_EMPTY_CLOUD; }
  s->bt_ptr.assign(n_seg, nullptr); s->bt_n.assign(n_seg, 0); s->last_error.clear();
  if (total >= 0xffffffffull) return QN_ERR_CAPACITY;
  if (total == 0) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  int rc = kf_reserve(s, total); if (rc != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->map_kfs, &s->map_kfs_cap, count, sizeof(qn::MapKf))) != QN_OK) return rc;     // (the map's scratch tables, not its slot)
  if ((rc = map_grow(s, (void**)&s->map_blk, &s->map_blk_cap, tiles, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->map_part, &s->map_part_cap, tiles, sizeof(qn::BBoxOut))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_kf_seg, &s->bt_kf_seg_cap, count, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_tile_off, &s->bt_tile_off_cap, n_seg + 1, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_segs, &s->bt_segs_cap, n_seg, sizeof(qn::BatchSeg))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_bbox, &s->bt_bbox_cap, n_seg, sizeof(qn::BBoxOut))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_res, &s->bt_res_cap, 2 * (size_t)n_seg, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = map_grow(s, (void**)&s->bt_ends, &s->bt_ends_cap, total, sizeof(uint32_t))) != QN_OK) return rc;
  if ((rc = pin_grow(s, (void**)&s->bt_bbox_host, &s->bt_bbox_host_cap, n_seg, sizeof(qn::BBoxOut))) != QN_OK) return rc;
  if ((rc = pin_grow(s, (void**)&s->bt_res_host, &s->bt_res_host_cap, 2 * (size_t)n_seg, sizeof(uint32_t))) != QN_OK) return rc;
  if ((size_t)count * 16 > s->poses_cap) { (void)hipFree(s->poses); s->poses = nullptr; s->poses_cap = 0; KFCHK(s, hipMalloc(&s->poses, sizeof(double) * 16 * (count + 8))); s->poses_cap = (size_t)16 * (count + 8); }
  // keyframe table, tile -> keyframe, keyframe -> submap, each submap's tile range and point range (host, O(count + tiles))
  std::vector<qn::MapKf> kfs(count); std::vector<uint32_t> blk(tiles), kseg(count), toff(n_seg + 1), p0(n_seg + 1);
  uint32_t off = 0, b0 = 0;
  for (uint32_t t = 0; t < n_seg; t++) {
    toff[t] = b0; p0[t] = off;
    for (uint32_t j = seg_off[t]; j < seg_off[t + 1]; j++) {
      const uint32_t k = j - e0, n = s->sizes[ids[j]], nt = (n + QN_MAP_TILE - 1) / QN_MAP_TILE;
      kfs[k] = qn::MapKf{s->clouds[ids[j]], off, n, b0, s->has_i[ids[j]]}; kseg[k] = t;
      for (uint32_t b = 0; b < nt; b++) blk[b0 + b] = k;
      off += n; b0 += nt;
    }
  }
  toff[n_seg] = b0; p0[n_seg] = off;
  hipStream_t st = s->stream;
  const uint32_t n = (uint32_t)total, nt = (uint32_t)tiles;
  KFCHK(s, hipMemcpyAsync(s->poses, poses + 16 * (size_t)e0, sizeof(double) * 16 * count, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->map_kfs, kfs.data(), sizeof(qn::MapKf) * count, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->map_blk, blk.data(), sizeof(uint32_t) * tiles, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->bt_kf_seg, kseg.data(), sizeof(uint32_t) * count, hipMemcpyHostToDevice, st));
  KFCHK(s, hipMemcpyAsync(s->bt_tile_off, toff.data(), sizeof(uint32_t) * (n_seg + 1), hipMemcpyHostToDevice, st));
  // transformPcd of every listed keyframe of every submap (k_map_transform: k_kf_transform's f64 order), per-tile boxes, per-submap reduce
  hipLaunchKernelGGL(qn::k_map_transform, dim3(nt), dim3(QN_BLOCK), 0, st, (const qn::MapKf*)s->map_kfs, (const uint32_t*)s->map_blk, (const double*)s->poses, s->concat, s->map_part);
  hipLaunchKernelGGL(qn::k_seg_bbox_reduce, dim3(n_seg), dim3(QN_BLOCK), 0, st, (const qn::BBoxOut*)s->map_part, (const uint32_t*)s->bt_tile_off, s->bt_bbox);
  KFCHK(s, hipMemcpyAsync(s->bt_bbox_host, s->bt_bbox, sizeof(qn::BBoxOut) * n_seg, hipMemcpyDeviceToHost, st));
  KFCHK(s, hipStreamSynchronize(st));                               // sync 1 of 2: each submap's box sizes its grid
  // per submap: pcl::VoxelGrid's grid and overflow guard (voxel_dims), its sentinel leaf and the key bits it needs
  std::vector<qn::BatchSeg> sg(n_seg); std::vector<int> lbits(n_seg); std::vector<uint32_t> nfin(n_seg), trip_off(n_seg, 0);
  std::vector<uint8_t> live(n_seg, 0);
  size_t sum_vox = 0, sum_trip = 0; bool any_nonfinite = false, any_trip = false;
  for (uint32_t t = 0; t < n_seg; t++) {
    qn::BatchSeg& g = sg[t];
    g = qn::BatchSeg{}; g.p0 = p0[t]; g.p1 = p0[t + 1]; g.sentinel = 1; g.tripped = 1; g.nvox = 0;
    const qn::BBoxOut bb = s->bt_bbox_host[t];
    nfin[t] = (g.p1 - g.p0) - bb.nonfinite;
    if (nfin[t]) {
      live[t] = 1; any_nonfinite |= bb.nonfinite != 0;
      long long cells = 1;
      if (voxel_dims(bb, leaf, &g.vd, &cells)) { g.tripped = 0; g.sentinel = (uint32_t)cells; g.nvox = nfin[t]; sum_vox += nfin[t]; }
      else { any_trip = true; trip_off[t] = (uint32_t)sum_trip; sum_trip += nfin[t]; }
    }
    lbits[t] = bits_for(g.sentinel);
  }
  if (any_nonfinite) s->last_error = "note: non-finite points dropped (pcl::VoxelGrid on a non-dense cloud)";
  if (any_trip) s->last_error = kOverflowWarning;
  if (sum_vox + sum_trip == 0) return QN_OK;                        // every submap empty
  // sort groups: consecutive submaps whose (submap, leaf) fields fit the 32 key bits above the point index
  struct Group { uint32_t s0, s1; int L, sb; };
  std::vector<Group> groups;
  { uint32_t g0 = 0; int L = 0;
    for (uint32_t t = 0; t < n_seg; t++) {
      const int L2 = std::max(L, lbits[t]);
      if (t > g0 && L2 + bits_for(t - g0) > 32) { groups.push_back(Group{g0, t, L, bits_for(t - 1 - g0)}); g0 = t; L = lbits[t]; }
      else L = L2;
    }
    groups.push_back(Group{g0, n_seg, L, bits_for(n_seg - 1 - g0)}); }
  for (const Group& gr : groups) for (uint32_t t = gr.s0; t < gr.s1; t++) sg[t].prefix = (t - gr.s0) << gr.L;
  if ((rc = map_grow(s, (void**)&s->bt_out, &s->bt_out_cap, sum_vox + sum_trip, sizeof(float4))) != QN_OK) return rc;
  KFCHK(s, hipMemcpyAsync(s->bt_segs, sg.data(), sizeof(qn::BatchSeg) * n_seg, hipMemcpyHostToDevice, st));
  const qn::MapKf* dkf = s->map_kfs; const uint32_t* dblk = s->map_blk; const uint32_t* dks = s->bt_kf_seg; const qn::BatchSeg* dsg = s->bt_segs;
  hipLaunchKernelGGL(qn::k_batch_keys, dim3(nt), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const float4*)s->concat, s->keys);
  // stable LSD passes over each group's (submap, leaf) bits only, on its own point range; every group's result ends in one buffer
  unsigned long long* fin = nullptr;
  for (const Group& gr : groups) {
    const uint32_t gp0 = p0[gr.s0], gn = p0[gr.s1] - gp0;
    if (!gn) continue;
    unsigned long long* sorted = s->keys + gp0; unsigned long long* other = s->keys_alt + gp0;
    const uint32_t rb = (gn + QN_MAP_TILE - 1) / QN_MAP_TILE, hn = rb * 256, hsb = (hn + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
    for (int shift = 32; shift < 32 + gr.L + gr.sb; shift += 8) {
      hipLaunchKernelGGL(qn::k_map_radix_hist, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, gn, shift, rb, s->hist);
      hipLaunchKernelGGL(qn::k_scan_block, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist, s->hist_sums);
      hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->hist_sums, hsb);
      hipLaunchKernelGGL(qn::k_scan_add, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist, hn, s->hist_sums, gn);
      hipLaunchKernelGGL(qn::k_map_radix_scatter, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, gn, shift, rb, (const uint32_t*)s->hist, other);
      std::swap(sorted, other);
    }
    unsigned long long* base = sorted - gp0;
    if (!fin) fin = base;
    else if (base != fin) KFCHK(s, hipMemcpyAsync(fin + gp0, sorted, sizeof(unsigned long long) * gn, hipMemcpyDeviceToDevice, st));
  }
  // leaves of all submaps at once: heads, exclusive scan, bounds, one thread per leaf
  const uint32_t sb = (n + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
  hipLaunchKernelGGL(qn::k_batch_leaf_flags, dim3(nt), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const unsigned long long*)fin, s->flag);
  hipLaunchKernelGGL(qn::k_scan_block, dim3(sb), dim3(QN_BLOCK), 0, st, s->flag, n, s->pos, s->sums);
  hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->sums, sb);
  hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sb), dim3(QN_BLOCK), 0, st, s->pos, n, s->sums, s->flag);
  if (sum_vox) {
    hipLaunchKernelGGL(qn::k_batch_leaf_bounds, dim3(nt), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const uint32_t*)s->flag, (const uint32_t*)s->pos, s->heads, s->bt_ends);
    hipLaunchKernelGGL(qn::k_batch_centroids, dim3((uint32_t)((sum_vox + 255) / 256)), dim3(256), 0, st, (const float4*)s->concat, (const unsigned long long*)fin,
                       (const uint32_t*)s->heads, (const uint32_t*)s->bt_ends, (const uint32_t*)(s->pos + n), s->bt_out);
  }
  for (uint32_t t = 0; t < n_seg; t++)                              // rare: tripped guards, their finite points unfiltered behind the leaves
    if (live[t] && sg[t].tripped)
      hipLaunchKernelGGL(qn::k_batch_gather, dim3((nfin[t] + 255) / 256), dim3(256), 0, st, (const unsigned long long*)fin + p0[t], nfin[t], (const float4*)s->concat, s->bt_out + sum_vox + trip_off[t]);
  hipLaunchKernelGGL(qn::k_batch_counts, dim3((n_seg + 255) / 256), dim3(256), 0, st, dsg, n_seg, (const uint32_t*)s->pos, s->bt_res);
  KFCHK(s, hipMemcpyAsync(s->bt_res_host, s->bt_res, sizeof(uint32_t) * 2 * n_seg, hipMemcpyDeviceToHost, st));
  KFCHK(s, hipGetLastError());
  KFCHK(s, hipStreamSynchronize(st));                               // sync 2 of 2: each submap's first leaf and leaf count
  for (uint32_t t = 0; t < n_seg; t++) {
    if (!live[t]) continue;
    const bool tr = sg[t].tripped != 0;
    s->bt_ptr[t] = s->bt_out + (tr ? sum_vox + trip_off[t] : s->bt_res_host[2 * t]);
    s->bt_n[t] = tr ? nfin[t] : s->bt_res_host[2 * t + 1];
    d_xyz_out[t] = (const float*)s->bt_ptr[t]; n_out[t] = s->bt_n[t]; status[t] = QN_OK;
  }
  return QN_OK;
}

extern "C" int qn_kf_batch_count(const qn_kf_store* s, uint32_t seg, uint32_t* n) {
  if (!s || !n || seg >= s->bt_n.size()) return QN_ERR_INVALID_ARG;
  *n = s->bt_n[seg];
  return QN_OK;
}
extern "C" int qn_kf_download_batch(qn_kf_store* s, uint32_t seg, float* xyz_out) {     // packed n x 3, for tests / visualisation
  if (!s || !xyz_out || seg >= s->bt_n.size()) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->bt_n[seg];
  if (!n) return QN_OK;
  KFCHK(s, hipSetDevice(s->device));
  KFCHK(s, hipMemcpy2D(xyz_out, 12, s->bt_ptr[seg], 16, 12, n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// LoopClosure::fetchClosestKeyframeIdx (loop_closure.cpp:34-56) generalised to the K best candidates (host code: O(#keyframes))
extern "C" int qn_loop_candidates(const double* pos_xyz, const double* stamps, uint32_t n, uint32_t query, double radius, double tdiff,
                                  uint32_t max_k, int32_t* out, uint32_t* n_out) {
  if (!pos_xyz || !stamps || !out || !n_out || query >= n) return QN_ERR_INVALID_ARG;
  std::vector<std::pair<double, int32_t>> c;
  for (uint32_t i = 0; i + 1 < n; i++) {                      // `keyframes.size() - 1`: the newest keyframe is the query itself
    const double dx = pos_xyz[3 * i] - pos_xyz[3 * query], dy = pos_xyz[3 * i + 1] - pos_xyz[3 * query + 1], dz = pos_xyz[3 * i + 2] - pos_xyz[3 * query + 2];
    const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (radius > d && tdiff < (stamps[query] - stamps[i])) c.emplace_back(d, (int32_t)i);
  }
  std::sort(c.begin(), c.end());
  uint32_t m = 0;
  for (const auto& e : c) { if (m >= max_k) break; out[m++] = e.second; }
  *n_out = m;
  return QN_OK;
}
