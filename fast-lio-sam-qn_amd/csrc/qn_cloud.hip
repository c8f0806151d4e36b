// qn_cloud.hip - the feeder of the hot path, on the GPU.  Own translation unit.
//   LoopClosure::setSrcAndDstCloud (fast_lio_sam_qn/src/loop_closure.cpp:58-108): per keyframe transformPcd
//   (include/utilities.hpp:164-175), concatenation, voxelizePcd = pcl::VoxelGrid (utilities.hpp:38-51);
//   LoopClosure::fetchClosestKeyframeIdx (loop_closure.cpp:34-56).
// Keyframe clouds (PosePcd::pcd_, sensor frame, immutable: include/pose_pcd.hpp:7-19) are uploaded ONCE into a store
// and stay resident in HBM; a loop attempt then assembles its source / target clouds on the device and hands the
// device pointers to qn_icp_alignment_device / the batch API - no point cloud crosses PCIe per attempt.
// ONE voxel-grid pipeline (voxel_submaps) serves all three entry points, each with its own output slot: qn_kf_assemble (one submap, slot
// 0 / 1), qn_kf_build_map (the corrected global map, fast_lio_sam_qn.cpp:302-316, 398-411, 435-448: one submap, intensity averaged) and
// qn_kf_assemble_batch (S submaps).  Every listed keyframe is transformed in one launch; one host sync brings each submap's bounding box
// back to size its grid.  VoxelGrid: 64-bit keys ((submap, leaf) << 32 | point index) are sorted with a hand-written STABLE LSD radix
// sort (8-bit digits, only as many passes as the keys have bits; the input is in ascending point order and stability keeps it so inside
// every leaf), leaf heads are compacted with the engine's own scan kernels and one thread per leaf sums its points in ascending point
// order in f32 - the order the oracle fixes (PCL's own order inside a leaf is unspecified).  A second sync brings the leaf counts back.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include <algorithm>
#include "../../include/qn_engine.h"
#include "qn_util_kernels.cuh"
#include "qn_kf_buf.h"

namespace qn {

struct VoxelDims { float inv; int minb[3]; int div0, div01; };
// Sized for 10^3 keyframes / 3e7 points: one transform launch for all keyframes, radix tiles of QN_MAP_TILE keys per block.
#define QN_MAP_TILE 4096
#define QN_MAP_ITEMS (QN_MAP_TILE / QN_BLOCK)
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the block's box (ordered ints) of its finite points and its non-finite count -> *dst, written by thread 0 (wave reductions, then one
// LDS row per wave in a fixed order: deterministic, no atomics).  Every thread of the block must call it.
__device__ __forceinline__ void block_bbox(int (&mn)[3], int (&mx)[3], int bad, BBoxOut* dst) {
  __shared__ int smn[QN_BLOCK / 64][3], smx[QN_BLOCK / 64][3], sbad[QN_BLOCK / 64];
#pragma unroll
  for (int d = 0; d < 3; d++) { mn[d] = wave_min_i(mn[d]); mx[d] = wave_max_i(mx[d]); }
  bad = wave_sum_i(bad);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { for (int d = 0; d < 3; d++) { smn[wid][d] = mn[d]; smx[wid][d] = mx[d]; } sbad[wid] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QN_BLOCK / 64; w++) { for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], smn[w][d]); mx[d] = max(mx[d], smx[w][d]); } bad += sbad[w]; }
    BBoxOut r; for (int d = 0; d < 3; d++) { r.mn[d] = mn[d]; r.mx[d] = mx[d]; } r.nonfinite = (uint32_t)bad;
    *dst = r;
  }
}
struct MapKf { const float4* src; uint32_t off, n, blk0, has_i; };     // one listed keyframe: its concatenation offset, first tile, pose = its list position
// transformPcd of every listed keyframe in ONE launch: tile b belongs to keyframe blk_kf[b] (f64 arithmetic, row by row in the order
// ((T0 x + T1 y) + T2 z) + T3); intensity = the resident .w for qn_kf_add_xyzi keyframes, 0 for qn_kf_add ones.  Fused: the tile's
// bounding box of the finite points and its count of non-finite ones -> part[b].
__global__ void __launch_bounds__(QN_BLOCK) k_map_transform(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const double* __restrict__ poses,
                                                            float4* __restrict__ out, BBoxOut* __restrict__ part) {
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
  block_bbox(mn, mx, bad, part + blockIdx.x);
}
// lanes of this wave whose digit equals mine (8 ballots), restricted to `valid` lanes
__device__ __forceinline__ unsigned long long match_digit8(uint32_t d, bool valid) {
  unsigned long long same = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) { const unsigned long long m = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? m : ~m; }
  return same;
}
// ---- stable LSD radix pass over bits [shift, shift + 8), kItems * QN_BLOCK keys per block (kItems = QN_MAP_ITEMS, or 1 for a small sort
// that would otherwise run on a handful of blocks): digit histogram in LDS (one LDS add per distinct digit of a wave, so a tile whose keys
// share their high digits does not serialise on one bank) ...
template <int kItems>
__global__ void __launch_bounds__(QN_BLOCK) k_map_radix_hist(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (kItems * QN_BLOCK) + threadIdx.x;
  const int lane = threadIdx.x & 63;
#pragma unroll 4
  for (int j = 0; j < kItems; j++) {
    const uint32_t i = base + j * QN_BLOCK;
    const bool valid = i < n;
    const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
    const unsigned long long same = match_digit8(d, valid);
    if (valid && (uint32_t)__popcll(same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&h[d], (uint32_t)__popcll(same));
  }
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];             // digit-major: the scan yields global offsets directly
}
// ... and the scatter: the tile is ranked in kItems rounds of QN_BLOCK consecutive keys (round order = key order, wave order inside a
// round, lane order inside a wave: stable), each digit's running output position kept in LDS across the rounds.
template <int kItems>
__global__ void __launch_bounds__(QN_BLOCK) k_map_radix_scatter(const unsigned long long* __restrict__ keys, uint32_t n, int shift, uint32_t nblocks,
                                                                const uint32_t* __restrict__ offs, unsigned long long* __restrict__ out) {
  __shared__ uint32_t wcount[QN_BLOCK / 64][256];
  __shared__ uint32_t run[256];
  for (int w = 0; w < QN_BLOCK / 64; w++) wcount[w][threadIdx.x] = 0;
  run[threadIdx.x] = offs[threadIdx.x * nblocks + blockIdx.x];
  const uint32_t base = blockIdx.x * (kItems * QN_BLOCK) + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long kv[kItems];
#pragma unroll
  for (int j = 0; j < kItems; j++) { const uint32_t i = base + j * QN_BLOCK; kv[j] = i < n ? keys[i] : 0ull; }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kItems; j++) {
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
// pack a strided PointXYZI-like host layout into float4 (x, y, z, intensity)
__global__ void k_pack_xyzi(const char* __restrict__ in, uint32_t stride, uint32_t ioff, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* r = in + (size_t)i * stride;
  const float* p = (const float*)r;
  out[i] = make_float4(p[0], p[1], p[2], *(const float*)(r + ioff));
}

// ---- the submaps of one call.  The listed keyframes of all submaps are transformed by k_map_transform (one launch; tiles never straddle
// keyframes, so a submap owns a contiguous tile range and a contiguous point range [p0, p1)).  Keys are ((seg << L | leaf) << 32 | point
// index): one stable sort orders every submap's points by leaf, finite points of a submap first (its non-finite ones carry the sentinel leaf).
struct BatchSeg { VoxelDims vd; uint32_t p0, p1, nvox, sentinel, prefix, tripped; };  // nvox: finite points that are voxelized (0 if tripped / empty)
// one block per submap over its tile range: the box of its finite points and its non-finite count, in a fixed order (no atomics)
__global__ void __launch_bounds__(QN_BLOCK) k_seg_bbox_reduce(const BBoxOut* __restrict__ part, const uint32_t* __restrict__ tile_off, BBoxOut* __restrict__ out) {
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int bad = 0;
  const uint32_t b1 = tile_off[blockIdx.x + 1];
  for (uint32_t b = tile_off[blockIdx.x] + threadIdx.x; b < b1; b += QN_BLOCK) {
    const BBoxOut r = part[b];
    for (int d = 0; d < 3; d++) { mn[d] = min(mn[d], r.mn[d]); mx[d] = max(mx[d], r.mx[d]); }
    bad += (int)r.nonfinite;
  }
  block_bbox(mn, mx, bad, out + blockIdx.x);
}
// the per-position kernels below run QN_MAP_ITEMS blocks per tile, one position per thread (one block per tile would walk 16 positions per
// thread: latency-bound on a small cloud); block b covers positions [(b % QN_MAP_ITEMS) * QN_BLOCK, + QN_BLOCK) of tile b / QN_MAP_ITEMS
__device__ __forceinline__ uint32_t tile_pos(const MapKf& f) {
  return (blockIdx.x / QN_MAP_ITEMS - f.blk0) * QN_MAP_TILE + (blockIdx.x % QN_MAP_ITEMS) * QN_BLOCK + threadIdx.x;
}
// keys, one position per thread: pcl::VoxelGrid's leaf index of a finite point from the submap's grid; the submap's sentinel for a non-finite
// point (the stable sort moves it behind all finite points, in its original order, and the leaf pass stops before it: no compaction pass);
// leaf 0 for every finite point of a submap whose guard tripped (the stable sort then keeps them in concatenation order for the gather)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_keys(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                         const BatchSeg* __restrict__ segs, const float4* __restrict__ pts, unsigned long long* __restrict__ keys) {
  const uint32_t k = blk_kf[blockIdx.x / QN_MAP_ITEMS];
  const MapKf f = kfs[k];
  const uint32_t i = tile_pos(f);
  if (i >= f.n) return;
  const BatchSeg sg = segs[kf_seg[k]];
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
// leaf heads over the sorted keys: a head is a voxelized position whose leaf differs from its predecessor's
// or that opens its submap (the submap field alone would not separate two submaps of different sort groups)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_leaf_flags(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                               const BatchSeg* __restrict__ segs, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ flag) {
  const uint32_t k = blk_kf[blockIdx.x / QN_MAP_ITEMS];
  const MapKf f = kfs[k];
  const uint32_t i = tile_pos(f);
  if (i >= f.n) return;
  const BatchSeg sg = segs[kf_seg[k]];
  const uint32_t g = f.off + i, fe = sg.p0 + sg.nvox;
  flag[g] = (g < fe && (g == sg.p0 || (keys[g] >> 32) != (keys[g - 1] >> 32))) ? 1u : 0u;
}
// after the exclusive scan pos of the flags: leaf m = [heads[m], ends[m]) (its position in the output = its rank over all submaps)
__global__ void __launch_bounds__(QN_BLOCK) k_batch_leaf_bounds(const MapKf* __restrict__ kfs, const uint32_t* __restrict__ blk_kf, const uint32_t* __restrict__ kf_seg,
                                                                const BatchSeg* __restrict__ segs, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                                uint32_t* __restrict__ heads, uint32_t* __restrict__ ends) {
  const uint32_t k = blk_kf[blockIdx.x / QN_MAP_ITEMS];
  const MapKf f = kfs[k];
  const uint32_t i = tile_pos(f);
  if (i >= f.n) return;
  const BatchSeg sg = segs[kf_seg[k]];
  const uint32_t g = f.off + i, fe = sg.p0 + sg.nvox;
  if (g >= fe) return;
  const uint32_t fl = flag[g], m = pos[g] + fl - 1;
  if (fl) heads[m] = g;
  if (g + 1 == fe || flag[g + 1]) ends[m] = g + 1;
}
// one thread per leaf: f32 sums of x, y, z (and intensity when kIntensity) in ascending concatenation order, each / (float)count; w = the
// mean intensity (a NaN intensity poisons its leaf's) or 1
template <bool kIntensity>
__global__ void k_batch_centroids(const float4* __restrict__ pts, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ heads,
                                  const uint32_t* __restrict__ ends, const uint32_t* __restrict__ nleaf_ptr, float4* __restrict__ out) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= *nleaf_ptr) return;
  const uint32_t a = heads[m], b = ends[m];
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  for (uint32_t t = a; t < b; t++) {
    const float4 p = pts[(uint32_t)keys[t]]; sx = sx + p.x; sy = sy + p.y; sz = sz + p.z;
    if (kIntensity) si = si + p.w;
  }
  const float cnt = (float)(b - a);
  out[m] = make_float4(sx / cnt, sy / cnt, sz / cnt, kIntensity ? si / cnt : 1.0f);
}
// each submap's first leaf and leaf count: res[2 s] = first, res[2 s + 1] = count
__global__ void k_batch_counts(const BatchSeg* __restrict__ segs, uint32_t nseg, const uint32_t* __restrict__ pos, uint32_t* __restrict__ res) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t a = pos[segs[s].p0];
  res[2 * s] = a; res[2 * s + 1] = pos[segs[s].p1] - a;
}
// a tripped submap under the finite-points rule: its finite points (the first n of its sorted range, in concatenation order), unfiltered, w = 1
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
  DevBuf<char> staging;                                                                         // qn_kf_add's upload
  // scratch of the voxel-grid pipeline (voxel_submaps), shared by every entry point: per point, per scan block / radix histogram entry,
  // per tile (its box), per submap (box, leaf range); the call's tables (Tables) in one device buffer, uploaded from one pinned buffer
  DevBuf<float4> concat; DevBuf<unsigned long long> keys, keys_alt; DevBuf<uint32_t> flag, pos, heads, ends;
  DevBuf<uint32_t> sums, hist, hist_sums; DevBuf<qn::BBoxOut> tile_box, seg_box; DevBuf<uint32_t> seg_res;
  DevBuf<char> tab; PinBuf<char> tab_host; PinBuf<qn::BBoxOut> seg_box_host; PinBuf<uint32_t> seg_res_host;
  // the output slots: qn_kf_assemble's 0 / 1, the corrected global map, qn_kf_assemble_batch's (all submaps in one buffer)
  DevBuf<float4> out[2]; uint32_t out_n[2] = {0, 0};
  DevBuf<float4> map; uint32_t map_n = 0; uint64_t map_gen = 0;                                 // map_gen: advanced by every attempt to build a map
  DevBuf<float4> bt_out; std::vector<const float4*> bt_ptr; std::vector<uint32_t> bt_n;
  // scratch of other translation units (the ray-caster, qn_sim.hip), in bytes, sized exactly as asked: see qn_kf_internal.h
  DevBuf<char> int_scratch[QN_KF_INT_SCRATCH]; PinBuf<char> int_pinned;
  void* ext[QN_KF_INT_EXT] = {}; qn_kf_int_release_fn ext_release[QN_KF_INT_EXT] = {};      // state of other translation units (qn_sc.hip)
  std::string last_error;
};
extern "C" int qn_kf_store_create(int device, qn_kf_store** out) {
  if (!out) return QN_ERR_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return QN_ERR_NO_DEVICE;
  qn_kf_store* s = new qn_kf_store(); s->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { delete s; return QN_ERR_HIP; }
  *out = s;
  return QN_OK;
}
extern "C" void qn_kf_store_destroy(qn_kf_store* s) {
  if (!s) return;
  (void)hipSetDevice(s->device); if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (float4* p : s->clouds) (void)hipFree(p);
  for (int k = 0; k < QN_KF_INT_EXT; k++) if (s->ext[k] && s->ext_release[k]) s->ext_release[k](s->ext[k]);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;                                                          // (every buffer of the store goes with its member)
}
extern "C" const char* qn_kf_last_error(const qn_kf_store* s) { return s ? s->last_error.c_str() : "null store"; }

// upload one keyframe cloud (sensor frame) - PosePcd::pcd_ - and keep it resident; ioff < 0: xyz only (.w = 1), else the intensity's byte offset
static int kf_add(qn_kf_store* s, const float* xyz, uint32_t n, uint32_t stride, int ioff, int32_t* id_out) {
  QN_KFCHK(s, hipSetDevice(s->device));
  float4* d = nullptr;
  if (n) {
    const size_t bytes = (size_t)(n - 1) * stride + (ioff < 0 ? 12 : std::max(12, ioff + 4));
    if (!s->staging.grow(s, bytes)) return QN_ERR_HIP;
    QN_KFCHK(s, hipMalloc(&d, sizeof(float4) * n));
    QN_KFCHK(s, hipMemcpyAsync(s->staging.p, xyz, bytes, hipMemcpyHostToDevice, s->stream));
    if (ioff < 0) hipLaunchKernelGGL(qn::k_pack_points, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->staging.p, stride, n, d);
    else hipLaunchKernelGGL(qn::k_pack_xyzi, dim3((n + 255) / 256), dim3(256), 0, s->stream, (const char*)s->staging.p, stride, (uint32_t)ioff, n, d);
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
  QN_KFCHK(s, hipSetDevice(s->device));
  float4* d = nullptr;
  QN_KFCHK(s, hipMalloc(&d, sizeof(float4) * n));
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
  if (which < 0 || which >= QN_KF_INT_SCRATCH || !s->int_scratch[which].grow(s, bytes, true)) return nullptr;
  return s->int_scratch[which].p;
}
const float4* qn_kf_int_keyframe(const qn_kf_store* s, int32_t id, uint32_t* n) { *n = s->sizes[id]; return s->clouds[id]; }
bool qn_kf_int_has_intensity(const qn_kf_store* s, int32_t id) { return s->has_i[id] != 0; }
void* qn_kf_int_ext(const qn_kf_store* s, int which) { return which >= 0 && which < QN_KF_INT_EXT ? s->ext[which] : nullptr; }
void qn_kf_int_set_ext(qn_kf_store* s, int which, void* p, qn_kf_int_release_fn release) {
  if (which < 0 || which >= QN_KF_INT_EXT) return;
  if (s->ext[which] && s->ext_release[which] && s->ext[which] != p) s->ext_release[which](s->ext[which]);
  s->ext[which] = p; s->ext_release[which] = release;
}
void* qn_kf_int_pinned(qn_kf_store* s, size_t bytes) { return s->int_pinned.grow(s, bytes, true) ? s->int_pinned.p : nullptr; }
extern "C" int qn_kf_add_device(qn_kf_store* s, const float* d_pts, uint32_t n, uint32_t stride, int32_t ioff, int32_t* id_out) {
  if (!s || !id_out || (n && !d_pts) || !device_layout_ok(stride, ioff) || ((uintptr_t)d_pts & 3)) return QN_ERR_INVALID_ARG;
  if (n) {        // the records must lie inside one device allocation of this store's device: a host pointer here would fault the GPU
    QN_KFCHK(s, hipSetDevice(s->device));
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
  QN_KFCHK(s, hipSetDevice(s->device));
  QN_KFCHK(s, hipMemcpy(xyzi_out, s->clouds[id], sizeof(float4) * n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// pcl::VoxelGrid::applyFilter's grid from the bounding box of the finite points: leaf-index origin and divisions, number of cells;
// returns false when the guard trips (PCL warns and sets output = *input_).  The guard, the same rule in the oracle (orc_voxel_guard) and the numpy
// restatement (voxel_guard, tests/test_kf_map_api.py), with inv = 1 / (float)leaf and everything below in f32 unless said otherwise - tripped when
//   (1) on any axis floor(min * inv) or floor(max * inv) is outside [-2^31, 2^31)            [deviation from PCL, which converts them to int unchecked]
//   (2) on any axis (max - min) * inv is not below 2^63, infinite or NaN included            [deviation from PCL, which converts it to int64 unchecked]
//   (3) pd = the product over the axes of int64((max - min) * inv) + 1 exceeds INT32_MAX     [PCL's own guard]
//   (4) cells = the product over the axes of floor(max * inv) - floor(min * inv) + 1 exceeds INT32_MAX   [deviation: PCL's index wraps; the keys need cells < 2^31]
// Every comparison is made in floating point before the conversion and the products leave at the first factor or partial product above INT32_MAX, so
// no conversion is out of range and no integer overflows.  Not tripped implies every leaf index k_batch_keys forms lies in [0, cells).
static bool voxel_dims(const qn::BBoxOut& bb, double leaf, qn::VoxelDims* vd, long long* cells_out) {
  vd->inv = 1.0f / (float)leaf;
  *cells_out = 0;
  const float two31 = 2147483648.0f, two63 = 9223372036854775808.0f;
  long long cells = 1, pd = 1; int divb[3];
  for (int d = 0; d < 3; d++) {
    const float mn = qn::ord2f(bb.mn[d]), mx = qn::ord2f(bb.mx[d]);
    const float lo = std::floor(mn * vd->inv), hi = std::floor(mx * vd->inv), ext = (mx - mn) * vd->inv;
    if (!(lo >= -two31 && lo < two31 && hi >= -two31 && hi < two31)) return false;
    if (!(ext < two63)) return false;
    const long long div = (long long)hi - (long long)lo + 1, pdf = (long long)ext + 1;
    if (pdf > (long long)INT32_MAX || div > (long long)INT32_MAX) return false;
    pd *= pdf; cells *= div;                                         // both factors <= INT32_MAX: no product above 2^62
    if (pd > (long long)INT32_MAX || cells > (long long)INT32_MAX) return false;
    vd->minb[d] = (int)lo; divb[d] = (int)div;
  }
  *cells_out = cells;
  vd->div0 = divb[0]; vd->div01 = divb[0] * divb[1];
  return true;
}
static const char* kOverflowWarning = "warning: leaf size is too small for the input dataset, integer indices would overflow: cloud passed through unfiltered (as pcl::VoxelGrid does)";
static const char* kNonFiniteNote = "note: non-finite points dropped (pcl::VoxelGrid on a non-dense cloud)";

static int bits_for(unsigned long long v) { int b = 0; while (b < 64 && (1ull << b) <= v) b++; return b; }      // smallest b with v < 2^b
static uint32_t tiles_of(size_t n) { return (uint32_t)((n + QN_MAP_TILE - 1) / QN_MAP_TILE); }
static uint32_t scan_blocks(size_t n) { return (uint32_t)((n + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS)); }
// keys per thread of the radix passes over n keys: QN_MAP_TILE-key tiles fill the chip's 256 CUs from 2^20 keys on; below that (one
// keyframe, a small submap) one key per thread, or the passes would run on a handful of blocks
static int radix_items(uint32_t n) { return n < 256u * QN_MAP_TILE ? 1 : QN_MAP_ITEMS; }
static uint32_t radix_blocks(uint32_t n) { const uint32_t tile = radix_items(n) * QN_BLOCK; return (n + tile - 1) / tile; }
static bool ids_valid(const qn_kf_store* s, const int32_t* ids, uint32_t a, uint32_t b) {
  for (uint32_t j = a; j < b; j++) if (ids[j] < 0 || (size_t)ids[j] >= s->clouds.size()) return false;
  return true;
}

// ---- the segment-tagged stable sort of the voxel-grid pipeline, as functions (voxel_submaps and the cell index of qn_kf_int_cell_index use them).
// sort groups: consecutive segments whose (segment, leaf) fields fit the 32 key bits above the point index; lbits[t] = the leaf bits segment t needs,
// p0[t] its first point.  Sets every segment's key prefix.
struct SortGroup { uint32_t s0, s1; int L, sb; };
static std::vector<SortGroup> sort_groups(const std::vector<int>& lbits, uint32_t n_seg, qn::BatchSeg* sg, const std::vector<uint32_t>& p0) {
  std::vector<SortGroup> groups;
  { uint32_t g0 = 0; int L = 0;
    for (uint32_t t = 0; t < n_seg; t++) {
      const int L2 = std::max(L, lbits[t]);
      if (t > g0 && L2 + bits_for(t - g0) > 32) { groups.push_back(SortGroup{g0, t, L, bits_for(t - 1 - g0)}); g0 = t; L = lbits[t]; }
      else L = L2;
    }
    groups.push_back(SortGroup{g0, n_seg, L, bits_for(n_seg - 1 - g0)}); }
  for (const SortGroup& gr : groups)
    for (uint32_t t = gr.s0; t < gr.s1; t++) sg[t].prefix = (t - gr.s0) << gr.L;
  return groups;
}
// the digit-major block histograms of the largest radix pass
static bool sort_scratch(qn_kf_store* s, const std::vector<SortGroup>& groups, const std::vector<uint32_t>& p0) {
  size_t hn = 0;
  for (const SortGroup& gr : groups) hn = std::max<size_t>(hn, 256 * (size_t)radix_blocks(p0[gr.s1] - p0[gr.s0]));
  return s->hist.grow(s, hn + 1) && s->hist_sums.grow(s, scan_blocks(hn));
}
// stable LSD passes over each group's (segment, leaf) bits only, on its own point range of s->keys; every group's result ends in one buffer, *fin
static int sort_segments(qn_kf_store* s, const std::vector<SortGroup>& groups, const std::vector<uint32_t>& p0, unsigned long long** fin_out) {
  hipStream_t st = s->stream;
  unsigned long long* fin = nullptr;
  for (const SortGroup& gr : groups) {
    const uint32_t gp0 = p0[gr.s0], gn = p0[gr.s1] - gp0;
    if (!gn) continue;
    unsigned long long* sorted = s->keys.p + gp0; unsigned long long* other = s->keys_alt.p + gp0;
    const bool small = radix_items(gn) == 1;
    const uint32_t rb = radix_blocks(gn), ghn = rb * 256, hsb = scan_blocks(ghn);
    for (int shift = 32; shift < 32 + gr.L + gr.sb; shift += 8) {
      hipLaunchKernelGGL(small ? qn::k_map_radix_hist<1> : qn::k_map_radix_hist<QN_MAP_ITEMS>, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, gn, shift, rb, s->hist.p);
      hipLaunchKernelGGL(qn::k_scan_block, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist.p, ghn, s->hist.p, s->hist_sums.p);
      hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->hist_sums.p, hsb);
      hipLaunchKernelGGL(qn::k_scan_add, dim3(hsb), dim3(QN_BLOCK), 0, st, s->hist.p, ghn, s->hist_sums.p, gn);
      hipLaunchKernelGGL(small ? qn::k_map_radix_scatter<1> : qn::k_map_radix_scatter<QN_MAP_ITEMS>, dim3(rb), dim3(QN_BLOCK), 0, st, (const unsigned long long*)sorted, gn, shift, rb,
                         (const uint32_t*)s->hist.p, other);
      std::swap(sorted, other);
    }
    unsigned long long* base = sorted - gp0;
    if (!fin) fin = base;
    else if (base != fin) QN_KFCHK(s, hipMemcpyAsync(fin + gp0, sorted, sizeof(unsigned long long) * gn, hipMemcpyDeviceToDevice, st));
  }
  *fin_out = fin;
  return QN_OK;
}

// ---- the one voxel-grid pipeline.  Submap t = the sources src[seg_off[t] .. seg_off[t + 1]) with the poses of the same entries, transformed,
// concatenated in list order and voxel-grid at `leaf`, every submap into `out` (the caller's slot).  A source is (records, count, has intensity):
// a resident keyframe for the callers that list ids (sources_of), or any device records of the same layout (qn_kf_int_build_map_from).
// carry_intensity: the centroids average .w (the map), else w = 1.  A submap that trips PCL's overflow guard is passed through behind the
// leaves: trip_whole = its whole concatenation, non-finite points and intensity included (the map: output = *input_), else its finite points
// in concatenation order with w = 1 (assemble, batch).  res[t] = its records, their count and QN_OK, or QN_ERR_EMPTY_CLOUD when it has no
// finite point; notes = what the callers may put in last_error.  Two host synchronisations: the per-submap boxes (grid sizes, sort bits),
// then the per-submap leaf counts.  Submaps are sorted in groups whose keys fit 32 bits - normally one group.
struct SubmapOut { const float4* ptr; uint32_t n; int status; };
// byte offsets of the call's tables in s->tab / s->tab_host: the poses, one row per listed keyframe, tile -> keyframe, keyframe -> submap,
// each submap's first tile (n_seg + 1), then the submap grids (uploaded after sync 1); every table 16-byte aligned
struct Tables {
  size_t pose, kf, blk, kseg, toff, seg, end;
  Tables(uint32_t count, size_t tiles, uint32_t n_seg) {
    pose = 0; kf = qn_up16(sizeof(double) * 16 * count); blk = qn_up16(kf + sizeof(qn::MapKf) * count); kseg = qn_up16(blk + 4 * tiles);
    toff = qn_up16(kseg + 4 * (size_t)count); seg = qn_up16(toff + 4 * ((size_t)n_seg + 1)); end = seg + sizeof(qn::BatchSeg) * n_seg;
  }
};
struct VoxelNotes { bool nonfinite, tripped; };      // a voxelized or tripped submap had non-finite points / some submap tripped the guard
struct VoxSrc { const float4* pts; uint32_t n; uint8_t has_i; };
// the resident keyframes ids[a .. b) (ids already checked) as sources, at the same positions a .. b of the result
static std::vector<VoxSrc> sources_of(const qn_kf_store* s, const int32_t* ids, uint32_t a, uint32_t b) {
  std::vector<VoxSrc> v(b);
  for (uint32_t j = a; j < b; j++) v[j] = VoxSrc{s->clouds[ids[j]], s->sizes[ids[j]], s->has_i[ids[j]]};
  return v;
}
static int voxel_submaps(qn_kf_store* s, const VoxSrc* src, const double* poses, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                         bool carry_intensity, bool trip_whole, DevBuf<float4>& out, SubmapOut* res, VoxelNotes* notes) {
  const uint32_t e0 = seg_off[0], count = seg_off[n_seg] - e0;
  size_t total = 0, tiles = 0;
  for (uint32_t j = e0; j < e0 + count; j++) { total += src[j].n; tiles += tiles_of(src[j].n); }
  for (uint32_t t = 0; t < n_seg; t++) res[t] = SubmapOut{nullptr, 0, QN_ERR_EMPTY_CLOUD};
  *notes = VoxelNotes{false, false};
  if (total >= 0xffffffffull) return QN_ERR_CAPACITY;
  if (total == 0) return QN_OK;
  QN_KFCHK(s, hipSetDevice(s->device));
  const uint32_t n = (uint32_t)total, nt = (uint32_t)tiles;
  const Tables tb(count, tiles, n_seg);
  if (!s->concat.grow(s, n) || !s->keys.grow(s, n) || !s->keys_alt.grow(s, n) || !s->flag.grow(s, n) || !s->pos.grow(s, n + 1) ||
      !s->heads.grow(s, n) || !s->ends.grow(s, n) || !s->sums.grow(s, scan_blocks(n)) || !s->tile_box.grow(s, nt) ||
      !s->seg_box.grow(s, n_seg) || !s->seg_res.grow(s, 2 * (size_t)n_seg) || !s->tab.grow(s, tb.end) || !s->tab_host.grow(s, tb.end) ||
      !s->seg_box_host.grow(s, n_seg) || !s->seg_res_host.grow(s, 2 * (size_t)n_seg)) return QN_ERR_HIP;
  // the tables in pinned memory (host, O(count + tiles)): poses, keyframe rows, tile -> keyframe, keyframe -> submap, each submap's tile range
  char* h = s->tab_host.p;
  qn::MapKf* kfs = (qn::MapKf*)(h + tb.kf); uint32_t* blk = (uint32_t*)(h + tb.blk); uint32_t* kseg = (uint32_t*)(h + tb.kseg); uint32_t* toff = (uint32_t*)(h + tb.toff);
  std::copy(poses + 16 * (size_t)e0, poses + 16 * ((size_t)e0 + count), (double*)(h + tb.pose));
  std::vector<uint32_t> p0(n_seg + 1);                              // each submap's point range
  uint32_t off = 0, b0 = 0;
  for (uint32_t t = 0; t < n_seg; t++) {
    toff[t] = b0; p0[t] = off;
    for (uint32_t j = seg_off[t]; j < seg_off[t + 1]; j++) {
      const uint32_t k = j - e0, nk = src[j].n, ntk = tiles_of(nk);
      kfs[k] = qn::MapKf{src[j].pts, off, nk, b0, src[j].has_i}; kseg[k] = t;
      for (uint32_t b = 0; b < ntk; b++) blk[b0 + b] = k;
      off += nk; b0 += ntk;
    }
  }
  toff[n_seg] = b0; p0[n_seg] = off;
  hipStream_t st = s->stream;
  QN_KFCHK(s, hipMemcpyAsync(s->tab.p, h, tb.seg, hipMemcpyHostToDevice, st));
  // transformPcd + operator+= of every listed keyframe of every submap (loop_closure.cpp:76,83,89,92,102), per-tile boxes, per-submap reduce
  const char* d = s->tab.p;
  const qn::MapKf* dkf = (const qn::MapKf*)(d + tb.kf); const uint32_t* dblk = (const uint32_t*)(d + tb.blk); const uint32_t* dks = (const uint32_t*)(d + tb.kseg);
  const qn::BatchSeg* dsg = (const qn::BatchSeg*)(d + tb.seg);
  hipLaunchKernelGGL(qn::k_map_transform, dim3(nt), dim3(QN_BLOCK), 0, st, dkf, dblk, (const double*)(d + tb.pose), s->concat.p, s->tile_box.p);
  hipLaunchKernelGGL(qn::k_seg_bbox_reduce, dim3(n_seg), dim3(QN_BLOCK), 0, st, (const qn::BBoxOut*)s->tile_box.p, (const uint32_t*)(d + tb.toff), s->seg_box.p);
  QN_KFCHK(s, hipMemcpyAsync(s->seg_box_host.p, s->seg_box.p, sizeof(qn::BBoxOut) * n_seg, hipMemcpyDeviceToHost, st));
  QN_KFCHK(s, hipStreamSynchronize(st));                            // sync 1 of 2: each submap's box sizes its grid
  // per submap: pcl::VoxelGrid's grid and overflow guard (voxel_dims), its sentinel leaf and the key bits it needs
  qn::BatchSeg* sg = (qn::BatchSeg*)(h + tb.seg); std::vector<int> lbits(n_seg); std::vector<uint32_t> nfin(n_seg), ntrip(n_seg, 0), trip_off(n_seg, 0);
  std::vector<uint8_t> live(n_seg, 0);
  size_t sum_vox = 0, sum_trip = 0;
  for (uint32_t t = 0; t < n_seg; t++) {
    qn::BatchSeg& g = sg[t];
    g = qn::BatchSeg{}; g.p0 = p0[t]; g.p1 = p0[t + 1]; g.sentinel = 1; g.tripped = 1; g.nvox = 0;
    const qn::BBoxOut bb = s->seg_box_host.p[t];
    nfin[t] = (g.p1 - g.p0) - bb.nonfinite;
    if (nfin[t]) {
      live[t] = 1; notes->nonfinite |= bb.nonfinite != 0;
      long long cells = 1;
      if (voxel_dims(bb, leaf, &g.vd, &cells)) { g.tripped = 0; g.sentinel = (uint32_t)cells; g.nvox = nfin[t]; sum_vox += nfin[t]; }
      else { notes->tripped = true; ntrip[t] = trip_whole ? g.p1 - g.p0 : nfin[t]; trip_off[t] = (uint32_t)sum_trip; sum_trip += ntrip[t]; }
    }
    lbits[t] = bits_for(bb.nonfinite ? g.sentinel : g.sentinel - 1);  // the sentinel leaf needs key bits only when some point carries it
  }
  if (sum_vox + sum_trip == 0) return QN_OK;                        // every submap empty
  const std::vector<SortGroup> groups = sort_groups(lbits, n_seg, sg, p0);
  if (!out.grow(s, sum_vox + sum_trip) || !sort_scratch(s, groups, p0)) return QN_ERR_HIP;
  QN_KFCHK(s, hipMemcpyAsync(s->tab.p + tb.seg, sg, tb.end - tb.seg, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(qn::k_batch_keys, dim3(nt * QN_MAP_ITEMS), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const float4*)s->concat.p, s->keys.p);
  unsigned long long* fin = nullptr;
  { const int src = sort_segments(s, groups, p0, &fin); if (src != QN_OK) return src; }
  // leaves of all submaps at once: heads, exclusive scan, bounds, one thread per leaf
  const uint32_t sb = scan_blocks(n);
  hipLaunchKernelGGL(qn::k_batch_leaf_flags, dim3(nt * QN_MAP_ITEMS), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const unsigned long long*)fin, s->flag.p);
  hipLaunchKernelGGL(qn::k_scan_block, dim3(sb), dim3(QN_BLOCK), 0, st, s->flag.p, n, s->pos.p, s->sums.p);
  hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, s->sums.p, sb);
  hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sb), dim3(QN_BLOCK), 0, st, s->pos.p, n, s->sums.p, s->flag.p);
  if (sum_vox) {
    hipLaunchKernelGGL(qn::k_batch_leaf_bounds, dim3(nt * QN_MAP_ITEMS), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const uint32_t*)s->flag.p, (const uint32_t*)s->pos.p, s->heads.p, s->ends.p);
    const dim3 cg((uint32_t)((sum_vox + 255) / 256));
    if (carry_intensity) hipLaunchKernelGGL(qn::k_batch_centroids<true>, cg, dim3(256), 0, st, (const float4*)s->concat.p, (const unsigned long long*)fin,
                                            (const uint32_t*)s->heads.p, (const uint32_t*)s->ends.p, (const uint32_t*)(s->pos.p + n), out.p);
    else hipLaunchKernelGGL(qn::k_batch_centroids<false>, cg, dim3(256), 0, st, (const float4*)s->concat.p, (const unsigned long long*)fin,
                            (const uint32_t*)s->heads.p, (const uint32_t*)s->ends.p, (const uint32_t*)(s->pos.p + n), out.p);
  }
  for (uint32_t t = 0; t < n_seg; t++) {                            // rare: tripped guards, passed through behind the leaves
    if (!live[t] || !sg[t].tripped) continue;
    float4* dst = out.p + sum_vox + trip_off[t];
    if (trip_whole) QN_KFCHK(s, hipMemcpyAsync(dst, s->concat.p + p0[t], sizeof(float4) * ntrip[t], hipMemcpyDeviceToDevice, st));
    else hipLaunchKernelGGL(qn::k_batch_gather, dim3((ntrip[t] + 255) / 256), dim3(256), 0, st, (const unsigned long long*)fin + p0[t], ntrip[t], (const float4*)s->concat.p, dst);
  }
  hipLaunchKernelGGL(qn::k_batch_counts, dim3((n_seg + 255) / 256), dim3(256), 0, st, dsg, n_seg, (const uint32_t*)s->pos.p, s->seg_res.p);
  QN_KFCHK(s, hipMemcpyAsync(s->seg_res_host.p, s->seg_res.p, sizeof(uint32_t) * 2 * n_seg, hipMemcpyDeviceToHost, st));
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipStreamSynchronize(st));                            // sync 2 of 2: each submap's first leaf and leaf count
  for (uint32_t t = 0; t < n_seg; t++) {
    if (!live[t]) continue;
    const bool tr = sg[t].tripped != 0;
    res[t] = SubmapOut{out.p + (tr ? sum_vox + trip_off[t] : s->seg_res_host.p[2 * t]), tr ? ntrip[t] : s->seg_res_host.p[2 * t + 1], QN_OK};
  }
  return QN_OK;
}

// ---- a sorted-key cell index over arbitrary device clouds, for bounded-radius searches (qn_overlap.hip): the front half of the voxel-grid pipeline with
// every cloud as its own segment under the identity pose - the same transform / box kernels, voxel_dims(), segment-tagged keys and stable radix passes.
// The cell edge of a cloud is at least (radius + 2^-21 max|coordinate|) (1 + 1e-5): two points whose f32 squared distance is <= float(radius^2) are at most
// radius (1 + 2^-21) apart along an axis, and their f32 cell coordinates floor(x * inv) each carry a rounding error of at most 2^-24 of their size
// (<= max|coordinate| / edge), so the two coordinates differ by at most 1 and the partner lies in the 3 x 3 x 3 block around the query's cell.  The edge is
// widened by a quarter at a time while the cloud's cell count needs more than QN_CELL_LEAF_BITS key bits (or trips voxel_dims' own guard): it depends on the
// cloud and the radius alone, never on the other clouds of the call.  One host synchronisation (the boxes).  The index lives in the pipeline's scratch.
#define QN_CELL_LEAF_BITS 26
int qn_kf_int_cell_index(qn_kf_store* s, const float4* const* clouds, const uint32_t* n_pts, uint32_t count, double radius,
                         qn_kf_int_cell_grid* grids, const float4** points, const unsigned long long** keys) {
  size_t total = 0, tiles = 0;
  for (uint32_t k = 0; k < count; k++) { total += n_pts[k]; tiles += tiles_of(n_pts[k]); grids[k] = qn_kf_int_cell_grid{}; }
  *points = nullptr; *keys = nullptr;
  if (total >= 0xffffffffull) return QN_ERR_CAPACITY;
  if (total == 0) return QN_OK;
  QN_KFCHK(s, hipSetDevice(s->device));
  const uint32_t n = (uint32_t)total, nt = (uint32_t)tiles;
  const Tables tb(count, tiles, count);
  if (!s->concat.grow(s, n) || !s->keys.grow(s, n) || !s->keys_alt.grow(s, n) || !s->tile_box.grow(s, nt) || !s->seg_box.grow(s, count) ||
      !s->tab.grow(s, tb.end) || !s->tab_host.grow(s, tb.end) || !s->seg_box_host.grow(s, count)) return QN_ERR_HIP;
  char* h = s->tab_host.p;
  qn::MapKf* kfs = (qn::MapKf*)(h + tb.kf); uint32_t* blk = (uint32_t*)(h + tb.blk); uint32_t* kseg = (uint32_t*)(h + tb.kseg); uint32_t* toff = (uint32_t*)(h + tb.toff);
  double* pose = (double*)(h + tb.pose);
  std::vector<uint32_t> p0(count + 1);
  uint32_t off = 0, b0 = 0;
  for (uint32_t k = 0; k < count; k++) {
    for (int i = 0; i < 16; i++) pose[16 * (size_t)k + i] = (i % 5 == 0) ? 1.0 : 0.0;
    const uint32_t ntk = tiles_of(n_pts[k]);
    toff[k] = b0; p0[k] = off; kseg[k] = k;
    kfs[k] = qn::MapKf{clouds[k], off, n_pts[k], b0, 0};
    for (uint32_t b = 0; b < ntk; b++) blk[b0 + b] = k;
    off += n_pts[k]; b0 += ntk;
  }
  toff[count] = b0; p0[count] = off;
  hipStream_t st = s->stream;
  QN_KFCHK(s, hipMemcpyAsync(s->tab.p, h, tb.seg, hipMemcpyHostToDevice, st));
  const char* d = s->tab.p;
  const qn::MapKf* dkf = (const qn::MapKf*)(d + tb.kf); const uint32_t* dblk = (const uint32_t*)(d + tb.blk); const uint32_t* dks = (const uint32_t*)(d + tb.kseg);
  const qn::BatchSeg* dsg = (const qn::BatchSeg*)(d + tb.seg);
  hipLaunchKernelGGL(qn::k_map_transform, dim3(nt), dim3(QN_BLOCK), 0, st, dkf, dblk, (const double*)(d + tb.pose), s->concat.p, s->tile_box.p);
  hipLaunchKernelGGL(qn::k_seg_bbox_reduce, dim3(count), dim3(QN_BLOCK), 0, st, (const qn::BBoxOut*)s->tile_box.p, (const uint32_t*)(d + tb.toff), s->seg_box.p);
  QN_KFCHK(s, hipMemcpyAsync(s->seg_box_host.p, s->seg_box.p, sizeof(qn::BBoxOut) * count, hipMemcpyDeviceToHost, st));
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipStreamSynchronize(st));                            // the one sync: each cloud's box sizes its cells
  qn::BatchSeg* sg = (qn::BatchSeg*)(h + tb.seg); std::vector<int> lbits(count);
  for (uint32_t k = 0; k < count; k++) {
    qn::BatchSeg& g = sg[k];
    g = qn::BatchSeg{}; g.p0 = p0[k]; g.p1 = p0[k + 1]; g.sentinel = 1; g.tripped = 0;
    g.vd = qn::VoxelDims{1.0f, {0, 0, 0}, 1, 1};
    const qn::BBoxOut bb = s->seg_box_host.p[k];
    const uint32_t nfin = n_pts[k] - bb.nonfinite;
    long long cells = 1;
    if (nfin) {
      double maxabs = 0.0;
      for (int a = 0; a < 3; a++) maxabs = std::max(maxabs, (double)std::max(std::fabs(qn::ord2f(bb.mn[a])), std::fabs(qn::ord2f(bb.mx[a]))));
      double edge = std::max((radius + std::ldexp(maxabs, -21)) * (1.0 + 1e-5), 1e-30);
      // the widening ends: edge >= 2^-21 max|coordinate| keeps every floor within 2^22, and a growing edge brings pd and cells down to at most 8 long
      // before (float)edge overflows - unless an extent itself is not a finite f32, which trips the guard (2) at every edge: such a cloud has no index
      for (int a = 0; a < 3; a++)
        if (!std::isfinite(qn::ord2f(bb.mx[a]) - qn::ord2f(bb.mn[a]))) {
          s->last_error = "cell index: the extent of a cloud overflows f32"; return QN_ERR_CAPACITY;
        }
      while (!voxel_dims(bb, edge, &g.vd, &cells) || cells >= (1ll << QN_CELL_LEAF_BITS)) edge *= 1.25;
      g.sentinel = (uint32_t)cells; g.nvox = nfin;
    }
    lbits[k] = bits_for(bb.nonfinite ? g.sentinel : g.sentinel - 1);
    qn_kf_int_cell_grid& o = grids[k];
    o.p0 = g.p0; o.n = n_pts[k]; o.n_finite = nfin; o.inv = g.vd.inv;
    for (int a = 0; a < 3; a++) o.minb[a] = g.vd.minb[a];
    o.div[0] = g.vd.div0; o.div[1] = g.vd.div01 / g.vd.div0; o.div[2] = (int)(cells / g.vd.div01);
  }
  const std::vector<SortGroup> groups = sort_groups(lbits, count, sg, p0);
  for (uint32_t k = 0; k < count; k++) grids[k].prefix = sg[k].prefix;
  if (!sort_scratch(s, groups, p0)) return QN_ERR_HIP;
  QN_KFCHK(s, hipMemcpyAsync(s->tab.p + tb.seg, sg, tb.end - tb.seg, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(qn::k_batch_keys, dim3(nt * QN_MAP_ITEMS), dim3(QN_BLOCK), 0, st, dkf, dblk, dks, dsg, (const float4*)s->concat.p, s->keys.p);
  unsigned long long* fin = nullptr;
  { const int src = sort_segments(s, groups, p0, &fin); if (src != QN_OK) return src; }
  QN_KFCHK(s, hipGetLastError());
  *points = s->concat.p; *keys = fin;
  return QN_OK;
}

// transform + concatenate `count` resident keyframes with their poses (row-major 4x4 f64) and voxel-grid them into output slot 0 (source)
// or 1 (target); returns the device pointer (float4, stride 16, w = 1) and the point count.  Non-finite points are dropped (a note in
// last_error); a tripped guard returns the finite points unfiltered (the warning replaces the note).  last_error is not cleared on entry.
extern "C" int qn_kf_assemble(qn_kf_store* s, const int32_t* ids, const double* poses, uint32_t count, double leaf, int slot,
                              const float** d_xyz_out, uint32_t* n_out) {
  if (!s || !ids || !poses || !d_xyz_out || !n_out || (slot != 0 && slot != 1) || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  *d_xyz_out = nullptr; *n_out = 0;
  if (!ids_valid(s, ids, 0, count)) return QN_ERR_INVALID_ARG;
  const uint32_t seg[2] = {0, count};
  SubmapOut r; VoxelNotes nt;
  const int rc = voxel_submaps(s, sources_of(s, ids, 0, count).data(), poses, seg, 1, leaf, false, false, s->out[slot], &r, &nt);
  if (rc != QN_OK) return rc;
  if (r.status != QN_OK) return r.status;
  if (nt.nonfinite) s->last_error = kNonFiniteNote;
  if (nt.tripped) s->last_error = kOverflowWarning;
  s->out_n[slot] = r.n; *d_xyz_out = (const float*)r.ptr; *n_out = r.n;
  return QN_OK;
}

extern "C" int qn_kf_download(qn_kf_store* s, int slot, float* xyz_out) {        // packed n x 3, for tests / visualisation
  if (!s || !xyz_out || (slot != 0 && slot != 1)) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->out_n[slot];
  if (!n) return QN_OK;
  QN_KFCHK(s, hipSetDevice(s->device));
  QN_KFCHK(s, hipMemcpy2D(xyz_out, 12, s->out[slot].p, 16, 12, n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// the corrected global map (fast_lio_sam_qn.cpp:302-316, 398-411, 435-448): every listed keyframe transformed with its corrected pose,
// concatenated in list order, voxel-grid at `leaf` with intensity; into the store's own map slot (never assemble slots 0 / 1).
// Unlike qn_kf_assemble, a tripped overflow guard passes the WHOLE concatenation through, non-finite points included (output = *input_).
static int build_map_sources(qn_kf_store* s, const VoxSrc* src, const double* poses, uint32_t count, double leaf, const float** d_xyzi_out, uint32_t* n_out) {
  const uint32_t seg[2] = {0, count};
  SubmapOut r; VoxelNotes nt;
  const int rc = voxel_submaps(s, src, poses, seg, 1, leaf, true, true, s->map, &r, &nt);
  if (rc != QN_OK) return rc;
  if (r.status != QN_OK) return r.status;
  if (nt.tripped) s->last_error = kOverflowWarning;
  s->map_n = r.n; *d_xyzi_out = (const float*)r.ptr; *n_out = r.n;
  return QN_OK;
}
extern "C" int qn_kf_build_map(qn_kf_store* s, const int32_t* ids, const double* poses, uint32_t count, double leaf,
                               const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || (count && (!ids || !poses)) || !d_xyzi_out || !n_out || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  *d_xyzi_out = nullptr; *n_out = 0;
  s->map_n = 0; s->map_gen++; s->last_error.clear();
  if (count == 0) return QN_ERR_EMPTY_CLOUD;
  if (!ids_valid(s, ids, 0, count)) return QN_ERR_INVALID_ARG;
  return build_map_sources(s, sources_of(s, ids, 0, count).data(), poses, count, leaf, d_xyzi_out, n_out);
}
int qn_kf_int_build_map_from(qn_kf_store* s, const float4* const* pts, const uint32_t* n, const uint8_t* has_i, const double* poses, uint32_t count, double leaf,
                             const float** d_xyzi_out, uint32_t* n_out) {
  *d_xyzi_out = nullptr; *n_out = 0;
  s->map_n = 0; s->map_gen++; s->last_error.clear();
  if (count == 0) return QN_ERR_EMPTY_CLOUD;
  std::vector<VoxSrc> src(count);
  for (uint32_t k = 0; k < count; k++) src[k] = VoxSrc{n[k] ? pts[k] : nullptr, n[k], has_i[k]};
  return build_map_sources(s, src.data(), poses, count, leaf, d_xyzi_out, n_out);
}

const float4* qn_kf_int_map(const qn_kf_store* s, uint32_t* n, uint64_t* generation) {
  *n = s->map_n; *generation = s->map_gen;
  return s->map_n ? s->map.p : nullptr;
}

// the first n_kept records at d_kept (device memory, not the slot itself; n_kept <= the slot's points) become the map slot, copied on the store's stream, and
// the slot's generation advances as after a build: what a filter of the map leaves behind (qn_mapoutliers.hip)
int qn_kf_int_map_shrink(qn_kf_store* s, const float4* d_kept, uint32_t n_kept) {
  if (n_kept > s->map_n || (n_kept && !d_kept)) return QN_ERR_INVALID_ARG;
  if (n_kept) QN_KFCHK(s, hipMemcpyAsync(s->map.p, d_kept, sizeof(float4) * (size_t)n_kept, hipMemcpyDeviceToDevice, s->stream));
  s->map_n = n_kept; s->map_gen++;
  return QN_OK;
}

// the map into host records: only the 12 xyz bytes (offset 0) and the 4 intensity bytes (offset ioff) of each are written
extern "C" int qn_kf_download_map(qn_kf_store* s, void* out, uint32_t stride, uint32_t ioff) {
  if (!s || !out || !xyzi_layout_ok(stride, ioff)) return QN_ERR_INVALID_ARG;
  const uint32_t n = s->map_n;
  if (!n) return QN_OK;
  QN_KFCHK(s, hipSetDevice(s->device));
  QN_KFCHK(s, hipMemcpy2D(out, stride, s->map.p, 16, 12, n, hipMemcpyDeviceToHost));
  QN_KFCHK(s, hipMemcpy2D((char*)out + ioff, stride, (const char*)s->map.p + 12, 16, 4, n, hipMemcpyDeviceToHost));
  return QN_OK;
}

// S loop-closure submaps in one pass (LoopClosure::setSrcAndDstCloud for one query and its candidates, loop_closure.cpp:58-108): submap t =
// ids[seg_off[t] .. seg_off[t + 1]) with the poses of the same entries, each what qn_kf_assemble builds for its list (the same pipeline),
// into the store's batch slot (never slots 0 / 1 or the map slot).  A submap with no finite point has status QN_ERR_EMPTY_CLOUD.
extern "C" int qn_kf_assemble_batch(qn_kf_store* s, const int32_t* ids, const double* poses, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                                    const float** d_xyz_out, uint32_t* n_out, int* status) {
  if (!s || !seg_off || n_seg == 0 || !d_xyz_out || !n_out || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  for (uint32_t t = 0; t < n_seg; t++) if (seg_off[t + 1] < seg_off[t]) return QN_ERR_INVALID_ARG;
  if (seg_off[n_seg] != seg_off[0] && (!ids || !poses)) return QN_ERR_INVALID_ARG;
  if (!ids_valid(s, ids, seg_off[0], seg_off[n_seg])) return QN_ERR_INVALID_ARG;
  qn_kf_int_verify_stale(s, QN_KF_VERIFY_FROM_BATCH, nullptr, 0);                                  // (a multi-pair GICP verification's segments are about to be replaced)
  for (uint32_t t = 0; t < n_seg; t++) { d_xyz_out[t] = nullptr; n_out[t] = 0; status[t] = QN_ERR_EMPTY_CLOUD; }
  s->bt_ptr.assign(n_seg, nullptr); s->bt_n.assign(n_seg, 0); s->last_error.clear();
  std::vector<SubmapOut> res(n_seg); VoxelNotes nt;
  const int rc = voxel_submaps(s, sources_of(s, ids, seg_off[0], seg_off[n_seg]).data(), poses, seg_off, n_seg, leaf, false, false, s->bt_out, res.data(), &nt);
  if (rc != QN_OK) return rc;
  if (nt.nonfinite) s->last_error = kNonFiniteNote;
  if (nt.tripped) s->last_error = kOverflowWarning;
  for (uint32_t t = 0; t < n_seg; t++) {
    if (res[t].status != QN_OK) continue;
    s->bt_ptr[t] = res[t].ptr; s->bt_n[t] = res[t].n;
    d_xyz_out[t] = (const float*)res[t].ptr; n_out[t] = res[t].n; status[t] = QN_OK;
  }
  return QN_OK;
}

int qn_kf_int_voxel_windows(qn_kf_store* s, const int32_t* ids, const double* poses, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                            DevBuf<float4>& block, const float4** ptr, uint32_t* n, int* status) {
  block.reset();
  for (uint32_t t = 0; t < n_seg; t++) { ptr[t] = nullptr; n[t] = 0; status[t] = QN_ERR_EMPTY_CLOUD; }
  if (n_seg == 0) return QN_OK;
  std::vector<SubmapOut> res(n_seg); VoxelNotes nt;
  s->last_error.clear();
  const int rc = voxel_submaps(s, sources_of(s, ids, seg_off[0], seg_off[n_seg]).data(), poses, seg_off, n_seg, leaf, false, false, block, res.data(), &nt);
  if (rc != QN_OK) { block.reset(); return rc; }
  if (nt.nonfinite) s->last_error = kNonFiniteNote;
  if (nt.tripped) s->last_error = kOverflowWarning;
  for (uint32_t t = 0; t < n_seg; t++) { ptr[t] = res[t].ptr; n[t] = res[t].n; status[t] = res[t].status; }
  return QN_OK;
}

int qn_kf_int_voxel_each(qn_kf_store* s, const int32_t* ids, uint32_t count, double leaf, DevBuf<float4>& block, const float4** ptr, uint32_t* n, int* status) {
  std::vector<uint32_t> seg(count + 1);
  for (uint32_t t = 0; t <= count; t++) seg[t] = t;
  std::vector<double> eye(16 * (size_t)count, 0.0);
  for (uint32_t t = 0; t < count; t++) for (int i = 0; i < 4; i++) eye[16 * (size_t)t + 5 * i] = 1.0;
  return qn_kf_int_voxel_windows(s, ids, eye.data(), seg.data(), count, leaf, block, ptr, n, status);
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
  QN_KFCHK(s, hipSetDevice(s->device));
  QN_KFCHK(s, hipMemcpy2D(xyz_out, 12, s->bt_ptr[seg], 16, 12, n, hipMemcpyDeviceToHost));
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
