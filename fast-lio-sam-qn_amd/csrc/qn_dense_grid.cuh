// qn_dense_grid.cuh - what every field over the dense occupancy grid shares, on the device and on the host: the W x H x D volume of qn_mapoccupancy.inc and the
// fields computed from it (qn_mapdistance.inc, qn_maproute.inc, qn_mapfrontier.inc, qn_mapview.inc), all part of qn_staticmap.hip's translation unit, which includes this file
// ahead of the five.  The next field over the grid starts from here, not from a copy of one of them:
//   geometry  OcGrid / oc_grid: the grid as the kernels take it; oc_voxel: the one world-point-to-cell quantisation (distance query, route goals, starts and
//             queries, the view gain's viewpoints); dg_index and its inverse oc_ijk: voxel <-> linear index, x fastest (the kernels of the four files - but k_md_x and k_md_axis, which want one
//             coordinate and keep their one division: EXPERIMENTS.md -, the tile numbering below, the host of qn_kf_map_frontier_costs); dg_cols / dg_cells / dg_blocks: the sizes every entry point derives from qn_occupancy_grid.
//   tile      the DG_T^3 tile of k_mr_relax and k_mf_tile, one voxel per lane, in LDS with a one-voxel rim: dg_local (lane -> place in the tile), dg_pos and
//             dg_lane_pos (place, lane -> LDS position), dg_step (the LDS offset of a neighbour), dg_tile_origin (tile number -> its first voxel), dg_tile_of
//             (voxel -> tile number: k_mr_goals, k_mf_mark), dg_in_tile / dg_tile_coord (k_mf_merge's rim and same-tile tests), dg_tiles (the host's counts).
//   walk      dg_each_neighbour: f(dx, dy, dz) for the 26 offsets, dz outermost, then dy, then dx, each -1, 0, +1, unrolled so that the offsets are constants in f
//             (k_mr_relax three times, k_mf_tile, k_mf_merge; the figures: profiles/EXPERIMENTS.md).  k_mr_path's run-time loop with its early exit stays its own.
//   stats     dg_block_stats: three counts, the largest and the u64 sum of one value a lane, behind block_count's barrier (k_md_axis<true>, k_mr_stats);
//             dg_fold_stats: the three launches that fold the blocks' slots into the 32-byte small block (qn_kf_map_distance, qn_kf_map_route).
//   band      dg_band: a caller's layer range clipped to the grid (the two slices, the route, the frontiers); k_dg_slice / dg_slice: one column per lane, a
//             band of layers folded (qn_kf_map_occupancy_slice: the largest class, qn_kf_map_distance_slice: the smallest d2).
//   list      k_dg_list_flag / k_scan_rows / k_dg_list_pick: the stable compaction of the voxels in linear order (the count, scan and rank idiom of qn_map_compact.cuh)
//             on a functor with the predicate and the payload (OcList, MfList); dg_list_count and dg_list_pick launch them (qn_kf_map_occupancy_list reads the
//             count between the two, qn_kf_map_frontier_list knows it already).
//   points    dg_points: n f64 points to scratch 0 and the launch grid of one point per lane (qn_kf_map_distance_query, qn_kf_map_route, _route_query, _route_path).
//   lifetime  DgLive / dg_live: the live results of the chain occupancy -> distance -> route, occupancy -> frontier and occupancy -> view together, null from where the chain is
//             broken (every entry point behind qn_kf_map_occupancy).  A result that outgrows its buffer: KfBuf::grow_beside / adopt (qn_kf_buf.h).
// Tested directly: the index split, the tile numbering, the rim position and the order of the walk through qn_kf_debug_map_prims (qn_map_selftest.hip, routine 8;
// tests/test_gpu_map_prims.py); the rest through the units.  Every kernel here is a template, so a unit carries only what it instantiates.
#pragma once
#include <algorithm>
#include <string>
#include "qn_kf_buf.h"
#include "qn_map_compact.cuh"

#define OC_S 10                                          // fractional bits of the fixed point
#define OC_COORD_LIMIT 1048576.0                         // 2^20 voxels
#define DG_T 8                                           // the tile's side, a power of two: an untuned choice
#define DG_TILE (DG_T * DG_T * DG_T)                     // voxels of a tile = lanes of a block of k_mr_relax and k_mf_tile
#define DG_H (DG_T + 2)                                  // the side with the rim
#define DG_LDS (DG_H * DG_H * DG_H)
static_assert((DG_T & (DG_T - 1)) == 0 && DG_TILE <= 1024, "a lane's place in the tile is taken from the bits of threadIdx.x; a tile is one block");

namespace {

struct OcGrid { int32_t minc[3]; uint32_t W, H, cells; };
struct DgIjk { int32_t x, y, z; };                       // a voxel; three int32 back to back, as the lists hold them
__host__ __device__ inline DgIjk operator+(const DgIjk& a, const DgIjk& b) { return DgIjk{a.x + b.x, a.y + b.y, a.z + b.z}; }

inline uint32_t dg_cols(const qn_occupancy_grid& g) { return g.width * g.height; }
inline uint32_t dg_cells(const qn_occupancy_grid& g) { return dg_cols(g) * g.depth; }      // at most QN_OCC_MAX_CELLS = 2^27
inline uint32_t dg_blocks(uint32_t n) { return (n + MO_BLOCK - 1) / MO_BLOCK; }            // blocks of one voxel, column or point a lane
inline OcGrid oc_grid(const qn_occupancy_grid& g) { return OcGrid{{g.minc[0], g.minc[1], g.minc[2]}, g.width, g.height, dg_cells(g)}; }

// The dense grid's cell of world point i, for every field over the grid (the distance and route queries, goals and starts), by the map's own quantisation: f64,
// every operation rounded on its own, half to even; false for a point that is not finite, 2^20 voxels or more from the origin, or outside the field of depth
// Df.  Planar: x and y choose the column, z must only pass the limit.  fixed (the view gain's viewpoints; nullptr elsewhere): the point's fixed-point
// integers themselves, 0 for a coordinate that fails the limit.
__device__ __forceinline__ bool oc_voxel(const double* __restrict__ xyz, uint32_t i, double inv, const OcGrid& G, uint32_t Df, uint32_t planar, uint32_t* cx, uint32_t* cy,
                                         uint32_t* cz, int32_t* fixed = nullptr) {
  const uint32_t side[3] = {G.W, G.H, Df};
  long long c[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double t = xyz[3 * (size_t)i + k] * inv;
    const bool in = fabs(t) < OC_COORD_LIMIT;                       // (a NaN fails the comparison, an infinity too)
    const long long a = in ? (long long)rint(t * 1024.0) : 0;       // |a| <= 2^30
    c[k] = in ? (a >> OC_S) - G.minc[k] : -1;
    if (fixed) fixed[k] = (int32_t)a;
    if (k == 2 && planar && in) c[k] = 0;
    ok = ok && in && c[k] >= 0 && c[k] < (long long)side[k];
  }
  *cx = (uint32_t)c[0]; *cy = (uint32_t)c[1]; *cz = (uint32_t)c[2];
  return ok;
}

// the linear index of voxel (x, y, z) of a grid W wide and H high, x fastest (32 bits hold it: 2^27 cells at most), and its inverse
__host__ __device__ inline uint32_t dg_index(uint32_t x, uint32_t y, uint32_t z, uint32_t W, uint32_t H) { return (z * H + y) * W + x; }
__host__ __device__ inline uint32_t dg_index(const DgIjk& v, uint32_t W, uint32_t H) { return dg_index((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, W, H); }
__host__ __device__ inline DgIjk oc_ijk(uint32_t i, uint32_t W, uint32_t H) {
  const uint32_t row = i / W, z = row / H;
  return DgIjk{(int32_t)(i - row * W), (int32_t)(row - z * H), (int32_t)z};
}

// ---- the tile: tiles are numbered like voxels, x fastest; lane l of a tile's block holds the tile's voxel at place dg_local(l), x fastest again
struct DgTiles { uint32_t x, y, z, n; };                 // tiles along each axis and in all
inline DgTiles dg_tiles(uint32_t W, uint32_t H, uint32_t D) {
  const uint32_t x = (W + DG_T - 1) / DG_T, y = (H + DG_T - 1) / DG_T, z = (D + DG_T - 1) / DG_T;
  return DgTiles{x, y, z, x * y * z};
}
__host__ __device__ inline uint32_t dg_tile_coord(uint32_t x) { return x / DG_T; }           // a voxel coordinate's tile along its axis
__host__ __device__ inline uint32_t dg_in_tile(uint32_t x) { return x % DG_T; }              // and its place inside that tile, 0 .. DG_T - 1
__host__ __device__ inline uint32_t dg_tile_of(uint32_t x, uint32_t y, uint32_t z, const DgTiles& t) { return dg_index(x / DG_T, y / DG_T, z / DG_T, t.x, t.y); }
__host__ __device__ inline DgIjk dg_tile_origin(uint32_t tile, const DgTiles& t) {           // the first voxel of tile number `tile`
  const DgIjk b = oc_ijk(tile, t.x, t.y);
  return DgIjk{b.x * DG_T, b.y * DG_T, b.z * DG_T};
}
__host__ __device__ inline DgIjk dg_local(uint32_t l) { return DgIjk{(int32_t)(l % DG_T), (int32_t)(l / DG_T % DG_T), (int32_t)(l / (DG_T * DG_T))}; }
// a tile in LDS with a one-voxel rim: the offset from a position to its neighbour at (dx, dy, dz), the position of place p and of lane l's voxel
__host__ __device__ constexpr int dg_step(int dx, int dy, int dz) { return (dz * DG_H + dy) * DG_H + dx; }
__host__ __device__ inline uint32_t dg_pos(const DgIjk& p) { return (uint32_t)dg_step(p.x + 1, p.y + 1, p.z + 1); }
__host__ __device__ inline uint32_t dg_lane_pos(uint32_t l) { return dg_pos(dg_local(l)); }

// f(dx, dy, dz) for the 26 neighbours of a voxel, dz outermost, then dy, then dx, each -1, 0, +1: unrolled, so the offsets are constants wherever f is inlined
template <typename F> __host__ __device__ __forceinline__ void dg_each_neighbour(F f) {
#pragma unroll
  for (int dz = -1; dz <= 1; dz++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        if ((dx | dy | dz) != 0) f(dx, dy, dz);
}

// ---- the statistics tail.  One value m a lane (0 where the lane has none) and three predicates, all lanes of an MO_BLOCK block here: cslots[3 b ..] = the
// block's three counts, mslots[b] = its largest m, tslots[b] = the u64 sum of its m
__device__ __forceinline__ void dg_block_stats(bool c0, bool c1, bool c2, uint32_t m, uint32_t* __restrict__ cslots, uint32_t* __restrict__ mslots,
                                               unsigned long long* __restrict__ tslots) {
  __shared__ unsigned long long wt[MO_WAVES];
  __shared__ uint32_t wm[MO_WAVES];
  const unsigned long long t = wave_sum((unsigned long long)m);
  const uint32_t mm = wave_max(m);
  if ((threadIdx.x & 63) == 0) { wt[threadIdx.x >> 6] = t; wm[threadIdx.x >> 6] = mm; }
  // its barrier is the one the sums wait for: block_max and block_sum, two barriers more, cost the distance call 0.8 % at 1e7 voxels (profiles/EXPERIMENTS.md)
  block_count(cslots + 3 * (size_t)blockIdx.x, c0, c1, c2);
  if (threadIdx.x == 0) {
    unsigned long long acc = 0; uint32_t top = 0;
    for (int w = 0; w < MO_WAVES; w++) { acc += wt[w]; top = max(top, wm[w]); }
    tslots[blockIdx.x] = acc; mslots[blockIdx.x] = top;
  }
}
// The cb blocks' slots folded into the 32-byte small block: the three counts, the largest (d_slots: the counts, then at 3 cb the blocks' largest) and the u64
// sum at byte 16.  Three launches; the caller checks hipGetLastError() and reads the block back
inline void dg_fold_stats(hipStream_t str, const uint32_t* d_slots, const unsigned long long* d_tslots, uint32_t cb, char* d_small) {
  hipLaunchKernelGGL((k_slot_fold<uint32_t, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, d_slots, cb, (uint32_t*)d_small);
  hipLaunchKernelGGL(k_slot_max<uint32_t>, dim3(1), dim3(MO_SCAN_BLOCK), 0, str, d_slots + 3 * (size_t)cb, cb, (uint32_t*)d_small + 3);
  hipLaunchKernelGGL((k_slot_fold<unsigned long long, 1>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, d_tslots, cb, (unsigned long long*)(d_small + 16));
}

// ---- band and slice.  The layers iz_lo .. iz_hi clipped to a grid `depth` layers deep; lo > hi: no layer of the grid in the range
struct DgBand { int32_t lo, hi; };
inline DgBand dg_band(int32_t iz_lo, int32_t iz_hi, uint32_t depth) { return DgBand{std::max<int32_t>(iz_lo, 0), (int32_t)std::min<int64_t>(iz_hi, (int64_t)depth - 1)}; }

// one column per lane: the layers lo .. hi of the volume folded by F (op_max, op_min: qn_map_compact.cuh), starting from `first`
template <typename T, typename F>
__global__ void __launch_bounds__(MO_BLOCK) k_dg_slice(uint32_t cols, const T* __restrict__ vol, uint32_t lo, uint32_t hi, uint32_t first, T* __restrict__ out) {
  const uint32_t c = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (c >= cols) return;
  uint32_t v = first;
  for (uint32_t z = lo; z <= hi; z++) v = F()(v, (uint32_t)vol[(size_t)z * cols + c]);
  out[c] = (T)v;
}
// The slice getters: the band iz_lo .. iz_hi of the volume d_vol folded column by column into out (scratch 1, one synchronisation); `fill`, the fold's
// neutral element, where the band misses the grid
template <typename T, typename F>
int dg_slice(qn_kf_store* s, const char* who, const qn_occupancy_grid& g, const T* d_vol, int32_t iz_lo, int32_t iz_hi, T fill, T* out) {
  const uint32_t cols = dg_cols(g);
  if (!cols) return QN_OK;
  const DgBand b = dg_band(iz_lo, iz_hi, g.depth);
  if (b.lo > b.hi) { std::fill(out, out + cols, fill); return QN_OK; }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  T* d_out = (T*)qn_kf_int_scratch(s, 1, sizeof(T) * (size_t)cols);
  if (!d_out) return qn_kf_fail(s, (std::string(who) + ": scratch allocation failed").c_str());
  hipLaunchKernelGGL((k_dg_slice<T, F>), dim3(dg_blocks(cols)), dim3(MO_BLOCK), 0, qn_kf_int_stream(s), cols, d_vol, (uint32_t)b.lo, (uint32_t)b.hi, (uint32_t)fill, d_out);
  QN_KFCHK(s, hipGetLastError());
  return qn_kf_download(s, out, d_out, sizeof(T) * (size_t)cols);
}

// ---- the voxel list.  A list L has keep(i), whether the voxel at linear index i is listed, and put(i, j), which writes its record at rank j.
// one voxel per lane: the block's listed voxels into its slot (what k_scan_rows goes on from)
template <typename L> __global__ void __launch_bounds__(MO_BLOCK) k_dg_list_flag(uint32_t cells, const L list, uint32_t* __restrict__ blk) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  block_count(blk + blockIdx.x, i < cells && list.keep(i));
}
// the block's listed voxels, in linear order, to rank off[block] ..
template <typename L> __global__ void __launch_bounds__(MO_BLOCK) k_dg_list_pick(uint32_t cells, const L list, const uint32_t* __restrict__ off) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool keep = i < cells && list.keep(i);
  const size_t j = block_rank(keep, off[blockIdx.x]);
  if (keep) list.put(i, j);
}
// flag and scan: the blocks' offsets (scratch 3: the blocks' counts, then their offsets and the total), the total at [dg_blocks(cells)]; nullptr without scratch
template <typename L> uint32_t* dg_list_count(qn_kf_store* s, uint32_t cells, const L& list) {
  const uint32_t nb = dg_blocks(cells);
  uint32_t* d_blk = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * (2 * (size_t)nb + 1));
  if (!d_blk) return nullptr;
  hipLaunchKernelGGL(k_dg_list_flag<L>, dim3(nb), dim3(MO_BLOCK), 0, qn_kf_int_stream(s), cells, list, d_blk);
  hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(MO_SCAN_BLOCK), 0, qn_kf_int_stream(s), (const uint32_t*)d_blk, nb, d_blk + nb, d_blk + 2 * (size_t)nb);
  return d_blk + nb;
}
template <typename L> void dg_list_pick(qn_kf_store* s, uint32_t cells, const L& list, const uint32_t* d_off) {
  hipLaunchKernelGGL(k_dg_list_pick<L>, dim3(dg_blocks(cells)), dim3(MO_BLOCK), 0, qn_kf_int_stream(s), cells, list, d_off);
}

// ---- point calls: the n f64 points of a query, goal or start list to scratch 0, on the store's stream; grid: one point per lane
struct DgPoints { const double* xyz; dim3 grid; };
inline int dg_points(qn_kf_store* s, const char* who, const double* xyz, uint32_t n, DgPoints* out) {
  double* d_xyz = (double*)qn_kf_int_scratch(s, 0, sizeof(double) * 3 * (size_t)n);
  if (!d_xyz) return qn_kf_fail(s, (std::string(who) + ": scratch allocation failed").c_str());
  QN_KFCHK(s, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, qn_kf_int_stream(s)));
  *out = DgPoints{d_xyz, dim3(dg_blocks(n))};
  return QN_OK;
}

// ---- result lifetime.  The results hang on each other - StaticState -> OccState -> DistState -> RouteState, OccState -> FrontierState, OccState -> ViewState, each in its
// unit's file - and each is live only while the one it was computed from is: the live ones together, nullptr from where the chain is broken.  Defined in qn_mapview.inc, the last.
struct DgLive { const struct OccState* occ; const struct DistState* dist; const struct RouteState* route; const struct FrontierState* frontier; const struct ViewState* view; };
DgLive dg_live(qn_kf_store* s);
template <typename T> T* dg_mut(const T* live) { return const_cast<T*>(live); }      // for the three calls that hang a result of their own on a live one

}  // namespace
