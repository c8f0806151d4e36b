// qn_map_selftest.hip - qn_kf_debug_map_prims (include/qn_engine.h): the device builds of what the map units share - the wave and block folds, the key walk,
// the slot folds, the row scan and the block rank of qn_map_compact.cuh, the two linkers of qn_union_find.cuh, the index, tile and rim arithmetic and the
// neighbourhood walk of qn_dense_grid.cuh - on caller-supplied inputs, one routine a call.
// The kernels here only carry a lane's input to the headers' own functions and the result back; k_slot_fold, k_slot_max and k_scan_rows are launched as they
// are.  The units can express only a few input patterns (a block's count is at most 256, a key is a region number, an edge joins geometric neighbours); here
// the patterns are the caller's: tests/test_gpu_map_prims.py against the plain references of tests/map_prims_cases.py.  What the units instantiate, by grep
// over csrc/ (each has a field here):
//   wave folds   int min / max (k_mf_relabel, k_oc_extent), uint32_t sum (k_mf_relabel, k_mg_extent_sum) / min (k_mc_info) / max (k_mc_info, k_mc_number,
//                dg_block_stats, k_slot_max), unsigned long long sum (dg_block_stats, k_slot_fold) / min (k_mf_costs), float min / max
//                (k_mg_extent, k_mg_extent_sum), long long sum (k_mc_info)
//   key walk     uint32_t keys (k_mf_flatten), int32_t keys (k_mf_relabel, k_mf_costs)
//   block folds  block_count of 1, 2, 3 and 5 predicates; block_sum<uint32_t> of one value (k_mf_mark), <unsigned long long> of one (k_mc_hook), of two
//                uint32_t values widened (k_oc_classify) and of three (k_mo_flag); block_max<uint32_t> of one (k_mf_roots)
//   slot folds   k_slot_fold<uint32_t, K> with K = 1, 2, 3, 5, 10; k_slot_fold<unsigned long long, K> with K = 1, 2, 3; k_slot_max<uint32_t>
//   grid         oc_ijk and dg_index (every kernel of the four dense-grid files), dg_tile_of (k_mr_goals, k_mf_mark, k_mr_relax), dg_in_tile (k_mf_merge), dg_lane_pos
//                over dg_local and dg_pos (k_mr_relax, k_mf_tile), dg_tile_origin (k_mr_relax, k_mf_tile), dg_each_neighbour (k_mr_relax, k_mf_tile, k_mf_merge)
// Test infrastructure: it runs on the store's stream with the store's scratch (buffers 0 and 1), and nothing on a product path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "qn_map_compact.cuh"
#include "qn_dense_grid.cuh"
#include "qn_union_find.cuh"

namespace {

#define ST_NONE 0xffffffffu

// ---------------------------------------------------------------------------------------------------------------- 0: the wave folds
struct StLane { int32_t i; uint32_t u; float f; uint32_t zero; unsigned long long q; long long s; };
struct StWave { int32_t imin, imax; uint32_t usum, umin, umax; float fmin, fmax; uint32_t zero; unsigned long long qsum, qmin; long long ssum; unsigned long long zero2; };
static_assert(sizeof(StLane) == 32 && sizeof(StWave) == 64, "the records of include/qn_engine.h");

__global__ void __launch_bounds__(MO_BLOCK) k_st_wave(const StLane* __restrict__ in, StWave* __restrict__ out) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  const StLane v = in[t];
  StWave r;
  r.imin = wave_min(v.i); r.imax = wave_max(v.i);
  r.usum = wave_sum(v.u); r.umin = wave_min(v.u); r.umax = wave_max(v.u);
  r.fmin = wave_min(v.f); r.fmax = wave_max(v.f);
  r.qsum = wave_sum(v.q); r.qmin = wave_min(v.q);
  r.ssum = wave_sum(v.s);
  r.zero = 0; r.zero2 = 0;
  if ((threadIdx.x & 63) == 0) out[t >> 6] = r;                     // (lane 0 holds the results)
}

// ---------------------------------------------------------------------------------------------------------------- 1: the key walk
struct StKey { uint32_t trip, lead, key, served; unsigned long long same; };
static_assert(sizeof(StKey) == 24, "the record of include/qn_engine.h");

// in: (has, key) per lane; out: the trip that served the lane (ST_NONE: none), with the key, the lead and the mask it was handed there, and how many trips
// had the lane in their mask; trips[wave] = the trips of the wave
template <typename K> __global__ void __launch_bounds__(MO_BLOCK) k_st_each_key(const uint32_t* __restrict__ in, StKey* __restrict__ out, uint32_t* __restrict__ trips) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
  const bool has = in[2 * (size_t)t] != 0;
  const K key = (K)in[2 * (size_t)t + 1];
  StKey r;
  r.trip = ST_NONE; r.lead = ST_NONE; r.key = 0; r.served = 0; r.same = 0;
  uint32_t trip = 0;
  wave_each_key(has, key, [&](K k0, int lead, unsigned long long same) {
    if ((same >> lane) & 1ull) { r.trip = trip; r.lead = (uint32_t)lead; r.key = (uint32_t)k0; r.same = same; r.served++; }
    trip++;
  });
  out[t] = r;
  if (lane == 0) trips[t >> 6] = trip;
}

// ---------------------------------------------------------------------------------------------------------------- 2: the block folds
struct StBlockIn { uint32_t pred, a[3]; unsigned long long b[3]; };
struct StBlockOut {
  uint32_t count[15], sum32[6], max32[6], again32;       // K = 1 | 2 | 3 (| 4 | 5) results one after the other
  unsigned long long sum64[6], max64[6], again64, wide[2];
};
static_assert(sizeof(StBlockIn) == 40 && sizeof(StBlockOut) == 232, "the records of include/qn_engine.h");

__global__ void __launch_bounds__(MO_BLOCK) k_st_block(const StBlockIn* __restrict__ in, StBlockOut* __restrict__ out) {
  const StBlockIn v = in[blockIdx.x * MO_BLOCK + threadIdx.x];
  StBlockOut* o = out + blockIdx.x;
  const bool p0 = v.pred & 1u, p1 = v.pred & 2u, p2 = v.pred & 4u, p3 = v.pred & 8u, p4 = v.pred & 16u;
  block_count(o->count, p0);
  block_count(o->count + 1, p0, p1);
  block_count(o->count + 3, p0, p1, p2);
  block_count(o->count + 6, p0, p1, p2, p3);
  block_count(o->count + 10, p0, p1, p2, p3, p4);
  block_sum(o->sum32, v.a[0]);
  block_sum(o->sum32 + 1, v.a[0], v.a[1]);
  block_sum(o->sum32 + 3, v.a[0], v.a[1], v.a[2]);
  block_max(o->max32, v.a[0]);
  block_max(o->max32 + 1, v.a[0], v.a[1]);
  block_max(o->max32 + 3, v.a[0], v.a[1], v.a[2]);
  block_sum(o->sum64, v.b[0]);
  block_sum(o->sum64 + 1, v.b[0], v.b[1]);
  block_sum(o->sum64 + 3, v.b[0], v.b[1], v.b[2]);
  block_max(o->max64, v.b[0]);
  block_max(o->max64 + 1, v.b[0], v.b[1]);
  block_max(o->max64 + 3, v.b[0], v.b[1], v.b[2]);
  block_sum(o->wide, v.a[0], v.a[1]);                    // (two uint32_t values into unsigned long long sums: k_oc_classify's)
  __syncthreads();                                       // the second calls of the one-value sums reuse the first calls' words
  block_sum(&o->again32, v.a[1]);
  block_sum(&o->again64, v.b[1]);
}

// ---------------------------------------------------------------------------------------------------------------- 5: the block rank
__global__ void __launch_bounds__(MO_BLOCK) k_st_rank(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ base, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  out[t] = block_rank(keep[t] != 0, base[blockIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------- 6, 7: the union-find
// the launch before the unions, as k_mc_init: the identity, or the caller's forest (k_mf_tile's place)
__global__ void __launch_bounds__(MO_BLOCK) k_st_uf_init(uint32_t n, const uint32_t* __restrict__ parent0, uint32_t* __restrict__ parent) {
  const uint32_t x = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (x < n) parent[x] = parent0 ? parent0[x] : x;
}

// lane t: the edges [t per, (t + 1) per) in turn, as k_mf_merge does its up to 13 unions
template <bool MIN> __global__ void __launch_bounds__(MO_BLOCK) k_st_uf_unite(uint32_t m, uint32_t per, const uint32_t* __restrict__ edges, uint32_t* parent) {
  const size_t e0 = ((size_t)blockIdx.x * MO_BLOCK + threadIdx.x) * per;
  for (size_t e = e0; e < e0 + per && e < m; e++) {
    const uint32_t a = edges[2 * e], b = edges[2 * e + 1];
    if (MIN) uf_unite_min(parent, a, b); else uf_unite(parent, a, b);
  }
}

// the launch after them, by plain loads as k_mc_flatten and k_mf_flatten read the forest: parent[] is left as the unions left it
__global__ void __launch_bounds__(MO_BLOCK) k_st_uf_flatten(uint32_t n, const uint32_t* __restrict__ parent, uint32_t* __restrict__ root) {
  const uint32_t x = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (x >= n) return;
  uint32_t r = x;
  for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;         // p < r every trip
  root[x] = r;
}

// ---------------------------------------------------------------------------------------------------------------- 8: the grid geometry
struct StVoxel { uint32_t x, y, z, index, tile, place, pos, zero; };
static_assert(sizeof(StVoxel) == 32 && sizeof(DgIjk) == 12, "the records of include/qn_engine.h");

// lane i: the split of linear index i, the index rebuilt from it, the voxel's tile, its place in the tile (the lane that holds it) and that place's LDS position
__global__ void __launch_bounds__(MO_BLOCK) k_st_grid_voxels(uint32_t n, uint32_t W, uint32_t H, const DgTiles tiles, StVoxel* __restrict__ out) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (i >= n) return;
  const DgIjk v = oc_ijk(i, W, H);
  StVoxel r;
  r.x = (uint32_t)v.x; r.y = (uint32_t)v.y; r.z = (uint32_t)v.z;
  r.index = dg_index(v, W, H); r.tile = dg_tile_of(r.x, r.y, r.z, tiles);
  r.place = dg_index(dg_in_tile(r.x), dg_in_tile(r.y), dg_in_tile(r.z), DG_T, DG_T); r.pos = dg_lane_pos(r.place); r.zero = 0;
  out[i] = r;
}

// lane t: the first voxel of tile t; lane 0 also walks the neighbourhood and writes the offsets in the order it is handed them
__global__ void __launch_bounds__(MO_BLOCK) k_st_grid_tiles(const DgTiles tiles, int32_t* __restrict__ origin, DgIjk* __restrict__ walk) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (t >= tiles.n) return;
  const DgIjk o = dg_tile_origin(t, tiles);
  origin[4 * (size_t)t] = o.x; origin[4 * (size_t)t + 1] = o.y; origin[4 * (size_t)t + 2] = o.z; origin[4 * (size_t)t + 3] = 0;
  if (t != 0) return;
  uint32_t k = 0;
  dg_each_neighbour([&](int dx, int dy, int dz) { walk[k++] = DgIjk{dx, dy, dz}; });
}

bool st_fold_k(uint32_t arg) {
  const uint32_t k = arg & 0xffu;
  if ((arg & ~0xffu) == 0) return k == 1 || k == 2 || k == 3 || k == 5 || k == 10;
  if ((arg & ~0xffu) == 0x100u) return k >= 1 && k <= 3;
  return arg == 0x200u;
}

template <typename W> void st_launch_fold(uint32_t k, const void* d_in, uint32_t nb, void* d_out, hipStream_t str) {
  const dim3 one(1), wide(MO_SCAN_BLOCK);
  const W* in = (const W*)d_in; W* out = (W*)d_out;
  switch (k) {
    case 1: hipLaunchKernelGGL((k_slot_fold<W, 1>), one, wide, 0, str, in, nb, out); break;
    case 2: hipLaunchKernelGGL((k_slot_fold<W, 2>), one, wide, 0, str, in, nb, out); break;
    case 3: hipLaunchKernelGGL((k_slot_fold<W, 3>), one, wide, 0, str, in, nb, out); break;
    case 5: hipLaunchKernelGGL((k_slot_fold<W, 5>), one, wide, 0, str, in, nb, out); break;
    default: hipLaunchKernelGGL((k_slot_fold<W, 10>), one, wide, 0, str, in, nb, out); break;
  }
}

}  // namespace

extern "C" int qn_kf_debug_map_prims(qn_kf_store* s, int which, const void* in, uint32_t n, uint32_t arg, void* out) {
  // ---- every argument is checked before anything runs
  if (!s || !in || !out || which < 0 || which >= QN_DEBUG_MAP_PRIMS_WHICH) return QN_ERR_INVALID_ARG;
  size_t in_bytes = 0, out_bytes = 0;
  uint32_t m = 0, forest = 0, rows = 0;
  DgTiles tiles = {0, 0, 0, 0};
  switch (which) {
    case 0:
      if (arg != 0 || n > QN_DEBUG_MAP_PRIMS_MAX_BLOCKS) return QN_ERR_INVALID_ARG;
      in_bytes = sizeof(StLane) * MO_BLOCK * (size_t)n; out_bytes = sizeof(StWave) * MO_WAVES * (size_t)n;
      break;
    case 1:
      if (arg > 1 || n > QN_DEBUG_MAP_PRIMS_MAX_BLOCKS) return QN_ERR_INVALID_ARG;
      in_bytes = 8 * MO_BLOCK * (size_t)n; out_bytes = (sizeof(StKey) * MO_BLOCK + sizeof(uint32_t) * MO_WAVES) * (size_t)n;
      break;
    case 2:
      if (arg != 0 || n > QN_DEBUG_MAP_PRIMS_MAX_BLOCKS) return QN_ERR_INVALID_ARG;
      in_bytes = sizeof(StBlockIn) * MO_BLOCK * (size_t)n; out_bytes = sizeof(StBlockOut) * (size_t)n;
      break;
    case 3: {
      if (!st_fold_k(arg) || n > QN_DEBUG_MAP_PRIMS_MAX_NODES) return QN_ERR_INVALID_ARG;
      const size_t k = arg == 0x200u ? 1 : arg & 0xffu, w = (arg & 0x100u) ? 8 : 4;
      in_bytes = w * k * n; out_bytes = w * k;
      break;
    }
    case 4:
      rows = arg & 0x7fffffffu;
      if (rows == 0 || rows > QN_DEBUG_MAP_PRIMS_MAX_BLOCKS || (uint64_t)rows * n > QN_DEBUG_MAP_PRIMS_MAX_NODES) return QN_ERR_INVALID_ARG;
      in_bytes = sizeof(uint32_t) * (size_t)rows * n; out_bytes = in_bytes + sizeof(uint32_t) * rows;
      break;
    case 5:
      if (arg != 0 || n > QN_DEBUG_MAP_PRIMS_MAX_BLOCKS) return QN_ERR_INVALID_ARG;
      in_bytes = (MO_BLOCK + sizeof(uint32_t)) * (size_t)n; out_bytes = sizeof(uint32_t) * MO_BLOCK * (size_t)n;
      break;
    case 8: {
      if (arg != 0 || n > QN_DEBUG_MAP_PRIMS_MAX_NODES) return QN_ERR_INVALID_ARG;
      const uint32_t* side = (const uint32_t*)in;                    // (n == 0: nothing is read)
      if (n && (side[0] == 0 || side[1] == 0 || side[2] == 0 || side[0] > n || side[1] > n || side[2] > n || (uint64_t)side[0] * side[1] * side[2] != n)) return QN_ERR_INVALID_ARG;
      if (n) tiles = dg_tiles(side[0], side[1], side[2]);
      in_bytes = sizeof(uint32_t) * 3; out_bytes = sizeof(StVoxel) * (size_t)n + 16 * (size_t)tiles.n + sizeof(DgIjk) * 26;
      break;
    }
    default: {
      if (arg < 1 || arg > 13 || n > QN_DEBUG_MAP_PRIMS_MAX_NODES) return QN_ERR_INVALID_ARG;
      const uint32_t* h = (const uint32_t*)in;
      m = h[0]; forest = h[1];
      if (m > QN_DEBUG_MAP_PRIMS_MAX_EDGES || forest > 1) return QN_ERR_INVALID_ARG;
      const uint32_t* p0 = h + 2;
      const uint32_t* e = p0 + (forest ? n : 0);
      if (forest) for (uint32_t x = 0; x < n; x++) if (p0[x] > x) return QN_ERR_INVALID_ARG;
      for (size_t k = 0; k < 2 * (size_t)m; k++) if (e[k] >= n) return QN_ERR_INVALID_ARG;
      in_bytes = sizeof(uint32_t) * (2 + (forest ? (size_t)n : 0) + 2 * (size_t)m); out_bytes = sizeof(uint32_t) * 2 * (size_t)n;
      break;
    }
  }
  if (n == 0) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  char* d_in = (char*)qn_kf_int_scratch(s, 0, qn_up16(in_bytes));
  char* d_out = (char*)qn_kf_int_scratch(s, 1, qn_up16(out_bytes));
  if (!d_in || !d_out) return qn_kf_fail(s, "qn_kf_debug_map_prims: scratch allocation failed");
  QN_KFCHK(s, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, str));
  const dim3 grid(n), block(MO_BLOCK), one(1), wide(MO_SCAN_BLOCK);
  switch (which) {
    case 0: hipLaunchKernelGGL(k_st_wave, grid, block, 0, str, (const StLane*)d_in, (StWave*)d_out); break;
    case 1: {
      StKey* o = (StKey*)d_out; uint32_t* trips = (uint32_t*)(d_out + sizeof(StKey) * MO_BLOCK * (size_t)n);
      if (arg) hipLaunchKernelGGL(k_st_each_key<int32_t>, grid, block, 0, str, (const uint32_t*)d_in, o, trips);
      else hipLaunchKernelGGL(k_st_each_key<uint32_t>, grid, block, 0, str, (const uint32_t*)d_in, o, trips);
      break;
    }
    case 2: hipLaunchKernelGGL(k_st_block, grid, block, 0, str, (const StBlockIn*)d_in, (StBlockOut*)d_out); break;
    case 3:
      if (arg == 0x200u) hipLaunchKernelGGL(k_slot_max<uint32_t>, one, wide, 0, str, (const uint32_t*)d_in, n, (uint32_t*)d_out);
      else if (arg & 0x100u) st_launch_fold<unsigned long long>(arg & 0xffu, d_in, n, d_out, str);
      else st_launch_fold<uint32_t>(arg & 0xffu, d_in, n, d_out, str);
      break;
    case 4: {
      uint32_t* off = (uint32_t*)d_out;
      const uint32_t* cnt = (const uint32_t*)d_in;
      if (arg & 0x80000000u) {                           // in place: the counts are copied to where the offsets go
        QN_KFCHK(s, hipMemcpyAsync(off, d_in, in_bytes, hipMemcpyDeviceToDevice, str));
        cnt = off;
      }
      hipLaunchKernelGGL(k_scan_rows, dim3(rows), wide, 0, str, cnt, n, off, off + (size_t)rows * n);
      break;
    }
    case 5:
      hipLaunchKernelGGL(k_st_rank, grid, block, 0, str, (const uint8_t*)d_in, (const uint32_t*)(d_in + MO_BLOCK * (size_t)n), (uint32_t*)d_out);
      break;
    case 8: {
      const uint32_t* side = (const uint32_t*)in;
      int32_t* origin = (int32_t*)(d_out + sizeof(StVoxel) * (size_t)n);
      hipLaunchKernelGGL(k_st_grid_voxels, dim3(dg_blocks(n)), block, 0, str, n, side[0], side[1], tiles, (StVoxel*)d_out);
      hipLaunchKernelGGL(k_st_grid_tiles, dim3(dg_blocks(tiles.n)), block, 0, str, tiles, origin, (DgIjk*)(origin + 4 * (size_t)tiles.n));
      break;
    }
    default: {
      const uint32_t* d_h = (const uint32_t*)d_in + 2;
      const uint32_t* d_edges = d_h + (forest ? n : 0);
      uint32_t* parent = (uint32_t*)d_out;
      const dim3 nodes((n + MO_BLOCK - 1) / MO_BLOCK);
      hipLaunchKernelGGL(k_st_uf_init, nodes, block, 0, str, n, forest ? d_h : (const uint32_t*)nullptr, parent);
      if (m) {
        const dim3 lanes((uint32_t)((((size_t)m + arg - 1) / arg + MO_BLOCK - 1) / MO_BLOCK));
        if (which == 7) hipLaunchKernelGGL(k_st_uf_unite<true>, lanes, block, 0, str, m, arg, d_edges, parent);
        else hipLaunchKernelGGL(k_st_uf_unite<false>, lanes, block, 0, str, m, arg, d_edges, parent);
      }
      hipLaunchKernelGGL(k_st_uf_flatten, nodes, block, 0, str, n, (const uint32_t*)parent, parent + n);
      break;
    }
  }
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}
