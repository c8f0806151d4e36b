// qn_cell_walk.cuh - the consumer side of the sorted-key cell index (qn_kf_int_cell_index, qn_cloud.hip), once, for every bounded-radius search over it
// (qn_overlap.hip, qn_mapnormals.hip, qn_mapoutliers.hip): the segment a kernel is given, the gather that lays a segment's sorted points and their cell
// words out flat, and the walk over the 3 x 3 x 3 block of cells around a query.
// Exactness at cell borders: the cell edge carries the margin derived in qn_cloud.hip (qn_kf_int_cell_index), so a point within r of the query has f32 cell
// coordinates within one of the query's on every axis, whichever way either rounds - provided the query's coordinates come from cell_coord below, the very
// expression k_batch_keys uses.  Every point within r, and so the nearest one when it lies within r and every point that ties with it, is among the
// candidates the walk visits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "qn_kf_internal.h"

#define QN_CW_BLOCK 256                                  // one point per lane in the gather and in the kernels that walk

namespace {

// one cloud of the index: its range [p0, p0 + n) of the flat arrays (p0 = 0 when the map slot is the only cloud), the nfin finite points in front
struct CellSeg { uint32_t p0, n, nfin, prefix; float inv; float minb[3]; int div[3]; };

inline CellSeg cell_seg(const qn_kf_int_cell_grid& g) {
  CellSeg o;
  o.p0 = g.p0; o.n = g.n; o.nfin = g.n_finite; o.prefix = g.prefix; o.inv = g.inv;
  for (int a = 0; a < 3; a++) { o.minb[a] = (float)g.minb[a]; o.div[a] = g.div[a]; }
  return o;
}

__device__ __forceinline__ int cell_coord(float x, float inv, float minb, int div) {
  // This must stay k_batch_keys' expression, operation for operation: the margin of the cell edge is derived for a query and a point that are both rounded
  // this way.  Clamped in float so that a query far outside the cloud's box stays a valid int (it then has no cell to visit); for a query that is a point
  // of the indexed cloud the clamp never binds.
  const float c = floorf(x * inv) - minb;
  return (int)fminf(fmaxf(c, -2.0f), (float)div + 1.0f);
}

// the sorted order laid out flat: point t of the segment's sorted range with its original index in the cloud (bits in .w), and its (prefix | cell) word
__device__ __forceinline__ void cell_gather(const CellSeg& S, const unsigned long long* __restrict__ keys, const float4* __restrict__ pts, float4* __restrict__ spts,
                                            uint32_t* __restrict__ cells) {
  const uint32_t t = blockIdx.x * QN_CW_BLOCK + threadIdx.x;
  if (t >= S.n) return;
  const uint32_t g = S.p0 + t;
  const unsigned long long key = keys[g];
  const uint32_t src = (uint32_t)key;
  const float4 p = pts[src];
  spts[g] = make_float4(p.x, p.y, p.z, __uint_as_float(src - S.p0));
  cells[g] = (uint32_t)(key >> 32);
}
// the one segment of a map unit, passed by value (qn_overlap.hip wraps the same body over a device array of segments)
__global__ void __launch_bounds__(QN_CW_BLOCK) k_cell_gather(const CellSeg S, const unsigned long long* __restrict__ keys, const float4* __restrict__ pts,
                                                              float4* __restrict__ spts, uint32_t* __restrict__ cells) {
  cell_gather(S, keys, pts, spts, cells);
}

// The finite points of segment T in the 27 cells around q's: visit(position in the flat arrays, record, d2) for each, in ascending position.  Nine x-runs
// (cells x-1 .. x+1 of one (y, z) are consecutive keys), each found by a binary search over the sorted cell words that starts where the previous run ended
// (runs are visited in ascending key order), then read four candidates a trip, the loads clamped to the last finite record.  d2 is the oracle's sqdist3:
// q - p per axis, the products summed in source order (the library is built without contraction).
template <typename Visit>
__device__ __forceinline__ void cell_walk(const CellSeg& T, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, const float4 q, Visit visit) {
  const int cx = cell_coord(q.x, T.inv, T.minb[0], T.div[0]), cy = cell_coord(q.y, T.inv, T.minb[1], T.div[1]), cz = cell_coord(q.z, T.inv, T.minb[2], T.div[2]);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, T.div[0] - 1);
  if (x0 > x1) return;
  uint32_t lo = T.p0;
  const uint32_t end = T.p0 + T.nfin;
  for (int dz = -1; dz <= 1; dz++) {
    const int z = cz + dz;
    if ((unsigned)z >= (unsigned)T.div[2]) continue;
    for (int dy = -1; dy <= 1; dy++) {
      const int y = cy + dy;
      if ((unsigned)y >= (unsigned)T.div[1]) continue;
      const uint32_t k0 = T.prefix | (uint32_t)(x0 + (y + z * T.div[1]) * T.div[0]), k1 = k0 + (uint32_t)(x1 - x0);
      uint32_t a = lo, b = end;
      while (a < b) { const uint32_t m = (a + b) >> 1; if (cells[m] < k0) a = m + 1; else b = m; }
      for (;;) {
        if (a >= end) break;
        uint32_t c[4]; float4 p[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { const uint32_t i = min(a + j, end - 1); c[j] = cells[i]; p[j] = spts[i]; }
        bool more = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          more = more && a + j < end && c[j] <= k1;
          if (more) {
            const float dx = q.x - p[j].x, dy2 = q.y - p[j].y, dz2 = q.z - p[j].z;
            visit(a + j, p[j], dx * dx + dy2 * dy2 + dz2 * dz2);
          }
        }
        if (!more) break;
        a += 4;
      }
      lo = a;
    }
  }
}

}  // namespace
