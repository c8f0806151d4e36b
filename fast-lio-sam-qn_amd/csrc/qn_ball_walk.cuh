// qn_ball_walk.cuh - the radius walks of the Quatro feature kernels (qn_quatro_kernels.cuh) over the cell-sorted grid: one query per lane, one query per group of
// lanes, and the group walk with its segment bounds fetched up front.  A header of their own so that csrc/qn_search_debug.hip can call them as they are without
// compiling the feature kernels a second time; the text is unchanged.
#pragma once
#include "qn_device.cuh"

namespace qn {

// Walk every point u of the grid whose cell intersects the ball (q, r); body(u, point).  One query per lane.
template <class Body>
__device__ __forceinline__ void for_each_in_ball_cells(const GridView& g, float qx, float qy, float qz, float r, Body&& body) {
  const int bx0 = cell_coord(qx - r, g.ox, g.inv_cell, g.nx), bx1 = cell_coord(qx + r, g.ox, g.inv_cell, g.nx);
  const int by0 = cell_coord(qy - r, g.oy, g.inv_cell, g.ny), by1 = cell_coord(qy + r, g.oy, g.inv_cell, g.ny);
  const int bz0 = cell_coord(qz - r, g.oz, g.inv_cell, g.nz), bz1 = cell_coord(qz + r, g.oz, g.inv_cell, g.nz);
  for (int rz = bz0; rz <= bz1; rz++) for (int ry = by0; ry <= by1; ry++) for (int tx = bx0 >> 3; tx <= (bx1 >> 3); tx++) {
    const int xa = max(bx0, tx << 3), xb = min(bx1, (tx << 3) + 7);
    const uint32_t k0 = cell_key(g, xa, ry, rz);
    const uint32_t s = g.cell_start[k0], e = g.cell_start[k0 + (xb - xa) + 1];
    for (uint32_t u = s; u < e; u++) body(u, g.pts[u]);
  }
}

// The same walk shared by a GROUP of QN_FG consecutive lanes that serve ONE query: lane g of the group takes the candidates g, g + QN_FG, ...
// of every segment (coalesced 16-byte loads).  With one query per lane a 30k-point cloud is 470 waves for 1024 SIMDs and every wave
// walks ~150 candidates through a chain of dependent loads: latency-bound with half the chip empty.  Eight lanes per query give 8x the
// waves and 8x the loads in flight per query.
#define QN_FG 8
template <int FG = QN_FG, class Body>
__device__ __forceinline__ void for_each_in_ball_cells_group(const GridView& g, float qx, float qy, float qz, float r, int gl, Body&& body) {
  const int bx0 = cell_coord(qx - r, g.ox, g.inv_cell, g.nx), bx1 = cell_coord(qx + r, g.ox, g.inv_cell, g.nx);
  const int by0 = cell_coord(qy - r, g.oy, g.inv_cell, g.ny), by1 = cell_coord(qy + r, g.oy, g.inv_cell, g.ny);
  const int bz0 = cell_coord(qz - r, g.oz, g.inv_cell, g.nz), bz1 = cell_coord(qz + r, g.oz, g.inv_cell, g.nz);
  for (int rz = bz0; rz <= bz1; rz++) for (int ry = by0; ry <= by1; ry++) for (int tx = bx0 >> 3; tx <= (bx1 >> 3); tx++) {
    const int xa = max(bx0, tx << 3), xb = min(bx1, (tx << 3) + 7);
    const uint32_t k0 = cell_key(g, xa, ry, rz);
    const uint32_t s = g.cell_start[k0], e = g.cell_start[k0 + (xb - xa) + 1];
    for (uint32_t u = s + gl; u < e; u += FG) body(u, g.pts[u]);
  }
}
// The same walk with the segment bounds fetched UP FRONT (round 5).  The loop above pays two dependent cell_start loads per segment before it can touch a point, segment
// after segment: a 5 x 5 x 5-cell box is ~50 segments of which ~8 hold points (surfaces), so a group spent most of its life waiting for the bounds of empty rows - 70 us for
// a kernel whose arithmetic is a few microseconds.  Here the FG lanes of the group fetch the bounds of ALL segments in parallel (lane gl takes segments gl, gl + FG, ...)
// into a small LDS table of the group, then walk the segments in the SAME order with the SAME dealing of the points to the lanes: body() sees exactly the sequence it saw
// before - bit-identical sums - minus ~40 dependent round trips and ~120 vector instructions of per-segment bookkeeping in every lane (tools/isa_loops.py: the segment loop of
// k_spfh is 121 VALU instructions around a 200-instruction point loop).  Measured, both clouds of a pair: at 100k points k_spfh 0.366 -> 0.339 ms, k_fpfh 0.476 -> 0.435,
// k_normals_group 0.125 -> 0.117; at 30k k_fpfh 0.157 -> 0.145, k_normals_group 0.069 -> 0.064, k_spfh unchanged (0.14: one round of waves, as long as its densest
// neighbourhoods).  Prefetching the next candidate's point on top of it measured SLOWER (0.170 / 0.078) and was dropped.  `seg`: this group's table (QN_SEG_CAP entries; a box with more segments takes the loop above).
// Every lane of the wave must call (the table hand-over is a wave-level LDS fence); on = false: nothing to walk.
#define QN_SEG_CAP 80
template <int FG, class Body>
__device__ __forceinline__ void for_each_in_ball_cells_group_pre(const GridView& g, bool on, float qx, float qy, float qz, float r, int gl, uint2* __restrict__ seg, Body&& body) {
  const int bx0 = cell_coord(qx - r, g.ox, g.inv_cell, g.nx), bx1 = cell_coord(qx + r, g.ox, g.inv_cell, g.nx);
  const int by0 = cell_coord(qy - r, g.oy, g.inv_cell, g.ny), by1 = cell_coord(qy + r, g.oy, g.inv_cell, g.ny);
  const int bz0 = cell_coord(qz - r, g.oz, g.inv_cell, g.nz), bz1 = cell_coord(qz + r, g.oz, g.inv_cell, g.nz);
  const int tx0 = bx0 >> 3, ntx = (bx1 >> 3) - tx0 + 1, ny = by1 - by0 + 1, nz = bz1 - bz0 + 1;
  const int nseg = on ? nz * ny * ntx : 0;
  const bool fits = on && nseg <= QN_SEG_CAP;      // (an inactive lane walks nothing and must not FILL anything either: its box is whatever its placeholder query gives - ADVICE r5: with fits true for nseg = 0 the
                                                   //  fill loop below ran over that box and could write past the group's QN_SEG_CAP entries)
  // lane gl takes the (y, z) rows gl, gl + FG, ... of the box (each row = ntx segments, 1 or 2).  No integer division: a 32-bit division is ~40 instructions on this
  // machine and four of them per segment cost what the table saves; row -> (y, z) through a float reciprocal, exact for these sizes ((r + 0.5) / ny is never an integer).
  const float inv_ny = 1.0f / (float)max(ny, 1);
  if (fits) for (int r = gl; r < ny * nz; r += FG) {
    const int rzi = (int)(((float)r + 0.5f) * inv_ny), ryi = r - rzi * ny;
    for (int it = 0; it < ntx; it++) {
      const int tx = tx0 + it;
      const int xa = max(bx0, tx << 3), xb = min(bx1, (tx << 3) + 7);
      const uint32_t k0 = cell_key(g, xa, by0 + ryi, bz0 + rzi);
      seg[r * ntx + it] = make_uint2(g.cell_start[k0], g.cell_start[k0 + (xb - xa) + 1]);
    }
  }
  wave_lds_fence();
  if (fits) {
    for (int si = 0; si < nseg; si++) { const uint2 se = seg[si]; for (uint32_t u = se.x + gl; u < se.y; u += FG) body(u, g.pts[u]); }
  } else if (on) {
    for (int rz = bz0; rz <= bz1; rz++) for (int ry = by0; ry <= by1; ry++) for (int tx = bx0 >> 3; tx <= (bx1 >> 3); tx++) {
      const int xa = max(bx0, tx << 3), xb = min(bx1, (tx << 3) + 7);
      const uint32_t k0 = cell_key(g, xa, ry, rz);
      const uint32_t s = g.cell_start[k0], e = g.cell_start[k0 + (xb - xa) + 1];
      for (uint32_t u = s + gl; u < e; u += FG) body(u, g.pts[u]);
    }
  }
  wave_lds_fence();                                                          // (the table is reused by the group's next walk, if any)
}
}  // namespace qn
