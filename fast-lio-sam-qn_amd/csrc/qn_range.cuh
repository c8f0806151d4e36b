// qn_range.cuh - what the range-image translation units share: the projection of a point into a keyframe's range image, the staging of the column table, the
// window gather and the class of a point (qn_freespace.hip: images and the loop-pair check; qn_staticmap.hip: the many-to-many votes of the static map), and the
// store's range-image state.  One text for both, so a record gets the same row, column, range and class whichever kernel asks.  The numpy twin
// qn_amd/freespace.py is the specification: f64 from the f32 records in a fixed order, no fused multiply-add (the build's -ffp-contract=off), no
// transcendental on the device, the twin's bisections evaluated at the same indices, the correctly rounded f64 sqrt.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"

#define FS_BLOCK 512
#define FS_ITERS 4
#define FS_TILE (FS_BLOCK * FS_ITERS)                   // records per block
#define FS_WAVES (FS_BLOCK / 64)
#define FS_LDS_MAX (64u << 10)                          // the column table is staged in LDS up to this size
#define FS_INF_BITS 0x7F800000u

namespace qn_range {

// the column table (16 bytes per column) in LDS when LDS, else read where it is; every thread of the block must call it
template <bool LDS> __device__ __forceinline__ const double2* fs_stage(const double2* __restrict__ g, uint32_t nc) {
  extern __shared__ __align__(16) unsigned char fs_smem[];
  if (!LDS) return g;
  double2* l = (double2*)fs_smem;
  for (uint32_t t = threadIdx.x; t < nc; t += FS_BLOCK) l[t] = g[t];
  __syncthreads();
  return l;
}

// the twin's project(): false for a dropped point (the coordinates are finite)
__device__ __forceinline__ bool fs_project(double x, double y, double z, const double* __restrict__ trow, uint32_t nr, const double2* cs, uint32_t nc, double min_range,
                                           uint32_t& row, uint32_t& col, double& r) {
  const double rho2 = x * x + y * y;
  const double rho = __builtin_sqrt(rho2);
  r = __builtin_sqrt(rho2 + z * z);
  uint32_t lo = 0, hi = nr + 1;
#pragma unroll 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (z >= rho * trow[mid]) lo = mid + 1; else hi = mid;
  }
  if (lo == 0 || lo == nr + 1 || !(r >= min_range)) return false;
  row = lo - 1;
  const int hp = (y > 0.0 || (y == 0.0 && x > 0.0)) ? 0 : 1;
  lo = 1; hi = nc;
#pragma unroll 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const double2 b = cs[mid];
    const int hb = (b.y > 0.0 || (b.y == 0.0 && b.x > 0.0)) ? 0 : 1;
    const double cr = b.x * y - b.y * x;
    if (hp > hb || (hp == hb && cr >= 0.0)) lo = mid + 1; else hi = mid;
  }
  col = lo - 1;
  return true;
}

// the twin's window_extrema() of one pixel, as f32 bit patterns (order-preserving for non-negative floats): rows clipped, columns wrapping
__device__ __forceinline__ void fs_window(const uint32_t* __restrict__ near, const uint32_t* __restrict__ far, uint32_t row, uint32_t col, uint32_t nr, uint32_t nc, int wr, int wc,
                                          uint32_t& rn, uint32_t& rf) {
  rn = FS_INF_BITS; rf = 0u;
#pragma unroll 1
  for (int dr = -wr; dr <= wr; dr++) {
    const int rr = (int)row + dr;
    if ((unsigned)rr >= nr) continue;
#pragma unroll 1
    for (int dc = -wc; dc <= wc; dc++) {
      int cc = (int)col + dc;                                  // 2 wc + 1 <= nc: one wrap is enough
      cc = cc < 0 ? cc + (int)nc : (cc >= (int)nc ? cc - (int)nc : cc);
      const uint32_t pix = (uint32_t)rr * nc + (uint32_t)cc;
      rn = min(rn, near[pix]); rf = max(rf, far[pix]);
    }
  }
}

// the class of a kept point with range r from its window's extrema: 1 unobserved, 2 seen through, 3 occluded, 4 agree
__device__ __forceinline__ uint32_t fs_class(double r, uint32_t rn, uint32_t rf, double tol_abs, double tol_rel) {
  const double tol = tol_abs + tol_rel * r;
  uint32_t cls = 4u;
  if (r > (double)__uint_as_float(rf) + tol) cls = 3u;
  if (r + tol < (double)__uint_as_float(rn)) cls = 2u;
  if (rn == FS_INF_BITS) cls = 1u;
  return cls;
}

// the class of a point already in the images' sensor frame (0: dropped); fin = its coordinates are finite
__device__ __forceinline__ uint32_t fs_classify(double px, double py, double pz, const double* __restrict__ trow, uint32_t nr, const double2* ct, uint32_t nc, double min_range,
                                                int wr, int wc, double tol_abs, double tol_rel, const uint32_t* __restrict__ near, const uint32_t* __restrict__ far, bool& fin) {
  fin = __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz);
  uint32_t row, col; double r;
  if (!fin || !fs_project(px, py, pz, trow, nr, ct, nc, min_range, row, col, r)) return 0u;
  uint32_t rn, rf;
  fs_window(near, far, row, col, nr, nc, wr, wc, rn, rf);
  return fs_class(r, rn, rf, tol_abs, tol_rel);
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct FsSlot { uint32_t p0[2], n[2]; };
// The store's range-image state (slot QN_KF_INT_EXT_RANGE, owned by qn_freespace.hip): parameters, the host tables on the device, image slots indexed by
// keyframe id (grown with the store), and the per-point classes of the latest check in a buffer of their own (the store's scratch may be reused by any other
// call).
struct RangeState {
  qn_range_params p{};
  DevBuf<double> tab;                                    // t [n_rows + 1], padded to 16 bytes, then (cos, sin) [n_cols]
  DevBuf<uint32_t> img;                                  // per keyframe id: near [n_rows * n_cols], far [n_rows * n_cols], as f32 bit patterns
  size_t cap = 0;                                        // keyframe slots of img
  std::vector<uint8_t> described;
  bool live = false; std::vector<FsSlot> slots; DevBuf<uint8_t> cls;
};
inline size_t range_cs_offset(uint32_t nr) { return ((size_t)nr + 2) & ~(size_t)1; }      // in doubles: the column table is 16-byte aligned
inline size_t range_lds_bytes(const RangeState* st) { const size_t b = sizeof(double2) * (size_t)st->p.n_cols; return b <= FS_LDS_MAX ? b : 0; }

}  // namespace qn_range
