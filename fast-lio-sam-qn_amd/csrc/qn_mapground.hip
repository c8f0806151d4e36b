// qn_mapground.hip - the ground of the store's map slot and its 2-D occupancy grid on the GPU (qn_kf_map_ground, qn_kf_map_ground_points, qn_kf_map_ground_grid,
// qn_kf_map_keep_classes: include/qn_engine.h).  The numpy twin qn_amd/mapground.py is the specification: heights are quantised once (zq = rint(z 2^e), the f32
// widened to f64, the product exact), every finite point falls into a column of the x-y grid by the voxel grid's cell arithmetic, a column's seed is its lowest
// zq, the ground envelope g is the greatest function below the seeds whose rise between neighbouring columns is at most step_s (straight) / step_d (diagonal),
// and a point's class follows from h = zq - g(column).  Everything after the quantisation is an integer and the envelope is unique, so every byte equals the
// twin's whatever the order of the atomics and whatever the relaxation schedule.
//   extent    k_mg_extent: the finite points' extremes in x, y and z and their number (wave_min, wave_max, a table of its own, block_count), one slot a block,
//             then one block over the slots (k_mg_extent_sum).  No atomics.  The host derives the grid, checks the capacity rules (|zq| from the extremes of z: the quantisation is monotone) and refuses before
//             anything grid-sized is allocated.
//   bin       k_mg_bin, one point per lane: zq and the column into scratch, atomicAdd on the column's count and atomicMin on its lowest zq - integer atomics,
//             independent of their order.  k_mg_seed turns (count, lowest) into the seed in place, writes the occupancy base (0 unknown, 1 free) and counts the
//             seeded columns.
//   envelope  k_mg_relax, one block per MG_TILE x MG_TILE tile: the tile and a halo of one column in LDS (34 x 34 words), relaxed in place to its local fixed
//             point (every thread four columns of a row, min over the eight neighbours plus their step, saturating at INF; at most MG_LOCAL_MAX passes, more than
//             the 34 a change needs to cross the tile), then written to the other of two grid buffers; a launch reads one buffer and writes the other, so a
//             round is a Jacobi step between tiles and its outcome does not depend on the order the blocks run in.  Every value is at all times an upper bound of
//             g that only falls, so any schedule ends at g.  A round sets its word of the flag array when a tile changed; the host launches
//             QN_GROUND_ROUNDS_PER_CHECK rounds, then reads the flags, and stops at the first round that changed nothing (both buffers then hold g).  A round
//             carries a change across at least one column, so max(W, H) + 2 rounds bound the loop (QN_ERR_INTERNAL beyond it).
//   classify  k_mg_classify, one point per lane in the map's own order: the class byte, height_q, the column's occupied byte (a plain store of the same value
//             by whoever finds an obstacle), the five class counts of the block into its slot.  k_mg_occ_count counts the occupied and the unknown columns.  Every
//             count of a block goes through block_count and is added up by k_slot_fold (qn_map_compact.cuh).
//   keep      qn_kf_map_keep_classes: k_mg_keep_flag (the removed byte from the class mask, the block's kept count), then the scan and the shared end of the
//             map's filters (qn_map_compact.cuh), which the outlier filter uses.
// Host synchronisations of a classify: 2 + ceil(rounds / QN_GROUND_ROUNDS_PER_CHECK) - the extent, the flags of every batch of rounds, the counts at the end.
// No f32 or f64 arithmetic on the device after k_mg_bin's quantisation.  Results are committed only on success (KfMapResults, qn_kf_buf.h), so a refused call
// leaves the previous results as they were.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_map_compact.cuh"

#define MG_BLOCK 256                                     // the point and column kernels' block
#define MG_TILE 32                                       // the envelope's tile edge
#define MG_LOCAL_MAX 72                                  // passes over a tile per round: 2 MG_TILE + 8 (a change crosses the 34 columns in at most 34)

namespace {

#define MG_SUM_BLOCK MO_SCAN_BLOCK
#define MG_HALO (MG_TILE + 2)
#define MG_INF INT32_MAX
#define MG_NO_COL 0xffffffffu
#define MG_LIMIT (1 << 30)
#define MG_MAX_SIDE (1u << 24)

static_assert(MG_BLOCK * 4 == MG_TILE * MG_TILE, "k_mg_relax: four columns of the tile per thread");
static_assert(MG_BLOCK == MO_BLOCK, "block_count and the block folds take MO_BLOCK threads");

// the finite points of the block: slots[8 b ..] = min x, min y, min z, max x, max y, max z (f32 bits), their number, 0
__global__ void __launch_bounds__(MG_BLOCK) k_mg_extent(uint32_t n, const float4* __restrict__ map, uint32_t* __restrict__ slots) {
  __shared__ float ws[6][MO_WAVES];
  const uint32_t i = blockIdx.x * MG_BLOCK + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool fin = false;
  if (i < n) {
    const float4 p = map[i];
    fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    if (fin) { lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z; }
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float l = wave_min(lo[a]), h = wave_max(hi[a]);
    if (lane == 0) { ws[a][wave] = l; ws[3 + a][wave] = h; }
  }
  // its barrier is the one the extremes wait for: block_min and block_max, two barriers more, cost the call 2 % at 3e7 points (profiles/EXPERIMENTS.md)
  block_count(slots + 8 * (size_t)blockIdx.x + 6, fin);
  if (threadIdx.x < 6) {
    float v = ws[threadIdx.x][0];
    for (int w = 1; w < MO_WAVES; w++) v = threadIdx.x < 3 ? fminf(v, ws[threadIdx.x][w]) : fmaxf(v, ws[threadIdx.x][w]);
    slots[8 * (size_t)blockIdx.x + threadIdx.x] = __float_as_uint(v);
  }
}

// one block: out[0 .. 7) = the nb slots of k_mg_extent folded
__global__ void __launch_bounds__(MG_SUM_BLOCK) k_mg_extent_sum(const uint32_t* __restrict__ slots, uint32_t nb, uint32_t* __restrict__ out) {
  __shared__ float ws[6][MG_SUM_BLOCK / 64];
  __shared__ uint32_t wc[MG_SUM_BLOCK / 64];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t c = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += MG_SUM_BLOCK) {
    const uint32_t* sl = slots + 8 * (size_t)b;
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __uint_as_float(sl[a])); hi[a] = fmaxf(hi[a], __uint_as_float(sl[3 + a])); }
    c += sl[6];
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float l = wave_min(lo[a]), h = wave_max(hi[a]);
    if (lane == 0) { ws[a][wave] = l; ws[3 + a][wave] = h; }
  }
  c = wave_sum(c);
  if (lane == 0) wc[wave] = c;
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = ws[threadIdx.x][0];
    for (int w = 1; w < MG_SUM_BLOCK / 64; w++) v = threadIdx.x < 3 ? fminf(v, ws[threadIdx.x][w]) : fmaxf(v, ws[threadIdx.x][w]);
    out[threadIdx.x] = __float_as_uint(v);
  } else if (threadIdx.x == 6) {
    uint32_t acc = 0;
    for (int w = 0; w < MG_SUM_BLOCK / 64; w++) acc += wc[w];
    out[6] = acc;
  }
}

struct MgGrid { uint32_t W, H; float inv, minbx, minby; };

// one point per lane: the quantised height and the column (MG_NO_COL: a non-finite record) into scratch, the column's count and lowest height by integer atomics
__global__ void __launch_bounds__(MG_BLOCK) k_mg_bin(uint32_t n, const float4* __restrict__ map, const MgGrid G, double scale, int32_t* __restrict__ zq_out,
                                                     uint32_t* __restrict__ col_out, uint32_t* __restrict__ cnt, int32_t* __restrict__ low) {
  const uint32_t i = blockIdx.x * MG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 p = map[i];
  uint32_t col = MG_NO_COL; int32_t zq = 0;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    zq = (int32_t)rint((double)p.z * scale);             // |.| < 2^30: the host checked the extremes, and the quantisation is monotone
    const int cx = (int)(floorf(p.x * G.inv) - G.minbx), cy = (int)(floorf(p.y * G.inv) - G.minby);
    if ((uint32_t)cx < G.W && (uint32_t)cy < G.H) {      // always (the extremes made the grid, the subtraction is exact below 2^24): kept as the store's guard
      col = (uint32_t)cy * G.W + (uint32_t)cx;
      atomicAdd(&cnt[col], 1u);
      atomicMin(&low[col], zq);
    }
  }
  zq_out[i] = zq; col_out[i] = col;
}

// one column per lane: (count, lowest) -> the seed in place, the occupancy base, the block's seeded columns into its slot
__global__ void __launch_bounds__(MG_BLOCK) k_mg_seed(uint32_t cells, const uint32_t* __restrict__ cnt, int32_t* __restrict__ seed, uint32_t min_points,
                                                      uint8_t* __restrict__ occ, uint32_t* __restrict__ slots) {
  const uint32_t c = blockIdx.x * MG_BLOCK + threadIdx.x;
  bool seeded = false;
  if (c < cells) {
    const uint32_t k = cnt[c];
    seeded = k >= min_points;
    if (!seeded) seed[c] = MG_INF;
    occ[c] = k ? 1 : 0;
  }
  block_count(slots + blockIdx.x, seeded);
}

__device__ __forceinline__ int mg_step(int v, int step) { return v > MG_INF - step ? MG_INF : v + step; }       // v + step saturating at INF (INF stays INF)

// one tile per block: src -> dst relaxed to the tile's fixed point under the halo src holds; *flag = 1 when a column of the tile changed
__global__ void __launch_bounds__(MG_BLOCK) k_mg_relax(const int32_t* __restrict__ src, int32_t* __restrict__ dst, uint32_t W, uint32_t H, uint32_t tiles_x,
                                                       int step_s, int step_d, uint32_t* __restrict__ flag) {
  __shared__ int t[MG_HALO * MG_HALO];
  const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
  const long long x0 = (long long)bx * MG_TILE - 1, y0 = (long long)by * MG_TILE - 1;
  for (uint32_t i = threadIdx.x; i < MG_HALO * MG_HALO; i += MG_BLOCK) {
    const long long gx = x0 + (i % MG_HALO), gy = y0 + (i / MG_HALO);
    t[i] = (gx >= 0 && gx < (long long)W && gy >= 0 && gy < (long long)H) ? src[(size_t)gy * W + (size_t)gx] : MG_INF;
  }
  __syncthreads();
  const uint32_t row = threadIdx.x >> 3, cx = (threadIdx.x & 7) * 4;
  const uint32_t gy = by * MG_TILE + row, gx = bx * MG_TILE + cx;
  const uint32_t base = (row + 1) * MG_HALO + cx + 1;
  int first[4]; bool in[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { first[j] = t[base + j]; in[j] = gy < H && gx + j < W; }
  for (int pass = 0; pass < MG_LOCAL_MAX; pass++) {
    bool ch = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t q = base + j;
      const int v = t[q];
      int m = min(min(t[q - 1], t[q + 1]), min(t[q - MG_HALO], t[q + MG_HALO]));
      const int d = min(min(t[q - MG_HALO - 1], t[q - MG_HALO + 1]), min(t[q + MG_HALO - 1], t[q + MG_HALO + 1]));
      m = min(mg_step(m, step_s), mg_step(d, step_d));
      if (in[j] && m < v) { t[q] = m; ch = true; }     // (a neighbour read while its owner lowers it is the old or the new word: both bound g from above)
    }
    if (!__syncthreads_or(ch)) break;
  }
  bool moved = false;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (in[j]) { const int v = t[base + j]; dst[(size_t)gy * W + gx + j] = v; moved = moved || v != first[j]; }
  }
  if (__syncthreads_or(moved) && threadIdx.x == 0) *flag = 1u;
}

// one point per lane in the map's own order: class, height_q, the column's occupied byte, the block's five class counts into slots[5 b ..]
__global__ void __launch_bounds__(MG_BLOCK) k_mg_classify(uint32_t n, const int32_t* __restrict__ zq, const uint32_t* __restrict__ col, const int32_t* __restrict__ g,
                                                          int tol_q, int clear_q, uint8_t* __restrict__ cls, int32_t* __restrict__ height, uint8_t* __restrict__ occ,
                                                          uint32_t* __restrict__ slots) {
  const uint32_t i = blockIdx.x * MG_BLOCK + threadIdx.x;
  int c = -1;                                            // (past the end: counted nowhere)
  if (i < n) {
    c = QN_GROUND_NONE;
    int32_t hq = INT32_MIN;
    const uint32_t k = col[i];
    if (k != MG_NO_COL) {
      const int32_t gc = g[k];
      if (gc != MG_INF) {
        const long long h = (long long)zq[i] - (long long)gc;        // above -2^32, below 2^31
        c = h < -(long long)tol_q ? QN_GROUND_BELOW : h <= (long long)tol_q ? QN_GROUND_GROUND : h <= (long long)clear_q ? QN_GROUND_OBSTACLE : QN_GROUND_OVERHEAD;
        hq = (int32_t)max(h, (long long)INT32_MIN + 1);
        if (c == QN_GROUND_OBSTACLE) occ[k] = 2;
      }
    }
    cls[i] = (uint8_t)c; height[i] = hq;
  }
  block_count(slots + 5 * (size_t)blockIdx.x, c == QN_GROUND_NONE, c == QN_GROUND_GROUND, c == QN_GROUND_OBSTACLE, c == QN_GROUND_OVERHEAD, c == QN_GROUND_BELOW);
}

// one column per lane: the block's occupied and unknown columns into slots[2 b ..]
__global__ void __launch_bounds__(MG_BLOCK) k_mg_occ_count(uint32_t cells, const uint8_t* __restrict__ occ, uint32_t* __restrict__ slots) {
  const uint32_t c = blockIdx.x * MG_BLOCK + threadIdx.x;
  const int v = c < cells ? (int)occ[c] : 1;
  block_count(slots + 2 * (size_t)blockIdx.x, v == 2, v == 0);
}

// one point per lane: removed = the class's bit is not in the mask; the block's kept records into its slot (what k_scan_rows / k_mo_compact go on from)
__global__ void __launch_bounds__(MO_BLOCK) k_mg_keep_flag(uint32_t n, const uint8_t* __restrict__ cls, uint32_t mask, uint8_t* __restrict__ removed,
                                                           uint32_t* __restrict__ blk_kept) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    keep = ((mask >> cls[i]) & 1u) != 0;
    removed[i] = keep ? 0 : 1;
  }
  block_count(blk_kept + blockIdx.x, keep);
}

// the store's ground state (slot QN_KF_INT_EXT_GROUND)
struct MgSet { DevBuf<uint8_t> cls, occ; DevBuf<int32_t> height, ground; qn_ground_grid info; };
typedef KfMapResults<MgSet> GroundState;

}  // namespace

const uint8_t* qn_kf_int_ground_classes(qn_kf_store* s) {
  const float4* map = nullptr; uint32_t n = 0;
  const MgSet* o = GroundState::lookup(s, QN_KF_INT_EXT_GROUND, &map, &n);
  return o ? o->cls.p : nullptr;
}

extern "C" void qn_ground_default_params(qn_ground_params* p) {
  if (!p) return;
  p->cell = 0.5; p->max_slope = 0.3; p->ground_tol = 0.2; p->clearance = 2.0; p->min_points = 1; p->reserved = 0;      // interface choices, not measurements
}

extern "C" int qn_kf_map_ground(qn_kf_store* s, const qn_ground_params* params, qn_ground_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !stats_out) return QN_ERR_INVALID_ARG;
  const qn_ground_params P = *params;
  if (!std::isfinite(P.cell) || !(P.cell > 0.0) || !std::isfinite(P.max_slope) || !(P.max_slope > 0.0) || !std::isfinite(P.ground_tol) || !(P.ground_tol >= 0.0) ||
      !std::isfinite(P.clearance) || !(P.clearance > P.ground_tol) || P.min_points < 1 || P.reserved != 0)
    return QN_ERR_INVALID_ARG;
  const int e = qn_quant_exponent(P.cell, 10);           // a cell is 2^9 .. 2^10 units: the steps, tolerances and |zq| refused at 2^30 span 2^20 cells, h fits 64 bits
  const double scale = std::ldexp(1.0, e);
  const double fs = std::rint(P.max_slope * P.cell * scale), ft = std::rint(P.ground_tol * scale), fc = std::rint(P.clearance * scale);
  if (!(fs < (double)MG_LIMIT && ft < (double)MG_LIMIT && fc < (double)MG_LIMIT)) return QN_ERR_INVALID_ARG;
  const int step_s = std::max(1, (int)fs);
  const long long sd = ((long long)step_s * 181) >> 7;
  if (sd >= (long long)MG_LIMIT) return QN_ERR_INVALID_ARG;
  const int step_d = (int)sd, tol_q = (int)ft, clear_q = (int)fc;
  uint32_t n = 0; uint64_t gen = 0;
  const float4* map = qn_kf_int_map(s, &n, &gen);
  if (!map) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  GroundState* st = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_GROUND, &st);
  if (rc != QN_OK) return rc;
  hipStream_t stream = qn_kf_int_stream(s);
  const uint32_t nb = (n + MG_BLOCK - 1) / MG_BLOCK;
  // ---- the extent of the finite points
  uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 8 * ((size_t)nb + 1));
  uint32_t* h = (uint32_t*)qn_kf_int_pinned(s, 64);
  if (!d_slots || !h) return qn_kf_fail(s, "qn_kf_map_ground: scratch allocation failed");
  hipLaunchKernelGGL(k_mg_extent, dim3(nb), dim3(MG_BLOCK), 0, stream, n, map, d_slots);
  hipLaunchKernelGGL(k_mg_extent_sum, dim3(1), dim3(MG_SUM_BLOCK), 0, stream, (const uint32_t*)d_slots, nb, d_slots + 8 * (size_t)nb);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_slots + 8 * (size_t)nb, sizeof(uint32_t) * 7, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 1: the extent
  float ext[6];
  memcpy(ext, h, sizeof(ext));
  const uint32_t nfin = h[6];
  qn_ground_stats r;
  memset(&r, 0, sizeof(r));
  r.n = n; r.n_finite = nfin; r.quant_exp = e; r.step_s = step_s; r.step_d = step_d; r.tol_q = tol_q; r.clear_q = clear_q;
  qn_ground_grid info;
  memset(&info, 0, sizeof(info));
  info.cell = P.cell; info.quant_exp = e;
  MgGrid G; G.W = G.H = 0; G.inv = (float)(1.0 / P.cell); G.minbx = G.minby = 0.0f;
  if (nfin) {
    const float two31 = 2147483648.0f;
    long long side[2]; float minb[2];
    for (int a = 0; a < 2; a++) {
      const float lo = std::floor(ext[a] * G.inv), hi = std::floor(ext[3 + a] * G.inv);
      if (!(lo >= -two31 && lo < two31 && hi >= -two31 && hi < two31)) {                        // (a NaN from 0 * inf fails every comparison)
        qn_kf_int_set_error(s, "qn_kf_map_ground: a column index outside the int32 range");
        return QN_ERR_CAPACITY;
      }
      side[a] = (long long)hi - (long long)lo + 1; minb[a] = lo;
    }
    if (side[0] > (long long)MG_MAX_SIDE || side[1] > (long long)MG_MAX_SIDE || side[0] * side[1] > (long long)QN_GROUND_MAX_CELLS) {
      qn_kf_int_set_error(s, "qn_kf_map_ground: a grid of more than 2^26 columns (or 2^24 a side)");
      return QN_ERR_CAPACITY;
    }
    if (!(std::fabs(std::rint((double)ext[2] * scale)) < (double)MG_LIMIT && std::fabs(std::rint((double)ext[5] * scale)) < (double)MG_LIMIT)) {
      qn_kf_int_set_error(s, "qn_kf_map_ground: a height of 2^30 units of 2^-e m or more");
      return QN_ERR_CAPACITY;
    }
    G.W = (uint32_t)side[0]; G.H = (uint32_t)side[1]; G.minbx = minb[0]; G.minby = minb[1];
    info.origin_x = (double)minb[0] * P.cell; info.origin_y = (double)minb[1] * P.cell; info.width = G.W; info.height = G.H;
  }
  r.width = G.W; r.height = G.H;
  const uint32_t cells = G.W * G.H, cb = (cells + MG_BLOCK - 1) / MG_BLOCK;
  // ---- the buffers: the spare result set, and scratch (1: zq, 2: columns, 3: slots and sums, 4: column counts, 5: the envelope's other buffer, 6: flags)
  MgSet& o = st->spare();
  if (!o.cls.grow(s, std::max<size_t>(n, 1)) || !o.height.grow(s, std::max<size_t>(n, 1)) || !o.occ.grow(s, std::max<size_t>(cells, 1)) ||
      !o.ground.grow(s, std::max<size_t>(cells, 1)))
    return QN_ERR_HIP;
  const size_t nslots = std::max<size_t>(8 * ((size_t)nb + 1), 5 * (size_t)std::max(nb, cb)) + 16;
  int32_t* d_zq = (int32_t*)qn_kf_int_scratch(s, 1, sizeof(int32_t) * (size_t)n);
  uint32_t* d_col = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (size_t)n);
  d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * nslots);
  uint32_t* d_cnt = (uint32_t*)qn_kf_int_scratch(s, 4, sizeof(uint32_t) * std::max<size_t>(cells, 1));
  int32_t* d_other = (int32_t*)qn_kf_int_scratch(s, 5, sizeof(int32_t) * std::max<size_t>(cells, 1));
  uint32_t* d_flags = (uint32_t*)qn_kf_int_scratch(s, 6, sizeof(uint32_t) * QN_GROUND_ROUNDS_PER_CHECK);
  if (!d_zq || !d_col || !d_slots || !d_cnt || !d_other || !d_flags) return qn_kf_fail(s, "qn_kf_map_ground: scratch allocation failed");
  uint32_t* d_sums = d_slots + nslots - 16;                          // 0: seeded, 1 .. 5: the classes, 6 .. 7: occupied, unknown
  QN_KFCHK(s, hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * 16, stream));
  if (cells) {
    QN_KFCHK(s, hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * (size_t)cells, stream));
    QN_KFCHK(s, hipMemsetD32Async((hipDeviceptr_t)o.ground.p, MG_INF, (size_t)cells, stream));
  }
  hipLaunchKernelGGL(k_mg_bin, dim3(nb), dim3(MG_BLOCK), 0, stream, n, map, G, scale, d_zq, d_col, d_cnt, o.ground.p);
  uint32_t rounds = 0;
  if (cells) {
    hipLaunchKernelGGL(k_mg_seed, dim3(cb), dim3(MG_BLOCK), 0, stream, cells, (const uint32_t*)d_cnt, o.ground.p, P.min_points, o.occ.p, d_slots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 1>), dim3(1), dim3(MG_SUM_BLOCK), 0, stream, (const uint32_t*)d_slots, cb, d_sums);
    QN_KFCHK(s, hipGetLastError());
    // ---- the envelope: rounds in batches, the flags read once a batch; max(W, H) + 2 rounds bound the loop
    const uint32_t tiles_x = (G.W + MG_TILE - 1) / MG_TILE, tiles_y = (G.H + MG_TILE - 1) / MG_TILE;
    const uint32_t limit = std::max(G.W, G.H) + 2;
    int32_t* buf[2] = {o.ground.p, d_other};
    bool settled = false;
    while (!settled && rounds < limit) {
      const uint32_t batch = std::min<uint32_t>(QN_GROUND_ROUNDS_PER_CHECK, limit - rounds);
      QN_KFCHK(s, hipMemsetAsync(d_flags, 0, sizeof(uint32_t) * QN_GROUND_ROUNDS_PER_CHECK, stream));
      for (uint32_t b = 0; b < batch; b++, rounds++)
        hipLaunchKernelGGL(k_mg_relax, dim3(tiles_x * tiles_y), dim3(MG_BLOCK), 0, stream, (const int32_t*)buf[rounds & 1], buf[(rounds + 1) & 1], G.W, G.H, tiles_x,
                           step_s, step_d, d_flags + b);
      QN_KFCHK(s, hipGetLastError());
      QN_KFCHK(s, hipMemcpyAsync(h, d_flags, sizeof(uint32_t) * QN_GROUND_ROUNDS_PER_CHECK, hipMemcpyDeviceToHost, stream));
      QN_KFCHK(s, hipStreamSynchronize(stream));         // one sync a batch of rounds
      for (uint32_t b = 0; b < batch; b++) settled = settled || h[b] == 0;      // a round that changed nothing: both buffers hold g from then on
    }
    if (!settled) {
      qn_kf_int_set_error(s, "qn_kf_map_ground: the envelope did not settle within max(W, H) + 2 rounds");
      return QN_ERR_INTERNAL;
    }
  }
  hipLaunchKernelGGL(k_mg_classify, dim3(nb), dim3(MG_BLOCK), 0, stream, n, (const int32_t*)d_zq, (const uint32_t*)d_col, (const int32_t*)o.ground.p, tol_q, clear_q,
                     o.cls.p, o.height.p, o.occ.p, d_slots);
  hipLaunchKernelGGL((k_slot_fold<uint32_t, 5>), dim3(1), dim3(MG_SUM_BLOCK), 0, stream, (const uint32_t*)d_slots, nb, d_sums + 1);
  if (cells) {
    hipLaunchKernelGGL(k_mg_occ_count, dim3(cb), dim3(MG_BLOCK), 0, stream, cells, (const uint8_t*)o.occ.p, d_slots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 2>), dim3(1), dim3(MG_SUM_BLOCK), 0, stream, (const uint32_t*)d_slots, cb, d_sums + 6);
  }
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_sums, sizeof(uint32_t) * 8, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // the last sync: the counts
  r.seeded = h[0];
  r.n_none = h[1]; r.n_ground = h[2]; r.n_obstacle = h[3]; r.n_overhead = h[4]; r.n_below = h[5];
  r.occupied = h[6]; r.unknown = h[7]; r.free = cells - h[6] - h[7];
  r.rounds = rounds;
  o.info = info;
  st->commit(gen, n);
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_ground_points(qn_kf_store* s, uint8_t* class_out, int32_t* height_q_out) {
  if (!s || (!class_out && !height_q_out)) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const MgSet* o = GroundState::lookup(s, QN_KF_INT_EXT_GROUND, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (class_out) QN_KFCHK(s, hipMemcpyAsync(class_out, o->cls.p, n, hipMemcpyDeviceToHost, stream));
  if (height_q_out) QN_KFCHK(s, hipMemcpyAsync(height_q_out, o->height.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_ground_grid(qn_kf_store* s, qn_ground_grid* info_out, int32_t* ground_q_out, uint8_t* occupancy_out) {
  if (!s || !info_out) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const MgSet* o = GroundState::lookup(s, QN_KF_INT_EXT_GROUND, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  const qn_ground_grid& g = o->info;
  const size_t cells = (size_t)g.width * g.height;
  *info_out = g;
  if (!cells || (!ground_q_out && !occupancy_out)) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (ground_q_out) QN_KFCHK(s, hipMemcpyAsync(ground_q_out, o->ground.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, stream));
  if (occupancy_out) QN_KFCHK(s, hipMemcpyAsync(occupancy_out, o->occ.p, cells, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_keep_classes(qn_kf_store* s, uint32_t class_mask, const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || !d_xyzi_out || !n_out || class_mask == 0 || (class_mask & ~31u)) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const MgSet* o = GroundState::lookup(s, QN_KF_INT_EXT_GROUND, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  const uint32_t nb = (n + MO_BLOCK - 1) / MO_BLOCK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  float4* d_kept = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)n);
  uint8_t* d_removed = (uint8_t*)qn_kf_int_scratch(s, 2, (size_t)n);
  uint32_t* d_blk = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * (2 * (size_t)nb + 1));      // the blocks' counts, then their offsets and the total
  uint32_t* h = (uint32_t*)qn_kf_int_pinned(s, 64);
  if (!d_kept || !d_removed || !d_blk || !h) return qn_kf_fail(s, "qn_kf_map_keep_classes: scratch allocation failed");
  uint32_t* d_off = d_blk + nb;
  hipLaunchKernelGGL(k_mg_keep_flag, dim3(nb), dim3(MO_BLOCK), 0, stream, n, (const uint8_t*)o->cls.p, class_mask, d_removed, d_blk);
  hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(MO_SCAN_BLOCK), 0, stream, (const uint32_t*)d_blk, nb, d_off, d_off + nb);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return qn_kf_map_compact_shrink(s, map, n, d_removed, d_off, d_kept, h[0], d_xyzi_out, n_out);
}
