// qn_mapdistance.inc - the exact Euclidean distance field of the 3-D occupancy map on the GPU (qn_kf_map_distance, qn_kf_map_distance_grid,
// qn_kf_map_distance_slice, qn_kf_map_distance_query: include/qn_engine.h).  The numpy twin qn_amd/mapdistance.py is the specification: a site is a voxel of
// the live occupancy volume whose class bit is in site_mask, d2[v] the smallest squared distance in voxels from v to a site, QN_DIST_FAR above max_dist^2 or
// without a site.  Everything is an integer, so every byte equals the twin's whatever the algorithm.  Three separable passes over two u16 grids:
//   x         k_md_x, one voxel per lane in linear order: the site flags of the block's 256 voxels and of up to max_dist voxels on either side are ballot words in
//             LDS (12 words of 64); a lane finds the nearest site to its left and right by clz / ctz over the words, no further than max_dist and no further than
//             its own row reaches (a row is contiguous, so the linear neighbours inside those limits are the row's).  f = the smaller distance squared, or FAR.
//   y, z      k_md_axis<LAST>, one voxel per lane in linear order, so the lanes run along x and every load is coalesced: min over d of f[. + d stride] + d d,
//             walking outwards from d = 0 and stopping once d d >= the best so far, which is exact (every later term is at least d d) and makes the cost the
//             distance to the answer, not max_dist.  Plain global loads: the neighbours of a block's voxels are the neighbours' blocks' voxels, served by L2.
//             A result above max_dist^2 becomes FAR: a site within max_dist has every per-axis offset within max_dist, so it survives the windowed passes.
//             The z pass (LAST) also counts: sites, reached and far voxels, the block's largest and summed reached d2 into slots of their own (dg_block_stats:
//             block_count(sites, reached, far), wave_max and wave_sum behind its barrier); dg_fold_stats folds the slots (k_slot_fold<uint32_t, 3>, k_slot_max).
//   slice     the smallest d2 over a band of layers: k_dg_slice<uint16_t, op_min> of qn_dense_grid.cuh, one column per lane.
//   query     k_md_query, one point per lane: the voxel of an f64 world point by the occupancy map's quantisation (oc_voxel; the only floating point in this file's kernels).
// Every voxel and every slot has one writer, nothing is read and modified in place; no scratch memory, no dynamically indexed private array.  Host synchronisations of qn_kf_map_distance: one - the statistics.
// Part of qn_staticmap.hip's translation unit (included after qn_mapoccupancy.inc): the field hangs on that file's OccState and takes no slot of its own; the
// index arithmetic, the statistics tail, the slice, the point upload and the lookup of the live results are qn_dense_grid.cuh's.

namespace {

#define MD_BLOCK MO_BLOCK
#define MD_WORDS (3 * MD_BLOCK / 64)                     // the ballot words of a block of k_md_x: its own voxels and a block's worth on either side
#define MD_NONE 0xffffffffu
static_assert(QN_DIST_MAX_RADIUS < MD_BLOCK, "the halo of k_md_x is one block on either side");

// the distance from position j down to the nearest set bit at or below it in the ballot words w, no further than lim (<= 255 <= j - 1); MD_NONE without one
__device__ __forceinline__ uint32_t md_left(const unsigned long long* w, uint32_t j, uint32_t lim) {
  uint32_t wi = j >> 6;
  unsigned long long m = w[wi] & (~0ull >> (63u - (j & 63u)));
  for (;;) {
    if (m) {
      const uint32_t d = j - (wi * 64u + 63u - (uint32_t)__builtin_clzll(m));
      return d <= lim ? d : MD_NONE;
    }
    if (wi == 0 || j - (wi * 64u - 1u) > lim) return MD_NONE;        // the nearest position of the next word is already too far
    m = w[--wi];
  }
}

// the same upwards: the nearest set bit at or above j
__device__ __forceinline__ uint32_t md_right(const unsigned long long* w, uint32_t j, uint32_t lim) {
  uint32_t wi = j >> 6;
  unsigned long long m = w[wi] & (~0ull << (j & 63u));
  for (;;) {
    if (m) {
      const uint32_t d = wi * 64u + (uint32_t)__builtin_ctzll(m) - j;
      return d <= lim ? d : MD_NONE;
    }
    if (wi == MD_WORDS - 1 || (wi + 1u) * 64u - j > lim) return MD_NONE;
    m = w[++wi];
  }
}

// one voxel per lane, linear order: f[v] = the squared distance along x to the nearest site of v's row within R, or FAR
__global__ void __launch_bounds__(MD_BLOCK) k_md_x(uint32_t cells, uint32_t W, const uint8_t* __restrict__ cls, uint32_t mask, uint32_t R, uint16_t* __restrict__ f) {
  __shared__ unsigned long long words[MD_WORDS];
  const uint32_t b0 = blockIdx.x * MD_BLOCK;
  // position j of the block's window is the voxel b0 - MD_BLOCK + j; the flags further than R from the block's own voxels are never read and stay 0
#pragma unroll
  for (uint32_t seg = 0; seg < 3; seg++) {
    const uint32_t j = seg * MD_BLOCK + threadIdx.x;
    const long long p = (long long)b0 - MD_BLOCK + j;
    bool site = false;
    if (j + R >= MD_BLOCK && j < 2 * MD_BLOCK + R && p >= 0 && p < (long long)cells) site = ((mask >> cls[p]) & 1u) != 0;
    const unsigned long long bal = __ballot(site);
    if ((threadIdx.x & 63) == 0) words[j >> 6] = bal;
  }
  __syncthreads();
  const uint32_t i = b0 + threadIdx.x;
  if (i >= cells) return;
  const uint32_t x = i % W, j = MD_BLOCK + threadIdx.x;
  const uint32_t dl = md_left(words, j, min(R, x)), dr = md_right(words, j, min(R, W - 1u - x));
  const uint32_t d = min(dl, dr);
  f[i] = (uint16_t)(d == MD_NONE ? QN_DIST_FAR : d * d);
}

// One voxel per lane, linear order: g[v] = min over |d| <= R, inside the axis, of f[v + d stride] + d d; above R^2: FAR.  n: the voxels along the axis, stride:
// between two of them - the kernel's own coordinate, not oc_ijk's split: with the split the call missed its timing bar twice (profiles/EXPERIMENTS.md).  LAST: the
// z pass, which also leaves the block's counts - cslots[3 b ..] = its sites, reached and far voxels, mslots[b] = the largest d2 of its reached voxels, tslots[b] = their sum.
template <bool LAST>
__global__ void __launch_bounds__(MD_BLOCK) k_md_axis(uint32_t cells, uint32_t stride, uint32_t n, uint32_t R, const uint16_t* __restrict__ f, uint16_t* __restrict__ g,
                                                      uint32_t* __restrict__ cslots, uint32_t* __restrict__ mslots, unsigned long long* __restrict__ tslots) {
  const uint32_t i = blockIdx.x * MD_BLOCK + threadIdx.x;
  const uint32_t R2 = R * R;
  uint32_t best = QN_DIST_FAR;
  if (i < cells) {
    const uint32_t c = (i / stride) % n;                             // the voxel's coordinate along the axis
    const uint32_t below = min(R, c), above = min(R, n - 1u - c);
    best = f[i];
    for (uint32_t d = 1; d <= max(below, above) && d * d < best; d++) {
      const uint32_t dd = d * d;
      if (d <= below) best = min(best, (uint32_t)f[i - d * stride] + dd);
      if (d <= above) best = min(best, (uint32_t)f[i + d * stride] + dd);
    }
    if (best > R2) best = QN_DIST_FAR;
    g[i] = (uint16_t)best;
  }
  if (LAST) {
    const bool in = i < cells, reached = in && best != 0 && best != QN_DIST_FAR;
    dg_block_stats(in && best == 0, reached, in && best == QN_DIST_FAR, reached ? best : 0u, cslots, mslots, tslots);
  }
}

// one point per lane: its voxel by the occupancy map's quantisation (oc_voxel: qn_dense_grid.cuh), then the field's value and the voxel's class there; FAR and
// OUTSIDE for a point that is not finite, 2^20 voxels or more from the origin, or outside the grid
__global__ void __launch_bounds__(MD_BLOCK) k_md_query(uint32_t n, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t D, const uint16_t* __restrict__ d2,
                                                       const uint8_t* __restrict__ cls, uint16_t* __restrict__ d2_out, uint8_t* __restrict__ cls_out) {
  const uint32_t i = blockIdx.x * MD_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x, y, z, v = QN_DIST_FAR, q = QN_DIST_OUTSIDE;
  if (oc_voxel(xyz, i, inv, G, D, 0u, &x, &y, &z)) {
    const uint32_t lin = dg_index(x, y, z, G.W, G.H);
    v = d2[lin]; q = cls[lin];
  }
  d2_out[i] = (uint16_t)v; cls_out[i] = (uint8_t)q;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The distance field of the latest successful call (a member of OccState); `live` ends with the occupancy result it was computed from
struct DistState {
  bool live = false;
  DevBuf<uint16_t> d2, tmp;
  qn_distance_params params;
  std::shared_ptr<struct RouteState> route;              // the route field of qn_maproute.inc (included behind this file, where the type is completed)
};
void mr_end(RouteState*);                                // (qn_maproute.inc) a new distance field ends the route field of the previous one; its buffer stays

void md_end(DistState* d) { if (d) { d->live = false; mr_end(d->route.get()); } }

}  // namespace

extern "C" void qn_distance_default_params(qn_distance_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->site_mask = 1u << QN_OCC_OCCUPIED; p->max_dist = 16;           // interface choices, not measurements
}

extern "C" int qn_kf_map_distance(qn_kf_store* s, const qn_distance_params* params, qn_distance_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !stats_out) return QN_ERR_INVALID_ARG;
  const qn_distance_params P = *params;
  if (P.site_mask == 0 || (P.site_mask & ~7u) || P.max_dist < 1 || P.max_dist > QN_DIST_MAX_RADIUS || P.reserved[0] != 0 || P.reserved[1] != 0) return QN_ERR_INVALID_ARG;
  OccState* o = dg_mut(dg_live(s).occ);
  if (!o) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t cells = dg_cells(g), cb = dg_blocks(cells);
  qn_distance_stats r;
  memset(&r, 0, sizeof(r));
  if (!o->dist) o->dist.reset(new (std::nothrow) DistState());
  if (!o->dist) return qn_kf_fail(s, "qn_kf_map_distance: out of memory");
  DistState* st = o->dist.get();
  if (cells) {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    const hipStream_t str = qn_kf_int_stream(s);
    // ---- the two grids: a larger one is allocated beside the previous field, which goes only once both are there
    DevBuf<uint16_t> na, nb;
    if (!st->d2.grow_beside(s, cells, na) || !st->tmp.grow_beside(s, cells, nb)) return QN_ERR_HIP;
    // ---- scratch (3: the blocks' three counts, then their largest d2; 4: their u64 sums; 5: the folded sums - sites, reached, far, max_d2 and sum_d2 at byte 16)
    uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 4 * (size_t)cb);
    unsigned long long* d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * (size_t)cb);
    char* d_small = (char*)qn_kf_int_scratch(s, 5, 32);
    char* h = (char*)qn_kf_int_pinned(s, 32);
    if (!d_slots || !d_tslots || !d_small || !h) return qn_kf_fail(s, "qn_kf_map_distance: scratch allocation failed");
    // ---- from here on the previous field is gone
    st->live = false;
    st->d2.adopt(na); st->tmp.adopt(nb);
    hipLaunchKernelGGL(k_md_x, dim3(cb), dim3(MD_BLOCK), 0, str, cells, g.width, (const uint8_t*)o->cls.p, P.site_mask, P.max_dist, st->d2.p);
    hipLaunchKernelGGL(k_md_axis<false>, dim3(cb), dim3(MD_BLOCK), 0, str, cells, g.width, g.height, P.max_dist, (const uint16_t*)st->d2.p, st->tmp.p, (uint32_t*)nullptr,
                       (uint32_t*)nullptr, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_md_axis<true>, dim3(cb), dim3(MD_BLOCK), 0, str, cells, dg_cols(g), g.depth, P.max_dist, (const uint16_t*)st->tmp.p, st->d2.p, d_slots, d_slots + 3 * (size_t)cb, d_tslots);
    dg_fold_stats(str, d_slots, d_tslots, cb, d_small);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h, d_small, 32, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                   // the one sync: the statistics
    const uint32_t* sums = (const uint32_t*)h;
    r.sites = sums[0]; r.reached = sums[1]; r.far = sums[2]; r.max_d2 = sums[3];
    memcpy(&r.sum_d2, h + 16, sizeof(r.sum_d2));
  }
  st->params = P;
  st->live = true;
  mr_end(st->route.get());
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_distance_grid(qn_kf_store* s, qn_occupancy_grid* info_out, qn_distance_params* params_out, uint16_t* d2_out) {
  if (!s || !info_out || !params_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.dist) return QN_ERR_NOT_READY;
  const size_t cells = dg_cells(L.occ->info);
  *info_out = L.occ->info; *params_out = L.dist->params;
  if (!cells || !d2_out) return QN_OK;
  return qn_kf_download(s, d2_out, L.dist->d2.p, sizeof(uint16_t) * cells);
}

extern "C" int qn_kf_map_distance_slice(qn_kf_store* s, int32_t iz_lo, int32_t iz_hi, uint16_t* d2_out) {
  if (!s || !d2_out || iz_lo > iz_hi) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.dist) return QN_ERR_NOT_READY;
  return dg_slice<uint16_t, op_min>(s, "qn_kf_map_distance_slice", L.occ->info, L.dist->d2.p, iz_lo, iz_hi, (uint16_t)QN_DIST_FAR, d2_out);
}

extern "C" int qn_kf_map_distance_query(qn_kf_store* s, const double* xyz, uint32_t n, uint16_t* d2_out, uint8_t* class_out) {
  if (!s || !xyz || n == 0 || !d2_out || !class_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.dist) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = L.occ->info;
  if (!dg_cells(g)) {                                                // an empty grid: every point is outside
    std::fill(d2_out, d2_out + n, (uint16_t)QN_DIST_FAR); memset(class_out, QN_DIST_OUTSIDE, n);
    return QN_OK;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (0: the points, 1: their d2, 2: their classes)
  uint16_t* d_d2 = (uint16_t*)qn_kf_int_scratch(s, 1, sizeof(uint16_t) * (size_t)n);
  uint8_t* d_cls = (uint8_t*)qn_kf_int_scratch(s, 2, n);
  if (!d_d2 || !d_cls) return qn_kf_fail(s, "qn_kf_map_distance_query: scratch allocation failed");
  DgPoints pts;
  if (dg_points(s, "qn_kf_map_distance_query", xyz, n, &pts) != QN_OK) return QN_ERR_HIP;
  hipLaunchKernelGGL(k_md_query, pts.grid, dim3(MD_BLOCK), 0, str, n, pts.xyz, 1.0 / g.voxel, oc_grid(g), g.depth, (const uint16_t*)L.dist->d2.p, (const uint8_t*)L.occ->cls.p, d_d2, d_cls);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(d2_out, d_d2, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipMemcpyAsync(class_out, d_cls, n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}
