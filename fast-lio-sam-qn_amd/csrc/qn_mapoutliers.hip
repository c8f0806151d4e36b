// qn_mapoutliers.hip - the isolated noise points of the store's map slot, found and removed on the GPU (qn_kf_map_outliers, qn_kf_map_outlier_points,
// qn_kf_map_remove_outliers: include/qn_engine.h).  The numpy twin qn_amd/mapoutliers.py is the specification: the neighbours of a finite map point are the
// finite map points at another index within r of it by the oracle's f32 sqdist3 (<= float(r * r), inclusive); with fewer than k of them the point is sparse and
// an outlier outright (PCL's RadiusOutlierRemoval with min_neighbors = k); otherwise the mean of its k smallest distances, quantised to an integer of 2^-e m,
// enters PCL's StatisticalOutlierRemoval threshold mean + std_mul * stddev over all dense points.  count and mean_q are integers and the statistics are integer
// sums, so everything equals the twin's bit for bit whatever order the neighbours are met in; the f64 arithmetic behind mean_q is the same IEEE operations in
// the same order (the library is built without contraction, the roots are made correctly rounded below).
//   index     qn_kf_int_cell_index (qn_cloud.hip) over the map as one cloud, as qn_mapnormals.hip uses it; k_cell_gather lays the sorted points (original index
//             in .w) and their cell words out flat (qn_cell_walk.cuh, with the walk and its exactness argument).
//   select    k_map_outliers<L>, one point per lane, 256 lanes a block, in the sorted order, over the candidates of the walk at another position than the
//             query's.  The L smallest d2 live in L registers as u32 bit patterns (d2 >= 0: the f32 order is the u32 order), sorted
//             ascending by a fully unrolled, statically indexed compare-exchange chain that is entered only when d2 < the current L-th; L is 8, 16 or 32, k
//             rounded up (the k smallest are the first k of the L smallest).  No dynamically indexed private array, so no scratch.  The k f64 roots and their
//             sum run once per point after the scan.  dense, sum_q and sum_q2 go through block_sum into the block's own slot; k_slot_fold adds
//             the slots up.  No atomics.
//   flag      k_mo_flag, one point per lane in the map's own order: removed = sparse or double(mean_q) > thr_q; the block's kept count into its slot;
//             k_scan_rows (one block) turns the counts into offsets, the last one the number kept.
//   compact   qn_kf_map_remove_outliers only: the shared end of the map's filters (qn_map_compact.cuh, with the count tail, the fold, the scan and the rank).
// Host synchronisations of a classify: the index's, one for the statistics (the threshold is host arithmetic), one at the end.  Results are committed only
// on success (KfMapResults, qn_kf_buf.h), so a refused call leaves the previous classification as it was.
// The map's other point filter, the clusters (qn_mapclusters.inc, included at the end), is part of this translation unit: it shares the index, the walk, the
// scan and the compaction instantiated here, and its results hang on this unit's slot of the store (MoUnit below).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_cell_walk.cuh"
#include "qn_map_compact.cuh"
#include "qn_union_find.cuh"

namespace {

#define MO_MAX_POINTS (1u << 30)
#define MO_NO_MEAN 0xffffffffu

static_assert(MO_BLOCK == QN_CW_BLOCK, "k_cell_gather and k_map_outliers share a grid");

// The correctly rounded f64 root of x >= 0.  y = RN(sqrt(x)) iff y pred(y) < x <= y succ(y) (in units of y's last place both sides are integers, and no root
// is a midpoint), and a fused multiply-add gives the sign of y y' - x exactly; so whatever the library's sqrt returns within one place of it is put right.
__device__ __forceinline__ double mo_sqrt(double x) {
  double y = sqrt(x);
  if (y > 0.0) {
    const double ym = __longlong_as_double(__double_as_longlong(y) - 1), yp = __longlong_as_double(__double_as_longlong(y) + 1);
    if (fma(y, ym, -x) >= 0.0) y = ym;
    else if (fma(y, yp, -x) < 0.0) y = yp;
  }
  return y;
}

template <int L>
__global__ void __launch_bounds__(MO_BLOCK) k_map_outliers(const CellSeg S, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, float r2, double scale,
                                                           uint32_t k, uint32_t* __restrict__ count, uint32_t* __restrict__ mean_q,
                                                           unsigned long long* __restrict__ slots) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool act = t < S.n;                              // (no early return: every thread of the block meets the barrier of block_sum)
  const bool fin = t < S.nfin;
  const float4 q = act ? spts[t] : make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t qi = __float_as_uint(q.w);
  uint32_t cnt = 0;
  uint32_t key[L];                                       // the L smallest d2 so far, ascending; only ever indexed by unrolled loop counters
#pragma unroll
  for (int j = 0; j < L; j++) key[j] = 0xffffffffu;
  if (fin) {
    cell_walk(S, spts, cells, q, [&](uint32_t pos, const float4&, float d2) {
      if (pos != t && d2 <= r2) {                        // another index than the query's: a duplicate of it elsewhere counts
        cnt++;
        uint32_t v = __float_as_uint(d2);
        if (v < key[L - 1]) {
#pragma unroll
          for (int i = 0; i < L; i++) { const uint32_t lo = min(key[i], v); v = max(key[i], v); key[i] = lo; }
        }
      }
    });
  }
  const bool dense = fin && cnt >= k;
  uint32_t mq = MO_NO_MEAN;
  if (dense) {
    double s = 0.0;                                      // (0 + the first root is the first root)
#pragma unroll
    for (int j = 0; j < L; j++) if ((uint32_t)j < k) s += mo_sqrt((double)__uint_as_float(key[j]));
    mq = (uint32_t)rint(s / (double)k * scale);
  }
  if (act) { count[qi] = cnt; mean_q[qi] = mq; }
  const unsigned long long m64 = dense ? (unsigned long long)mq : 0ull;
  block_sum(slots + 3 * (size_t)blockIdx.x, dense ? 1ull : 0ull, m64, m64 * m64);
}

// one point per lane in the map's own order: the removed byte, and the block's kept records into its slot
__global__ void __launch_bounds__(MO_BLOCK) k_mo_flag(uint32_t n, const float4* __restrict__ map, const uint32_t* __restrict__ count, const uint32_t* __restrict__ mean_q,
                                                      uint32_t k, double thr, uint8_t* __restrict__ removed, uint32_t* __restrict__ blk_kept) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const float4 p = map[i];
    const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    const bool rm = fin && (count[i] < k || (double)mean_q[i] > thr);
    removed[i] = rm ? 1 : 0;
    keep = !rm;
  }
  block_count(blk_kept + blockIdx.x, keep);
}

// the store's outlier state (slot QN_KF_INT_EXT_OUTLIERS): of the classified map's points `kept` stay
struct MoSet { DevBuf<uint32_t> count, mean_q, off; DevBuf<uint8_t> removed; uint32_t kept = 0; };
typedef KfMapResults<MoSet> OutlierState;
// what the slot holds: the outlier results in front (OutlierState::lookup reads the slot as them), and the cluster results of qn_mapclusters.inc, made on
// that unit's first use and released with the store
struct MoUnit {
  OutlierState outliers;
  void* clusters = nullptr; void (*release)(void*) = nullptr;
  ~MoUnit() { if (clusters) release(clusters); }
};
static_assert(offsetof(MoUnit, outliers) == 0, "OutlierState::lookup reads the slot as the outlier results");

}  // namespace

extern "C" void qn_outlier_default_params(qn_outlier_params* p) {
  if (!p) return;
  p->radius = 1.0; p->std_mul = 2.0; p->k = 8; p->reserved = 0;
}

extern "C" int qn_kf_map_outliers(qn_kf_store* s, const qn_outlier_params* params, qn_outlier_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !stats_out) return QN_ERR_INVALID_ARG;
  if (!std::isfinite(params->radius) || !(params->radius > 0.0) || !std::isfinite(params->std_mul) || !(params->std_mul >= 0.0) || params->k < 1 ||
      params->k > QN_OUTLIER_MAX_K || params->reserved != 0)
    return QN_ERR_INVALID_ARG;
  uint32_t n = 0; uint64_t gen = 0;
  const float4* map = qn_kf_int_map(s, &n, &gen);
  if (!map) return QN_ERR_NOT_READY;
  if (n >= MO_MAX_POINTS) {
    qn_kf_int_set_error(s, "qn_kf_map_outliers: 2^30 or more map points");
    return QN_ERR_CAPACITY;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  MoUnit* unit = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_OUTLIERS, &unit);
  if (rc != QN_OK) return rc;
  OutlierState* st = &unit->outliers;
  const uint32_t nb = (n + MO_BLOCK - 1) / MO_BLOCK;
  MoSet& o = st->spare();
  if (!o.count.grow(s, n) || !o.mean_q.grow(s, n) || !o.removed.grow(s, n) || !o.off.grow(s, (size_t)nb + 1)) return QN_ERR_HIP;
  qn_kf_int_cell_grid g;
  const float4* pts = nullptr; const unsigned long long* keys = nullptr;
  rc = qn_kf_int_cell_index(s, &map, &n, 1, params->radius, &g, &pts, &keys);       // sync 1 of 3
  if (rc != QN_OK) return rc;
  hipStream_t stream = qn_kf_int_stream(s);
  float4* d_spts = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)n);
  uint32_t* d_cells = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (size_t)n);
  unsigned long long* d_slots = (unsigned long long*)qn_kf_int_scratch(s, 3, sizeof(unsigned long long) * 3 * ((size_t)nb + 1));      // per block, then the sums
  uint32_t* d_blk = (uint32_t*)qn_kf_int_scratch(s, 4, sizeof(uint32_t) * (size_t)nb);
  char* h = (char*)qn_kf_int_pinned(s, 32);
  if (!d_spts || !d_cells || !d_slots || !d_blk || !h) return qn_kf_fail(s, "qn_kf_map_outliers: scratch allocation failed");
  unsigned long long* h_sum = (unsigned long long*)h; uint32_t* h_kept = (uint32_t*)(h + 24);
  const CellSeg seg = cell_seg(g);
  const double rr = params->radius * params->radius;
  const float r2 = (float)rr;
  const int e = qn_quant_exponent(params->radius, 16);     // mean_q <= 2^16 + 1: a u32, and its square summed over 2^30 points stays below 2^64
  const double scale = std::ldexp(1.0, e);
  const uint32_t k = params->k;
  const dim3 grid(nb);
  unsigned long long* d_sum = d_slots + 3 * (size_t)nb;
  hipLaunchKernelGGL(k_cell_gather, grid, dim3(MO_BLOCK), 0, stream, seg, keys, pts, d_spts, d_cells);
  if (k <= 8) hipLaunchKernelGGL(k_map_outliers<8>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  else if (k <= 16) hipLaunchKernelGGL(k_map_outliers<16>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  else hipLaunchKernelGGL(k_map_outliers<32>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  hipLaunchKernelGGL((k_slot_fold<unsigned long long, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, stream, (const unsigned long long*)d_slots, nb, d_sum);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_sum, d_sum, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 2 of 3: the statistics
  // ---- PCL's threshold on the quantised mean distances, f64, every operation rounded on its own
  qn_outlier_stats r;
  memset(&r, 0, sizeof(r));
  r.n = n; r.n_finite = g.n_finite; r.dense = (uint32_t)h_sum[0]; r.sparse = r.n_finite - r.dense; r.quant_exp = e;
  r.sum_q = h_sum[1]; r.sum_q2 = h_sum[2];
  if (r.dense) {
    const double N = (double)r.dense, sq = (double)r.sum_q, sq2 = (double)r.sum_q2;
    const double mean = sq / N;
    double var = r.dense > 1 ? (sq2 - sq * sq / N) / (double)(r.dense - 1) : 0.0;
    if (!(var > 0.0)) var = 0.0;
    r.mean_q = mean; r.std_q = std::sqrt(var); r.thr_q = mean + params->std_mul * r.std_q;
  }
  hipLaunchKernelGGL(k_mo_flag, grid, dim3(MO_BLOCK), 0, stream, n, map, (const uint32_t*)o.count.p, (const uint32_t*)o.mean_q.p, k, r.thr_q, o.removed.p, d_blk);
  hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(MO_SCAN_BLOCK), 0, stream, (const uint32_t*)d_blk, nb, o.off.p, o.off.p + nb);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_kept, o.off.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 3 of 3
  r.removed = n - *h_kept;
  o.kept = *h_kept;
  st->commit(gen, n);
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_outlier_points(qn_kf_store* s, uint32_t* count_out, uint32_t* mean_q_out, uint8_t* removed_out) {
  if (!s || (!count_out && !mean_q_out && !removed_out)) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const MoSet* o = OutlierState::lookup(s, QN_KF_INT_EXT_OUTLIERS, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (count_out) QN_KFCHK(s, hipMemcpyAsync(count_out, o->count.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (mean_q_out) QN_KFCHK(s, hipMemcpyAsync(mean_q_out, o->mean_q.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (removed_out) QN_KFCHK(s, hipMemcpyAsync(removed_out, o->removed.p, n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_remove_outliers(qn_kf_store* s, const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || !d_xyzi_out || !n_out) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const MoSet* o = OutlierState::lookup(s, QN_KF_INT_EXT_OUTLIERS, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  float4* d_kept = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)std::max<uint32_t>(o->kept, 1));
  if (!d_kept) return qn_kf_fail(s, "qn_kf_map_remove_outliers: scratch allocation failed");
  return qn_kf_map_compact_shrink(s, map, n, o->removed.p, o->off.p, d_kept, o->kept, d_xyzi_out, n_out);
}

#include "qn_mapclusters.inc"
