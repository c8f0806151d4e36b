// qn_mapoutliers.hip - the isolated noise points of the store's map slot, found and removed on the GPU (qn_kf_map_outliers, qn_kf_map_outlier_points,
// qn_kf_map_remove_outliers: include/qn_engine.h).  The numpy twin qn_amd/mapoutliers.py is the specification: the neighbours of a finite map point are the
// finite map points at another index within r of it by the oracle's f32 sqdist3 (<= float(r * r), inclusive); with fewer than k of them the point is sparse and
// an outlier outright (PCL's RadiusOutlierRemoval with min_neighbors = k); otherwise the mean of its k smallest distances, quantised to an integer of 2^-e m,
// enters PCL's StatisticalOutlierRemoval threshold mean + std_mul * stddev over all dense points.  count and mean_q are integers and the statistics are integer
// sums, so everything equals the twin's bit for bit whatever order the neighbours are met in; the f64 arithmetic behind mean_q is the same IEEE operations in
// the same order (the library is built without contraction, the roots are made correctly rounded below).
//   index     qn_kf_int_cell_index (qn_cloud.hip) over the map as one cloud, as qn_mapnormals.hip uses it; k_mo_gather lays the sorted points (original index
//             in .w) and their cell words out flat.
//   select    k_map_outliers<L>, one point per lane, 256 lanes a block, in the sorted order, the nine-x-run walk of k_map_normals (one resumed binary search
//             per run, candidates four a trip).  The L smallest d2 live in L registers as u32 bit patterns (d2 >= 0: the f32 order is the u32 order), sorted
//             ascending by a fully unrolled, statically indexed compare-exchange chain that is entered only when d2 < the current L-th; L is 8, 16 or 32, k
//             rounded up (the k smallest are the first k of the L smallest).  No dynamically indexed private array, so no scratch.  The k f64 roots and their
//             sum run once per point after the scan.  dense, sum_q and sum_q2 are reduced over the wave by shuffles, over the block through LDS, and stored
//             into the block's own slot; k_mo_reduce adds the slots up.  No atomics.
//   flag      k_mo_flag, one point per lane in the map's own order: removed = sparse or double(mean_q) > thr_q; the block's kept count into its slot;
//             k_mo_scan (one block) turns the counts into offsets, the last one the number kept.
//   compact   k_mo_scan and k_mo_compact live in qn_map_compact.cuh, shared with qn_mapground.hip.  k_mo_compact (qn_kf_map_remove_outliers only): the kept
//             records of a block to its offset, in order, by ballot / popcount ranks and the waves' counts through LDS - the static map's scheme: stable and the same on every run.  The records go to scratch and from there to the front of the
//             map slot (qn_kf_int_map_shrink), which advances the slot's generation.
// Host synchronisations of a classify: the index's, one for the statistics (the threshold is host arithmetic), one at the end.  Results are written into the
// spare one of two buffer sets and the sets are swapped on success, so a refused call leaves the previous classification as it was.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_map_compact.cuh"

namespace {

#define MO_MAX_POINTS (1u << 30)
#define MO_NO_MEAN 0xffffffffu

struct MoSeg { uint32_t n, nfin, prefix; float inv; float minb[3]; int div[3]; };

// the sorted order laid out flat (k_mn_gather's layout): sorted point t with its original index (bits in .w), and its cell word
__global__ void __launch_bounds__(MO_BLOCK) k_mo_gather(uint32_t n, const unsigned long long* __restrict__ keys, const float4* __restrict__ pts,
                                                        float4* __restrict__ spts, uint32_t* __restrict__ cells) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (t >= n) return;
  const unsigned long long key = keys[t];
  const uint32_t src = (uint32_t)key;
  const float4 p = pts[src];
  spts[t] = make_float4(p.x, p.y, p.z, __uint_as_float(src));
  cells[t] = (uint32_t)(key >> 32);
}

__device__ __forceinline__ int mo_cell_coord(float x, float inv, float minb, int div) {
  // k_batch_keys' expression (the query is a point of the indexed cloud: the clamp never binds, it only keeps the conversion defined)
  const float c = floorf(x * inv) - minb;
  return (int)fminf(fmaxf(c, -2.0f), (float)div + 1.0f);
}

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

__device__ __forceinline__ unsigned long long mo_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                              // (lane 0 holds the wave's sum)
}

template <int L>
__global__ void __launch_bounds__(MO_BLOCK) k_map_outliers(const MoSeg S, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, float r2, double scale,
                                                           uint32_t k, uint32_t* __restrict__ count, uint32_t* __restrict__ mean_q,
                                                           unsigned long long* __restrict__ slots) {
  __shared__ unsigned long long ws[3][MO_WAVES];
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool act = t < S.n;                              // (no early return: every thread of the block meets the barrier of the reduction)
  const bool fin = t < S.nfin;
  const float4 q = act ? spts[t] : make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t qi = __float_as_uint(q.w);
  uint32_t cnt = 0;
  uint32_t key[L];                                       // the L smallest d2 so far, ascending; only ever indexed by unrolled loop counters
#pragma unroll
  for (int j = 0; j < L; j++) key[j] = 0xffffffffu;
  if (fin) {
    const int cx = mo_cell_coord(q.x, S.inv, S.minb[0], S.div[0]), cy = mo_cell_coord(q.y, S.inv, S.minb[1], S.div[1]), cz = mo_cell_coord(q.z, S.inv, S.minb[2], S.div[2]);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, S.div[0] - 1);
    if (x0 <= x1) {
      uint32_t lo = 0;
      const uint32_t end = S.nfin;
      for (int dz = -1; dz <= 1; dz++) {
        const int z = cz + dz;
        if ((unsigned)z >= (unsigned)S.div[2]) continue;
        for (int dy = -1; dy <= 1; dy++) {
          const int y = cy + dy;
          if ((unsigned)y >= (unsigned)S.div[1]) continue;
          const uint32_t k0 = S.prefix | (uint32_t)(x0 + (y + z * S.div[1]) * S.div[0]), k1 = k0 + (uint32_t)(x1 - x0);
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
              if (more && a + j != t) {                  // another index than the query's: a duplicate of it elsewhere counts
                const float dx = q.x - p[j].x, dy2 = q.y - p[j].y, dz2 = q.z - p[j].z;
                const float d2 = dx * dx + dy2 * dy2 + dz2 * dz2;
                if (d2 <= r2) {
                  cnt++;
                  uint32_t v = __float_as_uint(d2);
                  if (v < key[L - 1]) {
#pragma unroll
                    for (int i = 0; i < L; i++) { const uint32_t lo_ = min(key[i], v); v = max(key[i], v); key[i] = lo_; }
                  }
                }
              }
            }
            if (!more) break;
            a += 4;
          }
          lo = a;
        }
      }
    }
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
  const unsigned long long r0 = mo_wave_sum(dense ? 1ull : 0ull), r1 = mo_wave_sum(m64), r2s = mo_wave_sum(m64 * m64);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = r0; ws[1][threadIdx.x >> 6] = r1; ws[2][threadIdx.x >> 6] = r2s; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long acc = 0;
    for (int w = 0; w < MO_WAVES; w++) acc += ws[threadIdx.x][w];
    slots[3 * (size_t)blockIdx.x + threadIdx.x] = acc;
  }
}

// one block: out[0 .. 3) = the sums of the nb blocks' slots
__global__ void __launch_bounds__(MO_SCAN_BLOCK) k_mo_reduce(const unsigned long long* __restrict__ slots, uint32_t nb, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long ws[3][MO_SCAN_BLOCK / 64];
  unsigned long long a0 = 0, a1 = 0, a2 = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += MO_SCAN_BLOCK) { a0 += slots[3 * (size_t)b]; a1 += slots[3 * (size_t)b + 1]; a2 += slots[3 * (size_t)b + 2]; }
  a0 = mo_wave_sum(a0); a1 = mo_wave_sum(a1); a2 = mo_wave_sum(a2);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = a0; ws[1][threadIdx.x >> 6] = a1; ws[2][threadIdx.x >> 6] = a2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long acc = 0;
    for (int w = 0; w < MO_SCAN_BLOCK / 64; w++) acc += ws[threadIdx.x][w];
    out[threadIdx.x] = acc;
  }
}

// one point per lane in the map's own order: the removed byte, and the block's kept records into its slot
__global__ void __launch_bounds__(MO_BLOCK) k_mo_flag(uint32_t n, const float4* __restrict__ map, const uint32_t* __restrict__ count, const uint32_t* __restrict__ mean_q,
                                                      uint32_t k, double thr, uint8_t* __restrict__ removed, uint32_t* __restrict__ blk_kept) {
  __shared__ uint32_t wk[MO_WAVES];
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const float4 p = map[i];
    const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    const bool rm = fin && (count[i] < k || (double)mean_q[i] > thr);
    removed[i] = rm ? 1 : 0;
    keep = !rm;
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(keep));
  if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int w = 0; w < MO_WAVES; w++) acc += wk[w];
    blk_kept[blockIdx.x] = acc;
  }
}

// The store's outlier state (slot QN_KF_INT_EXT_OUTLIERS): two sets of per-point buffers, the live one holding the classification of the latest successful
// call, for the map of generation `gen` with its n points of which `kept` stay; a call writes the other set and swaps on success.
struct MoSet { DevBuf<uint32_t> count, mean_q, off; DevBuf<uint8_t> removed; };
struct OutlierState {
  bool live = false; uint64_t gen = 0; uint32_t n = 0, kept = 0; int cur = 0;
  MoSet set[2];
};

// the live classification if it is that of the map slot as it stands, else nullptr
OutlierState* live_state(qn_kf_store* s, const float4** map) {
  OutlierState* st = (OutlierState*)qn_kf_int_ext(s, QN_KF_INT_EXT_OUTLIERS);
  uint32_t map_n = 0; uint64_t gen = 0;
  *map = qn_kf_int_map(s, &map_n, &gen);
  if (!st || !st->live || !*map || st->gen != gen || st->n != map_n) return nullptr;
  return st;
}

// the largest e with r 2^e <= 2^16, within the exponents of normal f32 powers of two (mapoutliers.quant_exponent)
int quant_exponent(double r) {
  int x = 0;
  const double m = std::frexp(r, &x);                    // r = m 2^x, 0.5 <= m < 1
  const int e = m == 0.5 ? 17 - x : 16 - x;
  return e < -126 ? -126 : e > 127 ? 127 : e;
}

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
  OutlierState* st = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_OUTLIERS, &st);
  if (rc != QN_OK) return rc;
  const uint32_t nb = (n + MO_BLOCK - 1) / MO_BLOCK;
  MoSet& o = st->set[st->live ? 1 - st->cur : st->cur];
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
  MoSeg seg;
  seg.n = g.n; seg.nfin = g.n_finite; seg.prefix = g.prefix; seg.inv = g.inv;
  for (int a = 0; a < 3; a++) { seg.minb[a] = (float)g.minb[a]; seg.div[a] = g.div[a]; }
  const double rr = params->radius * params->radius;
  const float r2 = (float)rr;
  const int e = quant_exponent(params->radius);
  const double scale = std::ldexp(1.0, e);
  const uint32_t k = params->k;
  const dim3 grid(nb);
  unsigned long long* d_sum = d_slots + 3 * (size_t)nb;
  hipLaunchKernelGGL(k_mo_gather, grid, dim3(MO_BLOCK), 0, stream, n, keys, pts, d_spts, d_cells);
  if (k <= 8) hipLaunchKernelGGL(k_map_outliers<8>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  else if (k <= 16) hipLaunchKernelGGL(k_map_outliers<16>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  else hipLaunchKernelGGL(k_map_outliers<32>, grid, dim3(MO_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, k, o.count.p, o.mean_q.p, d_slots);
  hipLaunchKernelGGL(k_mo_reduce, dim3(1), dim3(MO_SCAN_BLOCK), 0, stream, (const unsigned long long*)d_slots, nb, d_sum);
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
  hipLaunchKernelGGL(k_mo_scan, dim3(1), dim3(MO_SCAN_BLOCK), 0, stream, (const uint32_t*)d_blk, nb, o.off.p);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_kept, o.off.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 3 of 3
  r.removed = n - *h_kept;
  if (st->live) st->cur = 1 - st->cur;
  st->live = true; st->gen = gen; st->n = n; st->kept = *h_kept;
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_outlier_points(qn_kf_store* s, uint32_t* count_out, uint32_t* mean_q_out, uint8_t* removed_out) {
  if (!s || (!count_out && !mean_q_out && !removed_out)) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr;
  const OutlierState* st = live_state(s, &map);
  if (!st) return QN_ERR_NOT_READY;
  const MoSet& o = st->set[st->cur];
  const size_t n = st->n;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (count_out) QN_KFCHK(s, hipMemcpyAsync(count_out, o.count.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
  if (mean_q_out) QN_KFCHK(s, hipMemcpyAsync(mean_q_out, o.mean_q.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
  if (removed_out) QN_KFCHK(s, hipMemcpyAsync(removed_out, o.removed.p, n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_remove_outliers(qn_kf_store* s, const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || !d_xyzi_out || !n_out) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr;
  OutlierState* st = live_state(s, &map);
  if (!st) return QN_ERR_NOT_READY;
  const MoSet& o = st->set[st->cur];
  const uint32_t n = st->n, kept = st->kept;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  float4* d_kept = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)std::max<uint32_t>(kept, 1));
  if (!d_kept) return qn_kf_fail(s, "qn_kf_map_remove_outliers: scratch allocation failed");
  hipLaunchKernelGGL(k_mo_compact, dim3((n + MO_BLOCK - 1) / MO_BLOCK), dim3(MO_BLOCK), 0, stream, n, map, (const uint8_t*)o.removed.p, (const uint32_t*)o.off.p, d_kept);
  QN_KFCHK(s, hipGetLastError());
  // from here on the slot changes: its generation advances, so this classification and any map normals are stale
  const int rc = qn_kf_int_map_shrink(s, d_kept, kept);
  if (rc != QN_OK) return rc;
  QN_KFCHK(s, hipStreamSynchronize(stream));
  uint32_t m = 0; uint64_t gen = 0;
  *d_xyzi_out = (const float*)qn_kf_int_map(s, &m, &gen); *n_out = m;
  return QN_OK;
}
