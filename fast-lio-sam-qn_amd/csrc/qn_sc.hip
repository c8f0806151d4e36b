// qn_sc.hip - Scan Context place descriptors of resident keyframes and loop candidates by descriptor distance (qn_kf_sc_*).
// The numpy twin qn_amd/scancontext.py is the specification; include/qn_engine.h pins the definition.  Everything is f64 from the f32
// records in a fixed order, with no fused multiply-add (the build's -ffp-contract=off), no transcendental on the device (ring edges and
// sector directions come in host tables, sectors are decided by half plane and cross-product sign tests), IEEE division and the correctly
// rounded f64 sqrt - so descriptors, keys, distances, shifts and the order of the result equal the twin's bit for bit.
// Kernels:
//   k_sc_bin     describe: one pass over the records of many keyframes per launch; each block takes the bin maxima of a tile of one
//                keyframe with atomicMax on the order-preserving uint32 encoding of the value in LDS, then merges them into the keyframe's
//                global bins with atomicMax (a max is order-independent, so the result is exact whatever the interleaving).
//   k_sc_finish  decodes the bins into the store's descriptor slot of the keyframe, ring keys (one thread per ring) and column sums of
//                squares / norms (one thread per sector).
//   k_sc_ringkey prefilter: squared ring-key distance of each (query, keyframe), inadmissible ones get the sentinel key.
//   k_sc_dist    one wave per (query, candidate): the candidate's descriptor staged in LDS, one lane per shift sums its columns in order,
//                the wave's minimum (lowest shift on ties) becomes the candidate's 64-bit order key.
//   k_sc_select  one block per query: the K smallest (key, id) by radix select (8 key digits, 4 id digits), then a rank sort.
//   k_sc_gather  writes the chunk's (id, D, shift) rows into the call's result buffer.
// Queries are processed in chunks whose scratch stays under SC_SCRATCH_BYTES, all on the store's stream: one host synchronisation per call.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"

namespace qn {

#define SC_BIN_BLOCK 256
#define SC_BIN_TILE (SC_BIN_BLOCK * 16)                 // records per block of k_sc_bin
#define SC_DIST_ITERS 4                                 // candidates per wave of a k_sc_dist block
#define SC_SEL_BLOCK 256
#define SC_SENTINEL 0xFFFFFFFFFFFFFFFFull               // key of an inadmissible slot: above every finite double's order key
static_assert(QN_SC_MAX_TOP_K <= 1024 && QN_SC_MAX_PREFILTER <= 1024, "k_sc_select stages at most 1024 entries in LDS");
#define SC_SEL_MAX 1024

struct ScKf { const float4* pts; uint32_t n; int32_t id; };

__device__ __forceinline__ uint32_t sc_ord32(float v) {           // unsigned order of the result = float order; 0 is below every float
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float sc_unord32(uint32_t k) {         // 0 (no point in the bin) -> 0.0f
  if (k == 0u) return 0.0f;
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ unsigned long long sc_ord64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}
__device__ __forceinline__ double sc_unord64(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// grid (tiles of the largest keyframe of the launch, keyframes), dynamic LDS nr * ns * 4 bytes.  tab = edges2 [nr + 1], cos [ns], sin [ns].
__global__ void __launch_bounds__(SC_BIN_BLOCK) k_sc_bin(const ScKf* __restrict__ kfs, const double* __restrict__ tab, uint32_t nr, uint32_t ns,
                                                        double lidar_height, uint32_t* __restrict__ gbins) {
  extern __shared__ __align__(16) uint32_t sc_lb[];
  const ScKf kf = kfs[blockIdx.y];
  const uint32_t base = blockIdx.x * SC_BIN_TILE;
  if (base >= kf.n) return;                                        // uniform over the block
  const uint32_t nb = nr * ns;
  for (uint32_t t = threadIdx.x; t < nb; t += SC_BIN_BLOCK) sc_lb[t] = 0u;
  __syncthreads();
  const double* e = tab;
  const double* cs = tab + nr + 1;
  const double* sn = cs + ns;
  const double r2max = e[nr];
  const uint32_t end = min(kf.n, base + SC_BIN_TILE);
  for (uint32_t i = base + threadIdx.x; i < end; i += SC_BIN_BLOCK) {
    const float4 p = kf.pts[i];
    const double x = p.x, y = p.y, z = p.z;
    if (!__builtin_isfinite(x) || !__builtin_isfinite(y) || !__builtin_isfinite(z)) continue;
    if (x == 0.0 && y == 0.0) continue;
    const double r2 = x * x + y * y;
    if (!(r2 < r2max)) continue;
    uint32_t ring = 0;
    for (uint32_t k = 1; k < nr; k++) ring += r2 >= e[k] ? 1u : 0u;
    const int hp = (y > 0.0 || (y == 0.0 && x > 0.0)) ? 0 : 1;
    uint32_t sec = 0;
    for (uint32_t j = 1; j < ns; j++) {
      const double c = cs[j], s = sn[j];
      const int hb = (s > 0.0 || (s == 0.0 && c > 0.0)) ? 0 : 1;
      const double cr = c * y - s * x;
      sec += (hp > hb || (hp == hb && cr >= 0.0)) ? 1u : 0u;
    }
    atomicMax(&sc_lb[ring * ns + sec], sc_ord32((float)(z + lidar_height)));
  }
  __syncthreads();
  uint32_t* g = gbins + (size_t)blockIdx.y * nb;
  for (uint32_t t = threadIdx.x; t < nb; t += SC_BIN_BLOCK) {
    const uint32_t v = sc_lb[t];
    if (v) atomicMax(&g[t], v);
  }
}

// one block per described keyframe of the launch: descriptor, ring key, column sums of squares and norms into the store's slot kfs[b].id
__global__ void __launch_bounds__(SC_BIN_BLOCK) k_sc_finish(const ScKf* __restrict__ kfs, const uint32_t* __restrict__ gbins, uint32_t nr, uint32_t ns,
                                                           float* __restrict__ desc, double* __restrict__ rk, double* __restrict__ cn, double* __restrict__ ss) {
  const size_t nb = (size_t)nr * ns;
  const uint32_t* g = gbins + blockIdx.x * nb;
  const size_t id = (size_t)kfs[blockIdx.x].id;
  float* d = desc + id * nb;
  for (uint32_t t = threadIdx.x; t < nb; t += SC_BIN_BLOCK) d[t] = sc_unord32(g[t]);
  for (uint32_t i = threadIdx.x; i < nr; i += SC_BIN_BLOCK) {
    double acc = 0.0;
    for (uint32_t j = 0; j < ns; j++) acc = acc + (double)sc_unord32(g[i * ns + j]);
    rk[id * nr + i] = acc / (double)ns;
  }
  for (uint32_t j = threadIdx.x; j < ns; j += SC_BIN_BLOCK) {
    double acc = 0.0;
    for (uint32_t i = 0; i < nr; i++) { const double v = (double)sc_unord32(g[i * ns + j]); acc = acc + v * v; }
    ss[id * ns + j] = acc;
    cn[id * ns + j] = __builtin_sqrt(acc);
  }
}

__device__ __forceinline__ bool sc_admissible(int32_t q, int32_t c, const double* __restrict__ stamps, const uint8_t* __restrict__ valid, double tdiff) {
  return c != q && valid[c] && stamps[q] - stamps[c] > tdiff;          // loop_closure.cpp:45, strict
}

// grid (keyframes / 256, queries of the chunk): keys[row * n + c] = order key of sum over i of (rk_q[i] - rk_c[i])^2, or the sentinel
__global__ void __launch_bounds__(256) k_sc_ringkey(const double* __restrict__ rk, uint32_t nr, const int32_t* __restrict__ qids, const double* __restrict__ stamps,
                                                   const uint8_t* __restrict__ valid, double tdiff, uint32_t n, unsigned long long* __restrict__ keys) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (c >= n) return;
  const int32_t q = qids[row];
  unsigned long long key = SC_SENTINEL;
  if (sc_admissible(q, (int32_t)c, stamps, valid, tdiff)) {
    double acc = 0.0;
    for (uint32_t i = 0; i < nr; i++) { const double d = rk[(size_t)q * nr + i] - rk[(size_t)c * nr + i]; acc = acc + d * d; }
    key = sc_ord64(acc);
  }
  keys[(size_t)row * n + c] = key;
}

// grid (ceil(m / (waves * SC_DIST_ITERS)), queries of the chunk), block 64 * waves, dynamic LDS waves * stage bytes.  Slot t of row `row` is
// candidate list[row * m + t] (t < list_n[row]) or, without a list, candidate t itself.  keys / shifts [row * m + t].
__global__ void __launch_bounds__(256) k_sc_dist(const float* __restrict__ desc, const double* __restrict__ ss, uint32_t nr, uint32_t ns,
                                                const int32_t* __restrict__ qids, const double* __restrict__ stamps, const uint8_t* __restrict__ valid, double tdiff,
                                                const int32_t* __restrict__ list, const uint32_t* __restrict__ list_n, uint32_t m, uint32_t stage_bytes,
                                                unsigned long long* __restrict__ keys, int32_t* __restrict__ shifts) {
  extern __shared__ __align__(16) unsigned char sc_smem[];
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = blockIdx.y;
  double* css = (double*)(sc_smem + (size_t)wave * stage_bytes);  // the candidate's column sums of squares [ns], then its descriptor [nr * ns]
  float* cd = (float*)(css + ns);
  const uint32_t nb = nr * ns;
  const int32_t q = qids[row];
  const float* qd = desc + (size_t)q * nb;
  const double* qss = ss + (size_t)q * ns;
  for (uint32_t it = 0; it < SC_DIST_ITERS; it++) {
    const uint32_t slot = (blockIdx.x * SC_DIST_ITERS + it) * waves + wave;
    int32_t c = -1;
    if (slot < m) c = list ? (slot < list_n[row] ? list[(size_t)row * m + slot] : -1) : (int32_t)slot;
    const bool ok = c >= 0 && sc_admissible(q, c, stamps, valid, tdiff);          // uniform over the wave
    if (ok) {
      const float* src = desc + (size_t)c * nb;
      for (uint32_t t = lane; t < nb; t += 64) cd[t] = src[t];
      for (uint32_t t = lane; t < ns; t += 64) css[t] = ss[(size_t)c * ns + t];
    }
    __syncthreads();
    if (ok) {
      double best = INFINITY;
      uint32_t best_s = 0xFFFFFFFFu;
      for (uint32_t s = lane; s < ns; s += 64) {
        double sum = 0.0;
        uint32_t cnt = 0, k = s;                                     // k = (j + s) mod ns
        for (uint32_t j = 0; j < ns; j++) {
          const double a = qss[j], b = css[k];
          if (a != 0.0 && b != 0.0) {
            double dot = 0.0;
            for (uint32_t i = 0; i < nr; i++) dot = dot + (double)qd[i * ns + j] * (double)cd[i * ns + k];
            sum = sum + (1.0 - dot / __builtin_sqrt(a * b));
            cnt++;
          }
          k = (k + 1 == ns) ? 0u : k + 1;
        }
        const double D = cnt ? sum / (double)cnt : 1.0;
        if (D < best) { best = D; best_s = s; }
      }
      for (int off = 32; off >= 1; off >>= 1) {                       // the wave's minimum, the lowest shift on ties
        const double ob = __shfl_xor(best, off, 64);
        const uint32_t os = (uint32_t)__shfl_xor((int)best_s, off, 64);
        if (ob < best || (ob == best && os < best_s)) { best = ob; best_s = os; }
      }
      if (lane == 0) { keys[(size_t)row * m + slot] = sc_ord64(best); shifts[(size_t)row * m + slot] = (int32_t)best_s; }
    } else if (slot < m && lane == 0) {
      keys[(size_t)row * m + slot] = SC_SENTINEL;
    }
    __syncthreads();
  }
}

// one block per row: the want = min(k, #admissible) smallest (keys[row * m + t], id of t) - id = ids[row * m + t] or t - as slots t in
// ascending order into out[row * k ..], want into out_n[row].  Composite keys are distinct (ids are distinct within a row).
__global__ void __launch_bounds__(SC_SEL_BLOCK) k_sc_select(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ ids, uint32_t m, uint32_t k,
                                                           int32_t* __restrict__ out, uint32_t* __restrict__ out_n) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_cnt, s_bin, s_rank;
  __shared__ unsigned long long ck[SC_SEL_MAX];
  __shared__ uint32_t cid[SC_SEL_MAX];
  __shared__ int32_t cslot[SC_SEL_MAX];
  const uint32_t row = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* kr = keys + (size_t)row * m;
  const int32_t* ir = ids ? ids + (size_t)row * m : nullptr;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t t = tid; t < m; t += SC_SEL_BLOCK) mine += kr[t] != SC_SENTINEL ? 1u : 0u;
  atomicAdd(&s_cnt, mine);
  __syncthreads();
  const uint32_t want = min(k, s_cnt);
  if (want == 0) { if (tid == 0) out_n[row] = 0; return; }
  // radix select of the want-th smallest key (8-bit digits from the top), then of the id among the entries with that key
  unsigned long long kp = 0, km = 0;
  uint32_t ip = 0, im = 0, rank = want;
  for (int pass = 0; pass < 12; pass++) {
    const bool on_key = pass < 8;
    const int sh = on_key ? 56 - 8 * pass : 24 - 8 * (pass - 8);
    for (uint32_t t = tid; t < 256; t += SC_SEL_BLOCK) hist[t] = 0;
    __syncthreads();
    for (uint32_t t = tid; t < m; t += SC_SEL_BLOCK) {
      const unsigned long long key = kr[t];
      if (on_key) {
        if ((key & km) == kp) atomicAdd(&hist[(uint32_t)(key >> sh) & 255u], 1u);
      } else if (key == kp) {
        const uint32_t id = ir ? (uint32_t)ir[t] : t;
        if ((id & im) == ip) atomicAdd(&hist[(id >> sh) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0, b = 0;
      for (; b < 255u; b++) {
        if (cum + hist[b] >= rank) break;
        cum += hist[b];
      }
      s_bin = b; s_rank = rank - cum;
    }
    __syncthreads();
    const uint32_t b = s_bin;
    rank = s_rank;
    if (on_key) { kp |= (unsigned long long)b << sh; km |= 255ull << sh; }
    else { ip |= b << sh; im |= 255u << sh; }
    __syncthreads();                                                  // hist is cleared again by the next pass
  }
  // the want entries at or below (kp, ip), in any order, then ranked
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (uint32_t t = tid; t < m; t += SC_SEL_BLOCK) {
    const unsigned long long key = kr[t];
    const uint32_t id = ir ? (uint32_t)ir[t] : t;
    if (key < kp || (key == kp && id <= ip)) {
      const uint32_t pos = atomicAdd(&s_cnt, 1u);
      if (pos < SC_SEL_MAX) { ck[pos] = key; cid[pos] = id; cslot[pos] = (int32_t)t; }
    }
  }
  __syncthreads();
  const uint32_t got = min(s_cnt, want);
  for (uint32_t e = tid; e < got; e += SC_SEL_BLOCK) {
    const unsigned long long ke = ck[e];
    const uint32_t ie = cid[e];
    uint32_t r = 0;
    for (uint32_t f = 0; f < got; f++) r += (ck[f] < ke || (ck[f] == ke && cid[f] < ie)) ? 1u : 0u;
    out[(size_t)row * k + r] = cslot[e];
  }
  if (tid == 0) out_n[row] = got;
}

// thread per (row, rank): the chunk's result rows (id, D, shift) into the call's result buffers at row0
__global__ void k_sc_gather(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ shifts, const int32_t* __restrict__ list, uint32_t m,
                            const int32_t* __restrict__ sel, const uint32_t* __restrict__ sel_n, uint32_t rows, uint32_t k, uint32_t row0,
                            int32_t* __restrict__ ids_out, double* __restrict__ d_out, int32_t* __restrict__ sh_out, uint32_t* __restrict__ n_out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * k) return;
  const uint32_t row = t / k, r = t - row * k;
  const size_t o = (size_t)(row0 + row) * k + r;
  if (r == 0) n_out[row0 + row] = sel_n[row];
  if (r < sel_n[row]) {
    const uint32_t slot = (uint32_t)sel[(size_t)row * k + r];
    ids_out[o] = list ? list[(size_t)row * m + slot] : (int32_t)slot;
    d_out[o] = sc_unord64(keys[(size_t)row * m + slot]);
    sh_out[o] = shifts[(size_t)row * m + slot];
  } else {
    ids_out[o] = -1; d_out[o] = __longlong_as_double(0x7FF8000000000000ll); sh_out[o] = -1;
  }
}

}  // namespace qn
// ---------------------------------------------------------------------------------------------------------------- host side
#define SC_SCRATCH_BYTES (256ull << 20)                    // per-chunk scratch of a query call
#define SC_DESCRIBE_CHUNK 8192u                            // keyframes per describe launch (bins: <= 32 KB each)

// The store's Scan Context state: parameters, host tables on the device, and descriptor slots indexed by keyframe id (grown with the store).
struct ScState {
  qn_sc_params p{};
  DevBuf<double> tab;                                      // edges2 [nr + 1], cos [ns], sin [ns]
  DevBuf<float> desc; DevBuf<double> rk, cn, ss;           // per keyframe id: n_rings * n_sectors, n_rings, n_sectors, n_sectors
  size_t cap = 0;                                          // keyframe slots of the four
  std::vector<uint8_t> described;                          // per keyframe id, under the current parameters
};

static qn_sc_params sc_default_params() {
  qn_sc_params p{};
  p.n_rings = 20; p.n_sectors = 60; p.max_radius = 80.0; p.lidar_height = 2.0; p.ringkey_prefilter = 0;
  return p;
}
static bool sc_params_ok(const qn_sc_params& p) {
  return p.n_rings >= 1 && p.n_rings <= QN_SC_MAX_RINGS && p.n_sectors >= 1 && p.n_sectors <= QN_SC_MAX_SECTORS &&
         p.n_rings * p.n_sectors <= QN_SC_MAX_BINS && std::isfinite(p.max_radius) && p.max_radius > 0.0 && p.max_radius <= 1e6 &&
         std::isfinite(p.lidar_height) && std::fabs(p.lidar_height) <= 1e4 && p.ringkey_prefilter <= QN_SC_MAX_PREFILTER;
}
// the host tables (scancontext.tables): ring edges squared, and cos / sin of the sector boundaries from the C library.  The angle goes through
// a volatile so that cos and sin are the two library calls the twin makes (not a fused sincos).
static std::vector<double> sc_tables(const qn_sc_params& p) {
  const uint32_t nr = p.n_rings, ns = p.n_sectors;
  std::vector<double> t(nr + 1 + 2 * (size_t)ns);
  for (uint32_t i = 0; i < nr; i++) { const double r = (double)i * p.max_radius / nr; t[i] = r * r; }
  t[nr] = p.max_radius * p.max_radius;
  for (uint32_t j = 0; j < ns; j++) {
    volatile double a = 2.0 * M_PI * j / ns;
    t[nr + 1 + j] = std::cos((double)a);
    volatile double b = a;
    t[nr + 1 + ns + j] = std::sin((double)b);
  }
  return t;
}

static int sc_state(qn_kf_store* s, ScState** out) {
  return qn_kf_ext_state(s, QN_KF_INT_EXT_SC, out, [s](ScState* st) -> int {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    st->p = sc_default_params();
    const std::vector<double> t = sc_tables(st->p);
    return st->tab.assign(s, t.data(), t.size()) ? QN_OK : QN_ERR_HIP;
  });
}
// descriptor slots for every keyframe id < n (contents of existing slots kept).  All four arrays move or none: exact-size temporaries take the copies
// behind one synchronisation and are swapped in at the end; an early return frees them and leaves the old slots.
static int sc_reserve(qn_kf_store* s, ScState* st, size_t n) {
  if (n <= st->cap) return QN_OK;
  const size_t cap = std::max<size_t>({n, 2 * st->cap, 64});
  const size_t nr = st->p.n_rings, ns = st->p.n_sectors;
  DevBuf<float> d; DevBuf<double> r, c, q;
  if (!d.grow(s, nr * ns * cap, true) || !r.grow(s, nr * cap, true) || !c.grow(s, ns * cap, true) || !q.grow(s, ns * cap, true)) return QN_ERR_HIP;
  if (st->cap) {
    const hipStream_t str = qn_kf_int_stream(s);
    QN_KFCHK(s, hipMemcpyAsync(d.p, st->desc.p, sizeof(float) * st->desc.cap, hipMemcpyDeviceToDevice, str));
    QN_KFCHK(s, hipMemcpyAsync(r.p, st->rk.p, sizeof(double) * st->rk.cap, hipMemcpyDeviceToDevice, str));
    QN_KFCHK(s, hipMemcpyAsync(c.p, st->cn.p, sizeof(double) * st->cn.cap, hipMemcpyDeviceToDevice, str));
    QN_KFCHK(s, hipMemcpyAsync(q.p, st->ss.p, sizeof(double) * st->ss.cap, hipMemcpyDeviceToDevice, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                  // the old slots may go
  }
  st->desc.swap(d); st->rk.swap(r); st->cn.swap(c); st->ss.swap(q); st->cap = cap;      // (the old slots go with d, r, c, q)
  return QN_OK;
}

extern "C" int qn_kf_sc_set_params(qn_kf_store* s, const qn_sc_params* p) {
  if (!s || !p || !sc_params_ok(*p)) return QN_ERR_INVALID_ARG;
  ScState* st = nullptr;
  int rc = sc_state(s, &st);
  if (rc != QN_OK) return rc;
  const qn_sc_params& o = st->p;
  const bool same_shape = o.n_rings == p->n_rings && o.n_sectors == p->n_sectors && o.max_radius == p->max_radius && o.lidar_height == p->lidar_height;
  if (same_shape) { st->p.ringkey_prefilter = p->ringkey_prefilter; return QN_OK; }   // the descriptors do not depend on the prefilter
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  QN_KFCHK(s, hipStreamSynchronize(qn_kf_int_stream(s)));   // no launch of this store may still read the old slots
  st->desc.reset(); st->rk.reset(); st->cn.reset(); st->ss.reset(); st->cap = 0;
  st->described.assign(st->described.size(), 0);
  st->p = *p; st->p.pad_ = 0;
  const std::vector<double> t = sc_tables(st->p);
  return st->tab.assign(s, t.data(), t.size()) ? QN_OK : QN_ERR_HIP;
}
extern "C" int qn_kf_sc_get_params(qn_kf_store* s, qn_sc_params* p) {
  if (!s || !p) return QN_ERR_INVALID_ARG;
  ScState* st = nullptr;
  const int rc = sc_state(s, &st);
  if (rc != QN_OK) return rc;
  *p = st->p;
  return QN_OK;
}

extern "C" int qn_kf_sc_describe(qn_kf_store* s, const int32_t* ids, uint32_t count) {
  if (!s || !ids || count == 0) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t k = 0; k < count; k++) if (ids[k] < 0 || (size_t)ids[k] >= n_kf) return QN_ERR_INVALID_ARG;
  ScState* st = nullptr;
  int rc = sc_state(s, &st);
  if (rc != QN_OK) return rc;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  if (st->described.size() < n_kf) st->described.resize(n_kf, 0);
  // the ids not described yet, each once (describing again would write the same bits)
  std::vector<uint8_t> seen(n_kf, 0);
  std::vector<qn::ScKf> todo;
  for (uint32_t k = 0; k < count; k++) {
    const int32_t id = ids[k];
    if (st->described[id] || seen[id]) continue;
    seen[id] = 1;
    uint32_t n = 0;
    const float4* pts = qn_kf_int_keyframe(s, id, &n);
    todo.push_back(qn::ScKf{pts, n, id});
  }
  if (todo.empty()) return QN_OK;
  rc = sc_reserve(s, st, n_kf);
  if (rc != QN_OK) return rc;
  const uint32_t nr = st->p.n_rings, ns = st->p.n_sectors, nb = nr * ns;
  const uint32_t chunk = std::min<uint32_t>((uint32_t)todo.size(), SC_DESCRIBE_CHUNK);
  qn::ScKf* d_kfs = (qn::ScKf*)qn_kf_int_scratch(s, 0, sizeof(qn::ScKf) * todo.size());
  uint32_t* d_bins = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)nb * chunk);
  if (!d_kfs || !d_bins) { qn_kf_int_set_error(s, "qn_kf_sc_describe: scratch allocation failed"); return QN_ERR_HIP; }
  const hipStream_t str = qn_kf_int_stream(s);
  QN_KFCHK(s, hipMemcpyAsync(d_kfs, todo.data(), sizeof(qn::ScKf) * todo.size(), hipMemcpyHostToDevice, str));
  for (size_t a = 0; a < todo.size(); a += chunk) {
    const uint32_t m = (uint32_t)std::min<size_t>(chunk, todo.size() - a);
    uint32_t nmax = 0;
    for (uint32_t k = 0; k < m; k++) nmax = std::max(nmax, todo[a + k].n);
    QN_KFCHK(s, hipMemsetAsync(d_bins, 0, sizeof(uint32_t) * (size_t)nb * m, str));
    if (nmax)
      hipLaunchKernelGGL(qn::k_sc_bin, dim3((nmax + SC_BIN_TILE - 1) / SC_BIN_TILE, m), dim3(SC_BIN_BLOCK), sizeof(uint32_t) * nb, str,
                         (const qn::ScKf*)(d_kfs + a), (const double*)st->tab.p, nr, ns, st->p.lidar_height, d_bins);
    hipLaunchKernelGGL(qn::k_sc_finish, dim3(m), dim3(SC_BIN_BLOCK), 0, str, (const qn::ScKf*)(d_kfs + a), (const uint32_t*)d_bins, nr, ns,
                       st->desc.p, st->rk.p, st->cn.p, st->ss.p);
  }
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipStreamSynchronize(str));                   // the one synchronisation: the scratch (host table) may be reused
  for (const qn::ScKf& k : todo) st->described[k.id] = 1;
  return QN_OK;
}

extern "C" int qn_kf_sc_get(qn_kf_store* s, int32_t id, float* desc, double* ringkey, double* colnorm) {
  if (!s || id < 0 || (size_t)id >= qn_kf_int_count(s)) return QN_ERR_INVALID_ARG;
  ScState* st = (ScState*)qn_kf_int_ext(s, QN_KF_INT_EXT_SC);
  if (!st || (size_t)id >= st->described.size() || !st->described[id]) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  const size_t nr = st->p.n_rings, ns = st->p.n_sectors;
  if (desc) QN_KFCHK(s, hipMemcpyAsync(desc, st->desc.p + (size_t)id * nr * ns, sizeof(float) * nr * ns, hipMemcpyDeviceToHost, str));
  if (ringkey) QN_KFCHK(s, hipMemcpyAsync(ringkey, st->rk.p + (size_t)id * nr, sizeof(double) * nr, hipMemcpyDeviceToHost, str));
  if (colnorm) QN_KFCHK(s, hipMemcpyAsync(colnorm, st->cn.p + (size_t)id * ns, sizeof(double) * ns, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_sc_query(qn_kf_store* s, const int32_t* query_ids, uint32_t nq, const double* stamps, uint32_t n_stamps, double tdiff, uint32_t top_k,
                              int32_t* ids_out, double* dist_out, int32_t* shift_out, uint32_t* n_out) {
  // ---- every argument is checked before anything runs
  if (!s || !query_ids || nq == 0 || !stamps || !ids_out || !dist_out || !shift_out || !n_out) return QN_ERR_INVALID_ARG;
  if (std::isnan(tdiff) || top_k == 0 || top_k > QN_SC_MAX_TOP_K || (uint64_t)nq * top_k > QN_SC_MAX_RESULTS) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  if (n_stamps < n_kf) return QN_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < nq; k++) if (query_ids[k] < 0 || (size_t)query_ids[k] >= n_kf) return QN_ERR_INVALID_ARG;
  ScState* st = (ScState*)qn_kf_int_ext(s, QN_KF_INT_EXT_SC);
  for (uint32_t k = 0; k < nq; k++)
    if (!st || (size_t)query_ids[k] >= st->described.size() || !st->described[query_ids[k]]) return QN_ERR_NOT_READY;

  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  const uint32_t N = (uint32_t)n_kf, nr = st->p.n_rings, ns = st->p.n_sectors, P = st->p.ringkey_prefilter, K = top_k;
  const bool pre = P > 0;
  const uint32_t M = pre ? P : N;                          // slots of the distance stage per query
  // per-query scratch: the distance stage's keys and shifts, and with the prefilter its ring-key keys over all N and the list of P
  const size_t per_q = (size_t)M * 12 + (pre ? (size_t)N * 8 + (size_t)P * 4 + 4 : 0) + (size_t)K * 4 + 4;
  const uint32_t qc = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)nq, SC_SCRATCH_BYTES / per_q, 65535}));
  // inputs: query ids, stamps, described flags (one upload)
  const size_t in_bytes = sizeof(double) * N + sizeof(int32_t) * nq + N + 16;
  char* d_in = (char*)qn_kf_int_scratch(s, 0, in_bytes);
  unsigned long long* d_keys = (unsigned long long*)qn_kf_int_scratch(s, 1, sizeof(unsigned long long) * (size_t)qc * M);
  int32_t* d_shift = (int32_t*)qn_kf_int_scratch(s, 2, sizeof(int32_t) * (size_t)qc * M);
  unsigned long long* d_rkeys = pre ? (unsigned long long*)qn_kf_int_scratch(s, 3, sizeof(unsigned long long) * (size_t)qc * N) : nullptr;
  int32_t* d_list = pre ? (int32_t*)qn_kf_int_scratch(s, 4, sizeof(int32_t) * ((size_t)qc * P + qc)) : nullptr;
  int32_t* d_sel = (int32_t*)qn_kf_int_scratch(s, 5, sizeof(int32_t) * ((size_t)qc * K + qc));
  const size_t res_bytes = (sizeof(int32_t) * 2 + sizeof(double)) * (size_t)nq * K + sizeof(uint32_t) * nq;
  char* d_res = (char*)qn_kf_int_scratch(s, 6, res_bytes);
  char* h_res = (char*)qn_kf_int_pinned(s, res_bytes);
  if (!d_in || !d_keys || !d_shift || (pre && (!d_rkeys || !d_list)) || !d_sel || !d_res || !h_res) {
    qn_kf_int_set_error(s, "qn_kf_sc_query: scratch allocation failed"); return QN_ERR_HIP;
  }
  std::vector<char> h_in(in_bytes, 0);
  memcpy(h_in.data(), stamps, sizeof(double) * N);
  memcpy(h_in.data() + sizeof(double) * N, query_ids, sizeof(int32_t) * nq);
  for (uint32_t c = 0; c < N; c++) h_in[sizeof(double) * N + sizeof(int32_t) * nq + c] = c < st->described.size() ? (char)st->described[c] : 0;
  QN_KFCHK(s, hipMemcpyAsync(d_in, h_in.data(), in_bytes, hipMemcpyHostToDevice, str));
  const double* d_stamps = (const double*)d_in;
  const int32_t* d_q = (const int32_t*)(d_in + sizeof(double) * N);
  const uint8_t* d_valid = (const uint8_t*)(d_in + sizeof(double) * N + sizeof(int32_t) * nq);
  double* r_d = (double*)d_res;
  int32_t* r_ids = (int32_t*)(r_d + (size_t)nq * K);
  int32_t* r_sh = r_ids + (size_t)nq * K;
  uint32_t* r_n = (uint32_t*)(r_sh + (size_t)nq * K);
  // k_sc_dist: waves per block from the LDS stage of one candidate (column sums of squares, then the descriptor), 16-byte aligned
  const uint32_t stage = (uint32_t)qn_up16(sizeof(double) * ns + sizeof(float) * nr * ns);
  const uint32_t waves = std::max<uint32_t>(1, std::min<uint32_t>(4, (64u << 10) / stage));
  const uint32_t per_block = waves * SC_DIST_ITERS;
  for (uint32_t a = 0; a < nq; a += qc) {
    const uint32_t rows = std::min(qc, nq - a);
    const int32_t* qids = d_q + a;
    const int32_t* list = nullptr;
    const uint32_t* list_n = nullptr;
    if (pre) {
      hipLaunchKernelGGL(qn::k_sc_ringkey, dim3((N + 255) / 256, rows), dim3(256), 0, str, (const double*)st->rk.p, nr, qids, d_stamps, d_valid, tdiff, N, d_rkeys);
      uint32_t* ln = (uint32_t*)(d_list + (size_t)qc * P);
      hipLaunchKernelGGL(qn::k_sc_select, dim3(rows), dim3(SC_SEL_BLOCK), 0, str, (const unsigned long long*)d_rkeys, (const int32_t*)nullptr, N, P, d_list, ln);
      list = d_list; list_n = ln;
    }
    hipLaunchKernelGGL(qn::k_sc_dist, dim3((M + per_block - 1) / per_block, rows), dim3(64 * waves), (size_t)waves * stage, str,
                       (const float*)st->desc.p, (const double*)st->ss.p, nr, ns, qids, d_stamps, d_valid, tdiff, list, list_n, M, stage, d_keys, d_shift);
    uint32_t* sel_n = (uint32_t*)(d_sel + (size_t)qc * K);
    hipLaunchKernelGGL(qn::k_sc_select, dim3(rows), dim3(SC_SEL_BLOCK), 0, str, (const unsigned long long*)d_keys, list, M, K, d_sel, sel_n);
    hipLaunchKernelGGL(qn::k_sc_gather, dim3((rows * K + 255) / 256), dim3(256), 0, str, (const unsigned long long*)d_keys, (const int32_t*)d_shift, list, M,
                       (const int32_t*)d_sel, (const uint32_t*)sel_n, rows, K, a, r_ids, r_d, r_sh, r_n);
  }
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_res, d_res, res_bytes, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));                   // the one synchronisation of the call
  const size_t nk = (size_t)nq * K;
  memcpy(dist_out, h_res, sizeof(double) * nk);
  memcpy(ids_out, h_res + sizeof(double) * nk, sizeof(int32_t) * nk);
  memcpy(shift_out, h_res + (sizeof(double) + sizeof(int32_t)) * nk, sizeof(int32_t) * nk);
  memcpy(n_out, h_res + (sizeof(double) + 2 * sizeof(int32_t)) * nk, sizeof(uint32_t) * nq);
  return QN_OK;
}
