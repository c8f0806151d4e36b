// qn_freespace.hip - range images of resident keyframes and the free-space (see-through) check of loop pairs (qn_kf_range_*, qn_kf_freespace_*:
// include/qn_engine.h).  The numpy twin qn_amd/freespace.py is the specification.  Everything is f64 from the f32 records in a fixed order, with no fused
// multiply-add (the build's -ffp-contract=off), no transcendental on the device (row edges as tangents and column directions come in host tables; rows and
// columns are found by the twin's bisection over the twin's predicates, evaluated at the same indices) and the correctly rounded f64 sqrt - and every result
// is an integer or a min / max of f32 values, so images, classes and counts equal the twin's bit for bit whatever the interleaving.
// Kernels:
//   k_range_clear      describe: the listed keyframes' images to +inf (near) and 0 (far);
//   k_range_bin        one thread per record, the keyframe a grid dimension: projects the record and merges float(r) into the keyframe's global images with
//                      atomicMin / atomicMax on its bit pattern (order-preserving for non-negative floats); the kept points of each keyframe are counted;
//   k_freespace_check  one thread per record, (pair, direction) a grid dimension: transform, projection, the window's gathers, the class byte; the block's
//                      counts by ballots and popcounts into its own slot;
//   k_freespace_reduce one block per (pair, direction) over its blocks' slots in a fixed order.
// The projection, the column table's staging, the window gather and the class rule live in qn_range.cuh (shared with qn_staticmap.hip).
// The column table (16 bytes per column) is staged in LDS when it fits 64 KiB (up to 4096 columns); above that the bisection reads it from global memory (14
// reads per point, L2 resident), because a 128 KiB stage would leave one block per CU.  The row table is read from global memory: the bisection's index differs
// from lane to lane, so a scalar load cannot serve it.
// Host synchronisations: one per call (describe: the kept counts; check: the records).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_range.cuh"

namespace {
using namespace qn_range;      // fs_stage / fs_project / fs_classify, RangeState: shared with qn_staticmap.hip

#define FS_NCOUNT 5                                     // per block and per direction: finite, unobserved, seen through, occluded, agree

struct RgKf { const float4* pts; uint32_t n; int32_t id; };
struct FsSeg { const float4* pts; uint32_t n, p0, b0; int32_t img; double M[12]; };
struct FsCnt { uint32_t c[FS_NCOUNT]; };

// grid (pixel tiles, keyframes)
__global__ void __launch_bounds__(256) k_range_clear(const RgKf* __restrict__ kfs, uint32_t npix, uint32_t* __restrict__ img) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= npix) return;
  uint32_t* near = img + (size_t)kfs[blockIdx.y].id * 2 * npix;
  near[t] = FS_INF_BITS;
  near[npix + t] = 0u;
}

// grid (tiles of the largest keyframe of the launch, keyframes), dynamic LDS: the column table (LDS) or nothing
template <bool LDS>
__global__ void __launch_bounds__(FS_BLOCK) k_range_bin(const RgKf* __restrict__ kfs, const double* __restrict__ trow, const double2* __restrict__ cs, uint32_t nr, uint32_t nc,
                                                        double min_range, uint32_t* __restrict__ img, uint32_t* __restrict__ kept) {
  const RgKf kf = kfs[blockIdx.y];
  const uint32_t base = blockIdx.x * FS_TILE;
  if (base >= kf.n) return;                                          // uniform over the block
  const double2* ct = fs_stage<LDS>(cs, nc);
  const uint32_t npix = nr * nc;
  uint32_t* near = img + (size_t)kf.id * 2 * npix;
  uint32_t* far = near + npix;
  uint32_t mine = 0;
#pragma unroll 1
  for (uint32_t it = 0; it < FS_ITERS; it++) {
    const uint32_t i = base + it * FS_BLOCK + threadIdx.x;
    if (i >= kf.n) break;
    const float4 p = kf.pts[i];
    const double x = p.x, y = p.y, z = p.z;
    if (!__builtin_isfinite(x) || !__builtin_isfinite(y) || !__builtin_isfinite(z)) continue;
    uint32_t row, col; double r;
    if (!fs_project(x, y, z, trow, nr, ct, nc, min_range, row, col, r)) continue;
    const uint32_t bits = __float_as_uint((float)r);
    const uint32_t pix = row * nc + col;
    atomicMin(&near[pix], bits);
    atomicMax(&far[pix], bits);
    mine++;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&kept[blockIdx.y], mine);
}

// grid (tiles of the largest cloud of the call, 2 * pairs): segment 2 j = pair j's query records through T against the candidate's images, 2 j + 1 the reverse
template <bool LDS>
__global__ void __launch_bounds__(FS_BLOCK) k_freespace_check(const FsSeg* __restrict__ segs, const double* __restrict__ trow, const double2* __restrict__ cs, uint32_t nr,
                                                              uint32_t nc, double min_range, int wr, int wc, double tol_abs, double tol_rel,
                                                              const uint32_t* __restrict__ img, uint8_t* __restrict__ classes, FsCnt* __restrict__ slots) {
  __shared__ uint32_t wcnt[FS_WAVES][FS_NCOUNT];
  const FsSeg* S = &segs[blockIdx.y];
  const uint32_t n = S->n;
  const uint32_t base = blockIdx.x * FS_TILE;
  if (base >= n) return;                                             // uniform over the block
  const double2* ct = fs_stage<LDS>(cs, nc);
  const float4* pts = S->pts;
  const uint32_t npix = nr * nc;
  const uint32_t* near = img + (size_t)S->img * 2 * npix;
  const uint32_t* far = near + npix;
  uint8_t* out = classes + S->p0;
  const double m0 = S->M[0], m1 = S->M[1], m2 = S->M[2], m3 = S->M[3], m4 = S->M[4], m5 = S->M[5], m6 = S->M[6], m7 = S->M[7], m8 = S->M[8], m9 = S->M[9],
               m10 = S->M[10], m11 = S->M[11];
  uint32_t cf = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;                    // the wave's counts (the same in every lane)
#pragma unroll 1
  for (uint32_t it = 0; it < FS_ITERS; it++) {
    const uint32_t i = base + it * FS_BLOCK + threadIdx.x;
    uint32_t cls = 0; bool fin = false;
    if (i < n) {
      const float4 p = pts[i];
      const double x = p.x, y = p.y, z = p.z;
      const double px = ((m0 * x + m1 * y) + m2 * z) + m3;
      const double py = ((m4 * x + m5 * y) + m6 * z) + m7;
      const double pz = ((m8 * x + m9 * y) + m10 * z) + m11;
      cls = fs_classify(px, py, pz, trow, nr, ct, nc, min_range, wr, wc, tol_abs, tol_rel, near, far, fin);
      out[i] = (uint8_t)cls;
    }
    cf += __popcll(__ballot(fin));
    c1 += __popcll(__ballot(cls == 1u)); c2 += __popcll(__ballot(cls == 2u)); c3 += __popcll(__ballot(cls == 3u)); c4 += __popcll(__ballot(cls == 4u));
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wcnt[wave][0] = cf; wcnt[wave][1] = c1; wcnt[wave][2] = c2; wcnt[wave][3] = c3; wcnt[wave][4] = c4; }
  __syncthreads();
  if (threadIdx.x < FS_NCOUNT) {
    uint32_t acc = 0;
    for (int w = 0; w < FS_WAVES; w++) acc += wcnt[w][threadIdx.x];
    slots[S->b0 + blockIdx.x].c[threadIdx.x] = acc;
  }
}

// one block per (pair, direction): thread i sums slots i, i + 256, ..., then a butterfly inside each wave and the waves in order
__global__ void __launch_bounds__(256) k_freespace_reduce(const FsSeg* __restrict__ segs, const FsCnt* __restrict__ slots, FsCnt* __restrict__ res) {
  __shared__ uint32_t ws[4][FS_NCOUNT];
  const uint32_t n = segs[blockIdx.x].n, b0 = segs[blockIdx.x].b0;
  const uint32_t nb = (n + FS_TILE - 1) / FS_TILE;
  uint32_t acc[FS_NCOUNT] = {0, 0, 0, 0, 0};
  for (uint32_t b = threadIdx.x; b < nb; b += 256) {
    const FsCnt s = slots[b0 + b];
#pragma unroll
    for (int k = 0; k < FS_NCOUNT; k++) acc[k] += s.c[k];
  }
#pragma unroll
  for (int k = 0; k < FS_NCOUNT; k++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < FS_NCOUNT; k++) ws[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FsCnt r;
#pragma unroll
    for (int k = 0; k < FS_NCOUNT; k++) r.c[k] = ws[0][k] + ws[1][k] + ws[2][k] + ws[3][k];
    res[blockIdx.x] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define RG_DESCRIBE_CHUNK 32768u                         // keyframes per describe launch (the grid's y dimension)
const uint32_t kMaxPairs = 32767;                        // (pair, direction) is the grid's y dimension

qn_range_params range_default_params() {
  qn_range_params p{};
  p.n_rows = 64; p.n_cols = 1800; p.el_lo = -25.0 * M_PI / 180.0; p.el_hi = 2.2 * M_PI / 180.0; p.min_range = 2.0;
  p.window_rows = 1; p.window_cols = 1; p.tol_abs = 0.3; p.tol_rel = 0.02;
  return p;
}
bool range_params_ok(const qn_range_params& p) {
  return p.n_rows >= 1 && p.n_rows <= QN_RANGE_MAX_ROWS && p.n_cols >= 1 && p.n_cols <= QN_RANGE_MAX_COLS && std::isfinite(p.el_lo) && std::isfinite(p.el_hi) &&
         p.el_lo > -0.5 * M_PI && p.el_lo < p.el_hi && p.el_hi < 0.5 * M_PI && std::isfinite(p.min_range) && p.min_range >= 0.0 && std::isfinite(p.tol_abs) &&
         p.tol_abs >= 0.0 && std::isfinite(p.tol_rel) && p.tol_rel >= 0.0 && p.window_rows < p.n_rows && p.window_cols <= (QN_RANGE_MAX_COLS >> 1) &&
         2 * p.window_cols + 1 <= p.n_cols;
}
// the host tables (freespace.tables): row edges as tangents and the column boundary directions, from the C library.  The angles go through volatiles so that
// tan, cos and sin are the library calls the twin makes.
std::vector<double> range_tables(const qn_range_params& p) {
  const uint32_t nr = p.n_rows, nc = p.n_cols;
  const size_t off = range_cs_offset(nr);
  std::vector<double> t(off + 2 * (size_t)nc, 0.0);
  for (uint32_t i = 0; i <= nr; i++) {
    volatile double a = p.el_lo + (double)i * (p.el_hi - p.el_lo) / (double)nr;
    t[i] = std::tan((double)a);
  }
  for (uint32_t j = 0; j < nc; j++) {
    volatile double a = 2.0 * M_PI * j / nc;
    t[off + 2 * (size_t)j] = std::cos((double)a);
    volatile double b = a;
    t[off + 2 * (size_t)j + 1] = std::sin((double)b);
  }
  return t;
}
int range_state(qn_kf_store* s, RangeState** out) {
  return qn_kf_ext_state(s, QN_KF_INT_EXT_RANGE, out, [s](RangeState* st) -> int {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    st->p = range_default_params();
    const std::vector<double> t = range_tables(st->p);
    return st->tab.assign(s, t.data(), t.size()) ? QN_OK : QN_ERR_HIP;
  });
}
// image slots for every keyframe id < n (contents of existing slots kept)
int range_reserve(qn_kf_store* s, RangeState* st, size_t n) {
  if (n <= st->cap) return QN_OK;
  const size_t cap = std::max<size_t>({n, st->cap + st->cap / 2, 16});
  if (!st->img.grow_keep(s, 2 * (size_t)st->p.n_rows * st->p.n_cols * cap, qn_kf_int_stream(s))) return QN_ERR_HIP;
  st->cap = cap;
  return QN_OK;
}

}  // namespace

extern "C" int qn_kf_range_set_params(qn_kf_store* s, const qn_range_params* p) {
  if (!s || !p || !range_params_ok(*p)) return QN_ERR_INVALID_ARG;
  RangeState* st = nullptr;
  const int rc = range_state(s, &st);
  if (rc != QN_OK) return rc;
  const qn_range_params& o = st->p;
  const bool same_images = o.n_rows == p->n_rows && o.n_cols == p->n_cols && o.el_lo == p->el_lo && o.el_hi == p->el_hi && o.min_range == p->min_range;
  if (same_images) { st->p = *p; return QN_OK; }            // the images do not depend on the window or the tolerances
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  QN_KFCHK(s, hipStreamSynchronize(qn_kf_int_stream(s)));   // no launch of this store may still read the old images
  st->img.reset(); st->cap = 0;
  st->described.assign(st->described.size(), 0);
  st->p = *p;
  const std::vector<double> t = range_tables(st->p);
  return st->tab.assign(s, t.data(), t.size()) ? QN_OK : QN_ERR_HIP;
}
extern "C" int qn_kf_range_get_params(qn_kf_store* s, qn_range_params* p) {
  if (!s || !p) return QN_ERR_INVALID_ARG;
  RangeState* st = nullptr;
  const int rc = range_state(s, &st);
  if (rc != QN_OK) return rc;
  *p = st->p;
  return QN_OK;
}

extern "C" int qn_kf_range_describe(qn_kf_store* s, const int32_t* ids, uint32_t count, int* status) {
  if (!s || !ids || count == 0 || !status) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t k = 0; k < count; k++) if (ids[k] < 0 || (size_t)ids[k] >= n_kf) return QN_ERR_INVALID_ARG;
  RangeState* st = nullptr;
  int rc = range_state(s, &st);
  if (rc != QN_OK) return rc;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  // each listed keyframe once (an id listed twice gets the same image either way)
  std::vector<int32_t> slot_of(n_kf, -1);
  std::vector<RgKf> todo;
  for (uint32_t k = 0; k < count; k++) {
    const int32_t id = ids[k];
    if (slot_of[id] >= 0) continue;
    slot_of[id] = (int32_t)todo.size();
    uint32_t n = 0;
    const float4* pts = qn_kf_int_keyframe(s, id, &n);
    todo.push_back(RgKf{pts, n, id});
  }
  rc = range_reserve(s, st, n_kf);
  if (rc != QN_OK) return rc;
  if (st->described.size() < n_kf) st->described.resize(n_kf, 0);
  const uint32_t nr = st->p.n_rows, nc = st->p.n_cols, npix = nr * nc;
  const size_t m_all = todo.size();
  RgKf* d_kfs = (RgKf*)qn_kf_int_scratch(s, 0, sizeof(RgKf) * m_all);
  uint32_t* d_cnt = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * m_all);
  uint32_t* h_cnt = (uint32_t*)qn_kf_int_pinned(s, sizeof(uint32_t) * m_all);
  if (!d_kfs || !d_cnt || !h_cnt) return qn_kf_fail(s, "qn_kf_range_describe: scratch allocation failed");
  const hipStream_t str = qn_kf_int_stream(s);
  QN_KFCHK(s, hipMemcpyAsync(d_kfs, todo.data(), sizeof(RgKf) * m_all, hipMemcpyHostToDevice, str));
  QN_KFCHK(s, hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * m_all, str));
  const double* trow = st->tab.p;
  const double2* cs = (const double2*)(st->tab.p + range_cs_offset(nr));
  const size_t lds = range_lds_bytes(st);
  for (size_t a = 0; a < m_all; a += RG_DESCRIBE_CHUNK) {
    const uint32_t m = (uint32_t)std::min<size_t>(RG_DESCRIBE_CHUNK, m_all - a);
    uint32_t nmax = 0;
    for (uint32_t k = 0; k < m; k++) nmax = std::max(nmax, todo[a + k].n);
    hipLaunchKernelGGL(k_range_clear, dim3((npix + 255) / 256, m), dim3(256), 0, str, (const RgKf*)(d_kfs + a), npix, st->img.p);
    if (!nmax) continue;
    const dim3 grid((nmax + FS_TILE - 1) / FS_TILE, m);
    if (lds) hipLaunchKernelGGL(k_range_bin<true>, grid, dim3(FS_BLOCK), lds, str, (const RgKf*)(d_kfs + a), trow, cs, nr, nc, st->p.min_range, st->img.p, d_cnt + a);
    else hipLaunchKernelGGL(k_range_bin<false>, grid, dim3(FS_BLOCK), 0, str, (const RgKf*)(d_kfs + a), trow, cs, nr, nc, st->p.min_range, st->img.p, d_cnt + a);
  }
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_cnt, d_cnt, sizeof(uint32_t) * m_all, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));                   // the one synchronisation: the kept counts, and the scratch may be reused
  for (const RgKf& k : todo) st->described[k.id] = 1;
  for (uint32_t k = 0; k < count; k++) status[k] = h_cnt[slot_of[ids[k]]] ? QN_OK : QN_ERR_EMPTY_CLOUD;
  return QN_OK;
}

extern "C" int qn_kf_range_get(qn_kf_store* s, int32_t id, float* near_out, float* far_out) {
  if (!s || id < 0 || (size_t)id >= qn_kf_int_count(s) || (!near_out && !far_out)) return QN_ERR_INVALID_ARG;
  RangeState* st = (RangeState*)qn_kf_int_ext(s, QN_KF_INT_EXT_RANGE);
  if (!st || (size_t)id >= st->described.size() || !st->described[id]) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  const size_t npix = (size_t)st->p.n_rows * st->p.n_cols;
  const uint32_t* base = st->img.p + (size_t)id * 2 * npix;
  if (near_out) QN_KFCHK(s, hipMemcpyAsync(near_out, base, sizeof(float) * npix, hipMemcpyDeviceToHost, str));
  if (far_out) QN_KFCHK(s, hipMemcpyAsync(far_out, base + npix, sizeof(float) * npix, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_freespace_batch(qn_kf_store* s, const int32_t* query, const int32_t* cand, const double* T16, uint32_t n_pairs, qn_freespace* out, int* status) {
  // ---- every argument is checked before anything runs
  if (!s || !query || !cand || !T16 || n_pairs == 0 || !out || !status) return QN_ERR_INVALID_ARG;
  if (n_pairs > kMaxPairs) return QN_ERR_CAPACITY;
  const size_t n_kf = qn_kf_int_count(s);
  RangeState* st = (RangeState*)qn_kf_int_ext(s, QN_KF_INT_EXT_RANGE);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const int32_t q = query[j], c = cand[j];
    if (q < 0 || (size_t)q >= n_kf || c < 0 || (size_t)c >= n_kf || q == c) return QN_ERR_INVALID_ARG;
    if (!st || (size_t)std::max(q, c) >= st->described.size() || !st->described[q] || !st->described[c]) return QN_ERR_INVALID_ARG;
    for (int k = 0; k < 16; k++) if (!std::isfinite(T16[16 * (size_t)j + k])) return QN_ERR_INVALID_ARG;
  }
  const uint32_t S = 2 * n_pairs;
  std::vector<FsSlot> slots(n_pairs);
  uint64_t total = 0, blocks = 0; uint32_t nmax = 0;
  std::vector<uint32_t> b0(S);
  for (uint32_t j = 0; j < n_pairs; j++)
    for (int d = 0; d < 2; d++) {
      uint32_t n = 0;
      (void)qn_kf_int_keyframe(s, d == 0 ? query[j] : cand[j], &n);
      slots[j].p0[d] = (uint32_t)total; slots[j].n[d] = n; b0[2 * j + d] = (uint32_t)blocks;
      total += n; blocks += (n + FS_TILE - 1) / FS_TILE; nmax = std::max(nmax, n);
      if (total > 0xFFFFFFFFull) return QN_ERR_CAPACITY;
    }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  const size_t seg_bytes = qn_up16(sizeof(FsSeg) * S), res_bytes = sizeof(FsCnt) * S;
  FsSeg* d_seg = (FsSeg*)qn_kf_int_scratch(s, 0, seg_bytes);
  FsCnt* d_slots = (FsCnt*)qn_kf_int_scratch(s, 1, sizeof(FsCnt) * std::max<uint64_t>(blocks, 1));
  FsCnt* d_res = (FsCnt*)qn_kf_int_scratch(s, 2, res_bytes);
  char* h = (char*)qn_kf_int_pinned(s, seg_bytes + res_bytes);
  if (!d_seg || !d_slots || !d_res || !h) return qn_kf_fail(s, "qn_kf_freespace_batch: scratch allocation failed");
  st->live = false;                                         // from here on the previous check is gone
  if (!st->cls.grow(s, total)) return QN_ERR_HIP;
  FsSeg* h_seg = (FsSeg*)h; FsCnt* h_res = (FsCnt*)(h + seg_bytes);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const double* T = T16 + 16 * (size_t)j;
    double inv[12];                                         // [R^T | -R^T t], each -R^T t entry summed over k = 0 .. 2 in order (scancontext.relative_pose)
    for (int r = 0; r < 3; r++) {
      double acc = 0.0;
      for (int k = 0; k < 3; k++) { inv[4 * r + k] = T[4 * k + r]; acc = acc + T[4 * k + r] * T[4 * k + 3]; }
      inv[4 * r + 3] = -acc;
    }
    for (int d = 0; d < 2; d++) {
      FsSeg& g = h_seg[2 * j + d];
      uint32_t n = 0;
      g.pts = qn_kf_int_keyframe(s, d == 0 ? query[j] : cand[j], &n);
      g.n = n; g.p0 = slots[j].p0[d]; g.b0 = b0[2 * j + d]; g.img = d == 0 ? cand[j] : query[j];
      memcpy(g.M, d == 0 ? T : inv, sizeof(double) * 12);
    }
  }
  QN_KFCHK(s, hipMemcpyAsync(d_seg, h_seg, sizeof(FsSeg) * S, hipMemcpyHostToDevice, str));
  const qn_range_params& p = st->p;
  const double* trow = st->tab.p;
  const double2* cs = (const double2*)(st->tab.p + range_cs_offset(p.n_rows));
  const size_t lds = range_lds_bytes(st);
  if (nmax) {
    const dim3 grid((nmax + FS_TILE - 1) / FS_TILE, S);
    if (lds) hipLaunchKernelGGL(k_freespace_check<true>, grid, dim3(FS_BLOCK), lds, str, (const FsSeg*)d_seg, trow, cs, p.n_rows, p.n_cols, p.min_range, (int)p.window_rows,
                                (int)p.window_cols, p.tol_abs, p.tol_rel, (const uint32_t*)st->img.p, st->cls.p, d_slots);
    else hipLaunchKernelGGL(k_freespace_check<false>, grid, dim3(FS_BLOCK), 0, str, (const FsSeg*)d_seg, trow, cs, p.n_rows, p.n_cols, p.min_range, (int)p.window_rows,
                            (int)p.window_cols, p.tol_abs, p.tol_rel, (const uint32_t*)st->img.p, st->cls.p, d_slots);
  }
  hipLaunchKernelGGL(k_freespace_reduce, dim3(S), dim3(256), 0, str, (const FsSeg*)d_seg, (const FsCnt*)d_slots, d_res);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_res, d_res, res_bytes, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));                   // the one synchronisation of the call
  for (uint32_t j = 0; j < n_pairs; j++) {
    qn_freespace_dir* d[2] = {&out[j].q_in_c, &out[j].c_in_q};
    for (int k = 0; k < 2; k++) {
      const uint32_t* c = h_res[2 * j + k].c;
      d[k]->n = slots[j].n[k]; d[k]->n_finite = c[0]; d[k]->in_fov = c[1] + c[2] + c[3] + c[4]; d[k]->observed = c[2] + c[3] + c[4];
      d[k]->seen_through = c[2]; d[k]->occluded = c[3]; d[k]->agree = c[4]; d[k]->reserved = 0;
    }
    status[j] = (slots[j].n[0] == 0 || slots[j].n[1] == 0) ? QN_ERR_EMPTY_CLOUD : QN_OK;
  }
  st->slots.swap(slots);
  st->live = true;
  return QN_OK;
}

extern "C" int qn_kf_freespace_points(qn_kf_store* s, uint32_t pair_slot, int dir, uint8_t* class_out) {
  if (!s || (dir != 0 && dir != 1) || !class_out) return QN_ERR_INVALID_ARG;
  RangeState* st = (RangeState*)qn_kf_int_ext(s, QN_KF_INT_EXT_RANGE);
  if (!st || !st->live) return QN_ERR_NOT_READY;
  if (pair_slot >= st->slots.size()) return QN_ERR_INVALID_ARG;
  const FsSlot& o = st->slots[pair_slot];
  if (o.n[dir] == 0) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  QN_KFCHK(s, hipMemcpyAsync(class_out, st->cls.p + o.p0[dir], o.n[dir], hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}
