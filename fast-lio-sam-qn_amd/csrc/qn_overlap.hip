// qn_overlap.hip - the two-way overlap of cloud pairs on the GPU (qn_kf_overlap_batch, qn_kf_verify_overlap, qn_kf_overlap_points: include/qn_engine.h).
// For clouds A and B in one frame and a radius r: every point's exact nearest neighbour in the other cloud when it lies within r (f32 squared distance
// <= float(r * r), the oracle's sqdist3 arithmetic, ties to the lowest index), and per direction the number of such points and the f64 sum of their squared
// distances.  The numpy twin qn_amd/overlap.py is the specification; the results equal it bit for bit.
//   index   qn_kf_int_cell_index (qn_cloud.hip): the front half of the store's voxel-grid pipeline with every cloud a segment - boxes, cell keys, stable
//           radix passes - gives each cloud sorted by cell (edge >= r, x fastest), and k_overlap_gather lays the sorted points and their cells out flat;
//   search  k_overlap_search, one query per lane, the pair and direction a grid dimension, the walk of qn_cell_walk.cuh (the exactness argument at cell
//           borders is there) over the other cloud.  Queries are walked in the sorted order of their OWN cloud: neighbouring lanes are neighbouring points,
//           and since both grids have cells of about r they read the same or adjacent runs of the other cloud (sorting the queries a second time by the
//           other cloud's grid would buy the same locality for one more sort per cloud).  A minimum that is <= float(r * r) is found among the 27 cells,
//           and so is every point that ties with it; a minimum above it is reported as no partner;
//   reduce  k_overlap_reduce, one block per pair and direction over the per-point results in original point order: a fixed order, no atomics, so a rerun
//           gives the same bits and a pair's sums do not depend on which other pairs share the call.
// Host synchronisations per call: two, whatever the number of pairs (the boxes; the records).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include <algorithm>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_cell_walk.cuh"

namespace {

#define QN_OV_BLOCK 256                                  // k_overlap_reduce's block
struct OvRes { double sum; uint32_t inliers, pad; };

// qn_cell_walk.cuh's gather, the pair and direction a grid dimension
__global__ void __launch_bounds__(QN_CW_BLOCK) k_overlap_gather(const CellSeg* __restrict__ segs, const unsigned long long* __restrict__ keys, const float4* __restrict__ pts,
                                                                 float4* __restrict__ spts, uint32_t* __restrict__ cells) {
  cell_gather(segs[blockIdx.y], keys, pts, spts, cells);
}

// one query per lane: the nearest candidate of the walk, ties to the lowest original index
__global__ void __launch_bounds__(QN_CW_BLOCK) k_overlap_search(const CellSeg* __restrict__ segs, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, float r2,
                                                                 float* __restrict__ nn_d2, int32_t* __restrict__ nn_idx) {
  const CellSeg Q = segs[blockIdx.y];
  const uint32_t t = blockIdx.x * QN_CW_BLOCK + threadIdx.x;
  if (t >= Q.n) return;
  const CellSeg T = segs[blockIdx.y ^ 1u];
  const float4 q = spts[Q.p0 + t];
  const uint32_t qi = __float_as_uint(q.w);
  float best = INFINITY; uint32_t bi = 0xffffffffu;
  if (t < Q.nfin && T.nfin) {
    cell_walk(T, spts, cells, q, [&](uint32_t, const float4& p, float d2) {
      const uint32_t id = __float_as_uint(p.w);
      if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; }
    });
  }
  if (!(best <= r2)) { best = INFINITY; bi = 0xffffffffu; }
  nn_d2[Q.p0 + qi] = best;
  nn_idx[Q.p0 + qi] = (int32_t)bi;
}

// one block per pair and direction: thread i sums points i, i + 256, ... in f64, then a butterfly inside each wave and the waves in order
__global__ void __launch_bounds__(QN_OV_BLOCK) k_overlap_reduce(const CellSeg* __restrict__ segs, const float* __restrict__ nn_d2, OvRes* __restrict__ res) {
  __shared__ double wsum[QN_OV_BLOCK / 64];
  __shared__ uint32_t wcnt[QN_OV_BLOCK / 64];
  const CellSeg S = segs[blockIdx.x];
  double acc = 0.0; uint32_t cnt = 0;
  for (uint32_t i = threadIdx.x; i < S.n; i += QN_OV_BLOCK) {
    const float v = nn_d2[S.p0 + i];
    if (v < INFINITY) { acc = acc + (double)v; cnt++; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { acc = acc + __shfl_xor(acc, o); cnt += __shfl_xor(cnt, o); }
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = acc; wcnt[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QN_OV_BLOCK / 64; w++) { acc = acc + wsum[w]; cnt += wcnt[w]; }
    OvRes r; r.sum = acc; r.inliers = cnt; r.pad = 0;
    res[blockIdx.x] = r;
  }
}

// the per-point results of the latest overlap call (store slot QN_KF_INT_EXT_OVERLAP), in buffers of their own: the store's scratch may be reused by any
// other call before qn_kf_overlap_points asks
struct OvSlot { uint32_t p0[2], n[2]; int status; };
struct OverlapState {
  bool live = false; std::vector<OvSlot> slots;
  DevBuf<float> d2; DevBuf<int32_t> idx;
};

// the pairs (A_j = cl[2 j], B_j = cl[2 j + 1]) whose pre[j] is QN_OK; arguments already checked
int overlap_run(qn_kf_store* s, std::vector<const float4*>& cl, std::vector<uint32_t>& n, const std::vector<int>& pre, uint32_t P, double radius, qn_overlap* out, int* status) {
  OverlapState* st = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_OVERLAP, &st);
  if (rc != QN_OK) return rc;
  st->live = false;
  for (uint32_t j = 0; j < P; j++) {
    memset(&out[j], 0, sizeof(out[j]));
    status[j] = pre[j] != QN_OK ? pre[j] : (n[2 * j] == 0 || n[2 * j + 1] == 0) ? QN_ERR_EMPTY_CLOUD : QN_OK;
    if (status[j] != QN_OK) { n[2 * j] = n[2 * j + 1] = 0; cl[2 * j] = cl[2 * j + 1] = nullptr; }
  }
  const uint32_t S = 2 * P;
  std::vector<qn_kf_int_cell_grid> grid(S);
  const float4* pts = nullptr; const unsigned long long* keys = nullptr;
  rc = qn_kf_int_cell_index(s, cl.data(), n.data(), S, radius, grid.data(), &pts, &keys);      // sync 1 of 2
  if (rc != QN_OK) return rc;
  size_t total = 0; uint32_t nmax = 0;
  for (uint32_t k = 0; k < S; k++) { total += n[k]; nmax = std::max(nmax, n[k]); }
  st->slots.assign(P, OvSlot{});
  for (uint32_t j = 0; j < P; j++) {
    OvSlot& o = st->slots[j];
    for (int d = 0; d < 2; d++) { o.p0[d] = grid[2 * j + d].p0; o.n[d] = n[2 * j + d]; }
    o.status = status[j];
  }
  if (total == 0) { st->live = true; return QN_OK; }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (!st->d2.grow(s, total) || !st->idx.grow(s, total)) return QN_ERR_HIP;
  const size_t seg_bytes = qn_up16(sizeof(CellSeg) * S), res_bytes = sizeof(OvRes) * S;
  CellSeg* d_seg = (CellSeg*)qn_kf_int_scratch(s, 0, seg_bytes);
  float4* d_spts = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * total);
  uint32_t* d_cells = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * total);
  OvRes* d_res = (OvRes*)qn_kf_int_scratch(s, 3, res_bytes);
  char* h = (char*)qn_kf_int_pinned(s, seg_bytes + res_bytes);
  if (!d_seg || !d_spts || !d_cells || !d_res || !h) return qn_kf_fail(s, "qn_kf_overlap: scratch allocation failed");
  CellSeg* h_seg = (CellSeg*)h; OvRes* h_res = (OvRes*)(h + seg_bytes);
  for (uint32_t k = 0; k < S; k++) h_seg[k] = cell_seg(grid[k]);
  const double rr = radius * radius;
  const float r2 = (float)rr;
  const dim3 grid2((nmax + QN_CW_BLOCK - 1) / QN_CW_BLOCK, S);
  QN_KFCHK(s, hipMemcpyAsync(d_seg, h_seg, sizeof(CellSeg) * S, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_overlap_gather, grid2, dim3(QN_CW_BLOCK), 0, stream, (const CellSeg*)d_seg, keys, pts, d_spts, d_cells);
  hipLaunchKernelGGL(k_overlap_search, grid2, dim3(QN_CW_BLOCK), 0, stream, (const CellSeg*)d_seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, st->d2.p, st->idx.p);
  hipLaunchKernelGGL(k_overlap_reduce, dim3(S), dim3(QN_OV_BLOCK), 0, stream, (const CellSeg*)d_seg, (const float*)st->d2.p, d_res);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_res, d_res, res_bytes, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 2 of 2
  for (uint32_t j = 0; j < P; j++) {
    if (status[j] != QN_OK) continue;
    qn_overlap_dir* d[2] = {&out[j].a_to_b, &out[j].b_to_a};
    for (int k = 0; k < 2; k++) {
      d[k]->n = grid[2 * j + k].n; d[k]->n_finite = grid[2 * j + k].n_finite; d[k]->inliers = h_res[2 * j + k].inliers; d[k]->reserved = 0; d[k]->sum_d2 = h_res[2 * j + k].sum;
    }
  }
  st->live = true;
  return QN_OK;
}

// n records of 16 bytes inside one device allocation of the store's device (a host pointer would fault the GPU)
bool device_cloud_ok(int dev, const float* p, uint32_t n) {
  if (!n) return true;
  if (!p || ((uintptr_t)p & 15)) return false;
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != dev) { (void)hipGetLastError(); return false; }
  hipDeviceptr_t base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return (const char*)p >= (const char*)base && (size_t)((const char*)p - (const char*)base) + 16 * (size_t)n <= size;
}

bool radius_ok(double r) { return std::isfinite(r) && r > 0.0; }
const uint32_t kMaxPairs = 32767;       // the pair and direction are the grid's y dimension

}  // namespace

extern "C" int qn_kf_overlap_batch(qn_kf_store* s, const float* const* d_a, const uint32_t* n_a, const float* const* d_b, const uint32_t* n_b, uint32_t n_pairs,
                                   double radius, qn_overlap* out, int* status) {
  if (!s || !d_a || !n_a || !d_b || !n_b || n_pairs == 0 || !out || !status || !radius_ok(radius)) return QN_ERR_INVALID_ARG;
  if (n_pairs > kMaxPairs) return QN_ERR_CAPACITY;
  const int dev = qn_kf_int_device(s);
  QN_KFCHK(s, hipSetDevice(dev));
  for (uint32_t j = 0; j < n_pairs; j++) if (!device_cloud_ok(dev, d_a[j], n_a[j]) || !device_cloud_ok(dev, d_b[j], n_b[j])) return QN_ERR_INVALID_ARG;
  std::vector<const float4*> cl(2 * (size_t)n_pairs); std::vector<uint32_t> n(2 * (size_t)n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) { cl[2 * j] = (const float4*)d_a[j]; n[2 * j] = n_a[j]; cl[2 * j + 1] = (const float4*)d_b[j]; n[2 * j + 1] = n_b[j]; }
  return overlap_run(s, cl, n, std::vector<int>(n_pairs, QN_OK), n_pairs, radius, out, status);
}

extern "C" int qn_kf_verify_overlap(qn_kf_store* s, const uint32_t* pairs, uint32_t n_pairs, double radius, qn_overlap* out, int* status) {
  if (!s || n_pairs == 0 || !out || !status || !radius_ok(radius)) return QN_ERR_INVALID_ARG;
  if (n_pairs > kMaxPairs) return QN_ERR_CAPACITY;
  const uint32_t have = qn_kf_int_verify_pairs(s);
  if (!have) return QN_ERR_NOT_READY;
  if (!pairs && n_pairs != have) return QN_ERR_INVALID_ARG;
  if (pairs) {
    std::vector<uint8_t> seen(have, 0);
    for (uint32_t j = 0; j < n_pairs; j++) { if (pairs[j] >= have || seen[pairs[j]]) return QN_ERR_INVALID_ARG; seen[pairs[j]] = 1; }
  }
  std::vector<const float4*> cl(2 * (size_t)n_pairs, nullptr); std::vector<uint32_t> n(2 * (size_t)n_pairs, 0); std::vector<int> pre(n_pairs, QN_OK);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const uint32_t pj = pairs ? pairs[j] : j;
    int rc = qn_kf_int_verify_final_async(s, pj, &cl[2 * j], &n[2 * j]);
    if (rc == QN_OK) rc = qn_kf_verify_cloud(s, pj, QN_VERIFY_DST, (const float**)&cl[2 * j + 1], &n[2 * j + 1]);
    if (rc == QN_ERR_NOT_READY) { pre[j] = rc; cl[2 * j] = cl[2 * j + 1] = nullptr; n[2 * j] = n[2 * j + 1] = 0; }
    else if (rc != QN_OK) return rc;
  }
  return overlap_run(s, cl, n, pre, n_pairs, radius, out, status);
}

extern "C" int qn_kf_overlap_points(qn_kf_store* s, uint32_t pair_slot, int dir, float* nn_d2_out, int32_t* nn_idx_out) {
  if (!s || (dir != 0 && dir != 1) || (!nn_d2_out && !nn_idx_out)) return QN_ERR_INVALID_ARG;
  OverlapState* st = (OverlapState*)qn_kf_int_ext(s, QN_KF_INT_EXT_OVERLAP);
  if (!st || !st->live) return QN_ERR_NOT_READY;
  if (pair_slot >= st->slots.size()) return QN_ERR_INVALID_ARG;
  const OvSlot& o = st->slots[pair_slot];
  if (o.status != QN_OK) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (nn_d2_out) QN_KFCHK(s, hipMemcpyAsync(nn_d2_out, st->d2.p + o.p0[dir], sizeof(float) * o.n[dir], hipMemcpyDeviceToHost, stream));
  if (nn_idx_out) QN_KFCHK(s, hipMemcpyAsync(nn_idx_out, st->idx.p + o.p0[dir], sizeof(int32_t) * o.n[dir], hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}
