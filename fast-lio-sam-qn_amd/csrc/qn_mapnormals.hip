// qn_mapnormals.hip - a surface normal and a curvature for every point of the store's map slot, on the GPU (qn_kf_map_normals, qn_kf_download_map_normals,
// qn_kf_map_moments: include/qn_engine.h).  The numpy twin qn_amd/mapnormals.py is the specification: the neighbours of a point are the finite map points
// within r of it by the oracle's f32 sqdist3 (<= float(r * r), inclusive, the point itself included); their offsets, quantised to integers of 2^-e m, give the
// count, the three first and the six second moments as exact integers; the f64 covariance from them, its smallest eigenvector and eigenvalue share are the normal
// and the curvature; the nearest viewpoint orients the normal.  Count, moments and viewpoint index equal the twin's bit for bit, and so does the covariance:
// the integer sums do not depend on the order the neighbours are met in, and the f64 arithmetic behind them is the same IEEE operations in the same order (the
// library is built without contraction).  Only the eigen solve differs from the twin's LAPACK call, by what two backward-stable solves may differ.
//   index     qn_kf_int_cell_index (qn_cloud.hip) over the map as one cloud, one segment; k_cell_gather lays the sorted points (original index in .w) and their
//             cell words out flat (qn_cell_walk.cuh, with the walk and its exactness argument).
//   normals   k_map_normals, one point per lane, 256 lanes a block, in the sorted order: neighbouring lanes are neighbouring points and read the same runs.
//             The candidates of the walk within r: k, s1[3], s2[6] stay in registers (u32 and int64; di * dj is one 64-bit multiply-add).  Then the
//             viewpoints pass through LDS in tiles of 256 (three f64 planes, every lane reads the same address: a broadcast), the covariance and the cyclic
//             Jacobi solve (qn_eig3.cuh, a fixed sweep count) run in the same thread, and the results go back to the point's own index in the map.  No
//             atomics, no scratch memory; two host synchronisations a call (the index's, and one at the end).
// One lane per point rather than a few lanes per point with a cross-lane reduce: a map point at the usual leaf has tens of neighbours among one or two hundred
// candidates, the lanes of a wave walk the same runs, and the solve and the viewpoint loop - the larger part of the arithmetic - are per point either way.
// Overflow: |di| <= 2^20 + 1 (|d| <= r (1 + 2^-21) and r 2^e <= 2^20), so |di dj| < 2^41 and the int64 sums are exact below 2^21 neighbours.  The kernel
// counts the candidates it scans per point - the points of the 3 x 3 x 3 block - and raises a flag at 2^21; the call then returns QN_ERR_CAPACITY.  (The
// cell-count bound of the index does not exclude this by itself: a passed-through, unfiltered map may put any number of points into one cell.)  Results are
// committed only on success (KfMapResults, qn_kf_buf.h), so a refused call - this refusal included - leaves the previous results as they were.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_cell_walk.cuh"
#include "qn_eig3.cuh"

namespace {

#define MN_BLOCK QN_CW_BLOCK
#define MN_VTILE 256                                     // viewpoints per LDS tile (3 x 256 f64 = 6 KiB)
#define MN_MAX_BLOCK_POINTS (1u << 21)

__global__ void __launch_bounds__(MN_BLOCK) k_map_normals(const CellSeg S, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, float r2, float scale,
                                                          uint32_t min_nb, const double* __restrict__ views, uint32_t nv, float4* __restrict__ normals,
                                                          uint32_t* __restrict__ count, int32_t* __restrict__ view_idx, long long* __restrict__ s1_out,
                                                          long long* __restrict__ s2_out, uint32_t* __restrict__ flag) {
  __shared__ double vs[3][MN_VTILE];
  const uint32_t t = blockIdx.x * MN_BLOCK + threadIdx.x;
  const bool act = t < S.n;                              // (no early return: every thread of the block meets the barriers of the viewpoint loop)
  const bool fin = t < S.nfin;
  const float4 q = act ? spts[t] : make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t qi = __float_as_uint(q.w);
  uint32_t k = 0, scanned = 0;
  long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
  if (fin) {
    cell_walk(S, spts, cells, q, [&](uint32_t, const float4& p, float d2) {
      scanned++;
      if (d2 <= r2) {
        const int ix = (int)rintf((p.x - q.x) * scale), iy = (int)rintf((p.y - q.y) * scale), iz = (int)rintf((p.z - q.z) * scale);
        k++;
        sx += ix; sy += iy; sz += iz;
        sxx += (long long)ix * ix; sxy += (long long)ix * iy; sxz += (long long)ix * iz;
        syy += (long long)iy * iy; syz += (long long)iy * iz; szz += (long long)iz * iz;
      }
    });
    if (scanned >= MN_MAX_BLOCK_POINTS) *flag = 1u;      // (every writer stores the same word)
  }

  // the nearest viewpoint, the lowest index on ties
  const double px = q.x, py = q.y, pz = q.z;
  int best = -1; double bd = INFINITY;
  for (uint32_t base = 0; base < nv; base += MN_VTILE) {
    const uint32_t m = min((uint32_t)MN_VTILE, nv - base);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += MN_BLOCK) {
      const double* v = views + 3 * (size_t)(base + i);
      vs[0][i] = v[0]; vs[1][i] = v[1]; vs[2][i] = v[2];
    }
    __syncthreads();
    if (fin) {
      for (uint32_t i = 0; i < m; i++) {
        const double dx = vs[0][i] - px, dy = vs[1][i] - py, dz = vs[2][i] - pz;
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < bd || best < 0) { bd = d; best = (int)(base + i); }
      }
    }
  }
  if (!act) return;

  const float nanf_ = __uint_as_float(0x7fc00000u);
  float4 out = make_float4(nanf_, nanf_, nanf_, nanf_);
  if (fin && k >= min_nb) {
    const double kd = (double)k;
    const double mx = (double)sx / kd, my = (double)sy / kd, mz = (double)sz / kd;
    const double cxx = (double)sxx / kd - mx * mx, cxy = (double)sxy / kd - mx * my, cxz = (double)sxz / kd - mx * mz;
    const double cyy = (double)syy / kd - my * my, cyz = (double)syz / kd - my * mz, czz = (double)szz / kd - mz * mz;
    const double tr = (cxx + cyy) + czz;
    if (tr > 0.0) {
      double w[3], V[3][3];
      qn_eig3_jacobi(cxx, cxy, cxz, cyy, cyz, czz, w, V);
      // the smallest eigenvalue's column (the lowest on a tie), and the other two eigenvalues in order
      int j0 = 0; double wmin = w[0];
      if (w[1] < wmin) { wmin = w[1]; j0 = 1; }
      if (w[2] < wmin) { wmin = w[2]; j0 = 2; }
      const double wa = j0 == 0 ? w[1] : w[0], wb = j0 == 2 ? w[1] : w[2];
      const double l1 = fmin(wa, wb), l2 = fmax(wa, wb);
      const double l0 = fmax(wmin, 0.0);
      double nx = j0 == 0 ? V[0][0] : j0 == 1 ? V[0][1] : V[0][2];
      double ny = j0 == 0 ? V[1][0] : j0 == 1 ? V[1][1] : V[1][2];
      double nz = j0 == 0 ? V[2][0] : j0 == 1 ? V[2][1] : V[2][2];
      bool flip;
      if (best >= 0) {
        const double* v = views + 3 * (size_t)best;
        const double dx = v[0] - px, dy = v[1] - py, dz = v[2] - pz;
        flip = (nx * dx + ny * dy) + nz * dz < 0.0;
      } else {
        double lead = nx;
        if (fabs(ny) > fabs(lead)) lead = ny;
        if (fabs(nz) > fabs(lead)) lead = nz;
        flip = lead < 0.0;
      }
      if (flip) { nx = -nx; ny = -ny; nz = -nz; }
      out = make_float4((float)nx, (float)ny, (float)nz, (float)(l0 / ((l0 + l1) + l2)));
    }
  }
  normals[qi] = out;
  count[qi] = k;
  view_idx[qi] = fin ? best : -1;
  long long* s1 = s1_out + 3 * (size_t)qi; long long* s2 = s2_out + 6 * (size_t)qi;
  s1[0] = sx; s1[1] = sy; s1[2] = sz;
  s2[0] = sxx; s2[1] = sxy; s2[2] = sxz; s2[3] = syy; s2[4] = syz; s2[5] = szz;
}

// the store's normals state (slot QN_KF_INT_EXT_NORMALS)
struct MnSet { DevBuf<float4> normals; DevBuf<uint32_t> count; DevBuf<int32_t> view; DevBuf<long long> s1, s2; };
typedef KfMapResults<MnSet> NormalState;

}  // namespace

extern "C" void qn_normal_default_params(qn_normal_params* p) {
  if (!p) return;
  p->radius = 0.6; p->min_neighbors = 5; p->reserved = 0;
}

extern "C" int qn_kf_map_normals(qn_kf_store* s, const qn_normal_params* params, const double* viewpoints_xyz, uint32_t n_view, const float** d_normals_out,
                                 uint32_t* n_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !d_normals_out || !n_out || (n_view && !viewpoints_xyz)) return QN_ERR_INVALID_ARG;
  if (!std::isfinite(params->radius) || !(params->radius > 0.0) || params->min_neighbors < 3 || params->reserved != 0) return QN_ERR_INVALID_ARG;
  for (size_t i = 0; i < 3 * (size_t)n_view; i++) if (!std::isfinite(viewpoints_xyz[i])) return QN_ERR_INVALID_ARG;
  uint32_t n = 0; uint64_t gen = 0;
  const float4* map = qn_kf_int_map(s, &n, &gen);
  if (!map) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  NormalState* st = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_NORMALS, &st);
  if (rc != QN_OK) return rc;
  MnSet& o = st->spare();
  if (!o.normals.grow(s, n) || !o.count.grow(s, n) || !o.view.grow(s, n) || !o.s1.grow(s, 3 * (size_t)n) || !o.s2.grow(s, 6 * (size_t)n)) return QN_ERR_HIP;
  qn_kf_int_cell_grid g;
  const float4* pts = nullptr; const unsigned long long* keys = nullptr;
  rc = qn_kf_int_cell_index(s, &map, &n, 1, params->radius, &g, &pts, &keys);       // sync 1 of 2
  if (rc != QN_OK) return rc;
  hipStream_t stream = qn_kf_int_stream(s);
  const size_t view_bytes = qn_up16(sizeof(double) * 3 * (size_t)std::max<uint32_t>(n_view, 1));
  double* d_views = (double*)qn_kf_int_scratch(s, 0, view_bytes);
  float4* d_spts = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)n);
  uint32_t* d_cells = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (size_t)n);
  uint32_t* d_flag = (uint32_t*)qn_kf_int_scratch(s, 3, 16);
  char* h = (char*)qn_kf_int_pinned(s, view_bytes + 16);
  if (!d_views || !d_spts || !d_cells || !d_flag || !h) return qn_kf_fail(s, "qn_kf_map_normals: scratch allocation failed");
  uint32_t* h_flag = (uint32_t*)(h + view_bytes);
  if (n_view) {
    memcpy(h, viewpoints_xyz, sizeof(double) * 3 * (size_t)n_view);
    QN_KFCHK(s, hipMemcpyAsync(d_views, h, sizeof(double) * 3 * (size_t)n_view, hipMemcpyHostToDevice, stream));
  }
  QN_KFCHK(s, hipMemsetAsync(d_flag, 0, 16, stream));
  const CellSeg seg = cell_seg(g);
  const double rr = params->radius * params->radius;
  const float r2 = (float)rr;
  const float scale = std::ldexp(1.0f, qn_quant_exponent(params->radius, 20));          // r 2^e <= 2^20: the overflow bound of the header comment
  const dim3 grid((n + MN_BLOCK - 1) / MN_BLOCK);
  hipLaunchKernelGGL(k_cell_gather, grid, dim3(MN_BLOCK), 0, stream, seg, keys, pts, d_spts, d_cells);
  hipLaunchKernelGGL(k_map_normals, grid, dim3(MN_BLOCK), 0, stream, seg, (const float4*)d_spts, (const uint32_t*)d_cells, r2, scale, params->min_neighbors,
                     (const double*)d_views, n_view, o.normals.p, o.count.p, o.view.p, o.s1.p, o.s2.p, d_flag);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // sync 2 of 2
  if (*h_flag) {
    qn_kf_int_set_error(s, "qn_kf_map_normals: 2^21 or more map points in one 3 x 3 x 3 block of cells");
    return QN_ERR_CAPACITY;
  }
  st->commit(gen, n);
  *d_normals_out = (const float*)o.normals.p; *n_out = n;
  return QN_OK;
}

extern "C" int qn_kf_download_map_normals(qn_kf_store* s, float* normals4_out, uint32_t* count_out, int32_t* view_idx_out) {
  if (!s || (!normals4_out && !count_out && !view_idx_out)) return QN_ERR_INVALID_ARG;
  uint32_t n = 0; const float4* map = nullptr;
  const MnSet* o = NormalState::lookup(s, QN_KF_INT_EXT_NORMALS, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (normals4_out) QN_KFCHK(s, hipMemcpyAsync(normals4_out, o->normals.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (count_out) QN_KFCHK(s, hipMemcpyAsync(count_out, o->count.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (view_idx_out) QN_KFCHK(s, hipMemcpyAsync(view_idx_out, o->view.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_moments(qn_kf_store* s, int64_t* s1_out, int64_t* s2_out) {
  if (!s || (!s1_out && !s2_out)) return QN_ERR_INVALID_ARG;
  uint32_t n = 0; const float4* map = nullptr;
  const MnSet* o = NormalState::lookup(s, QN_KF_INT_EXT_NORMALS, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (s1_out) QN_KFCHK(s, hipMemcpyAsync(s1_out, o->s1.p, sizeof(long long) * 3 * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (s2_out) QN_KFCHK(s, hipMemcpyAsync(s2_out, o->s2.p, sizeof(long long) * 6 * (size_t)n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}
