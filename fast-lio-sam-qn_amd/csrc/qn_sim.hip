// qn_sim.hip - spinning-LiDAR scans ray-cast on the GPU straight into the keyframe store (qn_sim_lidar_to_store).
// The scene is a flat array of analytic primitives (qn_sim_prim: ground plane, walls, poles, boxes - the surfaces qn_amd/synth.py samples);
// one thread casts one ray (beam, col) of one scan, grid (rays / 256, scans).  The numpy twin qn_amd/synth.lidar_scan is the specification:
// the same f64 operations in the same order (the build's -ffp-contract=off keeps every a * b + c a rounded multiply and a rounded add),
// no transcendental on the device (cos / sin come in host tables), IEEE division and the correctly rounded f64 sqrt, one rounding to f32
// at the end - so the records are identical bit for bit.
// Hits are compacted in (beam, col) order with the engine's scan kernels; each scan becomes one keyframe (float4 x y z intensity, has_i = 1)
// through the adopt path of qn_kf_add_device.  Two host synchronisations per call: the per-scan counts, then the end of the copies.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_util_kernels.cuh"
#include "qn_kf_buf.h"

namespace qn {

#define QN_SIM_BLOCK 256
struct SimSensor { const double *cos_el, *sin_el, *cos_az, *sin_az; uint32_t n_beams, n_cols; double min_range, max_range, noise_k; };

__device__ __forceinline__ uint32_t sim_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ bool sim_in(double v, double lo, double hi) { return v >= lo && v <= hi; }

// One ray per thread.  Primitives are read at a wave-uniform index (scalar loads; the switch is uniform), so only the hit tests diverge.
__global__ void __launch_bounds__(QN_SIM_BLOCK) k_sim_cast(const qn_sim_prim* __restrict__ prims, uint32_t n_prims, SimSensor sen,
                                                          const double* __restrict__ poses, const uint32_t* __restrict__ seeds,
                                                          float4* __restrict__ res, uint32_t* __restrict__ flag) {
  const uint32_t rays = sen.n_beams * sen.n_cols;
  const uint32_t r = blockIdx.x * QN_SIM_BLOCK + threadIdx.x, s = blockIdx.y;
  if (r >= rays) return;
  const uint32_t beam = r / sen.n_cols, col = r - beam * sen.n_cols;
  const double* T = poses + 16 * (size_t)s;
  const double ce = sen.cos_el[beam], se = sen.sin_el[beam], ca = sen.cos_az[col], sa = sen.sin_az[col];
  const double ux = ce * ca, uy = ce * sa, uz = se;
  const double dx = T[0] * ux + T[1] * uy + T[2] * uz;
  const double dy = T[4] * ux + T[5] * uy + T[6] * uz;
  const double dz = T[8] * ux + T[9] * uy + T[10] * uz;
  const double ox = T[3], oy = T[7], oz = T[11];
  double best = INFINITY, cn = 0.0;
  uint32_t kind = 0;
  for (uint32_t i = 0; i < n_prims; i++) {
    const uint32_t k = prims[i].kind;
    const double* p = prims[i].p;
    if (k == QN_SIM_GROUND) {
      if (dz != 0.0) {
        const double t = (0.0 - oz) / dz;
        if (t > 0.0 && t < best && sim_in(ox + t * dx, p[0], p[2]) && sim_in(oy + t * dy, p[1], p[3])) { best = t; kind = k; cn = fabs(dz); }
      }
    } else if (k == QN_SIM_WALL) {
      if (p[3] == 0.0) {
        if (dy != 0.0) {
          const double t = (p[1] - oy) / dy;
          if (t > 0.0 && t < best && sim_in(ox + t * dx, p[0], p[0] + p[2]) && sim_in(oz + t * dz, 0.0, p[4])) { best = t; kind = k; cn = fabs(dy); }
        }
      } else if (dx != 0.0) {
        const double t = (p[0] - ox) / dx;
        if (t > 0.0 && t < best && sim_in(oy + t * dy, p[1], p[1] + p[3]) && sim_in(oz + t * dz, 0.0, p[4])) { best = t; kind = k; cn = fabs(dx); }
      }
    } else if (k == QN_SIM_POLE) {
      const double px = ox - p[0], py = oy - p[1], rr = p[2];
      const double a = dx * dx + dy * dy;
      const double b = px * dx + py * dy;
      const double c = px * px + py * py - rr * rr;
      const double disc = b * b - a * c;
      if (a > 0.0 && disc >= 0.0) {
        const double sq = __builtin_sqrt(disc);
        const double t1 = (-b - sq) / a, t2 = (-b + sq) / a;
        if (t1 > 0.0 && t1 < best && sim_in(oz + t1 * dz, 0.0, p[3])) { best = t1; kind = k; cn = fabs((px + t1 * dx) * dx + (py + t1 * dy) * dy) / rr; }
        if (t2 > 0.0 && t2 < best && sim_in(oz + t2 * dz, 0.0, p[3])) { best = t2; kind = k; cn = fabs((px + t2 * dx) * dx + (py + t2 * dy) * dy) / rr; }
      }
    } else {                                                   // QN_SIM_BOX (kinds are validated on the host)
      const double xlo = p[0] - 0.5 * p[2], xhi = p[0] + 0.5 * p[2], ylo = p[1] - 0.5 * p[3], yhi = p[1] + 0.5 * p[3], H = p[4];
      if (dx != 0.0) {
        const double t0 = (xlo - ox) / dx;
        if (t0 > 0.0 && t0 < best && sim_in(oy + t0 * dy, ylo, yhi) && sim_in(oz + t0 * dz, 0.0, H)) { best = t0; kind = k; cn = fabs(dx); }
        const double t1 = (xhi - ox) / dx;
        if (t1 > 0.0 && t1 < best && sim_in(oy + t1 * dy, ylo, yhi) && sim_in(oz + t1 * dz, 0.0, H)) { best = t1; kind = k; cn = fabs(dx); }
      }
      if (dy != 0.0) {
        const double t0 = (ylo - oy) / dy;
        if (t0 > 0.0 && t0 < best && sim_in(ox + t0 * dx, xlo, xhi) && sim_in(oz + t0 * dz, 0.0, H)) { best = t0; kind = k; cn = fabs(dy); }
        const double t1 = (yhi - oy) / dy;
        if (t1 > 0.0 && t1 < best && sim_in(ox + t1 * dx, xlo, xhi) && sim_in(oz + t1 * dz, 0.0, H)) { best = t1; kind = k; cn = fabs(dy); }
      }
      if (dz != 0.0) {
        const double t = (H - oz) / dz;
        if (t > 0.0 && t < best && sim_in(ox + t * dx, xlo, xhi) && sim_in(oy + t * dy, ylo, yhi)) { best = t; kind = k; cn = fabs(dz); }
      }
    }
  }
  const size_t g = (size_t)s * rays + r;
  uint32_t keep = 0;
  if (best < INFINITY) {
    const uint32_t base = sim_mix32(sim_mix32(sim_mix32(seeds[s]) ^ beam) ^ col);
    const double u0 = (double)sim_mix32(base) * 2.3283064365386962890625e-10, u1 = (double)sim_mix32(base + 1u) * 2.3283064365386962890625e-10;
    const double u2 = (double)sim_mix32(base + 2u) * 2.3283064365386962890625e-10, u3 = (double)sim_mix32(base + 3u) * 2.3283064365386962890625e-10;
    const double tp = best + sen.noise_k * ((((u0 + u1) + u2) + u3) - 2.0);
    if (tp >= sen.min_range && tp <= sen.max_range) {
      // intensity = base + gain * |n . d| per kind (ground, wall, pole, box): synth.SIM_INTENSITY
      const double ib = kind == QN_SIM_GROUND ? 0.1 : kind == QN_SIM_WALL ? 0.3 : kind == QN_SIM_POLE ? 0.5 : 0.2;
      const double ig = kind == QN_SIM_GROUND ? 0.3 : kind == QN_SIM_WALL ? 0.5 : kind == QN_SIM_POLE ? 0.4 : 0.6;
      res[g] = make_float4((float)(tp * ux), (float)(tp * uy), (float)(tp * uz), (float)(ib + ig * cn));
      keep = 1;
    }
  }
  flag[g] = keep;
}

// compacted position of every kept ray (pos = exclusive scan of flag over all scans, pos[total rays] = total)
__global__ void k_sim_compact(const float4* __restrict__ res, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t m, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m && flag[i]) out[pos[i]] = res[i];
}
// first compacted record of every scan, and the total: off[s] = pos[s * rays], s = 0 .. n_scans
__global__ void k_sim_offsets(const uint32_t* __restrict__ pos, uint32_t rays, uint32_t n_scans, uint32_t* __restrict__ off) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= n_scans) off[s] = pos[(size_t)s * rays];
}

}  // namespace qn

static bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }
static bool prims_ok(const qn_sim_prim* prims, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) {
    const qn_sim_prim& q = prims[i];
    if (q.kind > QN_SIM_BOX || !finite_all(q.p, 6)) return false;
    const double* p = q.p;
    if (q.kind == QN_SIM_GROUND && !(p[0] <= p[2] && p[1] <= p[3])) return false;
    if (q.kind == QN_SIM_WALL && !(p[2] >= 0 && p[3] >= 0 && p[4] >= 0)) return false;
    if (q.kind == QN_SIM_POLE && !(p[2] > 0 && p[3] >= 0)) return false;
    if (q.kind == QN_SIM_BOX && !(p[2] >= 0 && p[3] >= 0 && p[4] >= 0)) return false;
  }
  return true;
}
static bool table_ok(const double* v, uint32_t n) { if (!v) return false; for (uint32_t i = 0; i < n; i++) if (!(v[i] >= -1.0 && v[i] <= 1.0)) return false; return true; }

extern "C" int qn_sim_lidar_to_store(qn_kf_store* s, const qn_sim_prim* prims, uint32_t n_prims, const qn_sim_sensor* sen, const double* poses16,
                                     const uint32_t* seeds, uint32_t n_scans, int32_t* ids_out, uint32_t* n_out) {
  // ---- every argument is checked before anything is enqueued; the store is unchanged on any error return before the copies
  if (!s || !sen || !poses16 || !seeds || !ids_out || !n_out || (n_prims && !prims)) return QN_ERR_INVALID_ARG;
  if (n_scans == 0 || n_scans > QN_SIM_MAX_SCANS || n_prims > QN_SIM_MAX_PRIMS) return QN_ERR_INVALID_ARG;
  if (sen->n_beams == 0 || sen->n_cols == 0 || (uint64_t)sen->n_beams * sen->n_cols > QN_SIM_MAX_RAYS) return QN_ERR_INVALID_ARG;
  const uint32_t rays = sen->n_beams * sen->n_cols;
  if ((uint64_t)rays * n_scans > QN_SIM_MAX_TOTAL_RAYS) return QN_ERR_INVALID_ARG;
  if (!table_ok(sen->cos_el, sen->n_beams) || !table_ok(sen->sin_el, sen->n_beams) || !table_ok(sen->cos_az, sen->n_cols) || !table_ok(sen->sin_az, sen->n_cols)) return QN_ERR_INVALID_ARG;
  if (!std::isfinite(sen->min_range) || !std::isfinite(sen->max_range) || !std::isfinite(sen->sigma) || !(sen->min_range >= 0) ||
      !(sen->max_range > sen->min_range) || !(sen->sigma >= 0)) return QN_ERR_INVALID_ARG;
  if (!finite_all(poses16, 16 * (size_t)n_scans) || !prims_ok(prims, n_prims)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_count(s) + n_scans > 0x7fffffffull) return QN_ERR_CAPACITY;

  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t st = qn_kf_int_stream(s);
  const size_t m = (size_t)rays * n_scans;                          // <= 2^27: every index below fits in uint32_t
  const uint32_t sbf = (uint32_t)((m + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS));
  const size_t tab = sizeof(double) * (2 * (size_t)sen->n_beams + 2 * (size_t)sen->n_cols);
  char* d_in = (char*)qn_kf_int_scratch(s, 0, sizeof(qn_sim_prim) * (n_prims + 1) + tab + sizeof(double) * 16 * n_scans + sizeof(uint32_t) * n_scans + 64);
  float4* d_res = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * m);
  uint32_t* d_flag = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * m);
  uint32_t* d_pos = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * (m + 1));
  uint32_t* d_sums = (uint32_t*)qn_kf_int_scratch(s, 4, sizeof(uint32_t) * (sbf + 2));
  float4* d_cmp = (float4*)qn_kf_int_scratch(s, 5, sizeof(float4) * m);
  uint32_t* d_off = (uint32_t*)qn_kf_int_scratch(s, 6, sizeof(uint32_t) * (n_scans + 1));
  uint32_t* h_off = (uint32_t*)qn_kf_int_pinned(s, sizeof(uint32_t) * (n_scans + 1));
  if (!d_in || !d_res || !d_flag || !d_pos || !d_sums || !d_cmp || !d_off || !h_off) return qn_kf_fail(s, "qn_sim_lidar_to_store: scratch allocation failed");

  // inputs: primitives, the four tables, poses, seeds - one packed upload (8-byte aligned sections)
  char* w = d_in;
  qn_sim_prim* d_prims = (qn_sim_prim*)w; w += sizeof(qn_sim_prim) * (n_prims + 1);
  double* d_tab = (double*)w; w += tab;
  double* d_poses = (double*)w; w += sizeof(double) * 16 * n_scans;
  uint32_t* d_seeds = (uint32_t*)w;
  std::vector<char> h_in(w - d_in + sizeof(uint32_t) * n_scans);
  char* hw = h_in.data();
  if (n_prims) memcpy(hw, prims, sizeof(qn_sim_prim) * n_prims);
  hw += sizeof(qn_sim_prim) * (n_prims + 1);
  double* ht = (double*)hw;
  memcpy(ht, sen->cos_el, sizeof(double) * sen->n_beams); memcpy(ht + sen->n_beams, sen->sin_el, sizeof(double) * sen->n_beams);
  memcpy(ht + 2 * sen->n_beams, sen->cos_az, sizeof(double) * sen->n_cols); memcpy(ht + 2 * sen->n_beams + sen->n_cols, sen->sin_az, sizeof(double) * sen->n_cols);
  hw += tab;
  memcpy(hw, poses16, sizeof(double) * 16 * n_scans); hw += sizeof(double) * 16 * n_scans;
  memcpy(hw, seeds, sizeof(uint32_t) * n_scans);
  QN_KFCHK(s, hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, st));

  qn::SimSensor ss{d_tab, d_tab + sen->n_beams, d_tab + 2 * sen->n_beams, d_tab + 2 * sen->n_beams + sen->n_cols, sen->n_beams, sen->n_cols,
                   sen->min_range, sen->max_range, sen->sigma * 1.7320508075688772};
  hipLaunchKernelGGL(qn::k_sim_cast, dim3((rays + QN_SIM_BLOCK - 1) / QN_SIM_BLOCK, n_scans), dim3(QN_SIM_BLOCK), 0, st,
                     (const qn_sim_prim*)d_prims, n_prims, ss, (const double*)d_poses, (const uint32_t*)d_seeds, d_res, d_flag);
  hipLaunchKernelGGL(qn::k_scan_block, dim3(sbf), dim3(QN_BLOCK), 0, st, (const uint32_t*)d_flag, (uint32_t)m, d_pos, d_sums);
  hipLaunchKernelGGL(qn::k_scan_top, dim3(1), dim3(QN_BLOCK), 0, st, d_sums, sbf);
  hipLaunchKernelGGL(qn::k_scan_add_total, dim3(sbf), dim3(QN_BLOCK), 0, st, d_pos, (uint32_t)m, (const uint32_t*)d_sums, (const uint32_t*)d_flag);
  hipLaunchKernelGGL(qn::k_sim_compact, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, (const float4*)d_res, (const uint32_t*)d_flag, (const uint32_t*)d_pos, (uint32_t)m, d_cmp);
  hipLaunchKernelGGL(qn::k_sim_offsets, dim3((n_scans + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t*)d_pos, rays, n_scans, d_off);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h_off, d_off, sizeof(uint32_t) * (n_scans + 1), hipMemcpyDeviceToHost, st));
  QN_KFCHK(s, hipStreamSynchronize(st));                           // sync 1 of 2: the per-scan counts size the keyframes

  // each scan -> one keyframe through the adopt path of qn_kf_add_device (float4 records, intensity at byte 12)
  std::vector<float4*> bufs(n_scans, nullptr);
  std::vector<uint32_t> cnt(n_scans);
  for (uint32_t k = 0; k < n_scans; k++) cnt[k] = h_off[k + 1] - h_off[k];
  int status = QN_OK;
  for (uint32_t k = 0; k < n_scans && status == QN_OK; k++) status = qn_kf_int_copy_async(s, d_cmp + h_off[k], cnt[k], 16, 12, &bufs[k]);
  const hipError_t e = hipStreamSynchronize(st);                     // sync 2 of 2: the copies are done, the scratch may be reused
  if (status == QN_OK && e != hipSuccess) { qn_kf_int_set_error(s, (std::string("qn_sim_lidar_to_store -> ") + hipGetErrorString(e)).c_str()); status = QN_ERR_HIP; }
  if (status != QN_OK) { for (float4* b : bufs) (void)hipFree(b); return status; }
  qn_kf_int_append(s, bufs.data(), cnt.data(), n_scans, true, ids_out);
  for (uint32_t k = 0; k < n_scans; k++) n_out[k] = cnt[k];
  return QN_OK;
}
