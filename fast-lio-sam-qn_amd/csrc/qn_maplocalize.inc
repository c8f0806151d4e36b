// qn_maplocalize.inc - scans registered against the corrected map itself (qn_kf_map_crop, qn_kf_map_crop_get, qn_kf_map_localize[_c2f], include/qn_engine.h).
// Part of qn_verify.hip: the crops, the scan clouds and the record the calls leave live in that unit's VerifyState (store slot QN_KF_INT_EXT_VERIFY), so
// qn_kf_verify_cloud and qn_kf_verify_overlap serve a localisation pair like any verified loop pair.  The numpy twin qn_amd/maplocalize.py is the specification
// of the crop; the registration is qn_gicp_align_batch_guess / qn_coarse_to_fine_align_batch on device pairs, nothing of its own.
//   crop      Q neighbourhoods cut out of the N records of the map slot by brute force, QN_ML_PASS centres per streaming pass (a cell index would cost a sort;
//             the distance tests are noise beside the 16 B read per record):
//               k_ml_count    a block owns ML_BLOCK = 256 consecutive records, a thread loads its record once and tests it against the pass's centres (LDS, wave-uniform);
//                             a centre's count of the block = ballot / popcount per wave, lane c keeping centre c's, the waves added through LDS into cnt[c][block];
//                             any[block] = whether the block holds a member of any centre of the pass
//               k_scan_rows   (qn_map_compact.cuh) one block per centre, in place: cnt[c][b] becomes the members of centre c before block b, tot[c] their number
//               (one host read of tot sizes the crop block and its index buffer: crop c at base[c], the centres' totals added up in order)
//               k_ml_compact  a block with any[block] == 0 returns before it loads a record; else the count kernel's tests again, a member of centre c going to
//                             base[c] + cnt[c][block] + the members of the waves before + its ballot rank: ascending map index, no atomics, the same bytes on every run
//   localise  host sequencing: the distinct crop centres (f32 bits of the guesses' translations) cropped once, each distinct query voxel-filtered alone in its
//             sensor frame (qn_kf_int_voxel_each), then the pair driver of qn_verify.hip (qn_kf_int_verify_run): ONE batched registration, records in caller order
// (the scheme is qn_map_compact.cuh's, generalised from one predicate to QN_ML_PASS per pass: its scan kernel, its lane_rank, its block sizes)
#define QN_ML_PASS 64
#define QN_ML_MAX_CROPS 32767u
#define ML_BLOCK MO_BLOCK
#define ML_WAVES MO_WAVES

int qn_ctx_int_max_points(const qn_ctx* c);

namespace {

__device__ __forceinline__ bool ml_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the membership rule (twin: maplocalize.crop_indices): f32 differences, (dx dx + dy dy) + dz dz left to right (the build's -ffp-contract=off keeps every product
// a rounded multiply), inclusive; the cylinder leaves dz dz out.  p's coordinates are finite (the caller's test).
__device__ __forceinline__ bool ml_within(const float4 p, const float4 c, float r2, uint32_t shape) {
  const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
  float d2 = dx * dx + dy * dy;
  if (shape == QN_LOCALIZE_SPHERE) d2 = d2 + dz * dz;
  return d2 <= r2;
}

// lane c of every wave: the wave's members of centre c (0 for c >= nc)
__device__ __forceinline__ uint32_t ml_wave_counts(const float4 p, bool fin, const float4* sc, uint32_t nc, float r2, uint32_t shape) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t mine = 0;
  for (uint32_t c = 0; c < nc; c++) {
    const uint32_t k = (uint32_t)__popcll(__ballot(fin && ml_within(p, sc[c], r2, shape)));
    if (lane == c) mine = k;
  }
  return mine;
}

__global__ void __launch_bounds__(ML_BLOCK) k_ml_count(uint32_t n, const float4* __restrict__ map, const float4* __restrict__ ctr, uint32_t nc, float r2, uint32_t shape,
                                                       uint32_t nb, uint32_t* __restrict__ cnt, uint32_t* __restrict__ any) {
  __shared__ float4 sc[QN_ML_PASS];
  __shared__ uint32_t wk[ML_WAVES][QN_ML_PASS];
  const uint32_t i = blockIdx.x * ML_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < nc) sc[threadIdx.x] = ctr[threadIdx.x];
  const float4 p = i < n ? map[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const bool fin = i < n && ml_finite(p.x) && ml_finite(p.y) && ml_finite(p.z);
  __syncthreads();
  wk[wave][lane] = ml_wave_counts(p, fin, sc, nc, r2, shape);
  __syncthreads();
  if (threadIdx.x < 64) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < ML_WAVES; w++) t += wk[w][lane];
    if (lane < nc) cnt[(size_t)lane * nb + blockIdx.x] = t;
    const unsigned long long some = __ballot(t != 0);
    if (lane == 0) any[blockIdx.x] = some ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(ML_BLOCK) k_ml_compact(uint32_t n, const float4* __restrict__ map, const float4* __restrict__ ctr, uint32_t nc, float r2, uint32_t shape,
                                                         uint32_t nb, const uint32_t* __restrict__ off, const uint32_t* __restrict__ any,
                                                         const unsigned long long* __restrict__ base, float4* __restrict__ out, uint32_t* __restrict__ idx) {
  __shared__ float4 sc[QN_ML_PASS];
  __shared__ uint32_t wk[ML_WAVES][QN_ML_PASS];
  __shared__ uint32_t blk[QN_ML_PASS];
  __shared__ unsigned long long go[QN_ML_PASS];
  if (any[blockIdx.x] == 0) return;                                      // (the whole block: no member of any centre of this pass, no record loaded)
  const uint32_t i = blockIdx.x * ML_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < nc) sc[threadIdx.x] = ctr[threadIdx.x];
  const float4 p = i < n ? map[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const bool fin = i < n && ml_finite(p.x) && ml_finite(p.y) && ml_finite(p.z);
  __syncthreads();
  wk[wave][lane] = ml_wave_counts(p, fin, sc, nc, r2, shape);
  __syncthreads();
  if (threadIdx.x < 64) {                                                // centre `lane`: the waves' counts to the members of the waves before, its place in the crop block
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < ML_WAVES; w++) { const uint32_t u = wk[w][lane]; wk[w][lane] = t; t += u; }
    blk[lane] = t;
    if (t) go[lane] = base[lane] + off[(size_t)lane * nb + blockIdx.x];
  }
  __syncthreads();
  for (uint32_t c = 0; c < nc; c++) {
    if (blk[c] == 0) continue;
    const bool m = fin && ml_within(p, sc[c], r2, shape);
    const unsigned long long bal = __ballot(m);
    if (m) {
      const unsigned long long dst = go[c] + wk[wave][c] + lane_rank(bal);
      out[dst] = p; idx[dst] = i;
    }
  }
}

// what the crop and localise calls keep per store (a member of VerifyState)
struct MlState {
  bool live = false;                                                     // the crops below are those of the latest successful crop
  uint64_t gen = 0; uint32_t n_map = 0, n_crops = 0, passes = 0;
  std::vector<unsigned long long> base;                                  // crop c = records [base[c], base[c + 1]) of pts / idx
  DevBuf<float4> pts, ctr, scans;                                        // the crop block, the centres, the scan clouds of the latest localise call
  DevBuf<uint32_t> idx, cnt, any, tot;
  DevBuf<unsigned long long> dbase;
};

MlState* ml_state(qn_kf_store* s, int* rc);                              // (qn_verify.hip, behind VerifyState)
void ml_verify_drop(qn_kf_store* s);                                     // the verify record of an earlier localise call goes: its crops are about to be overwritten

// centres: nc x 3 f32.  Two host synchronisations (the totals; the end, so that another stream may read the crops).
int ml_crop(qn_kf_store* s, MlState& m, const float* centres, uint32_t nc, double radius, uint32_t shape, uint32_t* counts_out) {
  uint32_t n = 0; uint64_t gen = 0;
  const float4* map = qn_kf_int_map(s, &n, &gen);
  if (!map || n == 0) return QN_ERR_NOT_READY;
  if (nc > QN_ML_MAX_CROPS) return QN_ERR_CAPACITY;
  m.live = false; ml_verify_drop(s);
  hipStream_t stream = qn_kf_int_stream(s);
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const uint32_t nb = (n + ML_BLOCK - 1) / ML_BLOCK, passes = (nc + QN_ML_PASS - 1) / QN_ML_PASS;
  if (!m.ctr.grow(s, nc) || !m.cnt.grow(s, (size_t)nc * nb) || !m.any.grow(s, (size_t)passes * nb) || !m.tot.grow(s, nc) || !m.dbase.grow(s, nc)) return QN_ERR_HIP;
  std::vector<float4> hc(nc);
  for (uint32_t c = 0; c < nc; c++) hc[c] = make_float4(centres[3 * c], centres[3 * c + 1], centres[3 * c + 2], 0.f);
  QN_KFCHK(s, hipMemcpyAsync(m.ctr.p, hc.data(), sizeof(float4) * nc, hipMemcpyHostToDevice, stream));
  const float r2 = (float)(radius * radius);
  for (uint32_t ps = 0; ps < passes; ps++) {
    const uint32_t c0 = ps * QN_ML_PASS, k = std::min<uint32_t>(QN_ML_PASS, nc - c0);
    hipLaunchKernelGGL(k_ml_count, dim3(nb), dim3(ML_BLOCK), 0, stream, n, map, m.ctr.p + c0, k, r2, shape, nb, m.cnt.p + (size_t)c0 * nb, m.any.p + (size_t)ps * nb);
  }
  hipLaunchKernelGGL(k_scan_rows, dim3(nc), dim3(MO_SCAN_BLOCK), 0, stream, (const uint32_t*)m.cnt.p, nb, m.cnt.p, m.tot.p);
  QN_KFCHK(s, hipGetLastError());
  std::vector<uint32_t> ht(nc);
  QN_KFCHK(s, hipMemcpyAsync(ht.data(), m.tot.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  m.base.assign(nc + 1, 0);
  for (uint32_t c = 0; c < nc; c++) m.base[c + 1] = m.base[c] + ht[c];
  const unsigned long long total = m.base[nc];
  if (total > 0xffffffffull) return QN_ERR_CAPACITY;
  if (total) {
    if (!m.pts.grow(s, (size_t)total) || !m.idx.grow(s, (size_t)total)) return QN_ERR_HIP;
    QN_KFCHK(s, hipMemcpyAsync(m.dbase.p, m.base.data(), sizeof(unsigned long long) * nc, hipMemcpyHostToDevice, stream));
    for (uint32_t ps = 0; ps < passes; ps++) {
      const uint32_t c0 = ps * QN_ML_PASS, k = std::min<uint32_t>(QN_ML_PASS, nc - c0);
      hipLaunchKernelGGL(k_ml_compact, dim3(nb), dim3(ML_BLOCK), 0, stream, n, map, m.ctr.p + c0, k, r2, shape, nb, m.cnt.p + (size_t)c0 * nb, m.any.p + (size_t)ps * nb,
                         m.dbase.p + c0, m.pts.p, m.idx.p);
    }
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipStreamSynchronize(stream));
  }
  m.gen = gen; m.n_map = n; m.n_crops = nc; m.passes = passes; m.live = true;
  if (counts_out) for (uint32_t c = 0; c < nc; c++) counts_out[c] = ht[c];
  return QN_OK;
}

bool ml_params_ok(const qn_localize_params* p) {
  return p && std::isfinite(p->radius) && p->radius > 0 && std::isfinite(p->leaf) && p->leaf > 0 && !std::isnan(p->score_thr) &&
         (p->shape == QN_LOCALIZE_SPHERE || p->shape == QN_LOCALIZE_CYLINDER) && p->reserved == 0;
}

int ml_localize(qn_kf_store* s, qn_ctx* ctx, const qn_localize_params* params, const int32_t* query, const double* guess16, uint32_t n_pairs, bool c2f,
                qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status, qn_localize_stats* stats_out) {
  // ---- every argument before anything runs: the store, its crops, its verify record and the context stay as they were
  if (!s || !ctx || !query || !guess16 || n_pairs == 0 || !results || !valid || !status || (c2f && !T_total) || !ml_params_ok(params)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != qn_ctx_int_device(ctx)) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  std::vector<float> g(16 * (size_t)n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) {
    if (query[j] < 0 || (size_t)query[j] >= n_kf) return QN_ERR_INVALID_ARG;
    const double* G = guess16 + 16 * (size_t)j;
    for (int i = 0; i < 16; i++) { if (!std::isfinite(G[i])) return QN_ERR_INVALID_ARG; g[16 * (size_t)j + i] = (float)G[i]; }
    if (G[12] != 0.0 || G[13] != 0.0 || G[14] != 0.0 || G[15] != 1.0) return QN_ERR_INVALID_ARG;
    for (int i = 0; i < 12; i++) if (!std::isfinite(g[16 * (size_t)j + i])) return QN_ERR_INVALID_ARG;      // (a finite f64 beyond the f32 range)
  }
  uint32_t n_map = 0; uint64_t gen = 0;
  if (!qn_kf_int_map(s, &n_map, &gen) || n_map == 0) return QN_ERR_NOT_READY;
  int rc = QN_OK;
  MlState* m = ml_state(s, &rc);
  if (!m) return rc;
  // ---- the distinct queries and the distinct centres (the f32 bits of the guess's translation), in order of first appearance
  std::vector<int32_t> uq; std::vector<float> uc; std::vector<uint32_t> qi, ci(n_pairs);
  qn_kf_int_distinct(query, n_pairs, uq, qi);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const float t[3] = {g[16 * (size_t)j + 3], g[16 * (size_t)j + 7], g[16 * (size_t)j + 11]};
    uint32_t k = 0;
    while (3 * (size_t)k < uc.size() && memcmp(&uc[3 * (size_t)k], t, sizeof(t)) != 0) k++;
    if (3 * (size_t)k == uc.size()) uc.insert(uc.end(), t, t + 3);
    ci[j] = k;
  }
  const uint32_t nq = (uint32_t)uq.size(), ncr = (uint32_t)(uc.size() / 3);
  // ---- the crops (two host synchronisations), then every distinct scan alone in its sensor frame (two more)
  std::vector<uint32_t> cn(ncr, 0);
  if ((rc = ml_crop(s, *m, uc.data(), ncr, params->radius, params->shape, cn.data())) != QN_OK) return rc;
  std::vector<const float4*> vp(nq, nullptr); std::vector<uint32_t> vn(nq, 0); std::vector<int> vs(nq, QN_ERR_EMPTY_CLOUD);
  if ((rc = qn_kf_int_voxel_each(s, uq.data(), nq, params->leaf, m->scans, vp.data(), vn.data(), vs.data())) != QN_OK) return rc;
  // ---- the pairs whose clouds exist and fit through the driver: one batched registration, cand = -1 in the record
  const uint32_t cap = (uint32_t)qn_ctx_int_max_points(ctx);
  std::vector<qn_kf_int_verify_job> jobs(n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const uint32_t ns = vs[qi[j]] == QN_OK ? vn[qi[j]] : 0, nt = cn[ci[j]];
    const int pre = vs[qi[j]] != QN_OK ? vs[qi[j]] : (ns == 0 || nt == 0) ? QN_ERR_EMPTY_CLOUD : (ns > cap || nt > cap) ? QN_ERR_CAPACITY : QN_OK;
    jobs[j] = qn_kf_int_verify_job{ns ? vp[qi[j]] : nullptr, ns, nt ? m->pts.p + m->base[ci[j]] : nullptr, nt, query[j], -1, qi[j], pre, {}, nullptr, nullptr};
    memcpy(jobs[j].guess, g.data() + 16 * (size_t)j, sizeof(jobs[j].guess));
  }
  rc = qn_kf_int_verify_run(s, ctx, jobs.data(), n_pairs, params->score_thr, c2f, c2f ? QN_KF_VERIFY_MAP_C2F : QN_KF_VERIFY_MAP, results, T_total, T_quatro, valid, status);
  if (rc != QN_OK) return rc;
  if (stats_out) *stats_out = qn_localize_stats{n_map, n_pairs, nq, ncr, m->passes, 0, m->base[ncr], gen};
  return QN_OK;
}

}  // namespace

extern "C" void qn_localize_default_params(qn_localize_params* p) {
  if (!p) return;
  p->radius = 35.0; p->leaf = 0.3; p->score_thr = 1.5; p->shape = QN_LOCALIZE_SPHERE; p->reserved = 0;
}

extern "C" int qn_kf_map_crop(qn_kf_store* s, const double* centres_xyz, uint32_t n_crops, double radius, uint32_t shape, uint32_t* counts_out) {
  // ---- every argument before anything runs
  if (!s || !centres_xyz || n_crops == 0 || !counts_out || !std::isfinite(radius) || !(radius > 0) || (shape != QN_LOCALIZE_SPHERE && shape != QN_LOCALIZE_CYLINDER))
    return QN_ERR_INVALID_ARG;
  if (n_crops > QN_ML_MAX_CROPS) return QN_ERR_CAPACITY;
  std::vector<float> c(3 * (size_t)n_crops);
  for (size_t i = 0; i < c.size(); i++) {
    c[i] = (float)centres_xyz[i];
    if (!std::isfinite(centres_xyz[i]) || !std::isfinite(c[i])) return QN_ERR_INVALID_ARG;
  }
  uint32_t n_map = 0; uint64_t gen = 0;
  if (!qn_kf_int_map(s, &n_map, &gen) || n_map == 0) return QN_ERR_NOT_READY;
  int rc = QN_OK;
  MlState* m = ml_state(s, &rc);
  if (!m) return rc;
  return ml_crop(s, *m, c.data(), n_crops, radius, shape, counts_out);
}

extern "C" int qn_kf_map_crop_get(qn_kf_store* s, uint32_t crop, const float** d_xyzi, uint32_t* n, uint32_t* idx_out) {
  if (!s || !d_xyzi || !n) return QN_ERR_INVALID_ARG;
  *d_xyzi = nullptr; *n = 0;
  int rc = QN_OK;
  MlState* m = ml_state(s, &rc);
  if (!m) return rc;
  if (!m->live) return QN_ERR_NOT_READY;
  if (crop >= m->n_crops) return QN_ERR_INVALID_ARG;
  const uint32_t k = (uint32_t)(m->base[crop + 1] - m->base[crop]);
  if (k == 0) return QN_OK;
  if (idx_out) {
    hipStream_t stream = qn_kf_int_stream(s);
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    QN_KFCHK(s, hipMemcpyAsync(idx_out, m->idx.p + m->base[crop], sizeof(uint32_t) * k, hipMemcpyDeviceToHost, stream));
    QN_KFCHK(s, hipStreamSynchronize(stream));
  }
  *d_xyzi = (const float*)(m->pts.p + m->base[crop]); *n = k;
  return QN_OK;
}

extern "C" int qn_kf_map_localize(qn_kf_store* s, qn_ctx* ctx, const qn_localize_params* params, const int32_t* query, const double* guess16, uint32_t n_pairs,
                                  qn_gicp_result* results, int* valid, int* status, qn_localize_stats* stats_out) {
  return ml_localize(s, ctx, params, query, guess16, n_pairs, false, results, nullptr, nullptr, valid, status, stats_out);
}

extern "C" int qn_kf_map_localize_c2f(qn_kf_store* s, qn_ctx* ctx, const qn_localize_params* params, const int32_t* query, const double* guess16, uint32_t n_pairs,
                                      qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status, qn_localize_stats* stats_out) {
  return ml_localize(s, ctx, params, query, guess16, n_pairs, true, results, T_total, T_quatro, valid, status, stats_out);
}
