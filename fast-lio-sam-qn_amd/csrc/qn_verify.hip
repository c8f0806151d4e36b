// qn_verify.hip - drift-free verification of loop candidates from the keyframe store (qn_kf_verify_loop_candidates, include/qn_engine.h).
// The reference verifies a candidate with both clouds in the world frame of the corrected poses (LoopClosure::setSrcAndDstCloud,
// loop_closure.cpp:58-108) and GICP from identity: after more drift than the clouds overlap, which is when Scan Context finds revisits the
// radius search cannot, that registration cannot converge.  Here the source is the query scan in its own sensor frame and the target the
// candidate's submap in the candidate's sensor frame (keyframe i with inv(P_c) P_i: relative poses within the candidate's window, where the
// drift is small), and each pair starts from the candidate's Scan Context heading.  The result is the query-to-candidate transform itself.
// Host code only: the clouds are assembled by qn_kf_assemble_batch and registered by qn_gicp_align_batch_guess, both on the device.
// The numpy twins (qn_amd/scancontext.py: relative_pose, seed_from_yaw) restate the poses and guesses bit for bit; the build's
// -ffp-contract=off keeps every product a rounded multiply and a rounded add.
// qn_kf_verify_loop_pairs runs the same step for many queries at once (one assembly, one registration; the single-query call is that with the query repeated).
// Every verification entry point of the store - these two, the resident coarse-to-fine and submap forms (qn_kf_quatro.inc, qn_kf_submap.inc) and the map
// localisation (qn_maplocalize.inc) - hands its pairs to ONE driver here, qn_kf_int_verify_run: defaults, grouping by query, one batched registration, the
// records back in caller order, the verify record.  qn_kf_verify_cloud serves the debug clouds
// loopTimerFunc publishes after each attempt (fast_lio_sam_qn.cpp:245-248) for any pair of the latest multi-pair call, GICP or coarse-to-fine.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_kf_buf.h"
#include "qn_map_compact.cuh"

int qn_ctx_int_device(const qn_ctx* c);

namespace {

// inv(P_c) P_i: inv(P) = [R^T | -R^T t] (each -R^T t entry summed over k = 0..2 in order), then every entry of the product summed over k = 0..3 in order
void relative_pose(const double* Pc, const double* Pi, double* Q) {
  double A[16];
  for (int r = 0; r < 3; r++) {
    double acc = 0.0;
    for (int k = 0; k < 3; k++) { A[4 * r + k] = Pc[4 * k + r]; acc = acc + Pc[4 * k + r] * Pc[4 * k + 3]; }
    A[4 * r + 3] = -acc;
  }
  A[12] = 0.0; A[13] = 0.0; A[14] = 0.0; A[15] = 1.0;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      double acc = 0.0;
      for (int k = 0; k < 4; k++) acc = acc + A[4 * r + k] * Pi[4 * k + c];
      Q[4 * r + c] = acc;
    }
}

// Rz(-yaw) rounded to f32: the candidate's heading minus the query's is yaw, so R(inv(P_c) P_q) = Rz(h_q - h_c) = Rz(-yaw)
void seed_from_yaw(double yaw, float* g) {
  const double c = std::cos(-yaw), s = std::sin(-yaw);
  const double m[16] = {c, -s, 0.0, 0.0, s, c, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  for (int i = 0; i < 16; i++) g[i] = (float)m[i];
}

}  // namespace
void qn_kf_int_relative_pose(const double* Pc, const double* Pi, double* Q) { relative_pose(Pc, Pi, Q); }
void qn_kf_int_seed_from_yaw(double yaw, float* g) { seed_from_yaw(yaw, g); }
// ids / rel / seg of `count` candidate windows (qn_kf_internal.h)
int qn_kf_int_windows(const int32_t* centres, uint32_t count, const double* poses, uint32_t n_poses, size_t n_kf, uint32_t range, bool keep_newest,
                      std::vector<int32_t>& ids, std::vector<double>& rel, std::vector<uint32_t>& seg) {
  const long long end = (long long)n_poses - (keep_newest ? 0 : 1);
  for (uint32_t t = 0; t < count; t++) {
    const long long c = centres[t];
    for (long long i = c - (long long)range; i <= c + (long long)range; i++) {
      if (i < 0 || i >= end) continue;
      if ((size_t)i >= n_kf) return QN_ERR_INVALID_ARG;                             // (a pose without a keyframe inside a window)
      double Q[16];
      relative_pose(poses + 16 * (size_t)c, poses + 16 * (size_t)i, Q);
      ids.push_back((int32_t)i); rel.insert(rel.end(), Q, Q + 16);
    }
    seg.push_back((uint32_t)ids.size());
  }
  return QN_OK;
}

namespace {

void unset_record(qn_gicp_result* r) {       // what a registration that did not run reports (the batch's defaults)
  memset(r, 0, sizeof(*r)); r->fitness = DBL_MAX;
  for (int i = 0; i < 4; i++) { r->T[5 * i] = 1.f; r->T64[5 * i] = 1.0; }
}

}  // namespace

int qn_kf_int_verify_run(qn_kf_store* s, qn_ctx* ctx, const qn_kf_int_verify_job* jobs, uint32_t n, double score_thr, bool c2f, int kind,
                         qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  // ---- one batched registration over the jobs that may run, grouped by query (stable: caller order within a query) so that the candidates of one query
  //      sit in consecutive lanes and share the source's preparation
  std::vector<uint32_t> order(n);
  for (uint32_t j = 0; j < n; j++) order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].group < jobs[b].group; });
  std::vector<qn_pair_desc> pairs; std::vector<float> g; std::vector<C2fCached> cached; std::vector<uint32_t> which;
  bool rows = false;
  for (uint32_t j : order) {
    const qn_kf_int_verify_job& b = jobs[j];
    if (b.pre != QN_OK) continue;
    pairs.push_back(qn_pair_desc{(const float*)b.src, b.ns, (const float*)b.dst, b.nt, 16, 1});
    g.insert(g.end(), b.guess, b.guess + 16);
    cached.push_back(C2fCached{const_cast<float4*>(b.src), b.src_rows, const_cast<float4*>(b.dst), b.dst_rows});
    rows = rows || b.src_rows || b.dst_rows;
    which.push_back(j);
  }
  const uint32_t m = (uint32_t)pairs.size();
  std::vector<qn_gicp_result> res(m); std::vector<int> val(m, 0), st(m, QN_OK), stage(m, 0);
  std::vector<double> Tt(c2f ? 16 * (size_t)m : 0), Tq(c2f ? 16 * (size_t)m : 0);
  for (uint32_t k = 0; k < m; k++) unset_record(&res[k]);
  if (m) {
    const int rc = c2f ? qn_ctx_int_c2f_batch_stage(ctx, pairs.data(), m, score_thr, res.data(), Tt.data(), Tq.data(), val.data(), st.data(), rows ? cached.data() : nullptr, stage.data())
                       : qn_gicp_align_batch_guess(ctx, pairs.data(), g.data(), m, score_thr, res.data(), val.data(), st.data());
    if (rc != QN_OK) return rc;                                                    // (nothing written: the caller's arrays and the record are the previous call's)
  }
  // ---- every output as a registration that did not run leaves it, then the records back in caller order, and the record qn_kf_verify_cloud serves
  const double eye[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  std::vector<qn_kf_int_verify_pair> rec(n);
  for (uint32_t j = 0; j < n; j++) {
    const qn_kf_int_verify_job& b = jobs[j];
    unset_record(&results[j]); valid[j] = 0; status[j] = b.pre;
    if (T_total) memcpy(T_total + 16 * (size_t)j, eye, sizeof(eye));
    if (T_quatro) memcpy(T_quatro + 16 * (size_t)j, eye, sizeof(eye));
    rec[j] = qn_kf_int_verify_pair{b.src, b.ns, b.dst, b.nt, b.query, b.cand, 0, {}, {}};
  }
  for (uint32_t k = 0; k < m; k++) {
    const uint32_t j = which[k];
    results[j] = res[k]; valid[j] = val[k]; status[j] = st[k];
    qn_kf_int_verify_pair& r = rec[j];
    if (c2f) {
      memcpy(T_total + 16 * (size_t)j, Tt.data() + 16 * (size_t)k, 16 * sizeof(double));
      if (T_quatro) memcpy(T_quatro + 16 * (size_t)j, Tq.data() + 16 * (size_t)k, 16 * sizeof(double));
      r.stage = st[k] == QN_ERR_HIP ? 0 : stage[k];
      memcpy(r.Tq, Tq.data() + 16 * (size_t)k, sizeof(r.Tq));
      memcpy(r.Tg, res[k].T, sizeof(r.Tg));
    } else if (st[k] == QN_OK) { r.stage = 2; memcpy(r.Tg, res[k].T, sizeof(r.Tg)); }
  }
  return kind == QN_KF_VERIFY_KEEP ? QN_OK : qn_kf_int_verify_record(s, kind, rec.data(), n);
}

namespace {

// qn_kf_verify_loop_pairs, and with kind = QN_KF_VERIFY_KEEP and the query repeated qn_kf_verify_loop_candidates
int verify_pairs(qn_kf_store* s, qn_ctx* ctx, const int32_t* query, const int32_t* cand, const double* yaw, uint32_t n_pairs, const double* poses, uint32_t n_poses,
                 uint32_t submap_range, double leaf, double score_thr, int kind, qn_gicp_result* results, int* valid, int* status) {
  // ---- every argument before anything runs: the store's batch slot, its verify record and the context stay as they were
  if (!s || !ctx || !query || !cand || n_pairs == 0 || !poses || !results || !valid || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != qn_ctx_int_device(ctx)) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  auto bad_id = [&](int32_t id) { return id < 0 || (size_t)id >= n_kf || (uint32_t)id >= n_poses; };
  for (uint32_t j = 0; j < n_pairs; j++) {
    if (bad_id(query[j]) || bad_id(cand[j]) || cand[j] == query[j]) return QN_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < j; i++) if (query[i] == query[j] && cand[i] == cand[j]) return QN_ERR_INVALID_ARG;
    if (yaw && !std::isfinite(yaw[j])) return QN_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < (size_t)n_poses * 16; i++) if (!std::isfinite(poses[i])) return QN_ERR_INVALID_ARG;
  // ---- the lists: each distinct query alone with the identity, then each distinct candidate's window relative to it (loop_submap_ids(query, c, submap_range,
  //      False, False, n_poses)[1]), one segment per distinct keyframe: a window depends on c, the poses and submap_range, never on the query
  std::vector<int32_t> uq, uc; std::vector<uint32_t> qi, ci;
  qn_kf_int_distinct(query, n_pairs, uq, qi); qn_kf_int_distinct(cand, n_pairs, uc, ci);
  const uint32_t nq = (uint32_t)uq.size(), S = nq + (uint32_t)uc.size();
  std::vector<int32_t> ids; std::vector<double> rel; std::vector<uint32_t> seg(1, 0);
  const double eye[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  for (uint32_t k = 0; k < nq; k++) { ids.push_back(uq[k]); rel.insert(rel.end(), eye, eye + 16); seg.push_back((uint32_t)ids.size()); }
  int rc = qn_kf_int_windows(uc.data(), (uint32_t)uc.size(), poses, n_poses, n_kf, submap_range, false, ids, rel, seg);
  if (rc != QN_OK) return rc;
  // ---- one assembly (two host synchronisations), then the pairs whose clouds exist through the driver
  std::vector<const float*> d_xyz(S, nullptr); std::vector<uint32_t> n(S, 0); std::vector<int> ast(S, QN_OK);
  rc = qn_kf_assemble_batch(s, ids.data(), rel.data(), seg.data(), S, leaf, d_xyz.data(), n.data(), ast.data());
  if (rc != QN_OK) return rc;
  std::vector<qn_kf_int_verify_job> jobs(n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const uint32_t a = qi[j], b = nq + ci[j];
    jobs[j] = qn_kf_int_verify_job{(const float4*)d_xyz[a], n[a], (const float4*)d_xyz[b], n[b], query[j], cand[j], a, ast[a] != QN_OK ? ast[a] : ast[b], {}, nullptr, nullptr};
    seed_from_yaw(yaw ? yaw[j] : 0.0, jobs[j].guess);
  }
  return qn_kf_int_verify_run(s, ctx, jobs.data(), n_pairs, score_thr, false, kind, results, nullptr, nullptr, valid, status);
}

}  // namespace

extern "C" int qn_kf_verify_loop_candidates(qn_kf_store* s, qn_ctx* ctx, int32_t query, const int32_t* cand, const double* yaw, uint32_t n_cand,
                                            const double* poses, uint32_t n_poses, uint32_t submap_range, double leaf, double score_thr,
                                            qn_gicp_result* results, int* valid, int* status) {
  // the pairs form with the query repeated (segment 0 the source, segment 1 + j candidate j), leaving no record of its own
  const std::vector<int32_t> q(cand ? n_cand : 0, query);
  return verify_pairs(s, ctx, q.data(), cand, yaw, n_cand, poses, n_poses, submap_range, leaf, score_thr, QN_KF_VERIFY_KEEP, results, valid, status);
}

extern "C" int qn_kf_verify_loop_pairs(qn_kf_store* s, qn_ctx* ctx, const int32_t* query, const int32_t* cand, const double* yaw, uint32_t n_pairs,
                                       const double* poses, uint32_t n_poses, uint32_t submap_range, double leaf, double score_thr,
                                       qn_gicp_result* results, int* valid, int* status) {
  return verify_pairs(s, ctx, query, cand, yaw, n_pairs, poses, n_poses, submap_range, leaf, score_thr, QN_KF_VERIFY_GICP, results, valid, status);
}

// ------------------------------------------------------------------ scans against the map itself: the crops and qn_kf_map_localize[_c2f]
#include "qn_maplocalize.inc"

// ------------------------------------------------------------------ the record a call leaves and the clouds qn_kf_verify_cloud serves from it
namespace {

// the record of the latest qn_kf_verify_loop_pairs[_c2f] call (store slot QN_KF_INT_EXT_VERIFY) and the arena qn_kf_verify_cloud computes into:
// COARSE and FINAL of pair j at fixed places (2 * (sum of ns before j), then + ns), so every pointer handed out stays valid until the record is replaced
struct VerifyState {
  bool live = false; int kind = QN_KF_VERIFY_GICP;
  bool c2f() const { return kind == QN_KF_VERIFY_C2F || kind == QN_KF_VERIFY_SUBMAP_C2F || kind == QN_KF_VERIFY_MAP_C2F; }
  int from() const { return kind >= QN_KF_VERIFY_MAP ? QN_KF_VERIFY_FROM_MAP : kind >= QN_KF_VERIFY_SUBMAP ? QN_KF_VERIFY_FROM_SUBMAPS : kind; }
  std::vector<qn_kf_int_verify_pair> p; std::vector<size_t> off;
  DevBuf<float4> arena;
  MlState ml;                                                            // qn_maplocalize.inc: the crops and scan clouds a QN_KF_VERIFY_MAP[_C2F] record names
};

MlState* ml_state(qn_kf_store* s, int* rc) {
  VerifyState* st = nullptr;
  *rc = qn_kf_ext_state(s, QN_KF_INT_EXT_VERIFY, &st);
  return *rc == QN_OK ? &st->ml : nullptr;
}
void ml_verify_drop(qn_kf_store* s) {
  VerifyState* st = (VerifyState*)qn_kf_int_ext(s, QN_KF_INT_EXT_VERIFY);
  if (st && st->live && st->from() == QN_KF_VERIFY_FROM_MAP) st->live = false;
}

// the two clouds qn_kf_verify_cloud computes: COARSE = transformPcd(src, T_quatro) (k_transform_cloud_f64's f64 order, rounded to f32); FINAL = that (or src on
// the GICP path) through the GICP T as align() fills aligned_ (k_transform_cloud: xform_query<1> with the f32 entries).  One point per thread.
struct VerifyXf { double Tq[12]; float Tg[12]; int coarse, fine; };
__global__ void k_verify_cloud(const float4* __restrict__ in, uint32_t n, VerifyXf m, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  float x = p.x, y = p.y, z = p.z;
  if (m.coarse) {
    const double dx = x, dy = y, dz = z;
    x = (float)(((m.Tq[0] * dx + m.Tq[1] * dy) + m.Tq[2] * dz) + m.Tq[3]);
    y = (float)(((m.Tq[4] * dx + m.Tq[5] * dy) + m.Tq[6] * dz) + m.Tq[7]);
    z = (float)(((m.Tq[8] * dx + m.Tq[9] * dy) + m.Tq[10] * dz) + m.Tq[11]);
  }
  if (m.fine) {
    const float qx = m.Tg[0] * x + (m.Tg[1] * y + (m.Tg[2] * z + m.Tg[3]));
    const float qy = m.Tg[4] * x + (m.Tg[5] * y + (m.Tg[6] * z + m.Tg[7]));
    const float qz = m.Tg[8] * x + (m.Tg[9] * y + (m.Tg[10] * z + m.Tg[11]));
    x = qx; y = qy; z = qz;
  }
  out[i] = make_float4(x, y, z, 1.0f);
}

}  // namespace

int qn_kf_int_verify_record(qn_kf_store* s, int kind, const qn_kf_int_verify_pair* p, uint32_t n) {
  VerifyState* st = nullptr;
  const int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_VERIFY, &st);
  if (rc != QN_OK) return rc;
  st->kind = kind; st->p.assign(p, p + n); st->off.assign(n + 1, 0);
  for (uint32_t j = 0; j < n; j++) st->off[j + 1] = st->off[j] + 2 * (size_t)p[j].ns;
  st->live = true;
  return QN_OK;
}

void qn_kf_int_verify_stale(qn_kf_store* s, int from, const int32_t* ids, uint32_t count) {
  VerifyState* st = (VerifyState*)qn_kf_int_ext(s, QN_KF_INT_EXT_VERIFY);
  if (!st || !st->live || st->from() != from) return;
  if (from == QN_KF_VERIFY_FROM_BATCH || !ids) { st->live = false; return; }
  for (uint32_t i = 0; i < count; i++)
    for (const qn_kf_int_verify_pair& q : st->p)
      if (q.query == ids[i] || q.cand == ids[i]) { st->live = false; return; }
}

static int verify_cloud(qn_kf_store* s, uint32_t pair, int which, const float** d_xyz, uint32_t* n, bool sync);
extern "C" int qn_kf_verify_cloud(qn_kf_store* s, uint32_t pair, int which, const float** d_xyz, uint32_t* n) { return verify_cloud(s, pair, which, d_xyz, n, true); }
int qn_kf_int_verify_final_async(qn_kf_store* s, uint32_t pair, const float4** d_xyz, uint32_t* n) { return verify_cloud(s, pair, QN_VERIFY_FINAL, (const float**)d_xyz, n, false); }
uint32_t qn_kf_int_verify_pairs(const qn_kf_store* s) {
  const VerifyState* st = (const VerifyState*)qn_kf_int_ext(s, QN_KF_INT_EXT_VERIFY);
  return st && st->live ? (uint32_t)st->p.size() : 0u;
}
// sync = false (qn_kf_int_verify_final_async): the launch is left on the store's stream
static int verify_cloud(qn_kf_store* s, uint32_t pair, int which, const float** d_xyz, uint32_t* n, bool sync) {
  if (!s || !d_xyz || !n || which < QN_VERIFY_SRC || which > QN_VERIFY_FINAL) return QN_ERR_INVALID_ARG;
  *d_xyz = nullptr; *n = 0;
  VerifyState* st = (VerifyState*)qn_kf_int_ext(s, QN_KF_INT_EXT_VERIFY);
  if (!st || !st->live) return QN_ERR_NOT_READY;
  if (pair >= st->p.size()) return QN_ERR_INVALID_ARG;
  const qn_kf_int_verify_pair& q = st->p[pair];
  if (which == QN_VERIFY_SRC) { *d_xyz = (const float*)q.src; *n = q.ns; return QN_OK; }
  if (which == QN_VERIFY_DST) { *d_xyz = (const float*)q.dst; *n = q.nt; return QN_OK; }
  // COARSE needs the solved Quatro stage (coarse-to-fine only), FINAL the registration
  if (which == QN_VERIFY_COARSE ? (!st->c2f() || q.stage < 1) : q.stage < 2) return QN_ERR_NOT_READY;
  if (q.ns == 0 || !q.src) return QN_ERR_NOT_READY;
  hipStream_t stream = qn_kf_int_stream(s);
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  // the arena of the record's pairs, sized exactly; the record stays when it cannot be had (QN_ERR_HIP, the next call tries again)
  const size_t need = st->off.back();
  if (need > st->arena.cap && st->arena.p) (void)hipStreamSynchronize(stream);      // (clouds handed out unsynchronised may still be read)
  if (!st->arena.grow(s, need, true)) return QN_ERR_HIP;
  float4* out = st->arena.p + st->off[pair] + (which == QN_VERIFY_FINAL ? q.ns : 0);
  VerifyXf m{};
  m.coarse = st->c2f() ? 1 : 0; m.fine = which == QN_VERIFY_FINAL ? 1 : 0;
  for (int i = 0; i < 12; i++) { m.Tq[i] = q.Tq[i]; m.Tg[i] = q.Tg[i]; }
  hipLaunchKernelGGL(k_verify_cloud, dim3((q.ns + 255) / 256), dim3(256), 0, stream, q.src, q.ns, m, out);
  QN_KFCHK(s, hipGetLastError());
  if (sync) QN_KFCHK(s, hipStreamSynchronize(stream));
  *d_xyz = (const float*)out; *n = q.ns;
  return QN_OK;
}
