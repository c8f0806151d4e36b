// qn_verify.hip - drift-free verification of loop candidates from the keyframe store (qn_kf_verify_loop_candidates, include/qn_engine.h).
// The reference verifies a candidate with both clouds in the world frame of the corrected poses (LoopClosure::setSrcAndDstCloud,
// loop_closure.cpp:58-108) and GICP from identity: after more drift than the clouds overlap, which is when Scan Context finds revisits the
// radius search cannot, that registration cannot converge.  Here the source is the query scan in its own sensor frame and the target the
// candidate's submap in the candidate's sensor frame (keyframe i with inv(P_c) P_i: relative poses within the candidate's window, where the
// drift is small), and each pair starts from the candidate's Scan Context heading.  The result is the query-to-candidate transform itself.
// Host code only: the clouds are assembled by qn_kf_assemble_batch and registered by qn_gicp_align_batch_guess, both on the device.
// The numpy twins (qn_amd/scancontext.py: relative_pose, seed_from_yaw) restate the poses and guesses bit for bit; the build's
// -ffp-contract=off keeps every product a rounded multiply and a rounded add.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_kf_internal.h"

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

void unset_record(qn_gicp_result* r) {       // what a registration that did not run reports (the batch's defaults)
  memset(r, 0, sizeof(*r)); r->fitness = DBL_MAX;
  for (int i = 0; i < 4; i++) { r->T[5 * i] = 1.f; r->T64[5 * i] = 1.0; }
}

}  // namespace

extern "C" int qn_kf_verify_loop_candidates(qn_kf_store* s, qn_ctx* ctx, int32_t query, const int32_t* cand, const double* yaw, uint32_t n_cand,
                                            const double* poses, uint32_t n_poses, uint32_t submap_range, double leaf, double score_thr,
                                            qn_gicp_result* results, int* valid, int* status) {
  // ---- every argument before anything runs: the store's batch slot and the context stay as they were
  if (!s || !ctx || !cand || n_cand == 0 || !poses || !results || !valid || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != qn_ctx_int_device(ctx)) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  if (query < 0 || (size_t)query >= n_kf || (uint32_t)query >= n_poses) return QN_ERR_INVALID_ARG;
  for (uint32_t j = 0; j < n_cand; j++) {
    const int32_t c = cand[j];
    if (c < 0 || (size_t)c >= n_kf || (uint32_t)c >= n_poses || c == query) return QN_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < j; i++) if (cand[i] == c) return QN_ERR_INVALID_ARG;
    if (yaw && !std::isfinite(yaw[j])) return QN_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < (size_t)n_poses * 16; i++) if (!std::isfinite(poses[i])) return QN_ERR_INVALID_ARG;
  // ---- the lists: [query] with the identity, then each candidate's window (loop_submap_ids(query, c, submap_range, False, False, n_poses)[1]) relative to it
  std::vector<int32_t> ids; std::vector<double> rel; std::vector<uint32_t> seg(n_cand + 2, 0);
  ids.push_back(query);
  const double eye[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  rel.insert(rel.end(), eye, eye + 16);
  seg[1] = 1;
  for (uint32_t j = 0; j < n_cand; j++) {
    const long long c = cand[j];
    for (long long i = c - (long long)submap_range; i <= c + (long long)submap_range; i++) {
      if (i < 0 || i >= (long long)n_poses - 1) continue;                // the reference's `i < keyframes.size() - 1` (loop_closure.cpp:98-104)
      if ((size_t)i >= n_kf) return QN_ERR_INVALID_ARG;
      double Q[16];
      relative_pose(poses + 16 * (size_t)c, poses + 16 * (size_t)i, Q);
      ids.push_back((int32_t)i); rel.insert(rel.end(), Q, Q + 16);
    }
    seg[j + 2] = (uint32_t)ids.size();
  }
  std::vector<float> guess(16 * (size_t)n_cand);
  for (uint32_t j = 0; j < n_cand; j++) seed_from_yaw(yaw ? yaw[j] : 0.0, guess.data() + 16 * (size_t)j);
  // ---- one assembly (two host synchronisations): segment 0 the source, segment 1 + j candidate j
  const uint32_t S = n_cand + 1;
  std::vector<const float*> d_xyz(S, nullptr); std::vector<uint32_t> n(S, 0); std::vector<int> ast(S, QN_OK);
  int rc = qn_kf_assemble_batch(s, ids.data(), rel.data(), seg.data(), S, leaf, d_xyz.data(), n.data(), ast.data());
  if (rc != QN_OK) return rc;
  // ---- one batched registration over the candidates whose clouds exist, every pair naming the same source buffer (prepared once)
  std::vector<qn_pair_desc> pairs; std::vector<float> g; std::vector<uint32_t> which;
  for (uint32_t j = 0; j < n_cand; j++) {
    unset_record(&results[j]); valid[j] = 0;
    status[j] = ast[0] != QN_OK ? ast[0] : ast[1 + j];
    if (status[j] != QN_OK) continue;
    pairs.push_back(qn_pair_desc{d_xyz[0], n[0], d_xyz[1 + j], n[1 + j], 16, 1});
    g.insert(g.end(), guess.begin() + 16 * (size_t)j, guess.begin() + 16 * (size_t)j + 16);
    which.push_back(j);
  }
  if (pairs.empty()) return QN_OK;
  const uint32_t m = (uint32_t)pairs.size();
  std::vector<qn_gicp_result> res(m); std::vector<int> val(m, 0), st(m, QN_OK);
  rc = qn_gicp_align_batch_guess(ctx, pairs.data(), g.data(), m, score_thr, res.data(), val.data(), st.data());
  if (rc != QN_OK) return rc;
  for (uint32_t k = 0; k < m; k++) { results[which[k]] = res[k]; valid[which[k]] = val[k]; status[which[k]] = st[k]; }
  return QN_OK;
}
