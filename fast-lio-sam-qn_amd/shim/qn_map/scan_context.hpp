// Drop-in helper for the candidate step of FastLioSamQn::loopTimerFunc (fast_lio_sam_qn.cpp:203-252) when candidates come from Scan Context
// place descriptors instead of LoopClosure::fetchClosestKeyframeIdx's radius search on drifted poses (loop_closure.cpp:34-56).  The query's
// descriptor is made on the GPU from its resident keyframe (qn_kf_sc_describe, a no-op when it exists), the older keyframes' descriptors
// must already exist (describe each keyframe once, when it is added), and qn_kf_sc_query ranks them.  The indices feed
// qn_map::loopSubmapPairs (loop_submaps.hpp) and the batched registrations; yaw is the candidate's heading minus the query's, from the
// best column shift: verifyScanContextCandidates seeds each candidate's registration with it.  For the keyframes that arrived between two loop-timer
// ticks, scanContextCandidatesMany ranks them all in one query and verifyLoopPairs / verifyLoopPairsCoarseToFine check every (query, candidate) pair at once.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct ScCandidates {
  std::vector<int> idx;                            // keyframe indices (store ids), nearest first
  std::vector<double> dist;                        // Scan Context distance D in [0, 2]
  std::vector<double> yaw;                         // candidate heading minus query heading [rad], in [-pi, pi)
};

// The top_k keyframes older than `query` by more than tdiff (stamps[query] - stamps[c] > tdiff, loop_closure.cpp:45) nearest to it by
// Scan Context distance, keeping those with D < max_dist (the original's SC_DIST_THRES test).  stamps[i] = keyframes[i].timestamp_,
// at least one per keyframe in the store.
inline ScCandidates scanContextCandidates(qn_kf_store* store, const std::vector<double>& stamps, int query, double tdiff, int top_k, double max_dist) {
  if (top_k <= 0) throw std::invalid_argument("[qn_map] scanContextCandidates: top_k must be positive");
  qn_sc_params p{};
  int rc = qn_kf_sc_get_params(store, &p);
  const int32_t q = query;
  if (rc == QN_OK) rc = qn_kf_sc_describe(store, &q, 1);
  std::vector<int32_t> ids((size_t)top_k), shift((size_t)top_k);
  std::vector<double> d((size_t)top_k);
  uint32_t n = 0;
  if (rc == QN_OK) rc = qn_kf_sc_query(store, &q, 1, stamps.data(), (uint32_t)stamps.size(), tdiff, (uint32_t)top_k, ids.data(), d.data(), shift.data(), &n);
  detail::check(store, rc, "qn_kf_sc_query");
  ScCandidates out;
  const double pi = 3.14159265358979323846;
  for (uint32_t r = 0; r < n; r++) {
    if (!(d[r] < max_dist)) continue;
    double yaw = std::fmod(-2.0 * pi * shift[r] / p.n_sectors + pi, 2.0 * pi);
    if (yaw < 0) yaw += 2.0 * pi;
    out.idx.push_back(ids[r]); out.dist.push_back(d[r]); out.yaw.push_back(yaw - pi);
  }
  return out;
}

struct ScVerified {
  int idx;                                         // the candidate's keyframe index
  bool valid;                                      // loop_closure.cpp:129: converged and score < score_thr
  double score;                                    // fitness
  double T[16];                                    // row-major, query sensor frame -> candidate sensor frame: an estimate of inv(P_c) P_query
  int status;                                      // QN_OK, or QN_ERR_EMPTY_CLOUD for an empty candidate submap
};

// Drift-free verification of the candidates (qn_kf_verify_loop_candidates): the query scan in its own sensor frame against each candidate's
// scan-to-submap window in the candidate's sensor frame, seeded with ScCandidates::yaw, all in one batched registration on ctx (its NanoGICP
// parameters).  poses16 = the corrected poses (row-major 4x4 each), one per keyframe.  In loopTimerFunc the loop factor is then
// BetweenFactor(latest, c, inv(T), score) from T itself, in place of pose_between_eig_ * pose_corrected (fast_lio_sam_qn.cpp:224-233).
inline std::vector<ScVerified> verifyScanContextCandidates(qn_kf_store* store, qn_ctx* ctx, int query, const ScCandidates& c, const std::vector<double>& poses16,
                                                           int submap_range, double leaf, double score_thr) {
  std::vector<ScVerified> out;
  if (c.idx.empty()) return out;
  if (submap_range < 0 || poses16.size() % 16 != 0 || c.yaw.size() != c.idx.size())
    throw std::invalid_argument("[qn_map] verifyScanContextCandidates: bad submap_range, poses or candidates");
  const size_t K = c.idx.size();
  std::vector<int32_t> ids(c.idx.begin(), c.idx.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<int> valid(K), status(K);
  const int rc = qn_kf_verify_loop_candidates(store, ctx, query, ids.data(), c.yaw.data(), (uint32_t)K, poses16.data(), (uint32_t)(poses16.size() / 16),
                                              (uint32_t)submap_range, leaf, score_thr, r.data(), valid.data(), status.data());
  detail::check(store, rc, "qn_kf_verify_loop_candidates");
  for (size_t k = 0; k < K; k++) {
    ScVerified v{c.idx[k], valid[k] != 0, r[k].fitness, {}, status[k]};
    for (int i = 0; i < 16; i++) v.T[i] = (double)r[k].T[i];
    out.push_back(v);
  }
  return out;
}

struct ScVerifiedC2f {
  int idx;                                         // the candidate's keyframe index
  bool valid;                                      // Quatro converged, GICP converged and score < score_thr (loop_closure.cpp:129, 145-148)
  double score;                                    // the fine stage's fitness
  double T[16];                                    // row-major T_gicp * T_quatro, query sensor frame -> candidate sensor frame: an estimate of inv(P_c) P_query
  double T_quatro[16];                             // the coarse estimate
  int status;                                      // QN_OK, or QN_ERR_EMPTY_CLOUD for an empty side
};

// The reference's default check (quatro/enable true, enable_submap_matching false: Quatro -> transformPcd -> Nano-GICP scan to scan, loop_closure.cpp:138-159)
// made drift-free: the query and each candidate are keyframes in their own sensor frames, described once (qn_kf_quatro_describe: voxel grid at `leaf` and FPFH
// with ctx's Quatro radii, kept resident) and registered in one qn_kf_verify_loop_candidates_c2f on ctx (its NanoGICP and Quatro parameters).  Keyframes not yet
// described under ctx's radii are described here first, in one call.  In loopTimerFunc the loop factor is then BetweenFactor(latest, c, inv(T), score).
inline std::vector<ScVerifiedC2f> verifyScanContextCandidatesCoarseToFine(qn_kf_store* store, qn_ctx* ctx, int query, const ScCandidates& c, double leaf, double score_thr) {
  std::vector<ScVerifiedC2f> out;
  if (c.idx.empty()) return out;
  const size_t K = c.idx.size();
  std::vector<int32_t> ids(c.idx.begin(), c.idx.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<double> Tt(16 * K), Tq(16 * K);
  std::vector<int> valid(K), status(K);
  int rc = qn_kf_verify_loop_candidates_c2f(store, ctx, query, ids.data(), (uint32_t)K, score_thr, r.data(), Tt.data(), Tq.data(), valid.data(), status.data());
  if (rc == QN_ERR_INVALID_ARG) {                  // (a keyframe not described yet, or under other radii: describe the query and every candidate, then once more)
    std::vector<int32_t> all(ids); all.push_back(query);
    std::vector<int> st(all.size());
    rc = qn_kf_quatro_describe(store, ctx, all.data(), (uint32_t)all.size(), leaf, st.data());
    if (rc == QN_OK) rc = qn_kf_verify_loop_candidates_c2f(store, ctx, query, ids.data(), (uint32_t)K, score_thr, r.data(), Tt.data(), Tq.data(), valid.data(), status.data());
  }
  detail::check(store, rc, "qn_kf_verify_loop_candidates_c2f");
  for (size_t k = 0; k < K; k++) {
    ScVerifiedC2f v{c.idx[k], valid[k] != 0, r[k].fitness, {}, {}, status[k]};
    for (int i = 0; i < 16; i++) { v.T[i] = Tt[16 * k + i]; v.T_quatro[i] = Tq[16 * k + i]; }
    out.push_back(v);
  }
  return out;
}

struct ScPairs {                                   // flat (query, candidate) pairs, every query's candidates together, nearest first
  std::vector<int> query;                          // the query's keyframe index
  std::vector<int> cand;                           // the candidate's keyframe index
  std::vector<double> dist;                        // Scan Context distance D in [0, 2]
  std::vector<double> yaw;                         // candidate heading minus query heading [rad], in [-pi, pi)
};

// scanContextCandidates for many queries (the keyframes added since the last loop-timer tick) in ONE qn_kf_sc_query: each query is described (a no-op when
// its descriptor exists) and ranked against the keyframes older than it by more than tdiff; the kept candidates (D < max_dist) come back as flat pairs.
inline ScPairs scanContextCandidatesMany(qn_kf_store* store, const std::vector<double>& stamps, const std::vector<int>& queries, double tdiff, int top_k, double max_dist) {
  if (top_k <= 0) throw std::invalid_argument("[qn_map] scanContextCandidatesMany: top_k must be positive");
  ScPairs out;
  if (queries.empty()) return out;
  qn_sc_params p{};
  int rc = qn_kf_sc_get_params(store, &p);
  const std::vector<int32_t> q(queries.begin(), queries.end());
  const size_t nq = q.size(), k = (size_t)top_k;
  if (rc == QN_OK) rc = qn_kf_sc_describe(store, q.data(), (uint32_t)nq);
  std::vector<int32_t> ids(nq * k), shift(nq * k);
  std::vector<double> d(nq * k);
  std::vector<uint32_t> n(nq);
  if (rc == QN_OK) rc = qn_kf_sc_query(store, q.data(), (uint32_t)nq, stamps.data(), (uint32_t)stamps.size(), tdiff, (uint32_t)top_k, ids.data(), d.data(), shift.data(), n.data());
  detail::check(store, rc, "qn_kf_sc_query");
  const double pi = 3.14159265358979323846;
  for (size_t i = 0; i < nq; i++)
    for (uint32_t r = 0; r < n[i]; r++) {
      const size_t e = i * k + r;
      if (!(d[e] < max_dist)) continue;
      double yaw = std::fmod(-2.0 * pi * shift[e] / p.n_sectors + pi, 2.0 * pi);
      if (yaw < 0) yaw += 2.0 * pi;
      out.query.push_back(queries[i]); out.cand.push_back(ids[e]); out.dist.push_back(d[e]); out.yaw.push_back(yaw - pi);
    }
  return out;
}

struct ScVerifiedPair {
  int query;                                       // the query's keyframe index
  int idx;                                         // the candidate's keyframe index
  bool valid;                                      // loop_closure.cpp:129 (coarse to fine: and Quatro converged, :145-148)
  double score;                                    // fitness (of the fine stage)
  double T[16];                                    // row-major, query sensor frame -> candidate sensor frame: an estimate of inv(P_c) P_query
  double T_quatro[16];                             // the coarse estimate (coarse to fine only; identity otherwise)
  int status;                                      // QN_OK, or QN_ERR_EMPTY_CLOUD for an empty side
};

// verifyScanContextCandidates for every pair at once (qn_kf_verify_loop_pairs): one assembly of each distinct query scan and candidate window, one batched
// registration on ctx.  Pair j's result equals verifyScanContextCandidates of that pair alone.  In loopTimerFunc each query's best valid pair then gives
// BetweenFactor(query, c, inv(T), score).
inline std::vector<ScVerifiedPair> verifyLoopPairs(qn_kf_store* store, qn_ctx* ctx, const ScPairs& c, const std::vector<double>& poses16, int submap_range,
                                                   double leaf, double score_thr) {
  std::vector<ScVerifiedPair> out;
  if (c.cand.empty()) return out;
  if (submap_range < 0 || poses16.size() % 16 != 0 || c.query.size() != c.cand.size() || c.yaw.size() != c.cand.size())
    throw std::invalid_argument("[qn_map] verifyLoopPairs: bad submap_range, poses or pairs");
  const size_t K = c.cand.size();
  const std::vector<int32_t> q(c.query.begin(), c.query.end()), ids(c.cand.begin(), c.cand.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<int> valid(K), status(K);
  const int rc = qn_kf_verify_loop_pairs(store, ctx, q.data(), ids.data(), c.yaw.data(), (uint32_t)K, poses16.data(), (uint32_t)(poses16.size() / 16),
                                         (uint32_t)submap_range, leaf, score_thr, r.data(), valid.data(), status.data());
  detail::check(store, rc, "qn_kf_verify_loop_pairs");
  for (size_t k = 0; k < K; k++) {
    ScVerifiedPair v{c.query[k], c.cand[k], valid[k] != 0, r[k].fitness, {}, {}, status[k]};
    for (int i = 0; i < 16; i++) { v.T[i] = (double)r[k].T[i]; v.T_quatro[i] = i % 5 == 0 ? 1.0 : 0.0; }
    out.push_back(v);
  }
  return out;
}

// verifyScanContextCandidatesCoarseToFine for every pair at once (qn_kf_verify_loop_pairs_c2f): one run of the coarse-to-fine lanes from the resident
// features.  Keyframes not yet described under ctx's radii are described here first, in one call.
inline std::vector<ScVerifiedPair> verifyLoopPairsCoarseToFine(qn_kf_store* store, qn_ctx* ctx, const ScPairs& c, double leaf, double score_thr) {
  std::vector<ScVerifiedPair> out;
  if (c.cand.empty()) return out;
  if (c.query.size() != c.cand.size()) throw std::invalid_argument("[qn_map] verifyLoopPairsCoarseToFine: bad pairs");
  const size_t K = c.cand.size();
  const std::vector<int32_t> q(c.query.begin(), c.query.end()), ids(c.cand.begin(), c.cand.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<double> Tt(16 * K), Tq(16 * K);
  std::vector<int> valid(K), status(K);
  int rc = qn_kf_verify_loop_pairs_c2f(store, ctx, q.data(), ids.data(), (uint32_t)K, score_thr, r.data(), Tt.data(), Tq.data(), valid.data(), status.data());
  if (rc == QN_ERR_INVALID_ARG) {                  // (a keyframe not described yet, or under other radii: describe every query and candidate, then once more)
    std::vector<int32_t> all(ids); all.insert(all.end(), q.begin(), q.end());
    std::vector<int> st(all.size());
    rc = qn_kf_quatro_describe(store, ctx, all.data(), (uint32_t)all.size(), leaf, st.data());
    if (rc == QN_OK) rc = qn_kf_verify_loop_pairs_c2f(store, ctx, q.data(), ids.data(), (uint32_t)K, score_thr, r.data(), Tt.data(), Tq.data(), valid.data(), status.data());
  }
  detail::check(store, rc, "qn_kf_verify_loop_pairs_c2f");
  for (size_t k = 0; k < K; k++) {
    ScVerifiedPair v{c.query[k], c.cand[k], valid[k] != 0, r[k].fitness, {}, {}, status[k]};
    for (int i = 0; i < 16; i++) { v.T[i] = Tt[16 * k + i]; v.T_quatro[i] = Tq[16 * k + i]; }
    out.push_back(v);
  }
  return out;
}

// The reference's third mode (enable_submap_matching: the submap around the query against the submap around the candidate, loop_closure.cpp:70-84, 98-107) made
// drift-free: every keyframe's local submap is built once in that keyframe's own sensor frame (qn_kf_submap_describe: the keyframes within submap_range of it,
// each with inv(P_c) P_i, voxel grid at `leaf`; with_features also its FPFH rows under ctx's Quatro radii) and stays resident.  poses16 = 16 doubles per
// keyframe, raw odometry or corrected: only the relative poses inside a window matter.  Returns each id's status (QN_OK, QN_ERR_EMPTY_CLOUD, QN_ERR_CAPACITY).
inline std::vector<int> describeLocalSubmaps(qn_kf_store* store, qn_ctx* ctx, const std::vector<int>& ids, const std::vector<double>& poses16, int submap_range,
                                             double leaf, bool with_features) {
  std::vector<int> st(ids.size());
  if (ids.empty()) return st;
  if (submap_range < 0 || poses16.size() % 16 != 0) throw std::invalid_argument("[qn_map] describeLocalSubmaps: bad submap_range or poses");
  const std::vector<int32_t> id32(ids.begin(), ids.end());
  const int rc = qn_kf_submap_describe(store, ctx, id32.data(), (uint32_t)id32.size(), poses16.data(), (uint32_t)(poses16.size() / 16), (uint32_t)submap_range, leaf,
                                       with_features ? 1 : 0, st.data());
  detail::check(store, rc, "qn_kf_submap_describe");
  return st;
}

// every pair's described local submaps registered against each other in one batched Nano-GICP on ctx, seeded with the pair's Scan Context heading
// (qn_kf_verify_loop_pairs_submap).  The queries and candidates must have been described (describeLocalSubmaps).  T estimates inv(P_c) P_query.
inline std::vector<ScVerifiedPair> verifyLoopPairsSubmap(qn_kf_store* store, qn_ctx* ctx, const ScPairs& c, double score_thr) {
  std::vector<ScVerifiedPair> out;
  if (c.cand.empty()) return out;
  if (c.query.size() != c.cand.size() || c.yaw.size() != c.cand.size()) throw std::invalid_argument("[qn_map] verifyLoopPairsSubmap: bad pairs");
  const size_t K = c.cand.size();
  const std::vector<int32_t> q(c.query.begin(), c.query.end()), ids(c.cand.begin(), c.cand.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<int> valid(K), status(K);
  const int rc = qn_kf_verify_loop_pairs_submap(store, ctx, q.data(), ids.data(), c.yaw.data(), (uint32_t)K, score_thr, r.data(), valid.data(), status.data());
  detail::check(store, rc, "qn_kf_verify_loop_pairs_submap");
  for (size_t k = 0; k < K; k++) {
    ScVerifiedPair v{c.query[k], c.cand[k], valid[k] != 0, r[k].fitness, {}, {}, status[k]};
    for (int i = 0; i < 16; i++) { v.T[i] = (double)r[k].T[i]; v.T_quatro[i] = i % 5 == 0 ? 1.0 : 0.0; }
    out.push_back(v);
  }
  return out;
}

// the same pairs coarse to fine from the submaps' resident FPFH rows (qn_kf_verify_loop_pairs_submap_c2f); they must have been described with features
inline std::vector<ScVerifiedPair> verifyLoopPairsSubmapCoarseToFine(qn_kf_store* store, qn_ctx* ctx, const ScPairs& c, double score_thr) {
  std::vector<ScVerifiedPair> out;
  if (c.cand.empty()) return out;
  if (c.query.size() != c.cand.size()) throw std::invalid_argument("[qn_map] verifyLoopPairsSubmapCoarseToFine: bad pairs");
  const size_t K = c.cand.size();
  const std::vector<int32_t> q(c.query.begin(), c.query.end()), ids(c.cand.begin(), c.cand.end());
  std::vector<qn_gicp_result> r(K);
  std::vector<double> Tt(16 * K), Tq(16 * K);
  std::vector<int> valid(K), status(K);
  const int rc = qn_kf_verify_loop_pairs_submap_c2f(store, ctx, q.data(), ids.data(), (uint32_t)K, score_thr, r.data(), Tt.data(), Tq.data(), valid.data(), status.data());
  detail::check(store, rc, "qn_kf_verify_loop_pairs_submap_c2f");
  for (size_t k = 0; k < K; k++) {
    ScVerifiedPair v{c.query[k], c.cand[k], valid[k] != 0, r[k].fitness, {}, {}, status[k]};
    for (int i = 0; i < 16; i++) { v.T[i] = Tt[16 * k + i]; v.T_quatro[i] = Tq[16 * k + i]; }
    out.push_back(v);
  }
  return out;
}

// the two-way overlap of every pair of the latest verifyLoopPairs* call on `store` (qn_kf_verify_overlap): the pair's aligned source against its target, each
// way, within `radius`.  n_pairs = the size of that call's result.  A loop whose overlaps are small either way is a false positive whatever its score says;
// the inlier RMSE is a natural scale for the loop factor's noise.  status: QN_ERR_NOT_READY for a pair whose registration did not run (a zero record).
struct VerifiedOverlap { qn_overlap rec; int status; };
inline double overlapFraction(const qn_overlap_dir& d) { return d.n_finite ? (double)d.inliers / (double)d.n_finite : 0.0; }
inline double inlierRmse(const qn_overlap_dir& d) { return d.inliers ? std::sqrt(d.sum_d2 / (double)d.inliers) : 0.0; }
inline std::vector<VerifiedOverlap> verifyOverlap(qn_kf_store* store, size_t n_pairs, double radius) {
  std::vector<VerifiedOverlap> out;
  if (n_pairs == 0) return out;
  std::vector<qn_overlap> rec(n_pairs);
  std::vector<int> status(n_pairs);
  const int rc = qn_kf_verify_overlap(store, nullptr, (uint32_t)n_pairs, radius, rec.data(), status.data());
  detail::check(store, rc, "qn_kf_verify_overlap");
  for (size_t k = 0; k < n_pairs; k++) out.push_back(VerifiedOverlap{rec[k], status[k]});
  return out;
}

}  // namespace qn_map
