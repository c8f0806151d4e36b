// Drop-in helper for the candidate step of FastLioSamQn::loopTimerFunc (fast_lio_sam_qn.cpp:203-252) when candidates come from Scan Context
// place descriptors instead of LoopClosure::fetchClosestKeyframeIdx's radius search on drifted poses (loop_closure.cpp:34-56).  The query's
// descriptor is made on the GPU from its resident keyframe (qn_kf_sc_describe, a no-op when it exists), the older keyframes' descriptors
// must already exist (describe each keyframe once, when it is added), and qn_kf_sc_query ranks them.  The indices feed
// qn_map::loopSubmapPairs (loop_submaps.hpp) and the batched registrations; yaw is the candidate's heading minus the query's, from the
// best column shift, for callers that want an initial rotation.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"

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
  if (rc != QN_OK) throw std::runtime_error(std::string("[qn_map] qn_kf_sc_query: ") + qn_status_str(rc) + " " + qn_kf_last_error(store));
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

}  // namespace qn_map
