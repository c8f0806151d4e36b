// Drop-in helper for a free-space (see-through) veto after the loop verification of FastLioSamQn::loopTimerFunc (fast_lio_sam_qn.cpp:203-252): every verified
// pair's transform is checked against the two keyframes' range images.  A point of one scan that sits, under the transform, where the other scan's rays
// passed on their way to a farther surface contradicts that scan; a high share of such points in either direction says the transform is wrong whatever the
// score and the overlap say - and unlike those it does not depend on the partners the registration itself chose.  Keyframes are in their sensor frames
// (PosePcd::pcd_), which is the frame the images are made in: describe each keyframe once, when it is added.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

// the near / far range images of these keyframes under the store's range parameters (qn_kf_range_set_params), kept resident -> per keyframe its status
// (QN_ERR_EMPTY_CLOUD: no point inside the field of view, an all-empty image)
inline std::vector<int> describeRangeImages(qn_kf_store* store, const std::vector<int>& ids) {
  std::vector<int> status(ids.size());
  if (ids.empty()) return status;
  std::vector<int32_t> id32(ids.begin(), ids.end());
  const int rc = qn_kf_range_describe(store, id32.data(), (uint32_t)id32.size(), status.data());
  detail::check(store, rc, "qn_kf_range_describe");
  return status;
}

// seen_through / observed of one direction, 0 when nothing was observed
inline double seeThroughFraction(const qn_freespace_dir& d) { return d.observed ? (double)d.seen_through / (double)d.observed : 0.0; }

struct FreespaceChecked { qn_freespace rec; int status; };
// pair j = (query[j], cand[j]) with T16[16 j ..] = the row-major 4x4 that maps the query's sensor frame into the candidate's (ScVerified::T, or T_total of the
// coarse-to-fine calls): both directions of every pair in one pass (qn_kf_freespace_batch).  Reject a loop when seeThroughFraction of either direction
// exceeds a few percent.
inline std::vector<FreespaceChecked> freespaceBatch(qn_kf_store* store, const std::vector<int>& query, const std::vector<int>& cand, const std::vector<double>& T16) {
  if (query.size() != cand.size() || T16.size() != 16 * query.size()) throw std::invalid_argument("[qn_map] freespaceBatch: one candidate and 16 doubles per query");
  std::vector<FreespaceChecked> out;
  if (query.empty()) return out;
  std::vector<int32_t> q(query.begin(), query.end()), c(cand.begin(), cand.end());
  std::vector<qn_freespace> rec(q.size());
  std::vector<int> status(q.size());
  const int rc = qn_kf_freespace_batch(store, q.data(), c.data(), T16.data(), (uint32_t)q.size(), rec.data(), status.data());
  detail::check(store, rc, "qn_kf_freespace_batch");
  for (size_t k = 0; k < q.size(); k++) out.push_back(FreespaceChecked{rec[k], status[k]});
  return out;
}

}  // namespace qn_map
