// Drop-in helper for LoopClosure::setSrcAndDstCloud (fast_lio_sam_qn/src/loop_closure.cpp:58-108) when a query is registered against K
// candidates at once.  The keyframe lists follow the reference line by line (loopSubmapIds); the query's submap is assembled ONCE and every
// candidate's submap beside it in a single qn_kf_assemble_batch call on the keyframe store, and the result is a qn_pair_desc per candidate,
// all naming the same source buffer, so qn_gicp_align_batch / qn_coarse_to_fine_align_batch prepare the query cloud once (batch_share_source).
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Builds against real Eigen and against the stand-ins in
// tests/standins: it only uses Matrix4d's (row, col) accessor.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include <Eigen/Core>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct SubmapIds { std::vector<int32_t> src, dst; };

// setSrcAndDstCloud's keyframe lists: a submap takes keyframes [idx - submap_range, idx + submap_range] that exist, except the newest
// (`i < keyframes.size() - 1`, loop_closure.cpp:74,81,100); without submap matching the source is src_idx alone, and with Quatro so is the destination.
inline SubmapIds loopSubmapIds(int src_idx, int dst_idx, int submap_range, bool enable_quatro, bool enable_submap_matching, int n_keyframes) {
  SubmapIds r;
  auto around = [&](int c, std::vector<int32_t>& out) {
    for (int i = c - submap_range; i < c + submap_range + 1; ++i)
      if (i >= 0 && i < n_keyframes - 1) out.push_back(i);
  };
  if (enable_submap_matching) {
    around(src_idx, r.src);
    around(dst_idx, r.dst);
  } else {
    r.src.push_back(src_idx);
    if (enable_quatro) r.dst.push_back(dst_idx);
    else around(dst_idx, r.dst);
  }
  return r;
}

// The query's submap and one per candidate, in one qn_kf_assemble_batch on `store`, whose keyframe ids are the keyframe indices (poses[i] =
// keyframes[i].pose_corrected_eig_, poses.size() keyframes).  Returns one on-device pair per candidate (src = the query's submap, dst = the
// candidate's); status, if given, receives the query submap's status followed by each candidate's (QN_ERR_EMPTY_CLOUD: no finite point, n = 0).
// The pointers stay valid until the next qn_kf_assemble_batch on the store.
inline std::vector<qn_pair_desc> loopSubmapPairs(qn_kf_store* store, const std::vector<Eigen::Matrix4d>& poses, int query, const std::vector<int>& candidates,
                                                 int submap_range, double leaf, bool enable_quatro, bool enable_submap_matching, std::vector<int>* status = nullptr) {
  const int n_kf = (int)poses.size();
  std::vector<int32_t> ids; std::vector<uint32_t> seg_off(1, 0);
  const SubmapIds q = loopSubmapIds(query, query, submap_range, enable_quatro, enable_submap_matching, n_kf);
  ids.insert(ids.end(), q.src.begin(), q.src.end()); seg_off.push_back((uint32_t)ids.size());
  for (int c : candidates) {
    const SubmapIds d = loopSubmapIds(query, c, submap_range, enable_quatro, enable_submap_matching, n_kf);
    ids.insert(ids.end(), d.dst.begin(), d.dst.end()); seg_off.push_back((uint32_t)ids.size());
  }
  std::vector<double> T(16 * ids.size());
  for (size_t k = 0; k < ids.size(); k++) {
    if (ids[k] < 0 || ids[k] >= n_kf) throw std::out_of_range("[qn_map] keyframe index " + std::to_string(ids[k]));
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[16 * k + 4 * r + c] = poses[ids[k]](r, c);
  }
  const uint32_t S = (uint32_t)candidates.size() + 1;
  std::vector<const float*> ptr(S); std::vector<uint32_t> n(S); std::vector<int> st(S);
  const int rc = qn_kf_assemble_batch(store, ids.data(), T.data(), seg_off.data(), S, leaf, ptr.data(), n.data(), st.data());
  detail::check(store, rc, "qn_kf_assemble_batch");
  if (status) *status = st;
  std::vector<qn_pair_desc> pairs(candidates.size());
  for (size_t k = 0; k < candidates.size(); k++) pairs[k] = qn_pair_desc{ptr[0], n[0], ptr[k + 1], n[k + 1], 16u, 1};
  return pairs;
}

}  // namespace qn_map
