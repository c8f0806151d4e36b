// Drop-in helper for the static map: the corrected global map of FastLioSamQn (fast_lio_sam_qn.cpp:302-316 visTimerFunc, :398-411 saveFlagCallback) without
// the ghost trails of whatever moved while the sensor drove past.  A record of one keyframe is dropped when, carried with the corrected poses into its
// neighbours' sensor frames, at least min_see_through of them saw THROUGH the place it occupies (and more of them than agree with it): the free-space check of
// freespace.hpp taken many to many, on the keyframes' resident records and range images.  Describe each keyframe's range images once, when it is added
// (describeRangeImages); at the call sites above, call classifyStatic with every keyframe and its corrected pose, then buildStaticMap where the reference runs
// voxelizePcd, and fetch the map with qn_kf_download_map as after qn_kf_build_map.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct StaticWitnesses { std::vector<uint32_t> off, wit; };      // entry e's witnesses: wit[off[e] .. off[e + 1]), list positions

// the default witness list (qn_amd.staticmap.witnesses): for entry e the up to max_k other entries of another keyframe whose translation lies within `radius`
// of e's - squared f64 distance, summed x, y, z in order - ascending distance, ties to the lower position.  poses16: 16 doubles per entry, row-major,
// sensor -> world.  Host code, O(count^2).
inline StaticWitnesses staticMapWitnesses(const std::vector<int>& ids, const std::vector<double>& poses16, double radius, uint32_t max_k) {
  if (poses16.size() != 16 * ids.size()) throw std::invalid_argument("[qn_map] staticMapWitnesses: 16 doubles per entry");
  if (max_k > 255) throw std::invalid_argument("[qn_map] staticMapWitnesses: at most 255 witnesses per entry");
  StaticWitnesses out;
  out.off.push_back(0);
  const double r2 = radius * radius;
  std::vector<std::pair<double, uint32_t>> c;
  for (size_t e = 0; e < ids.size(); e++) {
    c.clear();
    for (size_t w = 0; w < ids.size(); w++) {
      if (ids[w] == ids[e]) continue;
      const double dx = poses16[16 * w + 3] - poses16[16 * e + 3], dy = poses16[16 * w + 7] - poses16[16 * e + 7], dz = poses16[16 * w + 11] - poses16[16 * e + 11];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= r2) c.emplace_back(d2, (uint32_t)w);
    }
    std::sort(c.begin(), c.end());
    for (size_t k = 0; k < c.size() && k < max_k; k++) out.wit.push_back(c[k].second);
    out.off.push_back((uint32_t)out.wit.size());
  }
  return out;
}

struct StaticClassified { std::vector<uint32_t> removed; std::vector<int> status; };      // per entry: its removed records, QN_ERR_EMPTY_CLOUD without records
// every record of every listed keyframe against the range images of its entry's witnesses, in one pass (qn_kf_static_classify); params NULL: the defaults
inline StaticClassified classifyStatic(qn_kf_store* store, const std::vector<int>& ids, const std::vector<double>& poses16, const StaticWitnesses& w,
                                       const qn_static_params* params = nullptr) {
  if (poses16.size() != 16 * ids.size() || w.off.size() != ids.size() + 1) throw std::invalid_argument("[qn_map] classifyStatic: 16 doubles and one witness range per entry");
  StaticClassified out;
  if (ids.empty()) return out;
  qn_static_params p = detail::params_or(params, qn_static_default_params);
  std::vector<int32_t> id32(ids.begin(), ids.end());
  out.removed.resize(ids.size()); out.status.resize(ids.size());
  const int rc = qn_kf_static_classify(store, id32.data(), poses16.data(), (uint32_t)id32.size(), w.off.data(), w.wit.empty() ? nullptr : w.wit.data(), &p,
                                       out.removed.data(), out.status.data());
  detail::check(store, rc, "qn_kf_static_classify");
  return out;
}

// the static map of the latest classifyStatic at `leaf`, into the store's map slot -> its number of points (0: nothing left); qn_kf_download_map fetches it
inline uint32_t buildStaticMap(qn_kf_store* store, double leaf) {
  const float* d_map = nullptr; uint32_t n = 0;
  const int rc = qn_kf_build_map_static(store, leaf, &d_map, &n);
  if (rc == QN_ERR_EMPTY_CLOUD) return 0;
  detail::check(store, rc, "qn_kf_build_map_static");
  return n;
}

}  // namespace qn_map
