// Drop-in helper for the outlier filter of the corrected global map: after qn_kf_build_map / buildStaticMap, where a user of the reference would run
// pcl::StatisticalOutlierRemoval or pcl::RadiusOutlierRemoval over the saved map on the host, mapOutliers classifies every point of the resident map on the
// GPU and removeMapOutliers drops the outliers from it in place; mapNormals and qn_kf_download_map then serve the filtered map.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapOutliers {
  qn_outlier_stats stats;
  std::vector<uint32_t> neighbors;                                 // per map point: its neighbours within the radius (the point itself not counted)
  std::vector<uint32_t> mean_q;                                    // per map point: the mean distance to its k nearest, in units of 2^-quant_exp m (0xffffffff: none)
  std::vector<uint8_t> removed;                                    // per map point: 1 = an outlier
  size_t size() const { return removed.size(); }
  double metres(double q) const { return std::ldexp(q, -stats.quant_exp); }      // mean_q, stats.mean_q / std_q / thr_q in metres
};

// the classification of the store's map slot (qn_kf_map_outliers); the slot is not touched.  params NULL: the defaults (radius 1.0, std_mul 2.0, k 8)
inline MapOutliers mapOutliers(qn_kf_store* store, const qn_outlier_params* params) {
  qn_outlier_params p = detail::params_or(params, qn_outlier_default_params);
  MapOutliers out;
  int rc = qn_kf_map_outliers(store, &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_outliers");
  const uint32_t n = out.stats.n;
  out.neighbors.resize(n); out.mean_q.resize(n); out.removed.resize(n);
  if (!n) return out;
  rc = qn_kf_map_outlier_points(store, out.neighbors.data(), out.mean_q.data(), out.removed.data());
  detail::check(store, rc, "qn_kf_map_outlier_points");
  return out;
}

// applies the latest mapOutliers to the map slot (qn_kf_map_remove_outliers) -> the points left; d_xyzi (optional): the device address of their float4 records
inline uint32_t removeMapOutliers(qn_kf_store* store, const float** d_xyzi = nullptr) {
  const float* d = nullptr; uint32_t n = 0;
  const int rc = qn_kf_map_remove_outliers(store, &d, &n);
  detail::check(store, rc, "qn_kf_map_remove_outliers");
  if (d_xyzi) *d_xyzi = d;
  return n;
}

}  // namespace qn_map
