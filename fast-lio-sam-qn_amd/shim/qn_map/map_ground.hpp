// Drop-in helper for the ground of the corrected global map and its 2-D occupancy grid: after qn_kf_build_map / buildStaticMap / removeMapOutliers, where a
// user of the reference would run a ground filter and a pcd-to-pgm tool over the saved map on the host, mapGround classifies every point of the resident map
// on the GPU (ground, obstacle, overhead), occupancyGrid fetches the grid a planner or map_server loads, and keepClasses drops classes from the map in place;
// mapNormals, mapOutliers and qn_kf_download_map then serve the kept map.
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

struct MapGround {
  qn_ground_stats stats;
  std::vector<uint8_t> classes;                                    // per map point: QN_GROUND_NONE / _GROUND / _OBSTACLE / _OVERHEAD / _BELOW
  std::vector<int32_t> height_q;                                   // per map point: its height above the ground envelope in units of 2^-quant_exp m (INT32_MIN: none)
  size_t size() const { return classes.size(); }
  double metres(double q) const { return std::ldexp(q, -stats.quant_exp); }
};

struct OccupancyGrid {
  qn_ground_grid info;                                             // origin_x / origin_y: the corner of cell (0, 0); cell; width along x, height along y
  std::vector<int32_t> ground_q;                                   // row-major, y the slow axis: the ground envelope in units of 2^-quant_exp m (INT32_MAX: none)
  std::vector<uint8_t> occupancy;                                  // 0 unknown, 1 free, 2 occupied
  uint8_t at(uint32_t ix, uint32_t iy) const { return occupancy[(size_t)iy * info.width + ix]; }
};

// the classes of the store's map slot (qn_kf_map_ground); the slot is not touched.  params NULL: the defaults (cell 0.5, slope 0.3, tolerance 0.2, clearance 2.0)
inline MapGround mapGround(qn_kf_store* store, const qn_ground_params* params) {
  qn_ground_params p = detail::params_or(params, qn_ground_default_params);
  MapGround out;
  int rc = qn_kf_map_ground(store, &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_ground");
  const uint32_t n = out.stats.n;
  out.classes.resize(n); out.height_q.resize(n);
  if (!n) return out;
  rc = qn_kf_map_ground_points(store, out.classes.data(), out.height_q.data());
  detail::check(store, rc, "qn_kf_map_ground_points");
  return out;
}

// the occupancy grid of the latest mapGround (qn_kf_map_ground_grid)
inline OccupancyGrid occupancyGrid(qn_kf_store* store) {
  OccupancyGrid g;
  int rc = qn_kf_map_ground_grid(store, &g.info, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_ground_grid");
  const size_t cells = (size_t)g.info.width * g.info.height;
  g.ground_q.resize(cells); g.occupancy.resize(cells);
  if (!cells) return g;
  rc = qn_kf_map_ground_grid(store, &g.info, g.ground_q.data(), g.occupancy.data());
  detail::check(store, rc, "qn_kf_map_ground_grid");
  return g;
}

// the records of the classes in class_mask (bit 1 << class) become the map slot, in order (qn_kf_map_keep_classes) -> the points left;
// d_xyzi (optional): the device address of their float4 records.  Everything but the ground: ~(1u << QN_GROUND_GROUND) & 31.
inline uint32_t keepClasses(qn_kf_store* store, uint32_t class_mask, const float** d_xyzi = nullptr) {
  const float* d = nullptr; uint32_t n = 0;
  const int rc = qn_kf_map_keep_classes(store, class_mask, &d, &n);
  detail::check(store, rc, "qn_kf_map_keep_classes");
  if (d_xyzi) *d_xyzi = d;
  return n;
}

}  // namespace qn_map
