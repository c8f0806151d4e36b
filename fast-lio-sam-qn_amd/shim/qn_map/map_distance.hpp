// Drop-in helper for the clearance a planner asks of the occupancy map: where a user of the reference would download the volume and run a host distance
// transform, mapDistance computes the exact Euclidean distance field of the latest qn_map::mapOccupancy on the GPU - per voxel the squared distance, in voxels,
// to the nearest occupied (or, by the mask, unknown) voxel - and keeps it there; distanceSlice fetches the clearance of an upright body over a band of layers
// as a 2-D grid, distanceAt the distance in metres at world points.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapDistance {
  qn_distance_stats stats;
  qn_distance_params params;
  qn_occupancy_grid grid;                                          // the occupancy map's: origin, voxel, width along x, height along y, depth along z
  size_t voxels() const { return (size_t)grid.width * grid.height * grid.depth; }
  // a squared distance in voxels as metres; QN_DIST_FAR (beyond max_dist, or no site at all): infinity
  double metres(uint16_t d2) const { return d2 == QN_DIST_FAR ? std::numeric_limits<double>::infinity() : std::sqrt((double)d2) * grid.voxel; }
  // the largest squared distance in voxels a body of radius r metres still collides at: floor((r / voxel)^2), for comparing with d2
  uint32_t radius2(double r) const { const double q = r / grid.voxel; return (uint32_t)std::floor(q * q); }
};

// the distance field of the latest mapOccupancy (qn_kf_map_distance).  params NULL: the defaults (sites: the occupied voxels, max_dist 16 voxels); unknown space
// as an obstacle: site_mask = (1u << QN_OCC_OCCUPIED) | (1u << QN_OCC_UNKNOWN).  The field stays resident until the next mapDistance or mapOccupancy.
inline MapDistance mapDistance(qn_kf_store* store, const qn_distance_params* params = nullptr) {
  qn_distance_params p = detail::params_or(params, qn_distance_default_params);
  if (p.max_dist < 1 || p.max_dist > QN_DIST_MAX_RADIUS) throw std::invalid_argument("[qn_map] mapDistance: max_dist of 1 .. 255 voxels");
  MapDistance out;
  int rc = qn_kf_map_distance(store, &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_distance");
  rc = qn_kf_map_distance_grid(store, &out.grid, &out.params, nullptr);
  detail::check(store, rc, "qn_kf_map_distance_grid");
  return out;
}

// per column the smallest squared distance over the layers iz_lo .. iz_hi (inclusive, clipped to the grid; QN_DIST_FAR when the band misses it): row-major with
// y the slow axis, width x height of the occupancy grid (qn_kf_map_distance_slice).  MapOccupancy::layerOf gives the layer of a world height.
inline std::vector<uint16_t> distanceSlice(qn_kf_store* store, int32_t iz_lo, int32_t iz_hi, qn_occupancy_grid* grid = nullptr) {
  qn_occupancy_grid g; qn_distance_params p;
  int rc = qn_kf_map_distance_grid(store, &g, &p, nullptr);
  detail::check(store, rc, "qn_kf_map_distance_grid");
  std::vector<uint16_t> d2((size_t)g.width * g.height);
  std::vector<uint16_t> pad(1);
  rc = qn_kf_map_distance_slice(store, iz_lo, iz_hi, d2.empty() ? pad.data() : d2.data());
  detail::check(store, rc, "qn_kf_map_distance_slice");
  if (grid) *grid = g;
  return d2;
}

// the distance in metres to the nearest site at the world points xyz (3 doubles each): infinity beyond max_dist and for a point outside the grid
// (qn_kf_map_distance_query); classes (optional): the class of each point's voxel, QN_DIST_OUTSIDE outside
inline std::vector<double> distanceAt(qn_kf_store* store, const std::vector<double>& xyz, std::vector<uint8_t>* classes = nullptr) {
  if (xyz.empty() || xyz.size() % 3 != 0) throw std::invalid_argument("[qn_map] distanceAt: 3 doubles per point, at least one point");
  qn_occupancy_grid g; qn_distance_params p;
  int rc = qn_kf_map_distance_grid(store, &g, &p, nullptr);
  detail::check(store, rc, "qn_kf_map_distance_grid");
  const uint32_t n = (uint32_t)(xyz.size() / 3);
  std::vector<uint16_t> d2(n); std::vector<uint8_t> cls(n);
  rc = qn_kf_map_distance_query(store, xyz.data(), n, d2.data(), cls.data());
  detail::check(store, rc, "qn_kf_map_distance_query");
  std::vector<double> out(n);
  for (uint32_t i = 0; i < n; i++) out[i] = d2[i] == QN_DIST_FAR ? std::numeric_limits<double>::infinity() : std::sqrt((double)d2[i]) * g.voxel;
  if (classes) classes->swap(cls);
  return out;
}

}  // namespace qn_map
