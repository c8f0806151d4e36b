// Drop-in helper for the question that decides between two frontier regions: standing here, how much unknown space would the sensor actually see?  Where a user
// of the reference would download the class volume and cast the sensor's rays on the host for every candidate at every replanning tick, mapViewGain casts them
// over the latest qn_map::mapOccupancy on the GPU - from each viewpoint every ray of the table until an occupied voxel, the grid's face or its end, counting the
// distinct unknown voxels passed through - and keeps the cover volume there; sensorRays makes the table of a spinning sensor, viewCover downloads, per voxel,
// the number of viewpoints that would see it.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapViewGain {
  qn_view_stats stats;
  qn_view_params params;
  qn_occupancy_grid grid;                                          // the occupancy map's: origin, voxel, width along x, height along y, depth along z
  std::vector<qn_view_info> views;                                 // one row per viewpoint: status, gain, the four ray ends, the grid voxel, steps
  size_t voxels() const { return (size_t)grid.width * grid.height * grid.depth; }
  // the viewpoint with the largest gain (the first on a tie), -1 when every viewpoint is OUTSIDE
  int best() const {
    int b = -1;
    for (size_t k = 0; k < views.size(); k++)
      if (views[k].status == QN_VIEW_OK && (b < 0 || views[k].gain > views[(size_t)b].gain)) b = (int)k;
    return b;
  }
};

// The ray table of a spinning sensor, beam-major (row = beam * n_azimuth + azimuth step): n_beams elevations from elev_lo_deg to elev_hi_deg, ends included,
// n_azimuth steps of a full turn, direction (cos e cos a, cos e sin a, sin e), offset = rint(direction * (max_range / voxel) * 1024): three int32 a ray, in the
// occupancy map's fixed point (qn_amd/mapview.py sensor_offsets).  The table is made once and reused for every call.
inline std::vector<int32_t> sensorRays(double voxel, double max_range, uint32_t n_beams, uint32_t n_azimuth, double elev_lo_deg, double elev_hi_deg) {
  if (!(voxel > 0.0) || !(max_range > 0.0) || !std::isfinite(voxel) || !std::isfinite(max_range)) throw std::invalid_argument("[qn_map] sensorRays: voxel and max_range finite and > 0");
  if (n_beams == 0 || n_azimuth == 0 || (uint64_t)n_beams * n_azimuth > (1u << 20)) throw std::invalid_argument("[qn_map] sensorRays: 1 .. 2^20 rays");
  const double scale = max_range / voxel * 1024.0, pi = 3.14159265358979323846;
  if (!(std::rint(scale) <= (double)QN_VIEW_MAX_OFFSET)) throw std::invalid_argument("[qn_map] sensorRays: max_range / voxel beyond the offset limit 2^25 / 1024");
  std::vector<int32_t> out(3 * (size_t)n_beams * n_azimuth);
  for (uint32_t b = 0; b < n_beams; b++) {
    const double e = (n_beams > 1 ? elev_lo_deg + (elev_hi_deg - elev_lo_deg) * (double)b / (double)(n_beams - 1) : elev_lo_deg) * pi / 180.0;
    for (uint32_t j = 0; j < n_azimuth; j++) {
      const double a = 2.0 * pi * (double)j / (double)n_azimuth;
      int32_t* o = &out[3 * ((size_t)b * n_azimuth + j)];
      o[0] = (int32_t)std::rint(std::cos(e) * std::cos(a) * scale); o[1] = (int32_t)std::rint(std::cos(e) * std::sin(a) * scale); o[2] = (int32_t)std::rint(std::sin(e) * scale);
    }
  }
  return out;
}

// the view gain of the viewpoints xyz (three doubles each, world coordinates) under the ray table `rays` (three int32 each: sensorRays) over the latest
// mapOccupancy (qn_kf_map_view_gain).  params NULL: the defaults (gain: the unknown voxels, stop: the occupied ones, no limit on the voxels passed through,
// every layer).  The result stays resident until the next mapViewGain or mapOccupancy; mapDistance, mapRoute and mapFrontiers do not touch it.
inline MapViewGain mapViewGain(qn_kf_store* store, const std::vector<double>& xyz, const std::vector<int32_t>& rays, const qn_view_params* params = nullptr) {
  qn_view_params p = detail::params_or(params, qn_view_default_params);
  if (xyz.empty() || xyz.size() % 3 != 0 || xyz.size() / 3 > (1u << 16)) throw std::invalid_argument("[qn_map] mapViewGain: three doubles per viewpoint, 1 .. 2^16 viewpoints");
  if (rays.empty() || rays.size() % 3 != 0 || rays.size() / 3 > (1u << 20)) throw std::invalid_argument("[qn_map] mapViewGain: three offsets per ray, 1 .. 2^20 rays");
  if (p.iz_lo > p.iz_hi) throw std::invalid_argument("[qn_map] mapViewGain: iz_lo <= iz_hi");
  if (p.gain_mask & p.stop_mask) throw std::invalid_argument("[qn_map] mapViewGain: gain_mask and stop_mask share a class");
  for (int32_t v : rays)
    if (v > QN_VIEW_MAX_OFFSET || v < -QN_VIEW_MAX_OFFSET) throw std::invalid_argument("[qn_map] mapViewGain: an offset beyond QN_VIEW_MAX_OFFSET");
  MapViewGain out;
  out.views.resize(xyz.size() / 3);
  int rc = qn_kf_map_view_gain(store, xyz.data(), (uint32_t)(xyz.size() / 3), rays.data(), (uint32_t)(rays.size() / 3), &p, out.views.data(), &out.stats);
  detail::check(store, rc, "qn_kf_map_view_gain");
  rc = qn_kf_map_view_grid(store, &out.grid, &out.params, nullptr);
  detail::check(store, rc, "qn_kf_map_view_grid");
  return out;
}

// per voxel the number of viewpoints of the latest mapViewGain that marked it, W H D values, x fastest (qn_kf_map_view_grid)
inline std::vector<uint32_t> viewCover(qn_kf_store* store) {
  qn_occupancy_grid g; qn_view_params p;
  int rc = qn_kf_map_view_grid(store, &g, &p, nullptr);
  detail::check(store, rc, "qn_kf_map_view_grid");
  std::vector<uint32_t> out((size_t)g.width * g.height * g.depth);
  if (out.empty()) return out;
  rc = qn_kf_map_view_grid(store, &g, &p, out.data());
  detail::check(store, rc, "qn_kf_map_view_grid");
  return out;
}

}  // namespace qn_map
