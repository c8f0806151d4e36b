// Drop-in helper for the second question a planner asks of the occupancy map: how far is it from here to there through free space with a given clearance,
// and along which voxels.  Where a user of the reference would download the volume and its distance field and run a shortest-path search on the host, mapRoute
// computes the cost-to-go field to a set of goals over the latest qn_map::mapOccupancy and qn_map::mapDistance on the GPU - per voxel the smallest 3-4-5
// chamfer path cost through passable voxels, no corner cut - and keeps it there; routeCostAt reads it at world points in metres, routePath walks the paths
// from world points down to a goal.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapRoute {
  qn_route_stats stats;
  qn_route_params params;
  qn_occupancy_grid grid;                                          // the occupancy map's: origin, voxel, width along x, height along y, depth along z
  uint32_t depth() const { return params.planar ? (grid.width && grid.height ? 1u : 0u) : grid.depth; }      // the field's: one layer of columns in planar mode
  size_t cells() const { return (size_t)grid.width * grid.height * depth(); }
  // a cost as metres: cost / 3 * voxel; QN_ROUTE_BLOCKED and QN_ROUTE_UNREACHED: infinity
  double metres(uint32_t cost) const { return cost >= QN_ROUTE_BLOCKED ? std::numeric_limits<double>::infinity() : (double)cost / 3.0 * grid.voxel; }
  // the centre of field voxel (i, j, k) in world coordinates; in planar mode z is the middle of the band's layers inside the grid
  std::array<double, 3> centre(int32_t i, int32_t j, int32_t k) const {
    std::array<double, 3> c = {(grid.minc[0] + i + 0.5) * grid.voxel, (grid.minc[1] + j + 0.5) * grid.voxel, (grid.minc[2] + k + 0.5) * grid.voxel};
    if (params.planar) {
      const int64_t lo = params.iz_lo > 0 ? params.iz_lo : 0, hi = params.iz_hi < (int64_t)grid.depth - 1 ? params.iz_hi : (int64_t)grid.depth - 1;
      c[2] = lo <= hi ? (grid.minc[2] + 0.5 * (double)(lo + hi + 1)) * grid.voxel : std::numeric_limits<double>::quiet_NaN();
    }
    return c;
  }
};

// one path of routePath: its true number of voxels and the first min(len, max_len) of them, (i, j, k) each
struct RoutePath {
  uint32_t len = 0;
  std::vector<std::array<int32_t, 3>> voxels;
};

// the cost-to-go field to `goals` (3 doubles per world point) over the latest mapOccupancy and mapDistance (qn_kf_map_route).  params NULL: the defaults (pass:
// the free voxels, min_d2 4, every layer, 3-D).  The field stays resident until the next mapRoute, mapDistance or mapOccupancy.
inline MapRoute mapRoute(qn_kf_store* store, const std::vector<double>& goals, const qn_route_params* params = nullptr) {
  if (goals.empty() || goals.size() % 3 != 0) throw std::invalid_argument("[qn_map] mapRoute: 3 doubles per goal, at least one goal");
  qn_route_params p = detail::params_or(params, qn_route_default_params);
  if (p.iz_lo > p.iz_hi) throw std::invalid_argument("[qn_map] mapRoute: iz_lo <= iz_hi");
  MapRoute out;
  int rc = qn_kf_map_route(store, goals.data(), (uint32_t)(goals.size() / 3), &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_route");
  rc = qn_kf_map_route_grid(store, &out.grid, &out.params, nullptr);
  detail::check(store, rc, "qn_kf_map_route_grid");
  return out;
}

// the path length in metres from the world points xyz (3 doubles each) to the nearest goal: infinity where the point is outside, blocked or cut off
// (qn_kf_map_route_query); costs (optional): the raw values, QN_ROUTE_BLOCKED / QN_ROUTE_UNREACHED among them
inline std::vector<double> routeCostAt(qn_kf_store* store, const std::vector<double>& xyz, std::vector<uint32_t>* costs = nullptr) {
  if (xyz.empty() || xyz.size() % 3 != 0) throw std::invalid_argument("[qn_map] routeCostAt: 3 doubles per point, at least one point");
  qn_occupancy_grid g; qn_route_params p;
  int rc = qn_kf_map_route_grid(store, &g, &p, nullptr);
  detail::check(store, rc, "qn_kf_map_route_grid");
  const uint32_t n = (uint32_t)(xyz.size() / 3);
  std::vector<uint32_t> c(n);
  rc = qn_kf_map_route_query(store, xyz.data(), n, c.data());
  detail::check(store, rc, "qn_kf_map_route_query");
  std::vector<double> out(n);
  for (uint32_t i = 0; i < n; i++) out[i] = c[i] >= QN_ROUTE_BLOCKED ? std::numeric_limits<double>::infinity() : (double)c[i] / 3.0 * g.voxel;
  if (costs) costs->swap(c);
  return out;
}

// the paths from the world points `starts` (3 doubles each) down the field to a goal, at most max_len voxels of each (qn_kf_map_route_path); len 0: the start
// is outside, blocked or cut off.  cost / 3 + 1 (routeCostAt's raw value) bounds a path's length.
inline std::vector<RoutePath> routePath(qn_kf_store* store, const std::vector<double>& starts, uint32_t max_len) {
  if (starts.empty() || starts.size() % 3 != 0) throw std::invalid_argument("[qn_map] routePath: 3 doubles per start, at least one start");
  if (max_len == 0) throw std::invalid_argument("[qn_map] routePath: max_len of at least 1");
  const uint32_t n = (uint32_t)(starts.size() / 3);
  std::vector<uint32_t> len(n);
  std::vector<int32_t> ijk(3 * (size_t)max_len * n);
  const int rc = qn_kf_map_route_path(store, starts.data(), n, max_len, len.data(), ijk.data());
  detail::check(store, rc, "qn_kf_map_route_path");
  std::vector<RoutePath> out(n);
  for (uint32_t i = 0; i < n; i++) {
    out[i].len = len[i];
    const uint32_t m = len[i] < max_len ? len[i] : max_len;
    out[i].voxels.resize(m);
    for (uint32_t k = 0; k < m; k++)
      for (int a = 0; a < 3; a++) out[i].voxels[k][a] = ijk[3 * ((size_t)max_len * i + k) + a];
  }
  return out;
}

}  // namespace qn_map
