// Drop-in helper for the question an explorer asks of the occupancy map: where to go next to see more.  Where a user of the reference would download the class
// volume after every map update and label the free voxels beside unknown space on the host, mapFrontiers finds them over the latest qn_map::mapOccupancy on
// the GPU - the free voxels with an unknown face neighbour, grouped into 26-connected regions of at least min_size voxels, numbered in ascending root - and
// keeps them there; frontierRegions returns the regions' rows (size, box, faces, centroid), frontierVoxels every frontier voxel with its label, and
// frontierCosts, with the field of the latest qn_map::mapRoute, what it costs to reach each region and where it is entered.
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

struct MapFrontiers {
  qn_frontier_stats stats;
  qn_frontier_params params;
  qn_occupancy_grid grid;                                          // the occupancy map's: origin, voxel, width along x, height along y, depth along z
  size_t voxels() const { return (size_t)grid.width * grid.height * grid.depth; }
  // the centroid of a region in world coordinates: (minc + sum / size + 0.5) * voxel
  std::array<double, 3> centroid(const qn_frontier_info& r) const {
    std::array<double, 3> c;
    for (int k = 0; k < 3; k++) c[k] = (grid.minc[k] + (double)r.sum[k] / (double)(r.size ? r.size : 1u) + 0.5) * grid.voxel;
    return c;
  }
  // the centre of voxel (i, j, k) in world coordinates
  std::array<double, 3> centre(int32_t i, int32_t j, int32_t k) const {
    return {(grid.minc[0] + i + 0.5) * grid.voxel, (grid.minc[1] + j + 0.5) * grid.voxel, (grid.minc[2] + k + 0.5) * grid.voxel};
  }
};

// what it costs to reach a region and the voxel where it is entered; cost QN_ROUTE_UNREACHED and voxel (0, 0, 0): no voxel of the region is reached
struct FrontierCost {
  uint32_t cost = QN_ROUTE_UNREACHED;
  std::array<int32_t, 3> voxel = {0, 0, 0};
  double metres(double voxel_edge) const { return cost >= QN_ROUTE_BLOCKED ? std::numeric_limits<double>::infinity() : (double)cost / 3.0 * voxel_edge; }
};

// the frontier regions of the latest mapOccupancy (qn_kf_map_frontiers).  params NULL: the defaults (candidates: the free voxels, unknown: the unknown voxels and
// the space outside the grid, min_size 8, every layer).  The result stays resident until the next mapFrontiers or mapOccupancy; mapDistance and mapRoute
// do not touch it.
inline MapFrontiers mapFrontiers(qn_kf_store* store, const qn_frontier_params* params = nullptr) {
  qn_frontier_params p = detail::params_or(params, qn_frontier_default_params);
  if (p.iz_lo > p.iz_hi) throw std::invalid_argument("[qn_map] mapFrontiers: iz_lo <= iz_hi");
  if (p.min_size == 0) throw std::invalid_argument("[qn_map] mapFrontiers: min_size of at least 1");
  if (p.free_mask & p.unknown_mask) throw std::invalid_argument("[qn_map] mapFrontiers: free_mask and unknown_mask share a class");
  MapFrontiers out;
  int rc = qn_kf_map_frontiers(store, &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_frontiers");
  rc = qn_kf_map_frontier_grid(store, &out.grid, &out.params, nullptr);
  detail::check(store, rc, "qn_kf_map_frontier_grid");
  return out;
}

// the regions' rows in region order (qn_kf_map_frontier_regions)
inline std::vector<qn_frontier_info> frontierRegions(qn_kf_store* store) {
  uint32_t n = 0;
  int rc = qn_kf_map_frontier_regions(store, nullptr, 0, &n);
  detail::check(store, rc, "qn_kf_map_frontier_regions", QN_ERR_CAPACITY);
  std::vector<qn_frontier_info> out(n);
  if (!n) return out;
  rc = qn_kf_map_frontier_regions(store, out.data(), n, &n);
  detail::check(store, rc, "qn_kf_map_frontier_regions");
  return out;
}

// every frontier voxel, kept or rejected, in ascending linear index: (i, j, k) each; labels (optional): the region number or QN_FRONTIER_REJECTED
// (qn_kf_map_frontier_list)
inline std::vector<std::array<int32_t, 3>> frontierVoxels(qn_kf_store* store, std::vector<int32_t>* labels = nullptr) {
  uint32_t n = 0;
  int rc = qn_kf_map_frontier_list(store, nullptr, nullptr, 0, &n);
  detail::check(store, rc, "qn_kf_map_frontier_list", QN_ERR_CAPACITY);
  std::vector<std::array<int32_t, 3>> out(n);
  std::vector<int32_t> lab(n);
  if (n) {
    rc = qn_kf_map_frontier_list(store, &out[0][0], lab.data(), n, &n);
    detail::check(store, rc, "qn_kf_map_frontier_list");
  }
  if (labels) labels->swap(lab);
  return out;
}

// per region the smallest cost of the latest mapRoute's field over its voxels and the voxel attaining it (qn_kf_map_frontier_costs)
inline std::vector<FrontierCost> frontierCosts(qn_kf_store* store) {
  uint32_t n = 0;
  int rc = qn_kf_map_frontier_regions(store, nullptr, 0, &n);
  detail::check(store, rc, "qn_kf_map_frontier_regions", QN_ERR_CAPACITY);
  std::vector<uint32_t> cost(n ? n : 1);
  std::vector<int32_t> ijk(3 * (size_t)(n ? n : 1));
  rc = qn_kf_map_frontier_costs(store, cost.data(), ijk.data());
  detail::check(store, rc, "qn_kf_map_frontier_costs");
  std::vector<FrontierCost> out(n);
  for (uint32_t k = 0; k < n; k++) { out[k].cost = cost[k]; out[k].voxel = {ijk[3 * (size_t)k], ijk[3 * (size_t)k + 1], ijk[3 * (size_t)k + 2]}; }
  return out;
}

}  // namespace qn_map
