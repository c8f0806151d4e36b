// Drop-in helper for a 3-D occupancy map of the corrected keyframes: where a user of the reference would download every keyframe and feed an OctoMap-style ray
// inserter on the host, mapOccupancy walks the ray of every record of the listed keyframes - from the keyframe's corrected sensor position to the world point -
// through a voxel grid on the GPU and leaves a volume in which every voxel is occupied, observed free or never observed; occupiedVoxels fetches the occupied
// voxels as a cloud of voxel centres, occupancySlice a 2-D grid over a band of layers with the values of qn_map::OccupancyGrid.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  PointT needs x, y, z and intensity (pcl::PointXYZI); builds against real
// PCL and against the stand-ins in tests/standins: it only touches cloud.clear() / reserve() / push_back().
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapOccupancy {
  qn_occupancy_stats stats;
  qn_occupancy_grid grid;                                          // origin: the corner of voxel (0, 0, 0); voxel; width along x, height along y, depth along z
  size_t voxels() const { return (size_t)grid.width * grid.height * grid.depth; }
  // the layer of world height z by the grid's own arithmetic (it may lie outside 0 .. depth - 1): for occupancySlice
  int32_t layerOf(double z) const { return (int32_t)((long long)__builtin_rint((z * (1.0 / grid.voxel)) * 1024.0) >> 10) - grid.minc[2]; }
};

// the volume of the keyframes ids[k] under the poses poses16[16 k ..] (row-major 4x4, sensor -> world): the list qn_kf_build_map takes (qn_kf_map_occupancy).
// params NULL: the defaults (voxel 0.3, ranges 0.5 .. 60, shell 1, min_hits 1, hit_weight 2).  The map slot is neither read nor touched.
inline MapOccupancy mapOccupancy(qn_kf_store* store, const std::vector<int32_t>& ids, const std::vector<double>& poses16, const qn_occupancy_params* params = nullptr) {
  if (poses16.size() != 16 * ids.size()) throw std::invalid_argument("[qn_map] mapOccupancy: 16 doubles per listed keyframe");
  qn_occupancy_params p = detail::params_or(params, qn_occupancy_default_params);
  MapOccupancy out;
  int rc = qn_kf_map_occupancy(store, ids.data(), poses16.data(), (uint32_t)ids.size(), &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_occupancy");
  rc = qn_kf_map_occupancy_grid(store, &out.grid, nullptr, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_occupancy_grid");
  return out;
}

// the resident volume brought to this list in place (qn_kf_map_occupancy_update): the entries whose id and pose bytes the volume already holds are kept, the
// others walked in, and what the list no longer names walked out again.  The arguments and the result are mapOccupancy's, byte for byte; update (optional):
// what the call did - the entries kept, added and removed, whether it started from nothing, the box of the new grid outside which no count changed.
inline MapOccupancy updateOccupancy(qn_kf_store* store, const std::vector<int32_t>& ids, const std::vector<double>& poses16, const qn_occupancy_params* params = nullptr,
                                    qn_occupancy_update* update = nullptr) {
  if (poses16.size() != 16 * ids.size()) throw std::invalid_argument("[qn_map] updateOccupancy: 16 doubles per listed keyframe");
  qn_occupancy_params p = detail::params_or(params, qn_occupancy_default_params);
  MapOccupancy out;
  qn_occupancy_update u;
  int rc = qn_kf_map_occupancy_update(store, ids.data(), poses16.data(), (uint32_t)ids.size(), &p, &out.stats, &u);
  detail::check(store, rc, "qn_kf_map_occupancy_update");
  rc = qn_kf_map_occupancy_grid(store, &out.grid, nullptr, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_occupancy_grid");
  if (update) *update = u;
  return out;
}

// the voxels of the latest mapOccupancy whose class bit is in class_mask (default: the occupied ones) as a cloud of voxel centres (minc + i + 0.5) * voxel, in
// ascending linear index, intensity = hits (qn_kf_map_occupancy_list); misses (optional): their miss counts -> the number of voxels
template <typename PointT>
inline uint32_t occupiedVoxels(qn_kf_store* store, pcl::PointCloud<PointT>& out, uint32_t class_mask = 1u << QN_OCC_OCCUPIED, std::vector<uint32_t>* misses = nullptr) {
  qn_occupancy_grid g;
  int rc = qn_kf_map_occupancy_grid(store, &g, nullptr, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_occupancy_grid");
  uint32_t n = 0;
  rc = qn_kf_map_occupancy_list(store, class_mask, &n, nullptr, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_occupancy_list");
  std::vector<int32_t> ijk(3 * (size_t)n); std::vector<uint32_t> hits(n), miss(n);
  if (n) {
    rc = qn_kf_map_occupancy_list(store, class_mask, &n, ijk.data(), hits.data(), miss.data());
    detail::check(store, rc, "qn_kf_map_occupancy_list");
  }
  out.clear(); out.reserve(n);
  for (uint32_t k = 0; k < n; k++) {
    PointT p;
    p.x = (float)(((double)g.minc[0] + (double)ijk[3 * (size_t)k] + 0.5) * g.voxel);
    p.y = (float)(((double)g.minc[1] + (double)ijk[3 * (size_t)k + 1] + 0.5) * g.voxel);
    p.z = (float)(((double)g.minc[2] + (double)ijk[3 * (size_t)k + 2] + 0.5) * g.voxel);
    p.intensity = (float)hits[k];
    out.push_back(p);
  }
  if (misses) misses->swap(miss);
  return n;
}

// per column over the layers iz_lo .. iz_hi (inclusive, clipped to the grid): 2 if any voxel is occupied, else 1 if any is free, else 0; row-major with y the
// slow axis, width x height of the latest mapOccupancy (qn_kf_map_occupancy_slice).  The values are qn_map::OccupancyGrid's; free here means that a ray passed.
inline std::vector<uint8_t> occupancySlice(qn_kf_store* store, int32_t iz_lo, int32_t iz_hi, qn_occupancy_grid* grid = nullptr) {
  qn_occupancy_grid g;
  int rc = qn_kf_map_occupancy_grid(store, &g, nullptr, nullptr, nullptr);
  detail::check(store, rc, "qn_kf_map_occupancy_grid");
  std::vector<uint8_t> occ((size_t)g.width * g.height);
  std::vector<uint8_t> pad(1);
  rc = qn_kf_map_occupancy_slice(store, iz_lo, iz_hi, occ.empty() ? pad.data() : occ.data());
  detail::check(store, rc, "qn_kf_map_occupancy_slice");
  if (grid) *grid = g;
  return occ;
}

}  // namespace qn_map
