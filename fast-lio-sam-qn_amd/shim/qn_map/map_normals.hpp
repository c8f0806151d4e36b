// Drop-in helper for the normals of the corrected global map: after qn_kf_build_map / buildStaticMap, where the reference would save or publish the map
// (fast_lio_sam_qn.cpp:398-411 saveFlagCallback), mapNormals gives every map point its surface normal and curvature from the resident map - point-to-plane
// localisation, meshing and ground extraction take the result as it is.  The viewpoints that orient the normals are the translations of the entries'
// corrected poses: a surface faces the keyframe that saw it from nearest.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL: MapWithNormals has the shape of a
// pcl::PointCloud<pcl::PointXYZINormal> (the 48-byte record, `points`), so its records can be copied into one byte for byte.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct alignas(16) PointXYZINormal {                               // pcl::PointXYZINormal's layout
  float x, y, z, pad0;
  float normal_x, normal_y, normal_z, pad1;
  float intensity, curvature, pad2[2];
};
static_assert(sizeof(PointXYZINormal) == 48 && offsetof(PointXYZINormal, normal_x) == 16 && offsetof(PointXYZINormal, intensity) == 32 &&
              offsetof(PointXYZINormal, curvature) == 36, "pcl::PointXYZINormal");
struct MapWithNormals {
  std::vector<PointXYZINormal> points;
  std::vector<uint32_t> neighbors;                                 // per point: the neighbours its normal was made from (fewer than min_neighbors: NaN normal)
  std::vector<int32_t> view;                                       // per point: the entry whose position oriented it (-1: a non-finite point, or no poses)
  size_t size() const { return points.size(); }
};

// the normals of the store's map slot (qn_kf_map_normals) and the map itself in one cloud; poses16: 16 doubles per entry, row-major, sensor -> world - the
// list the map was built from; params NULL: the defaults (radius 0.6, 5 neighbours)
inline MapWithNormals mapNormals(qn_kf_store* store, const qn_normal_params* params, const std::vector<double>& poses16) {
  if (poses16.size() % 16) throw std::invalid_argument("[qn_map] mapNormals: 16 doubles per entry");
  qn_normal_params p = detail::params_or(params, qn_normal_default_params);
  const uint32_t nv = (uint32_t)(poses16.size() / 16);
  std::vector<double> views(3 * (size_t)nv);
  for (uint32_t k = 0; k < nv; k++) { views[3 * k] = poses16[16 * k + 3]; views[3 * k + 1] = poses16[16 * k + 7]; views[3 * k + 2] = poses16[16 * k + 11]; }
  const float* d_normals = nullptr; uint32_t n = 0;
  int rc = qn_kf_map_normals(store, &p, nv ? views.data() : nullptr, nv, &d_normals, &n);
  detail::check(store, rc, "qn_kf_map_normals");
  MapWithNormals out;
  out.points.assign(n, PointXYZINormal{});
  out.neighbors.resize(n); out.view.resize(n);
  if (!n) return out;
  std::vector<float> nrm(4 * (size_t)n);
  rc = qn_kf_download_map_normals(store, nrm.data(), out.neighbors.data(), out.view.data());
  if (rc == QN_OK) rc = qn_kf_download_map(store, out.points.data(), sizeof(PointXYZINormal), offsetof(PointXYZINormal, intensity));
  detail::check(store, rc, "mapNormals download");
  for (uint32_t i = 0; i < n; i++) {
    PointXYZINormal& q = out.points[i];
    q.pad0 = 1.0f;
    q.normal_x = nrm[4 * (size_t)i]; q.normal_y = nrm[4 * (size_t)i + 1]; q.normal_z = nrm[4 * (size_t)i + 2]; q.curvature = nrm[4 * (size_t)i + 3];
  }
  return out;
}

}  // namespace qn_map
