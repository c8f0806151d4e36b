// Drop-in helper for the objects of the corrected global map: after qn_kf_build_map (and mapGround, when only what stands on the ground is wanted), where a
// user of the reference would run pcl::EuclideanClusterExtraction over the saved map on the host, mapClusters labels every point of the resident map on the GPU
// and lists the clusters with their size, box and centroid; dropRejectedClusters removes the clumps that are no cluster from the map in place.
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

struct MapCluster {
  uint32_t root, size;                                             // the smallest map index of the cluster, its points
  float lo[3], hi[3];                                              // its box
  double centroid[3];                                              // sum_q / size * 2^-quant_exp
};

struct MapClusters {
  qn_cluster_stats stats;
  std::vector<int32_t> label;                                      // per map point: the cluster's number, QN_CLUSTER_REJECTED or QN_CLUSTER_NONE
  std::vector<uint32_t> root, size;                                // per map point: its component's smallest map index (0xffffffff: no member) and size
  std::vector<qn_cluster_info> info;                               // per cluster, as the library serves it
  std::vector<MapCluster> clusters;                                // per cluster, with the centroid
};

// the clusters of the store's map slot (qn_kf_map_clusters); the slot is not touched.  params NULL: the defaults (tolerance 0.5, 10 .. 2^32 - 1 points, mask 0)
inline MapClusters mapClusters(qn_kf_store* store, const qn_cluster_params* params) {
  qn_cluster_params p = detail::params_or(params, qn_cluster_default_params);
  MapClusters out;
  int rc = qn_kf_map_clusters(store, &p, &out.stats);
  detail::check(store, rc, "qn_kf_map_clusters");
  const uint32_t n = out.stats.n, C = out.stats.clusters;
  out.label.resize(n); out.root.resize(n); out.size.resize(n);
  if (n) {
    rc = qn_kf_map_cluster_points(store, out.label.data(), out.root.data(), out.size.data());
    detail::check(store, rc, "qn_kf_map_cluster_points");
  }
  out.info.resize(C);
  uint32_t count = 0;
  rc = qn_kf_map_cluster_list(store, C ? out.info.data() : nullptr, C, &count);
  if (rc != QN_OK || count != C) throw std::runtime_error(detail::why("qn_kf_map_cluster_list", rc, store));
  out.clusters.resize(C);
  for (uint32_t c = 0; c < C; c++) {
    const qn_cluster_info& i = out.info[c];
    MapCluster& m = out.clusters[c];
    m.root = i.root; m.size = i.size;
    for (int a = 0; a < 3; a++) { m.lo[a] = i.lo[a]; m.hi[a] = i.hi[a]; m.centroid[a] = std::ldexp((double)i.sum_q[a] / (double)i.size, -out.stats.quant_exp); }
  }
  return out;
}

// applies the latest mapClusters to the map slot (qn_kf_map_drop_rejected_clusters) -> the points left; d_xyzi (optional): the device address of their records
inline uint32_t dropRejectedClusters(qn_kf_store* store, const float** d_xyzi = nullptr) {
  const float* d = nullptr; uint32_t n = 0;
  const int rc = qn_kf_map_drop_rejected_clusters(store, &d, &n);
  detail::check(store, rc, "qn_kf_map_drop_rejected_clusters");
  if (d_xyzi) *d_xyzi = d;
  return n;
}

}  // namespace qn_map
