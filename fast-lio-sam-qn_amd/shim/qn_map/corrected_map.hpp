// Drop-in helper for the corrected global map of FastLioSamQn (fast_lio_sam_qn/src/fast_lio_sam_qn.cpp:302-316 visTimerFunc,
// :398-411 saveFlagCallback, :435-448 the destructor's result.pcd).  Each of those call sites runs transformPcd on every keyframe
// with its corrected pose, concatenates, and runs voxelizePcd (pcl::VoxelGrid, include/utilities.hpp:38-51) at
// save_voxel_resolution.  Here the keyframes are uploaded once (addKeyframe, as they are created) and stay resident on the GPU; build()
// rebuilds the whole map there from the current corrected poses and copies only the result back.
// Header-only; every member forwards to the C-ABI in include/qn_engine.h (qn_kf_add_xyzi, qn_kf_build_map, qn_kf_download_map).
// Link with -lqn_engine.  PointT needs x, y, z and intensity (pcl::PointXYZI); the map's other bytes of each point stay as PointT's
// default constructor leaves them.  Builds against real PCL / Eigen and against the stand-ins in tests/standins: it only touches
// cloud.points / size() / clear() / reserve() / push_back() and Matrix4d's (row, col) accessor.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <Eigen/Core>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

template <typename PointT>
class CorrectedMap {
 public:
  explicit CorrectedMap(int device = 0) {
    const int rc = qn_kf_store_create(device, &store_);
    if (rc != QN_OK) throw std::runtime_error(detail::why("qn_kf_store_create", rc, nullptr));
  }
  ~CorrectedMap() { qn_kf_store_destroy(store_); }
  CorrectedMap(const CorrectedMap&) = delete;
  CorrectedMap& operator=(const CorrectedMap&) = delete;

  // one keyframe's sensor-frame cloud (PosePcd::pcd_); returns its index, which is its position in build()'s `poses`
  int addKeyframe(const pcl::PointCloud<PointT>& cloud) {
    int32_t id = -1;
    const PointT probe;
    const uint32_t ioff = (uint32_t)(reinterpret_cast<const char*>(&probe.intensity) - reinterpret_cast<const char*>(&probe));
    check(qn_kf_add_xyzi(store_, cloud.size() ? &cloud.points[0].x : nullptr, (uint32_t)cloud.size(), (uint32_t)sizeof(PointT), ioff, &id), "qn_kf_add_xyzi");
    return id;
  }

  // poses[k] = corrected pose of keyframe k (keyframes_[k].pose_corrected_eig_), for every keyframe added so far
  void build(const std::vector<Eigen::Matrix4d>& poses, float leaf, pcl::PointCloud<PointT>& out) {
    const uint32_t count = (uint32_t)poses.size();
    std::vector<int32_t> ids(count);
    std::vector<double> T(16 * (size_t)count);
    for (uint32_t k = 0; k < count; k++) {
      ids[k] = (int32_t)k;
      for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[16 * (size_t)k + 4 * r + c] = poses[k](r, c);
    }
    const float* d_map = nullptr; uint32_t n = 0;
    out.clear();
    const int rc = qn_kf_build_map(store_, ids.data(), T.data(), count, (double)leaf, &d_map, &n);
    if (rc == QN_ERR_EMPTY_CLOUD) return;                                         // no keyframes / no finite points: an empty map
    check(rc, "qn_kf_build_map");
    const char* note = qn_kf_last_error(store_);
    if (note && *note) std::fprintf(stderr, "[qn_map] %s\n", note);             // pcl::VoxelGrid's overflow warning, if it tripped
    std::vector<PointT> pts(n);
    const PointT probe;
    const uint32_t ioff = (uint32_t)(reinterpret_cast<const char*>(&probe.intensity) - reinterpret_cast<const char*>(&probe));
    if (n) check(qn_kf_download_map(store_, pts.data(), (uint32_t)sizeof(PointT), ioff), "qn_kf_download_map");
    out.reserve(n);
    for (const PointT& p : pts) out.push_back(p);
  }

 private:
  void check(int rc, const char* what) { detail::check(store_, rc, what); }
  qn_kf_store* store_ = nullptr;
};

}  // namespace qn_map
