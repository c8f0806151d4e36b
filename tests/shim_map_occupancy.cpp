// qn_map::mapOccupancy / occupiedVoxels / occupancySlice written against the stand-ins.
// Without arguments (no device needed): the record layouts the header states, the defaults, and both refusals - a list whose poses do not match it
// (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's status) by the three helpers.
// usage on a GPU: shim_map_occupancy keyframes.bin poses.bin voxel iz_lo iz_hi
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "occupancy <rays> <misses> <width> <height> <depth> <occupied> <free> <unknown>",
//          "voxels <count> <fnv1a64 of x, y, z, intensity and misses per voxel>" and "slice <fnv1a64 of its bytes>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <qn_map/map_occupancy.hpp>

static_assert(sizeof(qn_occupancy_params) == 48 && offsetof(qn_occupancy_params, min_range) == 8 && offsetof(qn_occupancy_params, shell) == 24 &&
              offsetof(qn_occupancy_params, hit_weight) == 32 && offsetof(qn_occupancy_params, reserved) == 36, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_occupancy_stats) == 64 && offsetof(qn_occupancy_stats, width) == 20 && offsetof(qn_occupancy_stats, occupied) == 32 &&
              offsetof(qn_occupancy_stats, reserved) == 44 && offsetof(qn_occupancy_stats, total_hits) == 48 && offsetof(qn_occupancy_stats, total_misses) == 56,
              "the layout include/qn_engine.h states");
static_assert(sizeof(qn_occupancy_grid) == 56 && offsetof(qn_occupancy_grid, voxel) == 24 && offsetof(qn_occupancy_grid, width) == 32 &&
              offsetof(qn_occupancy_grid, minc) == 44, "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_occupancy_params p{0.0, -1.0, -1.0, 9, 0, 0, {1, 2, 3}};
  qn_occupancy_default_params(&p);
  if (p.voxel != 0.3 || p.min_range != 0.5 || p.max_range != 60.0 || p.shell != 1 || p.min_hits != 1 || p.hit_weight != 2 || p.reserved[0] || p.reserved[1] || p.reserved[2]) return 1;
  if (QN_OCC_MAX_CELLS != (1u << 27) || QN_OCC_UNKNOWN != 0 || QN_OCC_FREE != 1 || QN_OCC_OCCUPIED != 2) return 1;
  qn_map::MapOccupancy m{};
  m.grid.voxel = 0.3; m.grid.minc[2] = -1;
  if (m.layerOf(-0.01) != 0 || m.layerOf(0.0) != 1 || m.layerOf(1.73) != 6) return 1;
  const std::vector<int32_t> ids = {0, 1};
  try {
    qn_map::mapOccupancy(nullptr, ids, std::vector<double>(31, 0.0));
    return 2;
  } catch (const std::invalid_argument& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::mapOccupancy(nullptr, ids, std::vector<double>(32, 0.0));
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    pcl::PointCloud<pcl::PointXYZI> cloud;
    qn_map::occupiedVoxels(nullptr, cloud);
    return 4;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::occupancySlice(nullptr, 0, 3);
    return 5;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("params %zu bytes, stats %zu bytes, grid %zu bytes\n", sizeof(qn_occupancy_params), sizeof(qn_occupancy_stats), sizeof(qn_occupancy_grid));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return selfCheck();
  qn_kf_store* store = nullptr;
  if (qn_kf_store_create(0, &store) != QN_OK) return 5;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<int32_t> ids;
  uint32_t n = 0;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::vector<float> c(4 * (size_t)n);
    if (n && std::fread(c.data(), 16, n, f) != n) return 3;
    int32_t id = -1;
    if (qn_kf_add_xyzi(store, c.data(), n, 16, 12, &id) != QN_OK) return 6;
    ids.push_back(id);
  }
  std::fclose(f);
  std::vector<double> poses(16 * ids.size());
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 3;
  std::fclose(f);
  qn_occupancy_params p;
  qn_occupancy_default_params(&p);
  p.voxel = std::atof(argv[3]);
  const qn_map::MapOccupancy m = qn_map::mapOccupancy(store, ids, poses, &p);
  std::printf("occupancy %u %llu %u %u %u %u %u %u\n", m.stats.n_rays, (unsigned long long)m.stats.total_misses, m.grid.width, m.grid.height, m.grid.depth, m.stats.occupied,
              m.stats.free, m.stats.unknown);
  pcl::PointCloud<pcl::PointXYZI> cloud;
  std::vector<uint32_t> misses;
  const uint32_t k = qn_map::occupiedVoxels(store, cloud, 1u << QN_OCC_OCCUPIED, &misses);
  if (k != m.stats.occupied || cloud.size() != k || misses.size() != k) return 8;
  unsigned long long hv = 1469598103934665603ull, hs = hv;
  for (uint32_t i = 0; i < k; i++) {
    const float rec[4] = {cloud.points[i].x, cloud.points[i].y, cloud.points[i].z, cloud.points[i].intensity};
    hv = fnv(hv, rec, 16); hv = fnv(hv, &misses[i], 4);
  }
  std::printf("voxels %u %016llx\n", k, hv);
  const std::vector<uint8_t> occ = qn_map::occupancySlice(store, std::atoi(argv[4]), std::atoi(argv[5]));
  if (occ.size() != (size_t)m.grid.width * m.grid.height) return 9;
  hs = fnv(hs, occ.data(), occ.size());
  std::printf("slice %016llx\n", hs);
  qn_kf_store_destroy(store);
  return 0;
}
