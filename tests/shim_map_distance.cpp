// qn_map::mapDistance / distanceSlice / distanceAt written against the stand-ins.
// Without arguments (no device needed): the record layouts the header states, the defaults, and the refusals - a max_dist outside 1 .. 255 and a point list
// that is no list of triples (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's status) by the
// three helpers.
// usage on a GPU: shim_map_distance keyframes.bin poses.bin voxel iz_lo iz_hi site_mask max_dist
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "distance <sites> <reached> <far> <max_d2> <sum_d2>", "slice <fnv1a64 of its bytes>" and
//          "at <fnv1a64 of the metres and classes of 64 points along the grid's diagonal>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <qn_map/map_occupancy.hpp>
#include <qn_map/map_distance.hpp>

static_assert(sizeof(qn_distance_params) == 16 && offsetof(qn_distance_params, max_dist) == 4 && offsetof(qn_distance_params, reserved) == 8,
              "the layout include/qn_engine.h states");
static_assert(sizeof(qn_distance_stats) == 32 && offsetof(qn_distance_stats, reached) == 4 && offsetof(qn_distance_stats, max_d2) == 12 &&
              offsetof(qn_distance_stats, sum_d2) == 16 && offsetof(qn_distance_stats, reserved) == 24, "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_distance_params p{9, 0, {1, 2}};
  qn_distance_default_params(&p);
  if (p.site_mask != (1u << QN_OCC_OCCUPIED) || p.max_dist != 16 || p.reserved[0] || p.reserved[1]) return 1;
  if (QN_DIST_FAR != 0xffffu || QN_DIST_MAX_RADIUS != 255u || QN_DIST_OUTSIDE != 0xffu) return 1;
  qn_map::MapDistance m{};
  m.grid.voxel = 0.25;
  if (m.metres(0) != 0.0 || m.metres(16) != 1.0 || !(m.metres(QN_DIST_FAR) > 1e300) || m.radius2(0.6) != 5 || m.radius2(0.5) != 4) return 1;
  p.max_dist = 256;
  try {
    qn_map::mapDistance(nullptr, &p);
    return 2;
  } catch (const std::invalid_argument& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::distanceAt(nullptr, std::vector<double>(4, 0.0));
    return 3;
  } catch (const std::invalid_argument& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::mapDistance(nullptr);
    return 4;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::distanceSlice(nullptr, 0, 3);
    return 5;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::distanceAt(nullptr, std::vector<double>(3, 0.0));
    return 6;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("params %zu bytes, stats %zu bytes\n", sizeof(qn_distance_params), sizeof(qn_distance_stats));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 8) return selfCheck();
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
  qn_occupancy_params op;
  qn_occupancy_default_params(&op);
  op.voxel = std::atof(argv[3]);
  const qn_map::MapOccupancy occ = qn_map::mapOccupancy(store, ids, poses, &op);
  qn_distance_params dp;
  qn_distance_default_params(&dp);
  dp.site_mask = (uint32_t)std::atoi(argv[6]); dp.max_dist = (uint32_t)std::atoi(argv[7]);
  const qn_map::MapDistance m = qn_map::mapDistance(store, &dp);
  if (m.voxels() != occ.voxels() || m.params.max_dist != dp.max_dist || m.stats.sites + m.stats.reached + m.stats.far != m.voxels()) return 8;
  std::printf("distance %u %u %u %u %llu\n", m.stats.sites, m.stats.reached, m.stats.far, m.stats.max_d2, (unsigned long long)m.stats.sum_d2);
  const std::vector<uint16_t> d2 = qn_map::distanceSlice(store, std::atoi(argv[4]), std::atoi(argv[5]));
  if (d2.size() != (size_t)m.grid.width * m.grid.height) return 9;
  std::printf("slice %016llx\n", fnv(1469598103934665603ull, d2.data(), 2 * d2.size()));
  // 64 points along the diagonal of the grid, the first and the last just outside it
  std::vector<double> xyz;
  const double side[3] = {(double)m.grid.width, (double)m.grid.height, (double)m.grid.depth};
  for (int i = 0; i < 64; i++)
    for (int k = 0; k < 3; k++) xyz.push_back(m.grid.origin[k] + ((double)i - 0.5) / 62.0 * side[k] * m.grid.voxel);
  std::vector<uint8_t> cls;
  const std::vector<double> dist = qn_map::distanceAt(store, xyz, &cls);
  if (dist.size() != 64 || cls.size() != 64 || cls[0] != QN_DIST_OUTSIDE || cls[63] != QN_DIST_OUTSIDE) return 10;
  unsigned long long h = 1469598103934665603ull;
  for (int i = 0; i < 64; i++) { h = fnv(h, &dist[i], 8); h = fnv(h, &cls[i], 1); }
  std::printf("at %016llx\n", h);
  qn_kf_store_destroy(store);
  return 0;
}
