// qn_map::mapGround / occupancyGrid / keepClasses written against the stand-ins.
// Without arguments (no device needed): the record layouts the headers state, the defaults, and the refusal of a null store by the three helpers.
// usage on a GPU: shim_map_ground keyframes.bin poses.bin leaf cell max_slope ground_tol clearance
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "ground <points> <ground> <obstacle> <overhead> <fnv1a64 of class and height_q per point>",
//          "grid <width> <height> <occupied> <free> <unknown> <fnv1a64 of ground_q and occupancy per column>" and
//          "kept <points> <fnv1a64 of the xyz and intensity bytes of the map without its ground>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <qn_map/map_ground.hpp>

static_assert(sizeof(qn_ground_params) == 40 && offsetof(qn_ground_params, max_slope) == 8 && offsetof(qn_ground_params, clearance) == 24 &&
              offsetof(qn_ground_params, min_points) == 32 && offsetof(qn_ground_params, reserved) == 36, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_ground_stats) == 80 && offsetof(qn_ground_stats, n_none) == 8 && offsetof(qn_ground_stats, width) == 28 &&
              offsetof(qn_ground_stats, seeded) == 36 && offsetof(qn_ground_stats, quant_exp) == 52 && offsetof(qn_ground_stats, rounds) == 72,
              "the layout include/qn_engine.h states");
static_assert(sizeof(qn_ground_grid) == 40 && offsetof(qn_ground_grid, cell) == 16 && offsetof(qn_ground_grid, width) == 24 &&
              offsetof(qn_ground_grid, quant_exp) == 32, "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_ground_params p{0.0, -1.0, -1.0, 0.0, 0, 9};
  qn_ground_default_params(&p);
  if (p.cell != 0.5 || p.max_slope != 0.3 || p.ground_tol != 0.2 || p.clearance != 2.0 || p.min_points != 1 || p.reserved != 0) return 1;
  if (QN_GROUND_MAX_CELLS != (1u << 26) || QN_GROUND_NONE != 0 || QN_GROUND_GROUND != 1 || QN_GROUND_OBSTACLE != 2 || QN_GROUND_OVERHEAD != 3 || QN_GROUND_BELOW != 4) return 1;
  try {
    qn_map::mapGround(nullptr, nullptr);
    return 2;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::occupancyGrid(nullptr);
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::keepClasses(nullptr, 1u << QN_GROUND_GROUND);
    return 4;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("params %zu bytes, stats %zu bytes, grid %zu bytes\n", sizeof(qn_ground_params), sizeof(qn_ground_stats), sizeof(qn_ground_grid));
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
  const float* d_map = nullptr; uint32_t nm = 0;
  if (qn_kf_build_map(store, ids.data(), poses.data(), (uint32_t)ids.size(), std::atof(argv[3]), &d_map, &nm) != QN_OK) return 7;
  qn_ground_params p;
  qn_ground_default_params(&p);
  p.cell = std::atof(argv[4]); p.max_slope = std::atof(argv[5]); p.ground_tol = std::atof(argv[6]); p.clearance = std::atof(argv[7]);
  const qn_map::MapGround m = qn_map::mapGround(store, &p);
  if (m.size() != nm) return 8;
  unsigned long long hp = 1469598103934665603ull, hg = hp, hm = hp;
  for (size_t i = 0; i < m.size(); i++) { hp = fnv(hp, &m.classes[i], 1); hp = fnv(hp, &m.height_q[i], 4); }
  std::printf("ground %zu %u %u %u %016llx\n", m.size(), m.stats.n_ground, m.stats.n_obstacle, m.stats.n_overhead, hp);
  const qn_map::OccupancyGrid g = qn_map::occupancyGrid(store);
  if (g.info.width != m.stats.width || g.info.height != m.stats.height) return 9;
  for (size_t c = 0; c < g.occupancy.size(); c++) { hg = fnv(hg, &g.ground_q[c], 4); hg = fnv(hg, &g.occupancy[c], 1); }
  std::printf("grid %u %u %u %u %u %016llx\n", g.info.width, g.info.height, m.stats.occupied, m.stats.free, m.stats.unknown, hg);
  const uint32_t left = qn_map::keepClasses(store, ~(1u << QN_GROUND_GROUND) & 31u);
  if (left != nm - m.stats.n_ground) return 10;
  std::vector<float> out(4 * (size_t)left + 4);
  if (left && qn_kf_download_map(store, out.data(), 16, 12) != QN_OK) return 11;
  for (size_t i = 0; i < left; i++) hm = fnv(hm, &out[4 * i], 16);
  std::printf("kept %u %016llx\n", left, hm);
  qn_kf_store_destroy(store);
  return 0;
}
