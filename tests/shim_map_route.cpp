// qn_map::mapRoute / routeCostAt / routePath written against the stand-ins.
// Without arguments (no device needed): the record layouts the header states, the defaults, and the refusals - a goal, point or start list that is no list of
// triples, a reversed band and a max_len of 0 (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's
// status) by the three helpers.
// usage on a GPU: shim_map_route keyframes.bin poses.bin voxel planar min_d2 gx gy gz sx sy sz
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "route <passable> <blocked> <reached> <unreached> <goals_used> <goals_blocked> <max_cost> <sum_cost>",
//          "at <fnv1a64 of the metres at 64 points along the grid's diagonal>" and "path <len> <fnv1a64 of its voxels>" for the start (sx, sy, sz)
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <qn_map/map_occupancy.hpp>
#include <qn_map/map_distance.hpp>
#include <qn_map/map_route.hpp>

static_assert(sizeof(qn_route_params) == 32 && offsetof(qn_route_params, min_d2) == 4 && offsetof(qn_route_params, iz_lo) == 8 && offsetof(qn_route_params, iz_hi) == 12 &&
              offsetof(qn_route_params, planar) == 16 && offsetof(qn_route_params, reserved) == 20, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_route_stats) == 64 && offsetof(qn_route_stats, goals_used) == 16 && offsetof(qn_route_stats, max_cost) == 24 && offsetof(qn_route_stats, sum_cost) == 32 &&
              offsetof(qn_route_stats, rounds) == 40 && offsetof(qn_route_stats, tile_visits) == 48 && offsetof(qn_route_stats, reserved) == 56,
              "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

template <typename E, typename F> static bool refuses(F f) {
  try {
    f();
    return false;
  } catch (const E& e) {
    std::printf("refused: %s\n", e.what());
    return true;
  }
}

static int selfCheck() {
  qn_route_params p{9, 0, 5, 1, 7, {1, 2, 3}};
  qn_route_default_params(&p);
  if (p.pass_mask != (1u << QN_OCC_FREE) || p.min_d2 != 4 || p.iz_lo != 0 || p.iz_hi != INT32_MAX || p.planar != 0 || p.reserved[0] || p.reserved[1] || p.reserved[2]) return 1;
  if (QN_ROUTE_BLOCKED != 0xfffffffeu || QN_ROUTE_UNREACHED != 0xffffffffu || QN_ROUTE_MAX_POINTS != (1u << 20)) return 1;
  qn_map::MapRoute m{};
  m.grid.voxel = 0.25; m.grid.depth = 6; m.grid.width = m.grid.height = 2; m.grid.minc[0] = -2; m.grid.minc[2] = 4;
  if (m.metres(0) != 0.0 || m.metres(12) != 1.0 || !(m.metres(QN_ROUTE_BLOCKED) > 1e300) || !(m.metres(QN_ROUTE_UNREACHED) > 1e300)) return 1;
  if (m.centre(1, 0, 2)[0] != -0.125 || m.centre(1, 0, 2)[2] != 1.625 || m.depth() != 6) return 1;
  m.params.planar = 1; m.params.iz_lo = 2; m.params.iz_hi = 9;
  if (m.centre(1, 0, 0)[2] != (4 + 4.0) * 0.25 || m.depth() != 1 || m.cells() != 4) return 1;
  const std::vector<double> one(3, 0.0), four(4, 0.0);
  qn_route_params rev;
  qn_route_default_params(&rev);
  rev.iz_lo = 3; rev.iz_hi = 2;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapRoute(nullptr, four); })) return 2;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapRoute(nullptr, one, &rev); })) return 3;
  if (!refuses<std::invalid_argument>([&] { qn_map::routeCostAt(nullptr, four); })) return 4;
  if (!refuses<std::invalid_argument>([&] { qn_map::routePath(nullptr, four, 8); })) return 5;
  if (!refuses<std::invalid_argument>([&] { qn_map::routePath(nullptr, one, 0); })) return 6;
  if (!refuses<std::runtime_error>([&] { qn_map::mapRoute(nullptr, one); })) return 7;
  if (!refuses<std::runtime_error>([&] { qn_map::routeCostAt(nullptr, one); })) return 8;
  if (!refuses<std::runtime_error>([&] { qn_map::routePath(nullptr, one, 8); })) return 9;
  std::printf("params %zu bytes, stats %zu bytes\n", sizeof(qn_route_params), sizeof(qn_route_stats));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 12) return selfCheck();
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
  qn_map::mapDistance(store);
  qn_route_params rp;
  qn_route_default_params(&rp);
  rp.planar = (uint32_t)std::atoi(argv[4]); rp.min_d2 = (uint32_t)std::atoi(argv[5]);
  const std::vector<double> goal = {std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8])}, start = {std::atof(argv[9]), std::atof(argv[10]), std::atof(argv[11])};
  const qn_map::MapRoute m = qn_map::mapRoute(store, goal, &rp);
  if (m.cells() != occ.voxels() || m.params.min_d2 != rp.min_d2 || (size_t)m.stats.passable + m.stats.blocked != m.cells() ||
      m.stats.reached + m.stats.unreached != m.stats.passable) return 8;
  std::printf("route %u %u %u %u %u %u %u %llu\n", m.stats.passable, m.stats.blocked, m.stats.reached, m.stats.unreached, m.stats.goals_used, m.stats.goals_blocked,
              m.stats.max_cost, (unsigned long long)m.stats.sum_cost);
  // 64 points along the diagonal of the grid, the first and the last just outside it
  std::vector<double> xyz;
  const double side[3] = {(double)m.grid.width, (double)m.grid.height, (double)m.grid.depth};
  for (int i = 0; i < 64; i++)
    for (int k = 0; k < 3; k++) xyz.push_back(m.grid.origin[k] + ((double)i - 0.5) / 62.0 * side[k] * m.grid.voxel);
  std::vector<uint32_t> raw;
  const std::vector<double> dist = qn_map::routeCostAt(store, xyz, &raw);
  if (dist.size() != 64 || raw.size() != 64 || raw[0] != QN_ROUTE_BLOCKED || raw[63] != QN_ROUTE_BLOCKED) return 10;
  std::printf("at %016llx\n", fnv(1469598103934665603ull, dist.data(), 8 * dist.size()));
  std::vector<uint32_t> at;
  qn_map::routeCostAt(store, start, &at);
  if (at[0] >= QN_ROUTE_BLOCKED) return 11;
  const std::vector<qn_map::RoutePath> paths = qn_map::routePath(store, start, at[0] / 3 + 1);
  if (paths.size() != 1 || paths[0].len != paths[0].voxels.size()) return 12;
  unsigned long long h = 1469598103934665603ull;
  for (const auto& v : paths[0].voxels) h = fnv(h, v.data(), 12);
  std::printf("path %u %016llx\n", paths[0].len, h);
  qn_kf_store_destroy(store);
  return 0;
}
