// qn_map::mapFrontiers / frontierRegions / frontierVoxels / frontierCosts written against the stand-ins.
// Without arguments (no device needed): the record layouts the header states, the defaults, and the refusals - a reversed band, a min_size of 0 and masks that
// share a class (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's status) by the four helpers.
// usage on a GPU: shim_map_frontier keyframes.bin poses.bin voxel min_size gx gy gz
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "frontiers <candidates> <frontier> <components> <regions> <too_small> <region_voxels> <rejected_voxels> <largest> <unknown_faces>",
//          "regions <R> <fnv1a64 of the rows>" and "costs <fnv1a64 of the costs> <fnv1a64 of the voxels>" under the route field (FREE, min_d2 0) to (gx, gy, gz)
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <qn_map/map_occupancy.hpp>
#include <qn_map/map_distance.hpp>
#include <qn_map/map_route.hpp>
#include <qn_map/map_frontier.hpp>

static_assert(sizeof(qn_frontier_params) == 32 && offsetof(qn_frontier_params, unknown_mask) == 4 && offsetof(qn_frontier_params, edge_unknown) == 8 &&
              offsetof(qn_frontier_params, min_size) == 12 && offsetof(qn_frontier_params, iz_lo) == 16 && offsetof(qn_frontier_params, iz_hi) == 20 &&
              offsetof(qn_frontier_params, reserved) == 24, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_frontier_stats) == 48 && offsetof(qn_frontier_stats, regions) == 12 && offsetof(qn_frontier_stats, largest) == 28 &&
              offsetof(qn_frontier_stats, unknown_faces) == 32 && offsetof(qn_frontier_stats, rounds) == 36 && offsetof(qn_frontier_stats, reserved) == 40,
              "the layout include/qn_engine.h states");
static_assert(sizeof(qn_frontier_info) == 64 && offsetof(qn_frontier_info, size) == 4 && offsetof(qn_frontier_info, lo) == 8 && offsetof(qn_frontier_info, hi) == 20 &&
              offsetof(qn_frontier_info, faces) == 32 && offsetof(qn_frontier_info, reserved) == 36 && offsetof(qn_frontier_info, sum) == 40,
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
  qn_frontier_params p{9, 9, 5, 0, 7, 1, {1, 2}};
  qn_frontier_default_params(&p);
  if (p.free_mask != (1u << QN_OCC_FREE) || p.unknown_mask != (1u << QN_OCC_UNKNOWN) || p.edge_unknown != 1 || p.min_size != 8 || p.iz_lo != 0 || p.iz_hi != INT32_MAX ||
      p.reserved[0] || p.reserved[1])
    return 1;
  if (QN_FRONTIER_REJECTED != -1 || QN_FRONTIER_NONE != -2) return 1;
  qn_map::MapFrontiers m{};
  m.grid.voxel = 0.25; m.grid.width = m.grid.height = 2; m.grid.depth = 6; m.grid.minc[0] = -2; m.grid.minc[2] = 4;
  qn_frontier_info r{};
  r.size = 4; r.sum[0] = 6; r.sum[2] = 2;
  if (m.centroid(r)[0] != (-2 + 1.5 + 0.5) * 0.25 || m.centroid(r)[2] != (4 + 0.5 + 0.5) * 0.25 || m.centre(1, 0, 2)[0] != -0.125 || m.voxels() != 24) return 1;
  qn_map::FrontierCost fc;
  if (!(fc.metres(0.25) > 1e300)) return 1;
  fc.cost = 12;
  if (fc.metres(0.25) != 1.0) return 1;
  qn_frontier_params rev, zero, both;
  qn_frontier_default_params(&rev); qn_frontier_default_params(&zero); qn_frontier_default_params(&both);
  rev.iz_lo = 3; rev.iz_hi = 2; zero.min_size = 0; both.unknown_mask = 3;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapFrontiers(nullptr, &rev); })) return 2;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapFrontiers(nullptr, &zero); })) return 3;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapFrontiers(nullptr, &both); })) return 4;
  if (!refuses<std::runtime_error>([&] { qn_map::mapFrontiers(nullptr); })) return 5;
  if (!refuses<std::runtime_error>([&] { qn_map::frontierRegions(nullptr); })) return 6;
  if (!refuses<std::runtime_error>([&] { qn_map::frontierVoxels(nullptr); })) return 7;
  if (!refuses<std::runtime_error>([&] { qn_map::frontierCosts(nullptr); })) return 8;
  std::printf("params %zu bytes, stats %zu bytes, info %zu bytes\n", sizeof(qn_frontier_params), sizeof(qn_frontier_stats), sizeof(qn_frontier_info));
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
  qn_frontier_params fp;
  qn_frontier_default_params(&fp);
  fp.min_size = (uint32_t)std::atoi(argv[4]);
  const qn_map::MapFrontiers m = qn_map::mapFrontiers(store, &fp);      // before any distance or route call: it needs neither
  if (m.voxels() != occ.voxels() || m.params.min_size != fp.min_size || m.stats.regions + m.stats.too_small != m.stats.components ||
      m.stats.region_voxels + m.stats.rejected_voxels != m.stats.frontier)
    return 8;
  std::printf("frontiers %u %u %u %u %u %u %u %u %u\n", m.stats.candidates, m.stats.frontier, m.stats.components, m.stats.regions, m.stats.too_small, m.stats.region_voxels,
              m.stats.rejected_voxels, m.stats.largest, m.stats.unknown_faces);
  const std::vector<qn_frontier_info> rows = qn_map::frontierRegions(store);
  if (rows.size() != m.stats.regions) return 9;
  std::printf("regions %zu %016llx\n", rows.size(), fnv(1469598103934665603ull, rows.data(), sizeof(qn_frontier_info) * rows.size()));
  std::vector<int32_t> labels;
  const std::vector<std::array<int32_t, 3>> vox = qn_map::frontierVoxels(store, &labels);
  if (vox.size() != m.stats.frontier || labels.size() != vox.size()) return 10;
  qn_map::mapDistance(store);
  qn_route_params rp;
  qn_route_default_params(&rp);
  rp.min_d2 = 0;
  const std::vector<double> goal = {std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7])};
  qn_map::mapRoute(store, goal, &rp);
  const std::vector<qn_map::FrontierCost> costs = qn_map::frontierCosts(store);
  if (costs.size() != rows.size()) return 11;
  unsigned long long hc = 1469598103934665603ull, hv = 1469598103934665603ull;
  for (const auto& c : costs) { hc = fnv(hc, &c.cost, 4); hv = fnv(hv, c.voxel.data(), 12); }
  std::printf("costs %016llx %016llx\n", hc, hv);
  qn_kf_store_destroy(store);
  return 0;
}
