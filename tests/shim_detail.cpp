// Every qn_map header in two translation units of one program (this one and shim_detail_second.cpp): the shared qn_map/detail.hpp is guarded and inline-clean.
// No device needed: one entry point per header is called with a null store - the constructor of CorrectedMap with a device that cannot exist - and the text of
// what it throws is printed, "<header>: <what()>" a line; the second unit adds a line of its own.
#include <cstdio>
#include <stdexcept>
#include <vector>
#include "shim_detail_headers.h"

int second_unit_lines();

template <typename F> static int line(const char* header, F f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    std::printf("%s: %s\n", header, e.what());
    return 0;
  }
  std::printf("%s: not refused\n", header);
  return 1;
}

int main() {
  const std::vector<double> one = {0.0, 0.0, 0.0};
  const std::vector<double> pose = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  Eigen::Matrix4d I;
  for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) I(r, c) = r == c ? 1.0 : 0.0;
  int bad = 0;
  bad += line("corrected_map.hpp", [&] { qn_map::CorrectedMap<pcl::PointXYZI> m(1 << 20); });
  bad += line("freespace.hpp", [&] { qn_map::describeRangeImages(nullptr, {0}); });
  bad += line("loop_submaps.hpp", [&] { qn_map::loopSubmapPairs(nullptr, {I, I}, 1, {0}, 1, 0.3, true, false); });
  bad += line("map_clusters.hpp", [&] { qn_map::mapClusters(nullptr, nullptr); });
  bad += line("map_distance.hpp", [&] { qn_map::mapDistance(nullptr); });
  bad += line("map_frontier.hpp", [&] { qn_map::mapFrontiers(nullptr); });
  bad += line("map_frontier.hpp", [&] { qn_map::frontierRegions(nullptr); });                      // the first call of a size probe
  bad += line("map_ground.hpp", [&] { qn_map::mapGround(nullptr, nullptr); });
  bad += line("map_localize.hpp", [&] { qn_map::cropMap(nullptr, {{0.0, 0.0, 0.0}}, 1.0); });
  bad += line("map_normals.hpp", [&] { qn_map::mapNormals(nullptr, nullptr, {}); });
  bad += line("map_occupancy.hpp", [&] { qn_map::mapOccupancy(nullptr, {0}, pose); });
  bad += line("map_outliers.hpp", [&] { qn_map::mapOutliers(nullptr, nullptr); });
  bad += line("map_route.hpp", [&] { qn_map::mapRoute(nullptr, one); });
  bad += line("map_view.hpp", [&] { qn_map::viewCover(nullptr); });
  bad += line("scan_context.hpp", [&] { qn_map::scanContextCandidates(nullptr, {0.0, 100.0}, 1, 30.0, 1, 0.5); });
  bad += line("static_map.hpp", [&] { qn_map::buildStaticMap(nullptr, 0.3); });
  return bad + second_unit_lines();
}
