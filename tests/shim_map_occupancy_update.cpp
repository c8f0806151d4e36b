// qn_map::updateOccupancy written against the stand-ins.  No device needed: the record layout the header states and both refusals - a list whose poses do not
// match it (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's status).
#include <cstdio>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <qn_map/map_occupancy.hpp>

static_assert(sizeof(qn_occupancy_update) == 64 && offsetof(qn_occupancy_update, entries_removed) == 8 && offsetof(qn_occupancy_update, rebuilt) == 12 &&
              offsetof(qn_occupancy_update, regridded) == 16 && offsetof(qn_occupancy_update, records_walked) == 20 && offsetof(qn_occupancy_update, dirty_lo) == 24 &&
              offsetof(qn_occupancy_update, dirty_hi) == 36 && offsetof(qn_occupancy_update, rays_added) == 48 && offsetof(qn_occupancy_update, rays_removed) == 56,
              "the layout include/qn_engine.h states");

int main() {
  const std::vector<int32_t> ids = {0, 1};
  qn_occupancy_update u;
  try {
    qn_map::updateOccupancy(nullptr, ids, std::vector<double>(31, 0.0));
    return 2;
  } catch (const std::invalid_argument& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::updateOccupancy(nullptr, ids, std::vector<double>(32, 0.0), nullptr, &u);
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("update %zu bytes\n", sizeof(qn_occupancy_update));
  return 0;
}
