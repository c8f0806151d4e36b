// qn_map::sensorRays / mapViewGain / viewCover written against the stand-ins.  No device needed: the record layouts the header states, the defaults, the ray
// table of a small sensor, and the refusals - a table beyond the offset limit and an empty one, no viewpoint, a ray of two numbers, a reversed band, masks that
// share a class and an offset beyond the limit (std::invalid_argument, before the library is called) and a null store (std::runtime_error from the library's
// status) by the two helpers that take one.
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <qn_map/map_view.hpp>

static_assert(sizeof(qn_view_params) == 32 && offsetof(qn_view_params, stop_mask) == 4 && offsetof(qn_view_params, max_through) == 8 && offsetof(qn_view_params, iz_lo) == 12 &&
              offsetof(qn_view_params, iz_hi) == 16 && offsetof(qn_view_params, reserved) == 20, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_view_info) == 48 && offsetof(qn_view_info, gain) == 4 && offsetof(qn_view_info, blocked) == 8 && offsetof(qn_view_info, escaped) == 12 &&
              offsetof(qn_view_info, spent) == 16 && offsetof(qn_view_info, reached) == 20 && offsetof(qn_view_info, ijk) == 24 && offsetof(qn_view_info, reserved) == 36 &&
              offsetof(qn_view_info, steps) == 40, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_view_stats) == 48 && offsetof(qn_view_stats, outside) == 4 && offsetof(qn_view_stats, rays) == 8 && offsetof(qn_view_stats, covered) == 12 &&
              offsetof(qn_view_stats, max_cover) == 16 && offsetof(qn_view_stats, passes) == 20 && offsetof(qn_view_stats, reserved) == 24 &&
              offsetof(qn_view_stats, total_gain) == 32 && offsetof(qn_view_stats, steps) == 40, "the layout include/qn_engine.h states");

template <typename E, typename F> static bool refuses(F f) {
  try {
    f();
    return false;
  } catch (const E& e) {
    std::printf("refused: %s\n", e.what());
    return true;
  }
}

int main() {
  qn_view_params p{9, 9, 5, 7, 1, {1, 2, 3}};
  qn_view_default_params(&p);
  if (p.gain_mask != (1u << QN_OCC_UNKNOWN) || p.stop_mask != (1u << QN_OCC_OCCUPIED) || p.max_through != 0 || p.iz_lo != 0 || p.iz_hi != INT32_MAX || p.reserved[0] ||
      p.reserved[1] || p.reserved[2])
    return 1;
  if (QN_VIEW_OK != 0 || QN_VIEW_OUTSIDE != 1 || QN_VIEW_MAX_OFFSET != 33554432) return 1;
  // two beams at -45 and +45 degrees, four steps of a turn, ten voxels: beam-major
  const std::vector<int32_t> t = qn_map::sensorRays(0.5, 5.0, 2, 4, -45.0, 45.0);
  if (t.size() != 24 || t[0] != 7241 || t[1] != 0 || t[2] != -7241 || t[3 * 1 + 1] != 7241 || t[3 * 4 + 2] != 7241 || t[3 * 6] != -7241) return 1;
  qn_map::MapViewGain m{};
  m.views.resize(3);
  m.views[0].status = QN_VIEW_OUTSIDE; m.views[0].gain = 99; m.views[1].gain = 4; m.views[2].gain = 4;
  m.grid.width = 2; m.grid.height = 3; m.grid.depth = 4;
  if (m.best() != 1 || m.voxels() != 24) return 1;
  const std::vector<double> one = {0.5, 0.5, 0.5};
  const std::vector<int32_t> ray = {1024, 0, 0};
  qn_view_params rev, both;
  qn_view_default_params(&rev); qn_view_default_params(&both);
  rev.iz_lo = 3; rev.iz_hi = 2; both.stop_mask = 5;
  if (!refuses<std::invalid_argument>([&] { qn_map::sensorRays(1.0, 32769.0, 1, 4, 0.0, 0.0); })) return 2;
  if (!refuses<std::invalid_argument>([&] { qn_map::sensorRays(0.3, 20.0, 0, 300, -15.0, 15.0); })) return 3;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapViewGain(nullptr, {}, ray); })) return 4;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapViewGain(nullptr, one, {1024, 0}); })) return 5;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapViewGain(nullptr, one, ray, &rev); })) return 6;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapViewGain(nullptr, one, ray, &both); })) return 7;
  if (!refuses<std::invalid_argument>([&] { qn_map::mapViewGain(nullptr, one, {0, QN_VIEW_MAX_OFFSET + 1, 0}); })) return 8;
  if (!refuses<std::runtime_error>([&] { qn_map::mapViewGain(nullptr, one, ray); })) return 9;
  if (!refuses<std::runtime_error>([&] { qn_map::viewCover(nullptr); })) return 10;
  std::printf("params %zu bytes, info %zu bytes, stats %zu bytes\n", sizeof(qn_view_params), sizeof(qn_view_info), sizeof(qn_view_stats));
  return 0;
}
