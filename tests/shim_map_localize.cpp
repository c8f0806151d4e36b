// qn_map::cropMap / localizeInMap / localizeInMapCoarseToFine written against the stand-ins.
// No device needed: the record layouts the headers state, the defaults, and the refusal of a null store by the three helpers.
#include <cstdio>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <qn_map/map_localize.hpp>

static_assert(sizeof(qn_localize_params) == 32 && offsetof(qn_localize_params, leaf) == 8 && offsetof(qn_localize_params, score_thr) == 16 &&
              offsetof(qn_localize_params, shape) == 24 && offsetof(qn_localize_params, reserved) == 28, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_localize_stats) == 40 && offsetof(qn_localize_stats, n_crops) == 12 && offsetof(qn_localize_stats, passes) == 16 &&
              offsetof(qn_localize_stats, crop_points) == 24 && offsetof(qn_localize_stats, generation) == 32, "the layout include/qn_engine.h states");

static int selfCheck() {
  qn_localize_params p{0.0, 0.0, 0.0, 7, 9};
  qn_localize_default_params(&p);
  if (p.radius != 35.0 || p.leaf != 0.3 || p.score_thr != 1.5 || p.shape != QN_LOCALIZE_SPHERE || p.reserved != 0 || QN_LOCALIZE_CYLINDER != 1) return 1;
  const std::vector<std::array<double, 3>> c{{0.0, 0.0, 0.0}};
  const std::vector<int32_t> q{0};
  std::array<double, 16> g{};
  for (int i = 0; i < 4; i++) g[5 * i] = 1.0;
  try { qn_map::cropMap(nullptr, c, 1.0); return 2; } catch (const std::runtime_error& e) { std::printf("refused: %s\n", e.what()); }
  try { qn_map::localizeInMap(nullptr, nullptr, q, {g}); return 3; } catch (const std::runtime_error& e) { std::printf("refused: %s\n", e.what()); }
  try { qn_map::localizeInMapCoarseToFine(nullptr, nullptr, q, {g}); return 4; } catch (const std::runtime_error& e) { std::printf("refused: %s\n", e.what()); }
  std::printf("params %zu bytes, stats %zu bytes\n", sizeof(qn_localize_params), sizeof(qn_localize_stats));
  return 0;
}

int main() { return selfCheck(); }
