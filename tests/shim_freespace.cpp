// qn_map::describeRangeImages / freespaceBatch / seeThroughFraction written against the stand-ins: the record layout the header states, the derived figure,
// and the refusal of a null store (which needs no device).  The GPU side is covered from Python (tests/test_gpu_freespace.py).
#include <cstdio>
#include <cstddef>
#include <qn_map/freespace.hpp>

static_assert(sizeof(qn_freespace_dir) == 32 && sizeof(qn_freespace) == 64 && sizeof(qn_range_params) == 56, "the layout include/qn_engine.h states");
static_assert(offsetof(qn_freespace_dir, seen_through) == 16 && offsetof(qn_freespace, c_in_q) == 32 && offsetof(qn_range_params, tol_abs) == 40, "the layout include/qn_engine.h states");

int main() {
  qn_freespace_dir d{100, 90, 80, 40, 10, 5, 25, 0}, none{3, 3, 0, 0, 0, 0, 0, 0};
  if (qn_map::seeThroughFraction(d) != 0.25 || qn_map::seeThroughFraction(none) != 0.0) return 1;
  std::printf("fraction %.2f\n", qn_map::seeThroughFraction(d));
  if (!qn_map::freespaceBatch(nullptr, {}, {}, {}).empty() || !qn_map::describeRangeImages(nullptr, {}).empty()) return 2;
  try {
    qn_map::freespaceBatch(nullptr, {1}, {0}, std::vector<double>(15, 0.0));
    return 3;
  } catch (const std::invalid_argument&) {
  }
  try {
    qn_map::describeRangeImages(nullptr, {0});
    return 4;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::freespaceBatch(nullptr, {1}, {0}, std::vector<double>(16, 0.0));
    return 5;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  return 0;
}
