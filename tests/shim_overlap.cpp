// qn_map::verifyOverlap / overlapFraction / inlierRmse written against the stand-ins: the record layout the header states, the derived figures, and the
// refusal of a null store (which needs no device).  With a store argument "gpu" it is not used; the GPU side is covered from Python (tests/test_gpu_overlap.py).
#include <cstdio>
#include <cstddef>
#include <qn_map/scan_context.hpp>

static_assert(sizeof(qn_overlap_dir) == 24 && sizeof(qn_overlap) == 48, "the layout include/qn_engine.h states");
static_assert(offsetof(qn_overlap_dir, sum_d2) == 16 && offsetof(qn_overlap, b_to_a) == 24, "the layout include/qn_engine.h states");

int main() {
  qn_overlap_dir d{10, 8, 4, 0, 1.0}, none{3, 0, 0, 0, 0.0};
  if (qn_map::overlapFraction(d) != 0.5 || qn_map::inlierRmse(d) != 0.5 || qn_map::overlapFraction(none) != 0.0 || qn_map::inlierRmse(none) != 0.0) return 1;
  if (!qn_map::verifyOverlap(nullptr, 0, 0.3).empty()) return 2;
  try {
    qn_map::verifyOverlap(nullptr, 2, 0.3);
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  return 0;
}
