// The second translation unit of tests/shim_detail.cpp: the same headers once more, and one refusal through them from here.
#include <cstdio>
#include <stdexcept>
#include "shim_detail_headers.h"

int second_unit_lines() {
  try {
    qn_map::distanceSlice(nullptr, 0, 1);
  } catch (const std::runtime_error& e) {
    std::printf("second unit: %s\n", e.what());
    return 0;
  }
  return 1;
}
