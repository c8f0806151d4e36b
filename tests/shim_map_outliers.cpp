// qn_map::mapOutliers / removeMapOutliers written against the stand-ins.
// Without arguments (no device needed): the record layouts the headers state, the defaults, and the refusal of a null store by both helpers.
// usage on a GPU: shim_map_outliers keyframes.bin poses.bin leaf radius std_mul k
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "outliers <points> <dense> <removed> <fnv1a64 of count, mean_q and removed per point>" and
//          "filtered <points> <fnv1a64 of the xyz and intensity bytes of the filtered map>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <qn_map/map_outliers.hpp>

static_assert(sizeof(qn_outlier_params) == 24 && offsetof(qn_outlier_params, std_mul) == 8 && offsetof(qn_outlier_params, k) == 16 &&
              offsetof(qn_outlier_params, reserved) == 20, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_outlier_stats) == 64 && offsetof(qn_outlier_stats, quant_exp) == 20 && offsetof(qn_outlier_stats, sum_q) == 24 &&
              offsetof(qn_outlier_stats, mean_q) == 40 && offsetof(qn_outlier_stats, thr_q) == 56, "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_outlier_params p{0.0, -1.0, 0, 9};
  qn_outlier_default_params(&p);
  if (p.radius != 1.0 || p.std_mul != 2.0 || p.k != 8 || p.reserved != 0 || QN_OUTLIER_MAX_K != 32) return 1;
  try {
    qn_map::mapOutliers(nullptr, nullptr);
    return 2;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::removeMapOutliers(nullptr);
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("params %zu bytes, stats %zu bytes\n", sizeof(qn_outlier_params), sizeof(qn_outlier_stats));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 7) return selfCheck();
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
  qn_outlier_params p;
  qn_outlier_default_params(&p);
  p.radius = std::atof(argv[4]); p.std_mul = std::atof(argv[5]); p.k = (uint32_t)std::atoi(argv[6]);
  const qn_map::MapOutliers m = qn_map::mapOutliers(store, &p);
  if (m.size() != nm) return 8;
  unsigned long long ho = 1469598103934665603ull, hm = ho;
  for (size_t i = 0; i < m.size(); i++) { ho = fnv(ho, &m.neighbors[i], 4); ho = fnv(ho, &m.mean_q[i], 4); ho = fnv(ho, &m.removed[i], 1); }
  std::printf("outliers %zu %u %u %016llx\n", m.size(), m.stats.dense, m.stats.removed, ho);
  const uint32_t left = qn_map::removeMapOutliers(store);
  if (left != nm - m.stats.removed) return 9;
  std::vector<float> out(4 * (size_t)left + 4);
  if (qn_kf_download_map(store, out.data(), 16, 12) != QN_OK) return 10;
  for (size_t i = 0; i < left; i++) hm = fnv(hm, &out[4 * i], 16);
  std::printf("filtered %u %016llx\n", left, hm);
  qn_kf_store_destroy(store);
  return 0;
}
