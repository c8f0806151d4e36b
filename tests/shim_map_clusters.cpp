// qn_map::mapClusters / dropRejectedClusters written against the stand-ins.
// Without arguments (no device needed): the record layouts the headers state, the defaults, and the refusal of a null store by both helpers.
// usage on a GPU: shim_map_clusters keyframes.bin poses.bin leaf tolerance min_size max_size
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "clusters <points> <components> <clusters> <edges> <fnv1a64 of label, root and size per point> <fnv1a64 of root, size, lo, hi and centroid per
//          cluster>" and "filtered <points> <fnv1a64 of the xyz and intensity bytes of the filtered map>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <qn_map/map_clusters.hpp>

static_assert(sizeof(qn_cluster_params) == 24 && offsetof(qn_cluster_params, min_size) == 8 && offsetof(qn_cluster_params, max_size) == 12 &&
              offsetof(qn_cluster_params, class_mask) == 16 && offsetof(qn_cluster_params, reserved) == 20, "the layout include/qn_engine.h states");
static_assert(sizeof(qn_cluster_info) == 56 && offsetof(qn_cluster_info, lo) == 8 && offsetof(qn_cluster_info, hi) == 20 && offsetof(qn_cluster_info, sum_q) == 32,
              "the layout include/qn_engine.h states");
static_assert(sizeof(qn_cluster_stats) == 56 && offsetof(qn_cluster_stats, components) == 12 && offsetof(qn_cluster_stats, largest) == 36 &&
              offsetof(qn_cluster_stats, quant_exp) == 40 && offsetof(qn_cluster_stats, edges) == 48, "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_cluster_params p{0.0, 0, 0, 7, 9};
  qn_cluster_default_params(&p);
  if (p.tolerance != 0.5 || p.min_size != 10 || p.max_size != 0xffffffffu || p.class_mask != 0 || p.reserved != 0 || QN_CLUSTER_REJECTED != -1 ||
      QN_CLUSTER_NONE != -2)
    return 1;
  try {
    qn_map::mapClusters(nullptr, nullptr);
    return 2;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::dropRejectedClusters(nullptr);
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  std::printf("params %zu bytes, info %zu bytes, stats %zu bytes\n", sizeof(qn_cluster_params), sizeof(qn_cluster_info), sizeof(qn_cluster_stats));
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
  qn_cluster_params p;
  qn_cluster_default_params(&p);
  p.tolerance = std::atof(argv[4]); p.min_size = (uint32_t)std::strtoul(argv[5], nullptr, 10); p.max_size = (uint32_t)std::strtoul(argv[6], nullptr, 10);
  const qn_map::MapClusters m = qn_map::mapClusters(store, &p);
  if (m.label.size() != nm) return 8;
  unsigned long long hp = 1469598103934665603ull, hc = hp, hm = hp;
  for (size_t i = 0; i < m.label.size(); i++) { hp = fnv(hp, &m.label[i], 4); hp = fnv(hp, &m.root[i], 4); hp = fnv(hp, &m.size[i], 4); }
  for (const qn_map::MapCluster& c : m.clusters) {
    hc = fnv(hc, &c.root, 4); hc = fnv(hc, &c.size, 4); hc = fnv(hc, c.lo, 12); hc = fnv(hc, c.hi, 12); hc = fnv(hc, c.centroid, 24);
  }
  std::printf("clusters %zu %u %u %llu %016llx %016llx\n", m.label.size(), m.stats.components, m.stats.clusters, (unsigned long long)m.stats.edges, hp, hc);
  const uint32_t left = qn_map::dropRejectedClusters(store);
  if (left != nm - m.stats.rejected_points) return 9;
  std::vector<float> out(4 * (size_t)left + 4);
  if (left && qn_kf_download_map(store, out.data(), 16, 12) != QN_OK) return 10;
  for (size_t i = 0; i < left; i++) hm = fnv(hm, &out[4 * i], 16);
  std::printf("filtered %u %016llx\n", left, hm);
  qn_kf_store_destroy(store);
  return 0;
}
