// qn_map::mapNormals written against the stand-ins.
// Without arguments (no device needed): the record layouts the headers state, the defaults, and the refusal of a null store and of a ragged pose list.
// usage on a GPU: shim_map_normals keyframes.bin poses.bin leaf radius min_neighbors
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe
//   prints "map <points> <fnv1a64 of the xyz and intensity bytes>" and "normals <points> <valid> <fnv1a64 of normal, curvature, neighbours and view>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <pcl/point_cloud.h>
#include <qn_map/map_normals.hpp>

static_assert(sizeof(qn_normal_params) == 16 && offsetof(qn_normal_params, min_neighbors) == 8 && offsetof(qn_normal_params, reserved) == 12,
              "the layout include/qn_engine.h states");

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static int selfCheck() {
  qn_normal_params p{0.0, 0, 9};
  qn_normal_default_params(&p);
  if (p.radius != 0.6 || p.min_neighbors != 5 || p.reserved != 0) return 1;
  try {
    qn_map::mapNormals(nullptr, nullptr, std::vector<double>(17, 0.0));
    return 2;
  } catch (const std::invalid_argument&) {
  }
  try {
    qn_map::mapNormals(nullptr, &p, std::vector<double>(16, 0.0));
    return 3;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  pcl::PointCloud<qn_map::PointXYZINormal> cloud;                   // the records fit the stand-in cloud as they fit PCL's
  cloud.push_back(qn_map::PointXYZINormal{});
  std::printf("record %zu bytes\n", sizeof(cloud[0]));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return selfCheck();
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
  qn_normal_params p;
  qn_normal_default_params(&p);
  p.radius = std::atof(argv[4]); p.min_neighbors = (uint32_t)std::atoi(argv[5]);
  const qn_map::MapWithNormals m = qn_map::mapNormals(store, &p, poses);
  if (m.size() != nm) return 8;
  unsigned long long hm = 1469598103934665603ull, hn = hm;
  size_t valid = 0;
  for (size_t i = 0; i < m.size(); i++) {
    const qn_map::PointXYZINormal& q = m.points[i];
    hm = fnv(hm, &q.x, 12); hm = fnv(hm, &q.intensity, 4);
    hn = fnv(hn, &q.normal_x, 12); hn = fnv(hn, &q.curvature, 4); hn = fnv(hn, &m.neighbors[i], 4); hn = fnv(hn, &m.view[i], 4);
    valid += std::isfinite(q.curvature) ? 1 : 0;
  }
  std::printf("map %zu %016llx\nnormals %zu %zu %016llx\n", m.size(), hm, m.size(), valid, hn);
  qn_kf_store_destroy(store);
  return 0;
}
