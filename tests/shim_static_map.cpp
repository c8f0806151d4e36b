// qn_map::staticMapWitnesses / classifyStatic / buildStaticMap written against the stand-ins.
// Without arguments (no device needed): the record layout the header states, the default witness list of a small hand-made trajectory, and the refusal of a
// null store.
// usage on a GPU: shim_static_map keyframes.bin poses.bin range_params.bin radius max_k leaf
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: 16 float64 per keyframe; range_params.bin: one qn_range_params
//   prints "witnesses" and the list, one "removed <entry> <count> <status>" line per keyframe, "map <points> <fnv1a64 of its bytes>"
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <vector>
#include <qn_map/freespace.hpp>
#include <qn_map/static_map.hpp>

static_assert(sizeof(qn_static_params) == 8 && offsetof(qn_static_params, agree_weight) == 4, "the layout include/qn_engine.h states");

static std::vector<double> posesAt(const std::vector<double>& xyz) {
  std::vector<double> P(16 * (xyz.size() / 3), 0.0);
  for (size_t k = 0; k < xyz.size() / 3; k++) {
    for (int i = 0; i < 4; i++) P[16 * k + 5 * i] = 1.0;
    P[16 * k + 3] = xyz[3 * k]; P[16 * k + 7] = xyz[3 * k + 1]; P[16 * k + 11] = xyz[3 * k + 2];
  }
  return P;
}

static int selfCheck() {
  qn_static_params p{0, 0};
  qn_static_default_params(&p);
  if (p.min_see_through != 2 || p.agree_weight != 1) return 1;
  // five entries on a line, entry 4 a second visit of keyframe 0 at 0.5: ties go to the lower position, the own id is never a witness
  const std::vector<int> ids = {0, 1, 2, 3, 0};
  const std::vector<double> P = posesAt({0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0, 0.5, 0, 0});
  const qn_map::StaticWitnesses w = qn_map::staticMapWitnesses(ids, P, 1.6, 2);
  const std::vector<uint32_t> off = {0, 1, 3, 5, 6, 8}, wit = {1, 4, 0, 1, 3, 2, 1, 2};
  if (w.off != off || w.wit != wit) return 2;
  std::printf("witnesses");
  for (uint32_t x : w.wit) std::printf(" %u", x);
  std::printf("\n");
  if (!qn_map::classifyStatic(nullptr, {}, {}, qn_map::StaticWitnesses{{0}, {}}).removed.empty()) return 3;
  try {
    qn_map::classifyStatic(nullptr, {0, 1}, std::vector<double>(31, 0.0), w);
    return 4;
  } catch (const std::invalid_argument&) {
  }
  try {
    qn_map::staticMapWitnesses(ids, P, 1.0, 256);
    return 5;
  } catch (const std::invalid_argument&) {
  }
  try {
    qn_map::classifyStatic(nullptr, ids, P, w);
    return 6;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  try {
    qn_map::buildStaticMap(nullptr, 0.3);
    return 7;
  } catch (const std::runtime_error& e) {
    std::printf("refused: %s\n", e.what());
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 7) return selfCheck();
  qn_kf_store* store = nullptr;
  if (qn_kf_store_create(0, &store) != QN_OK) return 5;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t n = 0;
  std::vector<int> ids;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::vector<float> rec(4 * (size_t)n);
    if (n && std::fread(rec.data(), 4, rec.size(), f) != rec.size()) return 4;
    int32_t id = -1;
    if (qn_kf_add_xyzi(store, n ? rec.data() : nullptr, n, 16, 12, &id) != QN_OK) return 5;
    ids.push_back(id);
  }
  std::fclose(f);
  std::vector<double> poses(16 * ids.size());
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 3;
  std::fclose(f);
  qn_range_params rp;
  f = std::fopen(argv[3], "rb");
  if (!f || std::fread(&rp, sizeof(rp), 1, f) != 1) return 3;
  std::fclose(f);
  if (qn_kf_range_set_params(store, &rp) != QN_OK) return 6;
  qn_map::describeRangeImages(store, ids);
  const qn_map::StaticWitnesses w = qn_map::staticMapWitnesses(ids, poses, std::atof(argv[4]), (uint32_t)std::atoi(argv[5]));
  std::printf("witnesses");
  for (uint32_t x : w.wit) std::printf(" %u", x);
  std::printf("\n");
  const qn_map::StaticClassified c = qn_map::classifyStatic(store, ids, poses, w);
  for (size_t e = 0; e < ids.size(); e++) std::printf("removed %zu %u %d\n", e, c.removed[e], c.status[e]);
  const uint32_t m = qn_map::buildStaticMap(store, std::atof(argv[6]));
  std::vector<float> map(4 * (size_t)m);
  if (m && qn_kf_download_map(store, map.data(), 16, 12) != QN_OK) return 7;
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)map.data();
  for (size_t k = 0; k < 16 * (size_t)m; k++) { h ^= b[k]; h *= 1099511628211ull; }
  std::printf("map %u %llu\n", m, h);
  qn_kf_store_destroy(store);
  return 0;
}
