// One Scan Context candidate query written against qn_map::scanContextCandidates: keyframes uploaded once, every one described on the GPU,
// the query ranked against the older ones.
// usage: shim_scan_context keyframes.bin stamps.bin query tdiff top_k max_dist
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z) float32; stamps.bin: one float64 per keyframe
//   prints one line per candidate: index, D and yaw (%.17g)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <qn_map/scan_context.hpp>

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  qn_kf_store* store = nullptr;
  if (qn_kf_store_create(0, &store) != QN_OK) return 5;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t n = 0;
  std::vector<int32_t> ids;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::vector<float> xyz(3 * (size_t)n);
    if (n && std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) return 4;
    int32_t id = -1;
    if (qn_kf_add(store, n ? xyz.data() : nullptr, n, 12, &id) != QN_OK) return 5;
    ids.push_back(id);
  }
  std::fclose(f);
  std::vector<double> stamps(ids.size());
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(stamps.data(), 8, stamps.size(), f) != stamps.size()) return 3;
  std::fclose(f);
  if (qn_kf_sc_describe(store, ids.data(), (uint32_t)ids.size()) != QN_OK) return 6;
  const qn_map::ScCandidates c = qn_map::scanContextCandidates(store, stamps, std::atoi(argv[3]), std::atof(argv[4]), std::atoi(argv[5]), std::atof(argv[6]));
  for (size_t k = 0; k < c.idx.size(); k++) std::printf("%d %.17g %.17g\n", c.idx[k], c.dist[k], c.yaw[k]);
  qn_kf_store_destroy(store);
  return 0;
}
