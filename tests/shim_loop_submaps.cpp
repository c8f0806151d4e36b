// One loop-closure query against K candidates written against qn_map::loopSubmapPairs: keyframes uploaded once, the query's submap and every
// candidate's in one qn_kf_assemble_batch, one on-device pair per candidate sharing the source.
// usage: shim_loop_submaps keyframes.bin poses.bin query submap_range leaf enable_quatro enable_submap_matching out.bin cand...
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z) float32; poses.bin: one row-major 4x4 float64 per keyframe
//   out.bin: per submap (query first, then each candidate) uint32 n, then n x (x, y, z) float32; prints the pair count and whether all share one source
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <qn_map/loop_submaps.hpp>

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  qn_kf_store* store = nullptr;
  if (qn_kf_store_create(0, &store) != QN_OK) return 5;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t n = 0;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::vector<float> xyz(3 * (size_t)n);
    if (n && std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size()) return 4;
    int32_t id = -1;
    if (qn_kf_add(store, n ? xyz.data() : nullptr, n, 12, &id) != QN_OK) return 5;
  }
  std::fclose(f);
  std::vector<Eigen::Matrix4d> poses;
  f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  double T[16];
  while (std::fread(T, 8, 16, f) == 16) { Eigen::Matrix4d M; for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M(r, c) = T[4 * r + c]; poses.push_back(M); }
  std::fclose(f);
  std::vector<int> cands;
  for (int a = 9; a < argc; a++) cands.push_back(std::atoi(argv[a]));
  std::vector<int> status;
  const std::vector<qn_pair_desc> pairs = qn_map::loopSubmapPairs(store, poses, std::atoi(argv[3]), cands, std::atoi(argv[4]), std::atof(argv[5]),
                                                                  std::atoi(argv[6]) != 0, std::atoi(argv[7]) != 0, &status);
  bool shared = true;
  for (const qn_pair_desc& p : pairs) shared = shared && p.src == pairs[0].src && p.ns == pairs[0].ns && p.on_device == 1 && p.stride_bytes == 16;
  f = std::fopen(argv[8], "wb");
  if (!f) return 3;
  for (uint32_t s = 0; s < (uint32_t)status.size(); s++) {
    const uint32_t m = s == 0 ? (pairs.empty() ? 0 : pairs[0].ns) : pairs[s - 1].nt;
    std::vector<float> xyz(3 * (size_t)m);
    if (m && qn_kf_download_batch(store, s, xyz.data()) != QN_OK) return 6;
    std::fwrite(&m, 4, 1, f); std::fwrite(xyz.data(), 4, xyz.size(), f);
  }
  std::fclose(f);
  std::printf("%zu %d\n", pairs.size(), shared ? 1 : 0);
  qn_kf_store_destroy(store);
  return 0;
}
