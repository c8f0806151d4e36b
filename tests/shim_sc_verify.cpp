// Scan Context candidates of one query verified drift-free, written against qn_map::scanContextCandidates + qn_map::verifyScanContextCandidates:
// keyframes uploaded once and described on the GPU, the query ranked against the older ones, its candidates registered in one batch.
// usage: shim_sc_verify keyframes.bin stamps.bin poses.bin query tdiff top_k max_dist submap_range leaf max_corr_dist
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z) float32; stamps.bin: one float64 per keyframe; poses.bin: 16 float64 per keyframe
//   NanoGICP as LoopClosure's ctor sets it (k 15, 32 iterations, transformation epsilon 0.01, max_corr_dist from the command line), score_thr 1.5
//   prints one line per candidate: index, valid, status, score (%.17g) and the 16 entries of T (%.9g)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <qn_map/scan_context.hpp>

int main(int argc, char** argv) {
  if (argc < 11) return 2;
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
  std::vector<double> stamps(ids.size()), poses(16 * ids.size());
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(stamps.data(), 8, stamps.size(), f) != stamps.size()) return 3;
  std::fclose(f);
  f = std::fopen(argv[3], "rb");
  if (!f || std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 3;
  std::fclose(f);
  if (qn_kf_sc_describe(store, ids.data(), (uint32_t)ids.size()) != QN_OK) return 6;
  qn_ctx* ctx = nullptr;
  if (qn_ctx_create(0, 200000, &ctx) != QN_OK) return 7;
  qn_gicp_params p;
  qn_gicp_default_params(&p);
  p.k_correspondences = 15; p.max_iterations = 32; p.transformation_epsilon = 0.01; p.max_corr_dist = std::atof(argv[10]);
  if (qn_gicp_set_params(ctx, &p) != QN_OK) return 8;
  const int query = std::atoi(argv[4]);
  const qn_map::ScCandidates c = qn_map::scanContextCandidates(store, stamps, query, std::atof(argv[5]), std::atoi(argv[6]), std::atof(argv[7]));
  const std::vector<qn_map::ScVerified> v = qn_map::verifyScanContextCandidates(store, ctx, query, c, poses, std::atoi(argv[8]), std::atof(argv[9]), 1.5);
  for (const qn_map::ScVerified& r : v) {
    std::printf("%d %d %d %.17g", r.idx, r.valid ? 1 : 0, r.status, r.score);
    for (int i = 0; i < 16; i++) std::printf(" %.9g", r.T[i]);
    std::printf("\n");
  }
  qn_ctx_destroy(ctx);
  qn_kf_store_destroy(store);
  return 0;
}
