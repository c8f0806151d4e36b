// Scan Context candidates of MANY queries verified drift-free submap against submap, written against qn_map::scanContextCandidatesMany +
// qn_map::describeLocalSubmaps + qn_map::verifyLoopPairsSubmap / qn_map::verifyLoopPairsSubmapCoarseToFine: keyframes uploaded once, every keyframe's local
// submap described once on the GPU, every query ranked in one qn_kf_sc_query, every (query, candidate) pair registered in one batch.
// usage: shim_submap_verify keyframes.bin stamps.bin poses.bin tdiff top_k max_dist submap_range leaf max_corr_dist c2f query...
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z) float32; stamps.bin: one float64 per keyframe; poses.bin: 16 float64 per keyframe
//   NanoGICP as LoopClosure's ctor sets it (k 15, 32 iterations, transformation epsilon 0.01, max_corr_dist from the command line), Quatro at its
//   defaults, score_thr 1.5; c2f 0: verifyLoopPairsSubmap, 1: verifyLoopPairsSubmapCoarseToFine.  Prints one line per pair: query, candidate, valid, status,
//   score (%.17g) and the 16 entries of T (%.17g)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <qn_map/scan_context.hpp>

int main(int argc, char** argv) {
  if (argc < 12) return 2;
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
  p.k_correspondences = 15; p.max_iterations = 32; p.transformation_epsilon = 0.01; p.max_corr_dist = std::atof(argv[9]);
  if (qn_gicp_set_params(ctx, &p) != QN_OK) return 8;
  qn_quatro_params qp;
  qn_quatro_default_params(&qp);
  if (qn_quatro_set_params(ctx, &qp) != QN_OK) return 8;
  std::vector<int> queries;
  for (int a = 11; a < argc; a++) queries.push_back(std::atoi(argv[a]));
  const qn_map::ScPairs c = qn_map::scanContextCandidatesMany(store, stamps, queries, std::atof(argv[4]), std::atoi(argv[5]), std::atof(argv[6]));
  const bool c2f = std::atoi(argv[10]) != 0;
  const std::vector<int> all(ids.begin(), ids.end());
  for (int st : qn_map::describeLocalSubmaps(store, ctx, all, poses, std::atoi(argv[7]), std::atof(argv[8]), c2f)) if (st != QN_OK) return 9;
  const std::vector<qn_map::ScVerifiedPair> v = c2f ? qn_map::verifyLoopPairsSubmapCoarseToFine(store, ctx, c, 1.5) : qn_map::verifyLoopPairsSubmap(store, ctx, c, 1.5);
  for (const qn_map::ScVerifiedPair& r : v) {
    std::printf("%d %d %d %d %.17g", r.query, r.idx, r.valid ? 1 : 0, r.status, r.score);
    for (int i = 0; i < 16; i++) std::printf(" %.17g", r.T[i]);
    std::printf("\n");
  }
  qn_ctx_destroy(ctx);
  qn_kf_store_destroy(store);
  return 0;
}
