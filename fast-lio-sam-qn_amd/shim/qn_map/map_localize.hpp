// Drop-in helper for localising scans in the corrected global map: where a user of the reference would save the map (config.yaml, save_map_bag) and run
// FAST-LIO-Localization-QN - Quatro + Nano-GICP of a scan against the neighbourhood of a pose guess - on the host, cropMap cuts the neighbourhoods out of the
// resident map on the GPU and localizeInMap / localizeInMapCoarseToFine register resident keyframes against them in one batched pass.
// Header-only; forwards to the C-ABI in include/qn_engine.h.  Link with -lqn_engine.  Uses nothing from Eigen or PCL.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "qn_engine.h"
#include "detail.hpp"

namespace qn_map {

struct MapCrop {
  const float* d_xyzi = nullptr;                                   // device address of the n float4 records x y z intensity (nullptr when empty);
  uint32_t n = 0;                                                  // valid until the next cropMap / localizeInMap on the store
  std::vector<uint32_t> idx;                                       // their map indices, ascending
};

struct MapLocalization {
  qn_gicp_result record;                                           // the (fine) registration's record
  bool valid = false;
  int status = QN_OK;                                              // QN_ERR_EMPTY_CLOUD: an empty scan or crop; QN_ERR_CAPACITY: above the context's max_points
  double pose[16];                                                 // map <- sensor, row-major: the record's T64 (GICP) or T_gicp * T_quatro (coarse to fine)
  double T_quatro[16];                                             // coarse to fine only (else the identity)
};

namespace detail {
inline void check_sizes(const std::vector<int32_t>& query, const std::vector<std::array<double, 16>>& guesses) {
  if (query.size() != guesses.size()) throw std::invalid_argument("[qn_map] localizeInMap: one guess per query");
}
}  // namespace detail

// the neighbourhoods of `centres` within `radius` of the store's map slot (qn_kf_map_crop), each with its map indices when with_indices
inline std::vector<MapCrop> cropMap(qn_kf_store* store, const std::vector<std::array<double, 3>>& centres, double radius, uint32_t shape = QN_LOCALIZE_SPHERE,
                                    bool with_indices = true) {
  std::vector<uint32_t> counts(centres.size() + 1, 0);
  int rc = qn_kf_map_crop(store, centres.empty() ? nullptr : centres[0].data(), (uint32_t)centres.size(), radius, shape, counts.data());
  if (rc != QN_OK) throw std::runtime_error(detail::why("qn_kf_map_crop", rc, store));
  std::vector<MapCrop> out(centres.size());
  for (uint32_t c = 0; c < (uint32_t)centres.size(); c++) {
    if (with_indices) out[c].idx.resize(counts[c]);
    rc = qn_kf_map_crop_get(store, c, &out[c].d_xyzi, &out[c].n, with_indices && counts[c] ? out[c].idx.data() : nullptr);
    if (rc != QN_OK || out[c].n != counts[c]) throw std::runtime_error(detail::why("qn_kf_map_crop_get", rc, store));
  }
  return out;
}

// keyframe query[j] registered against the map around guesses[j] (map <- sensor), seeded with it (qn_kf_map_localize).  params NULL: the defaults.
inline std::vector<MapLocalization> localizeInMap(qn_kf_store* store, qn_ctx* ctx, const std::vector<int32_t>& query, const std::vector<std::array<double, 16>>& guesses,
                                                  const qn_localize_params* params = nullptr, qn_localize_stats* stats = nullptr) {
  detail::check_sizes(query, guesses);
  const qn_localize_params p = detail::params_or(params, qn_localize_default_params);
  const size_t n = query.size();
  std::vector<qn_gicp_result> res(n + 1); std::vector<int> valid(n + 1, 0), status(n + 1, 0);
  const int rc = qn_kf_map_localize(store, ctx, &p, n ? query.data() : nullptr, n ? guesses[0].data() : nullptr, (uint32_t)n,
                                    res.data(), valid.data(), status.data(), stats);
  if (rc != QN_OK) throw std::runtime_error(detail::why("qn_kf_map_localize", rc, store));
  std::vector<MapLocalization> out(n);
  for (size_t j = 0; j < n; j++) {
    out[j].record = res[j]; out[j].valid = valid[j] != 0; out[j].status = status[j];
    std::memcpy(out[j].pose, res[j].T64, sizeof(out[j].pose));
    for (int i = 0; i < 16; i++) out[j].T_quatro[i] = i % 5 == 0 ? 1.0 : 0.0;
  }
  return out;
}

// the same coarse to fine: only the guess's translation is used, as the crop centre (qn_kf_map_localize_c2f)
inline std::vector<MapLocalization> localizeInMapCoarseToFine(qn_kf_store* store, qn_ctx* ctx, const std::vector<int32_t>& query,
                                                              const std::vector<std::array<double, 16>>& guesses, const qn_localize_params* params = nullptr,
                                                              qn_localize_stats* stats = nullptr) {
  detail::check_sizes(query, guesses);
  const qn_localize_params p = detail::params_or(params, qn_localize_default_params);
  const size_t n = query.size();
  std::vector<qn_gicp_result> res(n + 1); std::vector<int> valid(n + 1, 0), status(n + 1, 0);
  std::vector<double> Tt(16 * (n + 1)), Tq(16 * (n + 1));
  const int rc = qn_kf_map_localize_c2f(store, ctx, &p, n ? query.data() : nullptr, n ? guesses[0].data() : nullptr, (uint32_t)n,
                                        res.data(), Tt.data(), Tq.data(), valid.data(), status.data(), stats);
  if (rc != QN_OK) throw std::runtime_error(detail::why("qn_kf_map_localize_c2f", rc, store));
  std::vector<MapLocalization> out(n);
  for (size_t j = 0; j < n; j++) {
    out[j].record = res[j]; out[j].valid = valid[j] != 0; out[j].status = status[j];
    std::memcpy(out[j].pose, Tt.data() + 16 * j, sizeof(out[j].pose));
    std::memcpy(out[j].T_quatro, Tq.data() + 16 * j, sizeof(out[j].T_quatro));
  }
  return out;
}

}  // namespace qn_map
