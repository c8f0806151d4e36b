// qn_staticmap.hip - the corrected map without the records other keyframes saw through (qn_kf_static_classify / _points, qn_kf_build_map_static:
// include/qn_engine.h).  The numpy twin qn_amd/staticmap.py is the specification.  A record of list entry e is a vote "seen through" of witness w when,
// carried into w's sensor frame by M = inv(P_w) P_e, it lies where w's rays passed on their way to a farther surface: class 2 of the free-space check, by
// the same projection, images, window and tolerances (qn_range.cuh, shared with qn_freespace.hip).  The votes are integers, so the records removed and the map
// built from the rest equal the twin's bit for bit.
// Kernels:
//   k_static_vote     grid (tiles, entries), one thread per record, the witness loop inside the thread: the record is read once, the 12 f64 of M and the image
//                     slot of (entry, witness) come from a host-built table through wave-uniform loads, both counters stay in registers, the three bytes per
//                     record (seen through, agree, removed) are written once; the tile's kept count by ballots and popcounts into its own slot.  No atomics.
//   k_static_scan     one block: the exclusive scan of the tiles' kept counts in tile order (scan_row of qn_map_compact.cuh; the entries' kept records end up back
//                     to back in list order), and each entry's removed count.
//   k_static_compact  grid (tiles, entries): the kept records of a tile to its offset, in record order (ballot / popcount ranks inside a wave, the waves' and
//                     rounds' counts in a fixed order through LDS; lane_rank of qn_map_compact.cuh): stable and the same on every run.
// The column table is staged in LDS up to 4096 columns and read from global memory above, as in qn_freespace.hip.
// Host synchronisations: one per classify.  The map itself is the store's one voxel-grid pipeline over the kept records (qn_kf_int_build_map_from).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include "../../include/qn_engine.h"
#include "qn_range.cuh"
#include "qn_map_compact.cuh"
#include "qn_dense_grid.cuh"
#include "qn_union_find.cuh"

namespace {
using namespace qn_range;

#define SV_MAX_WITNESSES 255u                            // per entry: the u8 counters stay exact
#define SV_CHUNK 32768u                                  // entries per launch (the grid's y dimension), here and in qn_mapoccupancy.inc
#define SV_SCAN_BLOCK MO_SCAN_BLOCK

struct SvEntry { const float4* pts; uint32_t n, p0, w0, nw, b0, pad; };      // records, first record / witness row / tile of the entry
struct SvWit { double M[12]; int32_t img; int32_t pad[3]; };                 // inv(P_w) P_e and the witness's image slot (its keyframe id); 112 bytes

// grid (tiles of the largest entry of the launch, entries), dynamic LDS: the column table (LDS) or nothing
template <bool LDS>
__global__ void __launch_bounds__(FS_BLOCK) k_static_vote(const SvEntry* __restrict__ ents, const SvWit* __restrict__ wits, const double* __restrict__ trow,
                                                          const double2* __restrict__ cs, uint32_t nr, uint32_t nc, double min_range, int wr, int wc, double tol_abs,
                                                          double tol_rel, const uint32_t* __restrict__ img, uint32_t min_st, uint32_t agree_w, uint8_t* __restrict__ st_out,
                                                          uint8_t* __restrict__ ag_out, uint8_t* __restrict__ rm_out, uint32_t* __restrict__ tile_kept) {
  __shared__ uint32_t wkept[FS_WAVES];
  const SvEntry E = ents[blockIdx.y];
  const uint32_t n = E.n;
  const uint32_t base = blockIdx.x * FS_TILE;
  if (base >= n) return;                                             // uniform over the block
  const double2* ct = fs_stage<LDS>(cs, nc);
  const size_t npix2 = 2 * (size_t)nr * nc;
  const uint32_t npix = nr * nc;
  const SvWit* W = wits + E.w0;
  uint32_t kept = 0;                                                 // the wave's kept records (the same in every lane)
#pragma unroll 1
  for (uint32_t it = 0; it < FS_ITERS; it++) {
    const uint32_t i = base + it * FS_BLOCK + threadIdx.x;
    bool keep = false;
    if (i < n) {
      const float4 p = E.pts[i];
      const double x = p.x, y = p.y, z = p.z;
      uint32_t st = 0, ag = 0;
#pragma unroll 1
      for (uint32_t w = 0; w < E.nw; w++) {                          // the same trip count and the same M in every lane: scalar loads
        const double* M = W[w].M;
        const double px = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
        const double py = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
        const double pz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
        const uint32_t* near = img + (size_t)W[w].img * npix2;
        bool fin;
        const uint32_t cls = fs_classify(px, py, pz, trow, nr, ct, nc, min_range, wr, wc, tol_abs, tol_rel, near, near + npix, fin);
        st += cls == 2u; ag += cls == 4u;
      }
      const bool rm = st >= min_st && (unsigned long long)st > (unsigned long long)agree_w * ag;
      st_out[E.p0 + i] = (uint8_t)st; ag_out[E.p0 + i] = (uint8_t)ag; rm_out[E.p0 + i] = rm ? 1 : 0;
      keep = !rm;
    }
    kept += __popcll(__ballot(keep));
  }
  if ((threadIdx.x & 63) == 0) wkept[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int w = 0; w < FS_WAVES; w++) acc += wkept[w];
    tile_kept[E.b0 + blockIdx.x] = acc;
  }
}

// one block: off[t] = the kept records of the tiles before t, off[nt] = all (scan_row: qn_map_compact.cuh); then removed[e] = n_e - the kept records of e's tiles
__global__ void __launch_bounds__(SV_SCAN_BLOCK) k_static_scan(const uint32_t* __restrict__ cnt, uint32_t nt, uint32_t* off, const SvEntry* __restrict__ ents,
                                                                uint32_t count, uint32_t* __restrict__ removed) {
  const uint32_t run = scan_row(cnt, nt, off);
  if (threadIdx.x == SV_SCAN_BLOCK - 1) off[nt] = run;
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < count; e += SV_SCAN_BLOCK) {
    const uint32_t n = ents[e].n, b0 = ents[e].b0, nb = (n + FS_TILE - 1) / FS_TILE;
    removed[e] = n - (off[b0 + nb] - off[b0]);
  }
}

// grid as k_static_vote's: the tile's kept records, in record order, to kept[off[tile] ..]
__global__ void __launch_bounds__(FS_BLOCK) k_static_compact(const SvEntry* __restrict__ ents, const uint8_t* __restrict__ rm, const uint32_t* __restrict__ off,
                                                             float4* __restrict__ kept) {
  __shared__ uint32_t cnt[FS_ITERS][FS_WAVES];
  const SvEntry E = ents[blockIdx.y];
  const uint32_t base = blockIdx.x * FS_TILE;
  if (base >= E.n) return;                                           // uniform over the block
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 p[FS_ITERS]; bool keep[FS_ITERS]; unsigned long long bal[FS_ITERS];
#pragma unroll
  for (int it = 0; it < FS_ITERS; it++) {
    const uint32_t i = base + it * FS_BLOCK + threadIdx.x;
    keep[it] = false; p[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < E.n) { keep[it] = rm[E.p0 + i] == 0; p[it] = E.pts[i]; }
    bal[it] = __ballot(keep[it]);
    if (lane == 0) cnt[it][wave] = (uint32_t)__popcll(bal[it]);
  }
  __syncthreads();
  uint32_t acc = off[E.b0 + blockIdx.x];
#pragma unroll
  for (int it = 0; it < FS_ITERS; it++) {
    uint32_t before = acc;
#pragma unroll
    for (int w = 0; w < FS_WAVES; w++) { const uint32_t c = cnt[it][w]; if ((uint32_t)w < wave) before += c; acc += c; }
    if (keep[it]) kept[before + lane_rank(bal[it])] = p[it];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the launches of a kernel over the entries (anything with the record count n), SV_CHUNK of them at a time: f(first entry, grid), the grid's x the tiles (of
// `tile` records) of the chunk's largest entry; a chunk without a record is skipped
template <typename E, typename F> void sv_each_chunk(const E* ent, uint32_t count, uint32_t tile, F f) {
  for (uint32_t a = 0; a < count; a += SV_CHUNK) {
    const uint32_t m = std::min<uint32_t>(SV_CHUNK, count - a);
    uint32_t cmax = 0;
    for (uint32_t k = 0; k < m; k++) cmax = std::max(cmax, ent[a + k].n);
    if (cmax) f(a, dim3((cmax + tile - 1) / tile, m));
  }
}

struct SvHostEntry { const float4* pts; uint32_t n; uint32_t p0; uint32_t kept_off, kept_n; uint8_t has_i; };
// The store's static-map state (slot QN_KF_INT_EXT_STATIC): the list and poses of the latest classify, per record its three bytes (three planes of `total`
// bytes: seen through, agree, removed) and the kept records of every entry back to back in list order.
struct StaticState {
  bool live = false;
  std::vector<int32_t> ids; std::vector<double> poses; std::vector<SvHostEntry> ent;
  uint64_t total = 0;
  DevBuf<uint8_t> votes;                                 // three planes, those of the live call `total` apart
  DevBuf<float4> kept;
  std::shared_ptr<struct OccState> occ;                  // the occupancy map of qn_mapoccupancy.inc (included at the end, where the type is completed)
};

}  // namespace

extern "C" void qn_static_default_params(qn_static_params* p) {
  if (!p) return;
  p->min_see_through = 2; p->agree_weight = 1;
}

extern "C" int qn_kf_static_classify(qn_kf_store* s, const int32_t* ids, const double* poses16, uint32_t count, const uint32_t* wit_off, const uint32_t* wit,
                                     const qn_static_params* params, uint32_t* removed_per_entry, int* status) {
  // ---- every argument is checked before anything runs
  if (!s || !ids || !poses16 || count == 0 || !wit_off || !params || !removed_per_entry || !status) return QN_ERR_INVALID_ARG;
  if (params->min_see_through == 0) return QN_ERR_INVALID_ARG;
  for (uint32_t e = 0; e < count; e++) if (wit_off[e + 1] < wit_off[e]) return QN_ERR_INVALID_ARG;
  const uint32_t w_first = wit_off[0], n_wit = wit_off[count] - w_first;
  if (n_wit && !wit) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t e = 0; e < count; e++) {
    if (ids[e] < 0 || (size_t)ids[e] >= n_kf) return QN_ERR_INVALID_ARG;
    for (int k = 0; k < 16; k++) if (!std::isfinite(poses16[16 * (size_t)e + k])) return QN_ERR_INVALID_ARG;
  }
  RangeState* rs = (RangeState*)qn_kf_int_ext(s, QN_KF_INT_EXT_RANGE);
  for (uint32_t e = 0; e < count; e++)
    for (uint32_t k = wit_off[e]; k < wit_off[e + 1]; k++) {
      const uint32_t w = wit[k];
      if (w >= count || ids[w] == ids[e]) return QN_ERR_INVALID_ARG;
      if (!rs || (size_t)ids[w] >= rs->described.size() || !rs->described[ids[w]]) return QN_ERR_INVALID_ARG;      // a witness without images
    }
  for (uint32_t e = 0; e < count; e++) if (wit_off[e + 1] - wit_off[e] > SV_MAX_WITNESSES) return QN_ERR_CAPACITY;
  uint64_t total = 0, tiles = 0; uint32_t nmax = 0;
  std::vector<SvHostEntry> ent(count);
  for (uint32_t e = 0; e < count; e++) {
    uint32_t n = 0;
    const float4* pts = qn_kf_int_keyframe(s, ids[e], &n);
    ent[e] = SvHostEntry{pts, n, (uint32_t)total, 0, 0, (uint8_t)(qn_kf_int_has_intensity(s, ids[e]) ? 1 : 0)};
    total += n; tiles += (n + FS_TILE - 1) / FS_TILE; nmax = std::max(nmax, n);
    if (total > 0xFFFFFFFFull) return QN_ERR_CAPACITY;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  StaticState* st = nullptr;
  const int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_STATIC, &st);
  if (rc != QN_OK) return rc;
  const hipStream_t str = qn_kf_int_stream(s);
  const uint32_t nt = (uint32_t)tiles;
  const size_t ent_bytes = qn_up16(sizeof(SvEntry) * count), wit_bytes = qn_up16(sizeof(SvWit) * std::max<uint32_t>(n_wit, 1)), rem_bytes = sizeof(uint32_t) * count;
  SvEntry* d_ent = (SvEntry*)qn_kf_int_scratch(s, 0, ent_bytes);
  SvWit* d_wit = (SvWit*)qn_kf_int_scratch(s, 1, wit_bytes);
  uint32_t* d_tile = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (2 * (size_t)nt + 1));      // kept counts [nt], then offsets [nt + 1]
  uint32_t* d_rem = (uint32_t*)qn_kf_int_scratch(s, 3, rem_bytes);
  char* h = (char*)qn_kf_int_pinned(s, ent_bytes + wit_bytes + rem_bytes);
  if (!d_ent || !d_wit || !d_tile || !d_rem || !h) return qn_kf_fail(s, "qn_kf_static_classify: scratch allocation failed");
  // from here on the previous classify is gone
  st->live = false;
  // (3 * total bytes: grows at the same totals as a buffer of `total` three-byte records would)
  if (!st->votes.grow(s, 3 * (size_t)total) || !st->kept.grow(s, total)) return QN_ERR_HIP;
  SvEntry* h_ent = (SvEntry*)h; SvWit* h_wit = (SvWit*)(h + ent_bytes); uint32_t* h_rem = (uint32_t*)(h + ent_bytes + wit_bytes);
  uint32_t b0 = 0;
  for (uint32_t e = 0; e < count; e++) {
    const uint32_t w0 = wit_off[e] - w_first, nw = wit_off[e + 1] - wit_off[e];
    h_ent[e] = SvEntry{ent[e].pts, ent[e].n, ent[e].p0, w0, nw, b0, 0};
    b0 += (ent[e].n + FS_TILE - 1) / FS_TILE;
    for (uint32_t k = 0; k < nw; k++) {
      const uint32_t w = wit[wit_off[e] + k];
      SvWit& g = h_wit[w0 + k];
      double Q[16];
      qn_kf_int_relative_pose(poses16 + 16 * (size_t)w, poses16 + 16 * (size_t)e, Q);      // M = inv(P_w) P_e (scancontext.relative_pose)
      memcpy(g.M, Q, sizeof(double) * 12);
      g.img = ids[w]; g.pad[0] = g.pad[1] = g.pad[2] = 0;
    }
  }
  QN_KFCHK(s, hipMemcpyAsync(d_ent, h_ent, sizeof(SvEntry) * count, hipMemcpyHostToDevice, str));
  if (n_wit) QN_KFCHK(s, hipMemcpyAsync(d_wit, h_wit, sizeof(SvWit) * n_wit, hipMemcpyHostToDevice, str));
  uint8_t* d_st = st->votes.p; uint8_t* d_ag = d_st + total; uint8_t* d_rm = d_st + 2 * total;
  if (nt) {
    const qn_range_params p = rs ? rs->p : qn_range_params{};      // (records but no witness at all: nothing is projected, the tables are not read)
    const double* trow = rs ? rs->tab.p : nullptr;
    const double2* cs = rs ? (const double2*)(rs->tab.p + range_cs_offset(p.n_rows)) : nullptr;
    const size_t lds = rs ? range_lds_bytes(rs) : 0;
    const uint32_t* img = rs ? rs->img.p : nullptr;
    sv_each_chunk(ent.data(), count, FS_TILE, [&](uint32_t a, dim3 grid) {
      if (lds) hipLaunchKernelGGL(k_static_vote<true>, grid, dim3(FS_BLOCK), lds, str, (const SvEntry*)(d_ent + a), (const SvWit*)d_wit, trow, cs, p.n_rows, p.n_cols, p.min_range,
                                  (int)p.window_rows, (int)p.window_cols, p.tol_abs, p.tol_rel, img, params->min_see_through, params->agree_weight, d_st, d_ag, d_rm, d_tile);
      else hipLaunchKernelGGL(k_static_vote<false>, grid, dim3(FS_BLOCK), 0, str, (const SvEntry*)(d_ent + a), (const SvWit*)d_wit, trow, cs, p.n_rows, p.n_cols, p.min_range,
                              (int)p.window_rows, (int)p.window_cols, p.tol_abs, p.tol_rel, img, params->min_see_through, params->agree_weight, d_st, d_ag, d_rm, d_tile);
    });
    hipLaunchKernelGGL(k_static_scan, dim3(1), dim3(SV_SCAN_BLOCK), 0, str, (const uint32_t*)d_tile, nt, d_tile + nt, (const SvEntry*)d_ent, count, d_rem);
    sv_each_chunk(ent.data(), count, FS_TILE, [&](uint32_t a, dim3 grid) {
      hipLaunchKernelGGL(k_static_compact, grid, dim3(FS_BLOCK), 0, str, (const SvEntry*)(d_ent + a), (const uint8_t*)d_rm, (const uint32_t*)(d_tile + nt), st->kept.p);
    });
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h_rem, d_rem, rem_bytes, hipMemcpyDeviceToHost, str));
  } else {
    memset(h_rem, 0, rem_bytes);
  }
  QN_KFCHK(s, hipStreamSynchronize(str));                   // the one synchronisation of the call
  uint32_t koff = 0;
  for (uint32_t e = 0; e < count; e++) {
    ent[e].kept_off = koff; ent[e].kept_n = ent[e].n - h_rem[e]; koff += ent[e].kept_n;
    removed_per_entry[e] = h_rem[e];
    status[e] = ent[e].n ? QN_OK : QN_ERR_EMPTY_CLOUD;
  }
  st->ids.assign(ids, ids + count); st->poses.assign(poses16, poses16 + 16 * (size_t)count); st->ent.swap(ent); st->total = total;
  st->live = true;
  return QN_OK;
}

extern "C" int qn_kf_static_points(qn_kf_store* s, uint32_t entry, uint8_t* seen_through_out, uint8_t* agree_out, uint8_t* removed_out) {
  if (!s || (!seen_through_out && !agree_out && !removed_out)) return QN_ERR_INVALID_ARG;
  StaticState* st = (StaticState*)qn_kf_int_ext(s, QN_KF_INT_EXT_STATIC);
  if (!st || !st->live) return QN_ERR_NOT_READY;
  if (entry >= st->ent.size()) return QN_ERR_INVALID_ARG;
  const SvHostEntry& o = st->ent[entry];
  if (o.n == 0) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  uint8_t* out[3] = {seen_through_out, agree_out, removed_out};
  for (int k = 0; k < 3; k++)
    if (out[k]) QN_KFCHK(s, hipMemcpyAsync(out[k], st->votes.p + (size_t)k * st->total + o.p0, o.n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_build_map_static(qn_kf_store* s, double leaf, const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || !d_xyzi_out || !n_out || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  StaticState* st = (StaticState*)qn_kf_int_ext(s, QN_KF_INT_EXT_STATIC);
  if (!st || !st->live) return QN_ERR_NOT_READY;
  const uint32_t count = (uint32_t)st->ids.size();
  for (uint32_t e = 0; e < count; e++) {                    // the records the votes were taken on must still be the keyframes' records
    uint32_t n = 0;
    if ((size_t)st->ids[e] >= qn_kf_int_count(s) || qn_kf_int_keyframe(s, st->ids[e], &n) != st->ent[e].pts || n != st->ent[e].n) return QN_ERR_NOT_READY;
  }
  std::vector<const float4*> pts(count); std::vector<uint32_t> n(count); std::vector<uint8_t> has_i(count);
  for (uint32_t e = 0; e < count; e++) { pts[e] = st->kept.p + st->ent[e].kept_off; n[e] = st->ent[e].kept_n; has_i[e] = st->ent[e].has_i; }
  return qn_kf_int_build_map_from(s, pts.data(), n.data(), has_i.data(), st->poses.data(), count, leaf, d_xyzi_out, n_out);
}

#include "qn_mapoccupancy.inc"
#include "qn_mapoccupancy_update.inc"
#include "qn_mapdistance.inc"
#include "qn_maproute.inc"
#include "qn_mapfrontier.inc"
#include "qn_mapview.inc"
