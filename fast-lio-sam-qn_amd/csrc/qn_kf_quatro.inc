// qn_kf_quatro.inc - Quatro features of resident keyframes, described once and kept next to their points (qn_kf_quatro_describe), and the drift-free
// coarse-to-fine verification of loop candidates that borrows them (qn_kf_verify_loop_candidates_c2f, and for many queries at once qn_kf_verify_loop_pairs_c2f).  Included by qn_engine.hip behind qn_quatro_host.inc:
// it drives that file's batched coarse-to-fine machinery (c2f_batch) and qn_batch.inc's lane launches.
//
// Scan to scan (config.yaml: quatro/enable true, enable_submap_matching false; loop_closure.cpp:85-92) both clouds of a pair are functions of ONE keyframe each
// once they are taken in their own sensor frames: the voxelised cloud, its normals, SPFH and FPFH depend on no pose.  qn_coarse_to_fine_align_batch rebuilds the
// candidate's grid and K9-K11 for every pair, and again every time that keyframe comes back as a candidate of a later query; here each keyframe is described
// once and a pair runs only the matching (K12 / K13), the host solver and the GICP lanes.
//
// describe: the S keyframes' clouds come out of the store's one voxel-grid pipeline as a batch of S identity-pose submaps (qn_kf_int_voxel_each), then every
// keyframe's FPFH grid (cell r_f / 2, prep_grid: the same numbers as set_cloud gives that cloud on this context) and K9-K11 ride in NINE k_lanes launches - the
// keyframe is blockIdx.y, its entry of the argument table names its grid scratch and its place in the arena.  The functors are the ones quatro_fpfh's kernels
// wrap (NormalsK / SpfhK / FpfhK <8>, RowsToOriginalK), so the rows are bit-identical to qn_fpfh's by construction.  Grid scratch per keyframe: two cell tables
// of max_cells + 1 words; keyframes are taken in chunks whose scratch stays under QN_KFQ_SCRATCH_BYTES (one chunk for every S the budget holds).
#include <memory>
#include "qn_kf_buf.h"
#define QN_KFQ_SCRATCH_BYTES ((size_t)1 << 30)
#define QN_KFQ_MAX_CHUNK 4096u

namespace {

// one describe call's device memory: the clouds (the voxel pipeline's output buffer) and the FPFH rows; freed when no entry names it any more
struct KfqBlock { DevBuf<float4> pts; DevBuf<float> rows; };
struct KfqEntry {
  std::shared_ptr<KfqBlock> blk; float4* pts = nullptr; float* rows = nullptr; uint32_t n = 0;
  double leaf = 0, rn = 0, rf = 0; uint32_t max_cells = 0; int status = QN_OK; bool described = false;
};
// grid scratch of one keyframe slot of a chunk: the per-keyframe tables sit at fixed places (counters handed back at zero by k_scatter, bounding-box
// tickets handed back at zero by PackBBoxK, look-back status words tagged with an epoch that never repeats), initialised once when they are allocated
struct KfqSlot { uint32_t* cell_start; uint32_t* counts; unsigned long long* status; BBoxAcc* acc; GridDims* dims; };
struct KfqState {
  std::vector<KfqEntry> e;
  DevBuf<char> fixed; uint32_t fixed_slots = 0, fixed_cells = 0;      // every buffer here is sized exactly: the scratch runs up to QN_KFQ_SCRATCH_BYTES
  DevBuf<char> pts;
  PinBuf<GridDims> dims_host;
  uint32_t epoch = 0;
};
// a buffer of the store could not be grown: the context that was handed in says why too (qn_last_error)
int kfq_no_memory(qn_kf_store* s, qn_ctx* c) { c->last_error = qn_kf_last_error(s); return QN_ERR_HIP; }
size_t kfq_up(size_t b) { return (b + 255) & ~(size_t)255; }
uint32_t kfq_status_words(uint32_t max_cells) { return max_cells / (QN_BLOCK * QN_SCAN_ITEMS) + 2; }
// the slot tables, region by region: cell starts, cell counters, look-back status words, bounding-box accumulators, grid numbers - each region `slots` long
struct KfqFixed {
  size_t tab, stat, acc, dims, off_counts, off_stat, off_acc, off_dims, end;
  KfqFixed(uint32_t max_cells, uint32_t slots) {
    tab = kfq_up(sizeof(uint32_t) * ((size_t)max_cells + 1)); stat = kfq_up(sizeof(unsigned long long) * kfq_status_words(max_cells));
    acc = kfq_up(sizeof(BBoxAcc) * (QN_BBOX_MAX_BLOCKS + 1)); dims = kfq_up(sizeof(GridDims));
    off_counts = tab * slots; off_stat = off_counts + tab * slots; off_acc = off_stat + stat * slots; off_dims = off_acc + acc * slots; end = off_dims + dims * slots;
  }
  size_t per_slot() const { return 2 * tab + stat + acc + dims; }
};
size_t kfq_point_bytes(uint32_t n) {      // raw, sorted, sorted_tmp, normals, cell_of_pt, SPFH and sorted-order FPFH rows of one keyframe
  return 4 * kfq_up(sizeof(float4) * (size_t)n) + kfq_up(sizeof(uint32_t) * (size_t)n) + 2 * kfq_up(sizeof(float) * QN_FROW * (size_t)n);
}
KfqSlot kfq_slot(KfqState* st, uint32_t k) {
  const KfqFixed f(st->fixed_cells, st->fixed_slots);
  char* b = st->fixed.p;
  return KfqSlot{(uint32_t*)(b + f.tab * k), (uint32_t*)(b + f.off_counts + f.tab * k), (unsigned long long*)(b + f.off_stat + f.stat * k),
                 (BBoxAcc*)(b + f.off_acc + f.acc * k), (GridDims*)(b + f.off_dims + f.dims * k)};
}
// the slot tables for `slots` keyframes of a context with `max_cells`: (re)allocated and initialised on the context's stream when they do not fit
int kfq_fixed(qn_kf_store* s, qn_ctx* c, KfqState* st, uint32_t slots) {
  if (st->fixed.p && st->fixed_slots >= slots && st->fixed_cells == c->max_cells) return QN_OK;
  if (st->fixed.p) { HIPCHK(c, hipStreamSynchronize(c->stream)); st->fixed.reset(); st->fixed_slots = 0; }
  const KfqFixed f(c->max_cells, slots);
  if (!st->fixed.grow(s, f.end, true)) return kfq_no_memory(s, c);
  st->fixed_slots = slots; st->fixed_cells = c->max_cells;
  HIPCHK(c, hipMemsetAsync(st->fixed.p, 0, f.end, c->stream));
  // (the accumulator region is one array of slots x (QN_BBOX_MAX_BLOCKS + 1) entries: kfq_up keeps each slot's share a whole number of entries)
  hipLaunchKernelGGL(k_bbox_acc_init, dim3(1), dim3(256), 0, c->stream, (BBoxAcc*)(st->fixed.p + f.off_acc), (int)(f.acc / sizeof(BBoxAcc) * slots));
  HIPCHK(c, hipGetLastError());
  return QN_OK;
}

// K9-K11 of `count` resident clouds (vp / vn / vs: pointer, points, status; only the QN_OK ones are described) with c's Quatro radii, cloud i's rows at
// rows + QN_FROW * roff[i] in original point order: the grids and the three feature stages of a chunk of clouds ride in nine k_lanes launches, the cloud as
// blockIdx.y.  Shared by qn_kf_quatro_describe (single scans) and qn_kf_submap_describe (windows of scans); st = the scratch both use.  Ends synchronised.
int kfq_rows(qn_kf_store* s, qn_ctx* c, KfqState* st, const float4* const* vp, const uint32_t* vn, const int* vs, uint32_t count, float* rows, const size_t* roff) {
  // ---- K9-K11 of every non-empty keyframe, a chunk of keyframes per nine k_lanes launches
  int rc = QN_OK;
  const double rn_d = c->qparams.fpfh_normal_radius, rf_d = c->qparams.fpfh_radius;
  const float rn = (float)rn_d, rf = (float)rf_d, rn2 = (float)(rn_d * rn_d), rf2 = (float)(rf_d * rf_d);
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i < count; i++) if (vs[i] == QN_OK) live.push_back(i);
  const size_t slot_b = KfqFixed(c->max_cells, 1).per_slot();
  std::vector<std::pair<size_t, size_t>> chunks;                                   // [first, last) positions in `live`
  for (size_t a = 0; a < live.size();) {
    size_t b = a, bytes = 0;
    while (b < live.size() && b - a < QN_KFQ_MAX_CHUNK) {
      const size_t more = slot_b + kfq_point_bytes(vn[live[b]]);
      if (b > a && bytes + more > QN_KFQ_SCRATCH_BYTES) break;
      bytes += more; b++;
    }
    chunks.emplace_back(a, b); a = b;
  }
  if (!live.empty() && (rc = lane_args_arena(c)) != QN_OK) return rc;             // the argument arena of the lane launches (qn_batch.inc)
  uint32_t max_slots = 0; size_t max_pts = 0;
  for (const auto& ch : chunks) {
    max_slots = std::max<uint32_t>(max_slots, (uint32_t)(ch.second - ch.first));
    size_t p = 0; for (size_t j = ch.first; j < ch.second; j++) p += kfq_point_bytes(vn[live[j]]);
    max_pts = std::max(max_pts, p);
  }
  if (max_slots) {
    if ((rc = kfq_fixed(s, c, st, max_slots)) != QN_OK) return rc;
    // (a regrow waits for the context's stream first: that is where an asynchronous error of the previous call surfaces, with its message)
    if ((max_pts > st->pts.cap && st->pts.p) || (max_slots > st->dims_host.cap && st->dims_host.p)) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!st->pts.grow(s, max_pts, true) || !st->dims_host.grow(s, max_slots, true)) return kfq_no_memory(s, c);
  }
  for (size_t ci = 0; ci < chunks.size(); ci++) {
    if (ci > 0) HIPCHK(c, hipStreamSynchronize(c->stream));                       // (the argument arena and the scratch are the previous chunk's until then)
    LanePlan plan(c);
    std::vector<LaneEntry<PackBBoxK::Args>> v_pack; std::vector<LaneEntry<CellCountK::Args>> v_count; std::vector<LaneEntry<ScanLookbackK::Args>> v_scan;
    std::vector<LaneEntry<ScatterK::Args>> v_scat; std::vector<LaneEntry<StableCellsK::Args>> v_stab;
    std::vector<LaneEntry<NormalsK<8>::Args>> v_nrm; std::vector<LaneEntry<SpfhK<8>::Args>> v_spfh; std::vector<LaneEntry<FpfhK<8>::Args>> v_fpfh; std::vector<LaneEntry<RowsToOriginalK::Args>> v_rows;
    // prep_grid on a CloudBuf of the slot's scratch, with the context's grid rules (max_cells, stable cells) and cell r_f / 2 - the bounding-box accumulator,
    // look-back status words and epoch are the slot's (swapped in around the call)
    BBoxAcc* const save_acc = c->bbox_acc; unsigned long long* const save_status = c->scan_status; const uint32_t save_epoch = c->build_epoch; const double save_cell = c->lane.cell_override;
    c->lane.cell_override = rf_d * 0.5;
    char* p = st->pts.p;
    for (size_t j = chunks[ci].first; j < chunks[ci].second; j++) {
      const uint32_t i = live[j], n = vn[i], k = (uint32_t)(j - chunks[ci].first);
      const KfqSlot q = kfq_slot(st, k);
      CloudBuf b;
      b.n = n;
      b.raw = (float4*)p; p += kfq_up(sizeof(float4) * n);
      b.sorted = (float4*)p; p += kfq_up(sizeof(float4) * n);
      b.sorted_tmp = (float4*)p; p += kfq_up(sizeof(float4) * n);
      float4* nrm = (float4*)p; p += kfq_up(sizeof(float4) * n);
      b.cell_of_pt = (uint32_t*)p; p += kfq_up(sizeof(uint32_t) * n);
      float* spfh = (float*)p; p += kfq_up(sizeof(float) * QN_FROW * n);
      float* fpfh_s = (float*)p; p += kfq_up(sizeof(float) * QN_FROW * n);
      b.cell_start = q.cell_start; b.counts = q.counts; b.dims = q.dims; b.dims_host = st->dims_host.p + k;
      c->bbox_acc = q.acc; c->scan_status = q.status;
      if (((++st->epoch) & 0x3fffffffu) == 0u) ++st->epoch;                        // (0 = the tag of the zero-initialised status words)
      c->build_epoch = st->epoch - 1;                                               // (prep_grid tags the build with ++build_epoch)
      const GridLaunch G = prep_grid(c, b, (const char*)vp[i], 16, true);
      lane_push(v_pack, G.pack, G.pack_nb); lane_push(v_count, G.count, G.nb); lane_push(v_scan, G.scan, G.scan_nb); lane_push(v_scat, G.scat, G.nb);
      lane_push(v_stab, G.stab, G.nb);
      const uint32_t nb = (n + QN_BLOCK - 1) / QN_BLOCK;
      lane_push(v_nrm, NormalsK<8>::Args{b.grid, rn, rn2, nrm}, nb * 8u);
      lane_push(v_spfh, SpfhK<8>::Args{b.grid, rf, rf2, nrm, spfh}, nb * 8u);
      lane_push(v_fpfh, FpfhK<8>::Args{b.grid, rf, rf2, nrm, spfh, fpfh_s}, nb * 8u);
      lane_push(v_rows, RowsToOriginalK::Args{b.sorted, n, fpfh_s, rows + QN_FROW * roff[i], QN_FROW, QN_FROW}, nb);
    }
    c->bbox_acc = save_acc; c->scan_status = save_status; c->build_epoch = save_epoch; c->lane.cell_override = save_cell;
    plan.add<PackBBoxK>(v_pack, QN_K_GRID_BUILD); plan.add<CellCountK>(v_count, QN_K_GRID_BUILD); plan.add<ScanLookbackK>(v_scan, QN_K_GRID_BUILD); plan.add<ScatterK>(v_scat, QN_K_GRID_BUILD); plan.add<StableCellsK>(v_stab, QN_K_GRID_BUILD);
    plan.add<NormalsK<8>>(v_nrm, QN_K_FPFH_NORMALS); plan.add<SpfhK<8>>(v_spfh, QN_K_FPFH_SPFH); plan.add<FpfhK<8>>(v_fpfh, QN_K_FPFH_FPFH); plan.add<RowsToOriginalK>(v_rows, QN_K_FPFH_FPFH);
    if ((rc = plan.run()) != QN_OK) { (void)hipStreamSynchronize(c->stream); qn_kf_int_set_error(s, c->last_error.c_str()); return rc; }
  }
  if (!live.empty()) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->prof_collect();
  }
  return QN_OK;
}

}  // namespace

extern "C" int qn_kf_quatro_describe(qn_kf_store* s, qn_ctx* ctx, const int32_t* ids, uint32_t count, double leaf, int* status) {
  // ---- every argument before anything runs
  if (!s || !ctx || !ids || count == 0 || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != ctx->device) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t i = 0; i < count; i++) if (ids[i] < 0 || (size_t)ids[i] >= n_kf) return QN_ERR_INVALID_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  qn_ctx* c = ctx;
  if (!c->qparams_set) { qn_quatro_default_params(&c->qparams); c->qparams_set = true; }
  KfqState* st = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_QUATRO, &st);
  if (rc != QN_OK) return rc;
  // ---- the clouds: one batch of `count` identity-pose submaps through the store's voxel pipeline (two host synchronisations), into a new block
  std::vector<const float4*> vp(count, nullptr); std::vector<uint32_t> vn(count, 0); std::vector<int> vs(count, QN_ERR_EMPTY_CLOUD);
  auto blk = std::make_shared<KfqBlock>();
  rc = qn_kf_int_voxel_each(s, ids, count, leaf, blk->pts, vp.data(), vn.data(), vs.data());
  if (rc != QN_OK) return rc;                                                       // (an allocation failure: no entry changed)
  size_t total = 0; std::vector<size_t> roff(count, 0);
  for (uint32_t i = 0; i < count; i++) if (vs[i] == QN_OK) { roff[i] = total; total += vn[i]; }
  if (!blk->rows.grow(s, QN_FROW * total, true)) return kfq_no_memory(s, c);
  // ---- K9-K11 of every non-empty keyframe, a chunk of keyframes per nine k_lanes launches
  const double rn_d = c->qparams.fpfh_normal_radius, rf_d = c->qparams.fpfh_radius;
  if ((rc = kfq_rows(s, c, st, vp.data(), vn.data(), vs.data(), count, blk->rows.p, roff.data())) != QN_OK) return rc;
  // ---- the entries: describing again replaces (the block of a replaced entry goes when no entry names it)
  qn_kf_int_verify_stale(s, QN_KF_VERIFY_FROM_SCANS, ids, count);                                         // (a multi-pair coarse-to-fine record that names one of them goes)
  if (st->e.size() < n_kf) st->e.resize(n_kf);
  for (uint32_t i = 0; i < count; i++) {
    KfqEntry& e = st->e[ids[i]];
    e = KfqEntry{};
    e.described = true; e.leaf = leaf; e.rn = rn_d; e.rf = rf_d; e.max_cells = c->max_cells; e.status = vs[i];
    if (vs[i] == QN_OK) { e.blk = blk; e.pts = const_cast<float4*>(vp[i]); e.rows = blk->rows.p + QN_FROW * roff[i]; e.n = vn[i]; }
    status[i] = vs[i];
  }
  return QN_OK;
}

// the entry of keyframe `id` in a unit's per-store state (KfqState here, KfsState in qn_kf_submap.inc), nullptr until it is described
template <class State>
static auto kf_entry(const qn_kf_store* s, int slot, int32_t id) -> const typename decltype(State::e)::value_type* {
  const State* st = (const State*)qn_kf_int_ext(s, slot);
  if (!st || id < 0 || (size_t)id >= st->e.size() || !st->e[id].described) return nullptr;
  return &st->e[id];
}
typedef const KfqEntry* (*KfqLookup)(const qn_kf_store* s, int32_t id);            // how a call finds its entries: scan entries, local submaps, local submaps with rows
static const KfqEntry* kfq_entry(const qn_kf_store* s, int32_t id) { return kf_entry<KfqState>(s, QN_KF_INT_EXT_QUATRO, id); }

// what a coarse-to-fine call on ctx may borrow: an entry described with the context's current Quatro radii and grid capacity (the rows are what its lanes would make)
static bool kfq_usable(const KfqEntry* e, const qn_ctx* ctx) {
  qn_quatro_params qp;
  if (ctx->qparams_set) qp = ctx->qparams; else qn_quatro_default_params(&qp);
  return e && e->rn == qp.fpfh_normal_radius && e->rf == qp.fpfh_radius && e->max_cells == ctx->max_cells;
}

// the read-backs of an entry: its cloud (qn_kf_quatro_cloud, qn_kf_submap_cloud) and its FPFH rows (qn_kf_quatro_features, qn_kf_submap_features)
static int kfq_cloud(qn_kf_store* s, int32_t id, KfqLookup entry, const float** d_xyz, uint32_t* n) {
  if (!s || !d_xyz || !n || id < 0 || (size_t)id >= qn_kf_int_count(s)) return QN_ERR_INVALID_ARG;
  *d_xyz = nullptr; *n = 0;
  const KfqEntry* e = entry(s, id);
  if (!e) return QN_ERR_NOT_READY;
  *d_xyz = (const float*)e->pts; *n = e->n;
  return QN_OK;
}
static int kfq_features(qn_kf_store* s, int32_t id, KfqLookup entry, float* fpfh33_out, const char* failed) {
  if (!s || id < 0 || (size_t)id >= qn_kf_int_count(s)) return QN_ERR_INVALID_ARG;
  const KfqEntry* e = entry(s, id);
  if (!e) return QN_ERR_NOT_READY;
  if (!e->n) return QN_OK;
  if (!fpfh33_out) return QN_ERR_INVALID_ARG;
  if (hipSetDevice(qn_kf_int_device(s)) != hipSuccess ||
      hipMemcpy2D(fpfh33_out, 33 * sizeof(float), e->rows, QN_FROW * sizeof(float), 33 * sizeof(float), e->n, hipMemcpyDeviceToHost) != hipSuccess) {
    qn_kf_int_set_error(s, failed); return QN_ERR_HIP;
  }
  return QN_OK;
}

extern "C" int qn_kf_quatro_cloud(qn_kf_store* s, int32_t id, const float** d_xyz, uint32_t* n) { return kfq_cloud(s, id, kfq_entry, d_xyz, n); }
extern "C" int qn_kf_quatro_features(qn_kf_store* s, int32_t id, float* fpfh33_out) {
  return kfq_features(s, id, kfq_entry, fpfh33_out, "qn_kf_quatro_features: read-back failed");
}

// a coarse-to-fine call on resident entries (`entry` finds them; kind = the verify record the call leaves, qn_kf_internal.h).  Every argument is checked before
// anything runs: the store's entries, its verify record and the context stay as they were.  Then every pair goes to the pair driver (qn_kf_int_verify_run), the
// lanes borrowing both sides' points and rows; an empty side is the batch's to report.  qn_kf_verify_loop_pairs_c2f (scan entries),
// qn_kf_verify_loop_candidates_c2f (the same with the query repeated, no record) and qn_kf_verify_loop_pairs_submap_c2f (local submaps, qn_kf_submap.inc) are this.
static int kfq_pairs_c2f(qn_kf_store* s, qn_ctx* ctx, KfqLookup entry, int kind, const int32_t* query, const int32_t* cand, uint32_t n_pairs, double score_thr,
                         qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  if (!s || !ctx || !query || !cand || n_pairs == 0 || !results || !T_total || !valid || !status) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != ctx->device) return QN_ERR_INVALID_ARG;
  std::vector<qn_kf_int_verify_job> jobs(n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const KfqEntry* q = entry(s, query[j]); const KfqEntry* e = entry(s, cand[j]);
    if (cand[j] == query[j] || !kfq_usable(q, ctx) || !kfq_usable(e, ctx)) return QN_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < j; i++) if (query[i] == query[j] && cand[i] == cand[j]) return QN_ERR_INVALID_ARG;
    jobs[j] = qn_kf_int_verify_job{q->pts, q->n, e->pts, e->n, query[j], cand[j], 0, QN_OK, {}, q->rows, e->rows};
  }
  std::vector<int32_t> uq; std::vector<uint32_t> qi;
  qn_kf_int_distinct(query, n_pairs, uq, qi);
  for (uint32_t j = 0; j < n_pairs; j++) jobs[j].group = qi[j];
  return qn_kf_int_verify_run(s, ctx, jobs.data(), n_pairs, score_thr, true, kind, results, T_total, T_quatro, valid, status);
}

extern "C" int qn_kf_verify_loop_candidates_c2f(qn_kf_store* s, qn_ctx* ctx, int32_t query, const int32_t* cand, uint32_t n_cand, double score_thr,
                                                qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  const std::vector<int32_t> q(cand ? n_cand : 0, query);
  return kfq_pairs_c2f(s, ctx, kfq_entry, QN_KF_VERIFY_KEEP, q.data(), cand, n_cand, score_thr, results, T_total, T_quatro, valid, status);
}

extern "C" int qn_kf_verify_loop_pairs_c2f(qn_kf_store* s, qn_ctx* ctx, const int32_t* query, const int32_t* cand, uint32_t n_pairs, double score_thr,
                                           qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  return kfq_pairs_c2f(s, ctx, kfq_entry, QN_KF_VERIFY_C2F, query, cand, n_pairs, score_thr, results, T_total, T_quatro, valid, status);
}
