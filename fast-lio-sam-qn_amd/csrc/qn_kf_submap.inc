// qn_kf_submap.inc - a keyframe's local submap, in that keyframe's own frame, built once and kept resident (qn_kf_submap_describe), and the drift-free
// submap-to-submap verification of loop candidates that borrows it on both sides (qn_kf_verify_loop_pairs_submap, and coarse to fine from resident FPFH rows
// qn_kf_verify_loop_pairs_submap_c2f).  Included by qn_engine.hip behind qn_kf_quatro.inc, whose describe machinery (kfq_rows), read-backs and coarse-to-fine
// pair call (kfq_pairs_c2f) it shares.
//
// The reference's third mode (config.yaml: enable_submap_matching true; loop_closure.cpp:70-84, 98-107) registers the submap around the query against the
// submap around the candidate, both placed with the corrected poses - the whole trajectory's drift.  Here the submap around keyframe c is
//   voxel_grid( concat_i transformPcd(kf_i, inv(P_c) P_i) ),  i in local_submap_ids(c, r, n) = [c - r .. c + r] clipped to [0, n),
// in c's sensor frame: it depends on the relative poses inside its window only.  It is the candidate window of qn_kf_verify_loop_candidates (the same pose
// arithmetic, qn_kf_int_relative_pose, keyframe c itself included) except that the window keeps the newest keyframe: the reference drops it because its only
// query is keyframes_.back(); with many queries per call there is no such keyframe, and a submap without its own centre is not what anyone wants.
// An entry serves as the source when c is a query and as the target when c is a candidate; a pair's result estimates inv(P_c) P_q.
//
// describe: every listed window goes through the store's ONE voxel-grid pipeline as one batch (qn_kf_int_voxel_windows: what qn_kf_assemble_batch builds for
// the same lists, into a block of its own, no store slot touched); with features, kfq_rows gives every window its FPFH rows in the nine keyframe-as-grid-
// dimension launches per chunk.  Windows are several times a scan, so the 1 GiB chunking of the grids' scratch does run here.  No kernel of its own: the
// relative poses are a few dozen 4x4 products on the host and reach the device inside the pipeline's one table upload.
namespace {

struct KfsEntry : KfqEntry { uint32_t range = 0; bool has_rows = false; };
struct KfsState { std::vector<KfsEntry> e; };

const KfsEntry* kfs_entry(const qn_kf_store* s, int32_t id) { return kf_entry<KfsState>(s, QN_KF_INT_EXT_SUBMAP, id); }
const KfqEntry* kfs_cloud_entry(const qn_kf_store* s, int32_t id) { return kfs_entry(s, id); }
const KfqEntry* kfs_rows_entry(const qn_kf_store* s, int32_t id) { const KfsEntry* e = kfs_entry(s, id); return e && e->has_rows ? e : nullptr; }

}  // namespace

extern "C" int qn_kf_submap_describe(qn_kf_store* s, qn_ctx* ctx, const int32_t* ids, uint32_t count, const double* poses, uint32_t n_poses, uint32_t submap_range,
                                     double leaf, int with_features, int* status) {
  // ---- every argument before anything runs
  if (!s || !ctx || !ids || count == 0 || !poses || !status || !(leaf > 0)) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != ctx->device) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t i = 0; i < count; i++) if (ids[i] < 0 || (size_t)ids[i] >= n_kf || (uint32_t)ids[i] >= n_poses) return QN_ERR_INVALID_ARG;
  for (size_t i = 0; i < (size_t)n_poses * 16; i++) if (!std::isfinite(poses[i])) return QN_ERR_INVALID_ARG;
  // ---- the lists: window t = local_submap_ids(ids[t], submap_range, n_poses), keyframe i with inv(P_c) P_i
  std::vector<int32_t> wid; std::vector<double> rel; std::vector<uint32_t> seg(1, 0);
  if (qn_kf_int_windows(ids, count, poses, n_poses, n_kf, submap_range, true, wid, rel, seg) != QN_OK) return QN_ERR_INVALID_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  qn_ctx* c = ctx;
  if (!c->qparams_set) { qn_quatro_default_params(&c->qparams); c->qparams_set = true; }
  KfsState* st = nullptr; KfqState* scratch = nullptr;                               // (the grids' scratch is the scan entries' too: one arena per store)
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_SUBMAP, &st);
  if (rc == QN_OK && with_features) rc = qn_kf_ext_state(s, QN_KF_INT_EXT_QUATRO, &scratch);
  if (rc != QN_OK) return rc;
  // ---- the clouds: one batch of `count` windows through the store's voxel pipeline (two host synchronisations), into a new block
  std::vector<const float4*> vp(count, nullptr); std::vector<uint32_t> vn(count, 0); std::vector<int> vs(count, QN_ERR_EMPTY_CLOUD);
  auto blk = std::make_shared<KfqBlock>();
  rc = qn_kf_int_voxel_windows(s, wid.data(), rel.data(), seg.data(), count, leaf, blk->pts, vp.data(), vn.data(), vs.data());
  if (rc != QN_OK) return rc;                                                       // (an allocation failure: no entry changed)
  size_t total = 0; std::vector<size_t> roff(count, 0);
  for (uint32_t i = 0; i < count; i++) {
    if (vs[i] == QN_OK && vn[i] > c->max_points) vs[i] = QN_ERR_CAPACITY;           // (no lane of this context could take it)
    if (vs[i] == QN_OK) { roff[i] = total; total += vn[i]; }
  }
  if (with_features && total) {
    if (!blk->rows.grow(s, QN_FROW * total, true)) return kfq_no_memory(s, c);
    if ((rc = kfq_rows(s, c, scratch, vp.data(), vn.data(), vs.data(), count, blk->rows.p, roff.data())) != QN_OK) return rc;
  }
  // ---- the entries: describing again replaces (the block of a replaced entry goes when no entry names it); a window over capacity leaves no entry
  qn_kf_int_verify_stale(s, QN_KF_VERIFY_FROM_SUBMAPS, ids, count);
  if (st->e.size() < n_kf) st->e.resize(n_kf);
  for (uint32_t i = 0; i < count; i++) {
    KfsEntry& e = st->e[ids[i]];
    e = KfsEntry{};
    status[i] = vs[i];
    if (vs[i] == QN_ERR_CAPACITY) continue;
    e.described = true; e.leaf = leaf; e.rn = c->qparams.fpfh_normal_radius; e.rf = c->qparams.fpfh_radius; e.max_cells = c->max_cells; e.status = vs[i];
    e.range = submap_range; e.has_rows = with_features != 0;
    if (vs[i] == QN_OK) { e.blk = blk; e.pts = const_cast<float4*>(vp[i]); e.rows = with_features ? blk->rows.p + QN_FROW * roff[i] : nullptr; e.n = vn[i]; }
  }
  return QN_OK;
}

extern "C" int qn_kf_submap_cloud(qn_kf_store* s, int32_t id, const float** d_xyz, uint32_t* n) { return kfq_cloud(s, id, kfs_cloud_entry, d_xyz, n); }
extern "C" int qn_kf_submap_features(qn_kf_store* s, int32_t id, float* fpfh33_out) {
  return kfq_features(s, id, kfs_rows_entry, fpfh33_out, "qn_kf_submap_features: read-back failed");
}

extern "C" int qn_kf_submap_release(qn_kf_store* s, const int32_t* ids, uint32_t count) {
  if (!s || (ids == nullptr) != (count == 0)) return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t i = 0; i < count; i++) if (ids[i] < 0 || (size_t)ids[i] >= n_kf) return QN_ERR_INVALID_ARG;
  KfsState* st = (KfsState*)qn_kf_int_ext(s, QN_KF_INT_EXT_SUBMAP);
  if (!st) return QN_OK;
  // (the entries' blocks are device memory nothing in flight reads: every call that borrows them ends synchronised)
  qn_kf_int_verify_stale(s, QN_KF_VERIFY_FROM_SUBMAPS, ids, count);
  if (!ids) { st->e.clear(); return QN_OK; }
  for (uint32_t i = 0; i < count; i++) if ((size_t)ids[i] < st->e.size()) st->e[ids[i]] = KfsEntry{};
  return QN_OK;
}

extern "C" int qn_kf_verify_loop_pairs_submap(qn_kf_store* s, qn_ctx* ctx, const int32_t* query, const int32_t* cand, const double* yaw, uint32_t n_pairs,
                                              double score_thr, qn_gicp_result* results, int* valid, int* status) {
  // ---- every argument before anything runs: the entries, the verify record and the context stay as they were
  if (!s || !ctx || !query || !cand || n_pairs == 0 || !results || !valid || !status) return QN_ERR_INVALID_ARG;
  if (qn_kf_int_device(s) != ctx->device) return QN_ERR_INVALID_ARG;
  std::vector<qn_kf_int_verify_job> jobs(n_pairs);
  for (uint32_t j = 0; j < n_pairs; j++) {
    const KfsEntry* q = kfs_entry(s, query[j]); const KfsEntry* e = kfs_entry(s, cand[j]);
    if (cand[j] == query[j] || !q || !e) return QN_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < j; i++) if (query[i] == query[j] && cand[i] == cand[j]) return QN_ERR_INVALID_ARG;
    if (yaw && !std::isfinite(yaw[j])) return QN_ERR_INVALID_ARG;
    jobs[j] = qn_kf_int_verify_job{q->pts, q->n, e->pts, e->n, query[j], cand[j], 0, q->n == 0 || e->n == 0 ? QN_ERR_EMPTY_CLOUD : QN_OK, {}, nullptr, nullptr};
    qn_kf_int_seed_from_yaw(yaw ? yaw[j] : 0.0, jobs[j].guess);
  }
  // ---- the pairs whose clouds exist through the pair driver: one batched registration, grouped by query
  std::vector<int32_t> uq; std::vector<uint32_t> qi;
  qn_kf_int_distinct(query, n_pairs, uq, qi);
  for (uint32_t j = 0; j < n_pairs; j++) jobs[j].group = qi[j];
  return qn_kf_int_verify_run(s, ctx, jobs.data(), n_pairs, score_thr, false, QN_KF_VERIFY_SUBMAP, results, nullptr, nullptr, valid, status);
}

extern "C" int qn_kf_verify_loop_pairs_submap_c2f(qn_kf_store* s, qn_ctx* ctx, const int32_t* query, const int32_t* cand, uint32_t n_pairs, double score_thr,
                                                  qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  return kfq_pairs_c2f(s, ctx, kfs_rows_entry, QN_KF_VERIFY_SUBMAP_C2F, query, cand, n_pairs, score_thr, results, T_total, T_quatro, valid, status);
}
