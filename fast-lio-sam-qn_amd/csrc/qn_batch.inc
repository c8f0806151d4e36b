// qn_batch.inc - B candidate pairs per kernel launch on ONE context: the pair is a grid dimension (SURVEY.md 7.1 step 8, 8b `qn_gicp_align_batch`).
// Included by qn_engine.hip (it drives that file's prep_* functions: the SAME argument construction as the classic one-registration-per-stream path).
//
// The reference registers one candidate per timer tick (fast_lio_sam_qn.cpp:213-219) and every icpAlignment rebuilds both clouds' trees and covariances
// (loop_closure.cpp:116-124): candidate pairs share nothing, so B of them can ride through the kernel chain in lockstep.  A batch context owns B LANES
// (lane 0 = the context itself, lanes 1.. = sub-contexts with buffers of their own, all on the context's ONE stream); every kernel of the chain is launched
// once for all lanes as k_lanes<F> - blockIdx.y picks the lane's entry of a device-resident argument table, blockIdx.x is what the classic kernel calls
// blockIdx.x - so a registration costs ~45 / B launches instead of ~55, a launch carries B x 100k points instead of 100k (its tail - "a kernel lasts as long
// as its slowest wave" - is paid once per B pairs), and nothing in the chain is a single-block kernel with the chip idle around it.
// (the controller step rides in the last block of the launch that produced the rows - controller_tail - so there is no single-block controller launch in the chain at all)
// Each lane runs the batch-member form of gicp_align (fixed three unseeded iterations, far-query regime per lane, no persistent kernel): the host logic
// below is that function's, lane by lane; the kernels are the same functors with the same arguments => the records are bit-identical to the
// per-context path's (tests/test_gpu_batch.py).  Argument tables: one pinned staging arena + one device arena per context, ONE hipMemcpyAsync per
// segment (= the launches between two host synchronisations), never one per launch.

namespace {

template <class F> void lanes_launch(const void* tab, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lanes<F>), grid, dim3(F::TB), 0, s, (const LaneEntry<typename F::Args>*)tab);
}
template <class A> void lane_push(std::vector<LaneEntry<A>>& v, const A& a, uint32_t nbx) {
  LaneEntry<A> e; memset((void*)&e, 0, sizeof(e)); e.a = a; e.nbx = nbx; v.push_back(e);
}

struct LanePlan {                        // the launches of one segment and their argument tables
  qn_ctx* c; size_t off = 0; bool overflow = false; int flush_rc = QN_OK;
  struct Item { void (*fn)(const void*, dim3, hipStream_t); size_t off; dim3 grid; int family; };
  std::vector<Item> items;
  explicit LanePlan(qn_ctx* c_) : c(c_) {}
  template <class F> void add(const std::vector<LaneEntry<typename F::Args>>& e, int family) {      // family: the profiling family of qn_prof_get (hipEvents around the launch when profiling is on)
    if (e.empty()) return;
    const size_t bytes = sizeof(LaneEntry<typename F::Args>) * e.size();
    const size_t a = reserve(bytes);
    if (a == SIZE_MAX) return;
    put<F>(e, a, family);
  }
  // the same with `blob_bytes` bytes of data the entries point to (per-lane initial guesses) in front of the table, in ONE reservation: a flush of the arena can
  // never fall between the data and its launch.  fix(entries, device address of the blob) sets the entries' pointers once the place is known.
  template <class F, class Fix> void add(std::vector<LaneEntry<typename F::Args>>& e, int family, const void* blob, size_t blob_bytes, Fix fix) {
    if (e.empty()) return;
    const size_t head = (blob_bytes + 255) & ~(size_t)255, bytes = head + sizeof(LaneEntry<typename F::Args>) * e.size();
    const size_t a = reserve(bytes);
    if (a == SIZE_MAX) return;
    memcpy(c->args_h + a, blob, blob_bytes);
    fix(e, (const char*)(c->args_d + a));
    put<F>(e, a + head, family);
  }
  template <class F> void put(const std::vector<LaneEntry<typename F::Args>>& e, size_t a, int family) {
    const size_t bytes = sizeof(LaneEntry<typename F::Args>) * e.size();
    memcpy(c->args_h + a, e.data(), bytes);
    uint32_t gx = 0; for (const auto& x : e) gx = std::max(gx, x.nbx);
    gx = (gx + 7u) & ~7u;                                              // a multiple of 8: (linear workgroup id) mod 8 - the XCD - stays blockIdx.x mod 8 in every lane (xcd_block)
    items.push_back(Item{&lanes_launch<F>, a, dim3(gx, (uint32_t)e.size()), family});
    off = a + bytes;
  }
  size_t reserve(size_t bytes) {                                       // the arena offset of `bytes` more (SIZE_MAX: overflow, reported by run())
    size_t a = (off + 255) & ~(size_t)255;
    if (a + bytes > c->args_cap) {
      // the segment's tables outgrow the arena (forced runs of hundreds of iterations x many lanes): launch what is planned, wait until the device has consumed the
      // pinned staging copy, and carry on from the start of the arena - stream order keeps the chain's meaning, the host merely looks in once more (ADVICE r4)
      if (items.empty() || bytes > c->args_cap || flush_rc != QN_OK) { overflow = true; return SIZE_MAX; }
      flush_rc = run();
      if (flush_rc == QN_OK && hipStreamSynchronize(c->stream) != hipSuccess) { c->last_error = "batch: stream synchronisation failed while flushing the argument arena"; flush_rc = QN_ERR_HIP; }
      if (flush_rc != QN_OK) { overflow = true; return SIZE_MAX; }
      a = 0;
    }
    return a;
  }
  int run() {                                                          // one upload, then the launches in order; the arena is free again after the caller's next synchronisation
    if (overflow) { if (flush_rc == QN_OK) c->last_error = "batch: argument arena too small for one launch's table"; return QN_ERR_HIP; }
    if (items.empty()) return QN_OK;
    HIPCHK(c, hipMemcpyAsync(c->args_d, c->args_h, off, hipMemcpyHostToDevice, c->stream));
    for (const Item& it : items) { c->prof_begin(it.family, (int)it.grid.y); it.fn(c->args_d + it.off, it.grid, c->stream); c->prof_end(); }
    c->batch_launches += items.size();
    items.clear(); off = 0;
    HIPCHK(c, hipGetLastError());
    return QN_OK;
  }
};

// the second scratch set of a context (scan status, k-NN lists and index table, bounding box, landing zone): the TARGET cloud of a lane is prepared in the same
// launches as its SOURCE cloud, each with scratch of its own (the classic path uses the set for its second stream: TargetScope)
struct ScratchSwap {
  qn_ctx* c;
  static void sw(qn_ctx* c) {
    std::swap(c->scan_sums, c->scan_sums2); std::swap(c->fb_list, c->fb_list2); std::swap(c->big_list, c->big_list2); std::swap(c->fb_count2, c->fb_count2b);
    std::swap(c->knn_idx, c->knn_idx2); std::swap(c->bbox_acc, c->bbox_acc2); std::swap(c->scan_status, c->scan_status2); std::swap(c->staging, c->staging2); std::swap(c->pin_up, c->pin_up2);
  }
  explicit ScratchSwap(qn_ctx* c_) : c(c_) { sw(c); }
  ~ScratchSwap() { sw(c); }
};

struct LaneRun {
  qn_ctx* c = nullptr; uint32_t pair = 0; bool active = false;
  int alias = -1;                         // >= 0: this lane registers against the source cloud lane `alias` of the same run holds (the candidates of ONE query: one source preparation per run, not per lane)
  int ticks_left = 0, chunk = 0, chunk_start = 0, next = 0; bool first_chunk = true; long budget = 0;
  bool build_source = true;
};

// setInputSource / setInputTarget of one lane: validation and upload as set_cloud, the grid build's arguments instead of its launches
int lane_set_cloud(qn_ctx* c, int which, const float* xyz, uint32_t n, uint32_t stride, bool on_device, hipStream_t s, GridLaunch* out) {
  CloudBuf& b = c->cloud[which];
  b.n = 0; b.has_grid = b.has_cov = false;
  if (n == 0) return QN_ERR_EMPTY_CLOUD;
  if (!xyz || stride < 12 || (stride & 3)) return QN_ERR_INVALID_ARG;
  if (n > c->max_points) return QN_ERR_CAPACITY;
  const char* dsrc = (const char*)xyz;
  if (!on_device) { const int rc = upload_host_cloud(c, xyz, n, stride, s, &dsrc); if (rc != QN_OK) return rc; }
  b.n = n;
  *out = prep_grid(c, b, dsrc, stride, true);
  return QN_OK;
}

bool batch_supported(const qn_ctx* c) {      // everything else takes the classic path, pair by pair (same results)
  const qn_gicp_params& p = c->params;
  const int maxit = p.force_iterations > 0 ? p.force_iterations : p.max_iterations;
  return c->knob.batch_lanes >= 2 && !c->lanes_failed && maxit > 0 && c->knob.far_enabled && c->knob.knn_hist && !c->knob.verify_track && !c->clk_probe && !c->list_probe && !c->dbg_counters;
}

// the context's argument arena of the lane launches (pinned + device, 4 MB each), made on first use
int lane_args_arena(qn_ctx* c) {
  if (c->args_h) return QN_OK;
  c->args_cap = (size_t)4 << 20;
  HIPCHK(c, hipHostMalloc(&c->args_h, c->args_cap, hipHostMallocDefault));
  HIPCHK(c, hipMalloc(&c->args_d, c->args_cap));
  return QN_OK;
}

int batch_ensure_lanes(qn_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  const int B = std::max(1, std::min(c->knob.batch_lanes, 64));
  if (c->lanes.empty()) c->lanes.push_back(c);
  while ((int)c->lanes.size() < B) {
    qn_ctx* l = nullptr;
    const int rc = (c->knob.fail_lane_create > 0 && (int)c->lanes.size() >= c->knob.fail_lane_create) ? QN_ERR_HIP : ctx_create(c->device, c->max_points, c->stream, &l);
    if (rc != QN_OK) {      // (out of memory, typically: batch_lanes x a full max_points slab) - the lanes created so far are freed again, both entry points then take the one-pair path
      c->last_error = "batch: lane context creation failed (lanes need batch_lanes x the context's device memory)";
      while (c->lanes.size() > 1) { qn_ctx_destroy(c->lanes.back()); c->lanes.pop_back(); }
      // the failed hipMalloc left a sticky error on this thread: the one-pair path that takes over on this very thread checks hipGetLastError() after its first launches and
      // would report the stale out-of-memory as ITS failure (ADVICE r5); and the next call must not try again (GBs of hipMalloc / hipFree churn per call): remembered until
      // the caller sets batch_lanes anew
      (void)hipGetLastError();
      c->lanes_failed = true;
      return rc;
    }
    c->lanes.push_back(l);
  }
  { const int rc = lane_args_arena(c); if (rc != QN_OK) return rc; }
  for (qn_ctx* l : c->lanes) {            // every lane registers with the owner's parameters and knobs, as a batch member (no second stream, no persistent launches)
    if (l == c) continue;
    if (l->params.k_correspondences != c->params.k_correspondences) l->cloud[0].has_cov = l->cloud[1].has_cov = false;
    l->params = c->params;
    l->lane = c->lane;
  }
  return QN_OK;
}

// m <= B pairs through the chain in lockstep.  idx[l] = the pair lane l registers; guesses16 (or null: identity) = 16 floats per PAIR, align(output, guess).
int batch_register(qn_ctx* owner, const qn_pair_desc* pairs, const uint32_t* idx, uint32_t m, double thr, qn_gicp_result* results, int* valid, int* status,
                   std::vector<const float*>& last_src, std::vector<uint64_t>& last_key, const float* guesses16) {
  hipStream_t s = owner->stream;
  const auto t_call = std::chrono::steady_clock::now();
  const qn_gicp_params& p = owner->params;
  const int k = p.k_correspondences;
  LanePlan plan(owner);
  std::vector<LaneRun> L(m);
  // lanes that borrow another lane's source cloud (read-only for every kernel of an align: sorted points, raw points, normals, grid numbers) get their own buffers back when the run ends
  struct AliasGuard {
    std::vector<LaneRun>& L; std::vector<CloudBuf> saved; std::vector<double*> saved_nrm; std::vector<const float*>& last_src;
    AliasGuard(std::vector<LaneRun>& L_, std::vector<const float*>& ls) : L(L_), saved(L_.size()), saved_nrm(L_.size(), nullptr), last_src(ls) {}
    void borrow(size_t l, qn_ctx* from) { qn_ctx* c = L[l].c; saved[l] = c->cloud[0]; saved_nrm[l] = c->nrm_s_sorted; c->cloud[0] = from->cloud[0]; c->nrm_s_sorted = from->nrm_s_sorted; }
    ~AliasGuard() { for (size_t l = 0; l < L.size(); l++) if (L[l].alias >= 0 && saved_nrm[l]) { qn_ctx* c = L[l].c; c->cloud[0] = saved[l]; c->nrm_s_sorted = saved_nrm[l]; c->cloud[0].has_grid = c->cloud[0].has_cov = false; c->cloud[0].n = 0; c->cloud[0].knn_tab = nullptr; last_src[l] = nullptr; } }
  } alias_guard(L, last_src);
  // a failure of the batch machinery itself (a HIP error: the function returns it) must not leave a pair that was still under way reported as QN_OK
  struct FailGuard { std::vector<LaneRun>& L; int* status; bool armed = true; ~FailGuard() { if (armed) for (const LaneRun& R : L) if (R.active) status[R.pair] = QN_ERR_HIP; } } fail_guard{L, status};
  // ---- setInputSource / calculateSourceCovariances / setInputTarget / calculateTargetCovariances (loop_closure.cpp:120-123) of every lane: ten launches
  std::vector<LaneEntry<PackBBoxK::Args>> v_pack; std::vector<LaneEntry<CellCountK::Args>> v_count; std::vector<LaneEntry<ScanLookbackK::Args>> v_scan;
  std::vector<LaneEntry<ScatterK::Args>> v_scat; std::vector<LaneEntry<StableCellsK::Args>> v_stab;
  std::vector<LaneEntry<KnnHistArgs>> v_sel, v_lst; std::vector<LaneEntry<KnnSingleK::Args>> v_single; std::vector<LaneEntry<KnnCovArgs>> v_tail; std::vector<LaneEntry<CovFromIdxK::Args>> v_cov;
  auto push_grid = [&](const GridLaunch& G) {
    lane_push(v_pack, G.pack, G.pack_nb); lane_push(v_count, G.count, G.nb); lane_push(v_scan, G.scan, G.scan_nb); lane_push(v_scat, G.scat, G.nb);
    lane_push(v_stab, G.stab, G.nb);
  };
  auto push_knn = [&](const KnnLaunch& K) {
    lane_push(v_sel, K.sel, K.sel_nb); lane_push(v_lst, K.lst, K.lst_nb); lane_push(v_single, K.single, K.single_nb); lane_push(v_tail, K.tail, K.tail_nb); lane_push(v_cov, K.cov, K.cov_nb);
  };
  for (uint32_t l = 0; l < m; l++) {
    LaneRun& R = L[l]; R.c = owner->lanes[l]; R.pair = idx[l];
    qn_ctx* c = R.c;
    const qn_pair_desc& pd = pairs[R.pair];
    qn_gicp_result* out = &results[R.pair];
    valid[R.pair] = 0; memset(out, 0, sizeof(*out)); out->fitness = DBL_MAX;
    for (int i = 0; i < 4; i++) { out->T[5 * i] = 1.f; out->T64[5 * i] = 1.0; }
    c->knob.pair_pipeline = false; c->knob.persist_batch_off = true; c->tgt_pending = false; c->tgt_on_stream2 = false;
    const uint64_t key = ((uint64_t)pd.ns << 32) ^ ((uint64_t)pd.stride_bytes << 1) ^ (uint64_t)(pd.on_device ? 1 : 0);
    // the candidates of ONE query share their source cloud (qn_icp_alignment_same_source): a lane that still holds this source - same buffer within this call - keeps its grid and covariances
    R.build_source = !(owner->knob.batch_share_source && last_src[l] == pd.src && last_key[l] == key && pd.src != nullptr && c->cloud[0].has_grid && c->cloud[0].has_cov && c->cloud[0].n == pd.ns);
    if (R.build_source && owner->knob.batch_share_source && pd.src != nullptr && pd.ns > 0) {      // an earlier lane of this run with the same source buffer: borrow its preparation
      for (uint32_t j = 0; j < l; j++) {
        const qn_pair_desc& pj = pairs[L[j].pair];
        if (L[j].active && L[j].alias < 0 && pj.src == pd.src && pj.ns == pd.ns && pj.stride_bytes == pd.stride_bytes && pj.on_device == pd.on_device) { R.alias = (int)j; break; }
      }
      if (R.alias >= 0) { alias_guard.borrow(l, L[R.alias].c); R.build_source = false; }
    }
    int rc = QN_OK; GridLaunch gs, gt;
    if (R.build_source) { last_src[l] = nullptr; rc = lane_set_cloud(c, QN_SOURCE, pd.src, pd.ns, pd.stride_bytes, pd.on_device != 0, s, &gs); }       // :120
    if (rc == QN_OK) { ScratchSwap sw(c); rc = lane_set_cloud(c, QN_TARGET, pd.dst, pd.nt, pd.stride_bytes, pd.on_device != 0, s, &gt); }                 // :122
    if (rc == QN_ERR_HIP) return rc;
    status[R.pair] = rc;
    if (rc != QN_OK) {      // the lane drops out BEFORE its grid entries are pushed: a source prepared above (prep_grid marked it has_grid) was never built - leave no stale flag behind (ADVICE r4)
      if (R.build_source) { c->cloud[0].has_grid = c->cloud[0].has_cov = false; c->cloud[0].n = 0; }
      c->cloud[1].has_grid = c->cloud[1].has_cov = false; c->cloud[1].n = 0;
      continue;
    }
    if (R.build_source) { push_grid(gs); push_knn(prep_knn(c, c->cloud[0], k, c->knn_idx, nullptr, true)); c->cloud[0].has_cov = true; note_knn_table(c, c->cloud[0], c->knn_idx, k); }      // :121
    { ScratchSwap sw(c); push_grid(gt); push_knn(prep_knn(c, c->cloud[1], k, c->knn_idx, nullptr, true)); c->cloud[1].has_cov = true; note_knn_table(c, c->cloud[1], c->knn_idx, k); }         // :123
    last_src[l] = R.alias >= 0 ? nullptr : pd.src; last_key[l] = key;
    R.active = true;
  }
  plan.add<PackBBoxK>(v_pack, QN_K_GRID_BUILD); plan.add<CellCountK>(v_count, QN_K_GRID_BUILD); plan.add<ScanLookbackK>(v_scan, QN_K_GRID_BUILD); plan.add<ScatterK>(v_scat, QN_K_GRID_BUILD); plan.add<StableCellsK>(v_stab, QN_K_GRID_BUILD);
  // (knn_mm 0: the VALU-scoring forms of both histogram passes)
  if (k <= 24) {
    if (owner->lane.knn_mm) { plan.add<KnnHistK<false, 32>>(v_sel, QN_K_KNN_SELECT); plan.add<KnnHistK<true, 32>>(v_lst, QN_K_KNN_COV); }
    else { plan.add<KnnHistK<false, 32, false>>(v_sel, QN_K_KNN_SELECT); plan.add<KnnHistK<true, 32, false>>(v_lst, QN_K_KNN_COV); }
  } else {
    if (owner->lane.knn_mm) { plan.add<KnnHistK<false, 48>>(v_sel, QN_K_KNN_SELECT); plan.add<KnnHistK<true, 48>>(v_lst, QN_K_KNN_COV); }
    else { plan.add<KnnHistK<false, 48, false>>(v_sel, QN_K_KNN_SELECT); plan.add<KnnHistK<true, 48, false>>(v_lst, QN_K_KNN_COV); }
  }
  plan.add<KnnSingleK>(v_single, QN_K_KNN_COV);
  if (k <= 16) plan.add<KnnCovK<16, true, 4>>(v_tail, QN_K_KNN_COV); else if (k <= 20) plan.add<KnnCovK<20, true, 4>>(v_tail, QN_K_KNN_COV); else if (k <= 24) plan.add<KnnCovK<24, true, 4>>(v_tail, QN_K_KNN_COV); else plan.add<KnnCovK<32, true, 4>>(v_tail, QN_K_KNN_COV);
  plan.add<CovFromIdxK>(v_cov, QN_K_KNN_COV);

  // ---- align() (loop_closure.cpp:124): gicp_align's batch-member form, every lane with its own chunk boundaries and far-query regime
  const int per_outer = p.optimizer == QN_OPT_LM ? 2 : 1;
  const int maxit = p.force_iterations > 0 ? p.force_iterations : p.max_iterations;
  const int fixed_unseeded = fixed_unseeded_iterations(owner) * per_outer;
  const bool exact_ticks = p.force_iterations > 0 && p.optimizer == QN_OPT_GN;
  {
    std::vector<LaneEntry<InitStateK::Args>> v_init; std::vector<float> g16;
    for (LaneRun& R : L) {
      if (!R.active) continue;
      qn_ctx* c = R.c;
      c->gen = 0; c->part_rows = 0; c->far_mode = 2; c->clear_far_now = true; c->unseeded_until = fixed_unseeded; c->count_far_now = false;
      c->result_host->phase = 0;
      R.ticks_left = exact_ticks ? maxit : 1 << 30;
      R.chunk = std::min(fixed_unseeded, R.ticks_left); R.chunk_start = 0; R.next = R.chunk; R.first_chunk = true;
      R.budget = (long)maxit * (p.optimizer == QN_OPT_LM ? (p.lm_max_iterations + 1) : 1) + 2;
      lane_push(v_init, InitStateK::Args{st_cur(c), c->guess_tmp, guesses16 ? 1 : 0, 0, c->far_stats}, 1u);
      if (guesses16) g16.insert(g16.end(), guesses16 + 16 * (size_t)R.pair, guesses16 + 16 * (size_t)R.pair + 16);
    }
    if (!guesses16) plan.add<InitStateK>(v_init, QN_K_SOLVE);
    else                   // the lanes' guesses ride in the segment's one arena upload, in front of the table that points at them (k_init_state's `guess` of gicp_align)
      plan.add<InitStateK>(v_init, QN_K_SOLVE, g16.data(), sizeof(float) * g16.size(), [](std::vector<LaneEntry<InitStateK::Args>>& e, const char* d) {
        for (size_t j = 0; j < e.size(); j++) e[j].a.guess = (const float*)(d + sizeof(float) * 16 * j);
      });
  }
  auto finish_lane = [&](LaneRun& R, int rc) {
    qn_ctx* c = R.c;
    R.active = false;
    status[R.pair] = rc;
    if (rc != QN_OK) return;
    results[R.pair] = c->result_host->r;
    c->trace_len = c->result_host->trace_len; c->aligned_valid = true;
    valid[R.pair] = (results[R.pair].converged && results[R.pair].fitness < thr) ? 1 : 0;                                                                 // :129
  };
  struct ProfFlush { qn_ctx* c; ~ProfFlush() { c->prof_collect(); } } prof_flush{owner};
  int tick_no = 0;
  for (;;) {
    int stop = 1 << 30; bool any = false;
    for (const LaneRun& R : L) if (R.active) { any = true; stop = std::min(stop, R.next); }
    if (!any) break;
    for (; tick_no < stop; tick_no++) {
      // every lane is in its own regime (unseeded_until: the fixed unseeded ticks, plus the outer iterations a lane whose pose still moves by metres adds - unseeded_goes_on)
      {                    // unseeded lanes: grid search + list pass, accumulation with the controller step in its last block (enqueue_tick)
        std::vector<LaneEntry<NnSearchArgs>> v_g, v_l; std::vector<LaneEntry<AccumulateK::Args>> v_acc;
        bool group = true, lane = true;
        for (LaneRun& R : L) {
          if (!R.active || tick_no >= R.c->unseeded_until) continue;
          qn_ctx* c = R.c;
          const int t = tick_no - R.chunk_start;
          c->count_far_now = R.first_chunk && (t / per_outer == (R.chunk - 1) / per_outer);      // far-query statistics: the chunk's last unseeded linearisation
          const NnLaunch N = prep_nn(c, 0, c->sqd, 0);
          group = group && N.group; lane = lane && N.lane;
          lane_push(v_g, N.grid, N.grid_nb); lane_push(v_l, N.list, N.list_nb);
          const uint32_t nb = acc_blocks(c);
          lane_push(v_acc, prep_accumulate(c, 0, true), nb);
          c->count_far_now = false;
        }
        if (lane) plan.add<NnLaneK<0>>(v_g, QN_K_NN_SEARCH); else plan.add<NnSearchK<0, false, QN_NN_BLOCK>>(v_g, QN_K_NN_SEARCH);
        if (group) plan.add<NnSearchK<0, true, QN_BLOCK, true>>(v_l, QN_K_NN_FALLBACK); else plan.add<NnSearchK<0, true, QN_BLOCK>>(v_l, QN_K_NN_FALLBACK);
        plan.add<AccumulateK>(v_acc, QN_K_ACCUMULATE);
      }
      {                    // tracked lanes: the fused tick (controller step in its last block); lanes in the refresh regime get k_far + k_far_reduce behind it, which then runs the step (enqueue_tick_fused)
        std::vector<LaneEntry<TickArgs>> v_t; std::vector<LaneEntry<FarArgs>> v_f; std::vector<LaneEntry<FarReduceK::Args>> v_r;
        for (LaneRun& R : L) {
          if (!R.active || tick_no < R.c->unseeded_until) continue;
          qn_ctx* c = R.c;
          const TickArgs a = tick_args(c);
          lane_push(v_t, a, tick_blocks(c));
          if (a.far_mode == 1) { lane_push(v_f, far_args(c), (uint32_t)QN_FAR_BLOCKS); lane_push(v_r, far_reduce_args(c), 1u); }
          c->gen++; c->part_rows = -1;
        }
        plan.add<TickK<TICK_TB, 4, 0, false>>(v_t, QN_K_GN_TICK_FUSED); plan.add<FarK>(v_f, QN_K_FAR); plan.add<FarReduceK>(v_r, QN_K_FAR);
      }
    }
    // chunk ends of the lanes whose boundary this is: the statistics block only (forced Gauss-Newton runs that cannot be done yet), or the closing pass
    {
      std::vector<LaneEntry<FinalizeK::Args>> v_fin; std::vector<LaneEntry<TickArgs>> v_close; std::vector<LaneEntry<FinalizeFitK::Args>> v_fit;
      for (LaneRun& R : L) {
        if (!R.active || R.next != stop) continue;
        qn_ctx* c = R.c;
        if (exact_ticks && R.ticks_left > R.chunk) lane_push(v_fin, FinalizeK::Args{st_cur(c), c->result_host, c->far_stats}, 1u);
        else {             // enqueue_epilogue, fused form (tick_no > 0 here: every chunk holds at least one tick)
          const TickArgs a = tick_args(c, 1);
          const uint32_t nb = tick_blocks(c);
          lane_push(v_close, a, nb);
          lane_push(v_fit, FinalizeFitK::Args{st_cur(c), c->result_host, c->far_stats, c->fit_psum, c->fit_pcnt, (int)tick_rows(c)}, 1u);
        }
      }
      plan.add<FinalizeK>(v_fin, QN_K_SOLVE); plan.add<TickK<TICK_TB, 4, 1, false>>(v_close, QN_K_FITNESS); plan.add<FinalizeFitK>(v_fit, QN_K_FITNESS);
    }
    const auto tt0 = std::chrono::steady_clock::now();
    int rc = plan.run();
    if (rc != QN_OK) return rc;
    const auto tt1 = std::chrono::steady_clock::now();
    HIPCHK(owner, hipStreamSynchronize(s));
    if (owner->knob.batch_trace) { const auto tt2 = std::chrono::steady_clock::now();
      fprintf(stderr, "qn batch %p: segment to tick %d  prep+enqueue %.0f us  sync %.0f us  (since call %.0f us)\n", (void*)owner, stop, std::chrono::duration<double, std::micro>(tt1 - tt0).count(),
              std::chrono::duration<double, std::micro>(tt2 - tt1).count(), std::chrono::duration<double, std::micro>(tt2 - t_call).count()); }
    for (LaneRun& R : L) {
      if (!R.active || R.next != stop) continue;
      qn_ctx* c = R.c;
      if (R.first_chunk && (rc = clouds_valid(c)) != QN_OK) { last_src[&R - &L[0]] = nullptr; finish_lane(R, rc); continue; }
      R.budget -= std::max(R.chunk, 1); R.ticks_left -= R.chunk;
      if (c->result_host->phase == 2) { finish_lane(R, QN_OK); continue; }
      if (R.budget <= 0) { c->last_error = "align: device state machine did not terminate"; owner->last_error = c->last_error; finish_lane(R, QN_ERR_HIP); continue; }
      if (R.first_chunk && unseeded_goes_on(c, stop, per_outer, R.ticks_left)) {      // the pose still moves by more than a fraction of a cell: one more unseeded outer iteration, then look again
        c->unseeded_until = stop + per_outer; R.chunk = per_outer; R.chunk_start = stop; R.next = stop + R.chunk;
        continue;                                        // (first_chunk stays set: the far-query statistics are those of the LAST unseeded linearisation)
      }
      const qn::ResultBlock* rb = c->result_host;      // far queries: keep the refresh kernel in the chain only while ticks actually ask for refreshes
      if (R.first_chunk) c->far_mode = rb->far_queries * 16u > c->cloud[0].n ? 1 : 2;
      else c->far_mode = (c->far_mode == 1 ? rb->far_requests : rb->far_misses / (uint32_t)std::max(1, R.chunk)) > 256u ? 1 : 2;
      if (!exact_ticks) R.chunk = R.first_chunk ? TICKS_PER_CHUNK : std::max(2 * per_outer, TICKS_PER_CHUNK / 2);
      else R.chunk = c->far_mode == 1 ? std::min(R.ticks_left, FAR_CHUNK) : R.ticks_left;
      if (R.budget <= 0 || R.chunk <= 0) { c->last_error = "align: device state machine did not terminate"; owner->last_error = c->last_error; finish_lane(R, QN_ERR_HIP); continue; }
      R.first_chunk = false; R.chunk_start = stop; R.next = stop + R.chunk;
    }
  }
  owner->batch_pairs += m;
  fail_guard.armed = false;
  return QN_OK;
}

}  // namespace

// SURVEY.md 8b: n_pairs independent LoopClosure::icpAlignment calls (loop_closure.cpp:110-136) on ONE context, `batch_lanes` of them per kernel launch.
// Parameters are the context's (qn_gicp_set_params).  status[i] = the pair's own status; the return value is QN_OK unless the batch machinery itself failed.
// guesses16 (n_pairs x 16 floats, row-major; null = identity): pair i is align(output, guess i) - NanoGICP::align with a guess, what qn_gicp_align(guess) runs.
extern "C" int qn_gicp_align_batch_guess(qn_ctx* c, const qn_pair_desc* pairs, const float* guesses16, uint32_t n_pairs, double score_thr, qn_gicp_result* results, int* valid, int* status) {
  if (!c || (n_pairs && (!pairs || !results || !valid || !status))) return QN_ERR_INVALID_ARG;
  if (guesses16)
    for (uint32_t i = 0; i < n_pairs; i++) {
      const float* g = guesses16 + 16 * (size_t)i;
      for (int j = 0; j < 16; j++) if (!std::isfinite(g[j])) { c->last_error = "align_batch_guess: non-finite guess entry"; return QN_ERR_INVALID_ARG; }
      if (g[12] != 0.f || g[13] != 0.f || g[14] != 0.f || g[15] != 1.f) { c->last_error = "align_batch_guess: a guess's last row is not 0 0 0 1"; return QN_ERR_INVALID_ARG; }
    }
  if (n_pairs == 0) return QN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (join_target(c) != QN_OK) return QN_ERR_HIP;
  int rc = batch_supported(c) ? batch_ensure_lanes(c) : QN_ERR_NOT_READY;
  if (rc != QN_OK) {                       // knobs that rule the lanes out, or no memory for them: the classic path, pair by pair, as a batch member (same results; what qn_icp_alignment_batch does too)
    const bool sp = c->knob.pair_pipeline, sb = c->knob.persist_batch_off; c->knob.pair_pipeline = false; c->knob.persist_batch_off = true;
    for (uint32_t i = 0; i < n_pairs; i++) {
      const qn_pair_desc& p = pairs[i];
      const bool same = c->knob.batch_share_source && i > 0 && status[i - 1] == QN_OK && pairs[i - 1].src == p.src && pairs[i - 1].ns == p.ns && pairs[i - 1].stride_bytes == p.stride_bytes && pairs[i - 1].on_device == p.on_device;
      status[i] = icp_alignment(c, p.src, p.ns, p.dst, p.nt, p.stride_bytes, score_thr, &results[i], &valid[i], p.on_device ? 1 : 0, same,
                                guesses16 ? guesses16 + 16 * (size_t)i : nullptr);
    }
    c->knob.pair_pipeline = sp; c->knob.persist_batch_off = sb;
    return QN_OK;
  }
  const bool sp = c->knob.pair_pipeline, sb = c->knob.persist_batch_off;
  const uint32_t B = (uint32_t)c->lanes.size();
  std::vector<const float*> last_src(B, nullptr); std::vector<uint64_t> last_key(B, 0);      // (within THIS call: same pointer = same cloud)
  std::vector<uint32_t> idx(B);
  for (uint32_t base = 0; base < n_pairs && rc == QN_OK; base += B) {
    const uint32_t m = std::min(B, n_pairs - base);
    for (uint32_t l = 0; l < m; l++) idx[l] = base + l;
    rc = batch_register(c, pairs, idx.data(), m, score_thr, results, valid, status, last_src, last_key, guesses16);
  }
  c->knob.pair_pipeline = sp; c->knob.persist_batch_off = sb;
  if (rc != QN_OK) (void)hipStreamSynchronize(c->stream);
  return rc;
}
extern "C" int qn_gicp_align_batch(qn_ctx* c, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr, qn_gicp_result* results, int* valid, int* status) {
  return qn_gicp_align_batch_guess(c, pairs, nullptr, n_pairs, score_thr, results, valid, status);
}
