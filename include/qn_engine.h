/* qn_engine.h - C-ABI of the MI355X-native loop-closure registration engine.
 *
 * This is the drop-in boundary for the ONE hot path of engcang/FAST-LIO-SAM-QN: the
 * Nano-GICP + Quatro scan matching that FastLioSamQn::loopTimerFunc triggers
 * (fast_lio_sam_qn/src/fast_lio_sam_qn.cpp:203-252 -> LoopClosure::icpAlignment /
 * coarseToFineAlignment, fast_lio_sam_qn/src/loop_closure.cpp:110-159).
 *
 * The reference has no FFI: its boundary is two C++ class templates,
 * nano_gicp::NanoGICP<> and quatro<> (includes at include/loop_closure.h:16-19, members at
 * :75-76).  The header-only C++ shims in fast-lio-sam-qn_amd/shim/ reproduce those classes and
 * call ONLY the functions declared here; each entry point below names the reference call it
 * stands behind.  Plain C: int status returns, caller-owned buffers, no exceptions, no torch
 * or PCL/Eigen types.  One context per host thread (the reference enters the engines from one
 * timer thread at a time); a context is NOT re-entrant.
 *
 * Matrices are 4x4 ROW-major.  Point buffers are `n` points of 3 leading floats (x, y, z) with
 * `stride_bytes` between points (32 for pcl::PointXYZI, 16 for float4, 12 for packed xyz).
 * "_device" variants take HIP device pointers (same layout) and do no host<->device copies.
 */
#ifndef QN_ENGINE_H
#define QN_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qn_ctx qn_ctx;

enum {
  QN_OK = 0,
  QN_ERR_INVALID_ARG = 1,     /* null pointer, bad stride, bad enum                          */
  QN_ERR_EMPTY_CLOUD = 2,     /* a cloud with 0 points (registration yields valid = 0)       */
  QN_ERR_CAPACITY = 3,        /* cloud larger than the context's max_points                  */
  QN_ERR_NOT_READY = 4,       /* align before both clouds and both covariance sets exist     */
  QN_ERR_HIP = 5,             /* a HIP runtime call failed; see qn_last_error()              */
  QN_ERR_NO_DEVICE = 6,       /* no gfx950 device: the engine has NO CPU fallback            */
  QN_ERR_INTERNAL = 7         /* a bounded device loop did not end within its proven bound   */
};

enum { QN_SOURCE = 0, QN_TARGET = 1 };
enum { QN_OPT_LM = 0, QN_OPT_GN = 1 };

/* Mirrors what LoopClosure's ctor pushes through the 8 NanoGICP setters
 * (loop_closure.cpp:9-16; struct NanoGICPConfig, include/loop_closure.h:25-36) plus the
 * LsqRegistration knobs the reference leaves at their defaults.          */
typedef struct {
  int32_t k_correspondences;       /* setCorrespondenceRandomness  (loop_closure.cpp:10); default 20  */
  int32_t max_iterations;          /* setMaximumIterations         (loop_closure.cpp:11); default 64  */
  double  max_corr_dist;           /* setMaxCorrespondenceDistance (loop_closure.cpp:13); default FLT_MAX */
  double  transformation_epsilon;  /* setTransformationEpsilon     (loop_closure.cpp:14); default 5e-4 */
  double  rotation_epsilon;        /* LsqRegistration default 2e-3 (no setter called by the reference) */
  int32_t optimizer;               /* QN_OPT_LM (reference default) | QN_OPT_GN                        */
  int32_t lm_max_iterations;       /* 10                                                               */
  double  lm_init_lambda_factor;   /* 1e-9                                                             */
  int32_t force_iterations;        /* bench only: > 0 runs exactly this many outer iterations          */
  int32_t ransac_iterations;       /* setRANSACIterations (loop_closure.cpp:12): stored, unused by the LSQ path */
  double  ransac_outlier_threshold;/* setRANSACOutlierRejectionThreshold (loop_closure.cpp:16): stored, unused  */
  double  euclidean_fitness_epsilon;/* setEuclideanFitnessEpsilon (loop_closure.cpp:15): stored, unused         */
} qn_gicp_params;

/* What icpAlignment reads back (loop_closure.cpp:127-133): getFitnessScore(), hasConverged(),
 * getFinalTransformation() - plus the f64 state and iteration trace used by the parity tests. */
typedef struct {
  float   T[16];          /* final_transformation_ (f32, as the reference returns it)            */
  double  T64[16];        /* the f64 estimate before the cast                                     */
  double  H[36];          /* final_hessian_                                                       */
  double  fitness;        /* pcl getFitnessScore(): mean squared NN distance over all src points  */
  int32_t iterations;     /* outer iterations executed                                            */
  int32_t converged;      /* hasConverged()                                                       */
  int32_t lm_failed;      /* "lm not converged!!" path taken                                      */
  int32_t reserved;
} qn_gicp_result;

/* one row per outer iteration, for trajectory parity */
typedef struct { double y0, lambda, rho, max_dR, max_dt; int32_t inner, accepted; } qn_iter_trace;

typedef struct {           /* device-side accounting of one kernel family (bench roofline leg) */
  double  total_ms;
  int64_t launches;
} qn_kernel_stat;

enum {                     /* kernel families for qn_prof_get */
  QN_K_GRID_BUILD = 0, QN_K_KNN_COV = 1, QN_K_NN_SEARCH = 2, QN_K_NN_FALLBACK = 3,
  QN_K_ACCUMULATE = 4, QN_K_SOLVE = 5, QN_K_FITNESS = 6, QN_K_TRANSFORM = 7,
  QN_K_FPFH_NORMALS = 8, QN_K_FPFH_SPFH = 9, QN_K_FPFH_FPFH = 10, QN_K_FEAT_MATCH = 11,
  QN_K_GN_TICK_FUSED = 12,   /* fused Gauss-Newton tick: tracking NN + leftovers + accumulation in one kernel       */
  QN_K_KNN_SELECT = 13,      /* k-NN selection kernel alone (QN_K_KNN_COV then holds its list tail + covariances)  */
  QN_K_FAR = 15,             /* refresh of far queries' candidate lists (k_far)                                     */
  QN_K_MATCH_TAIL = 14,      /* Matcher tail on the device: means, cross-check + gate, tuple test, hand-over        */
  QN_K_ALIGN_PERSIST = 16,   /* the persistent align kernel: every tracked tick + closing pass of one align in ONE launch */
  QN_K_COUNT = 17
};

/* ---- lifetime ------------------------------------------------------------------------- */
/* max_points: the largest cloud the context takes, at most QN_CTX_MAX_POINTS; a larger value returns QN_ERR_CAPACITY before anything is allocated
 * (qn_multi_init inherits the limit).  The k-NN screen packs a point's position in the cell-sorted cloud into a 26-bit field (qn_knn_hist.cuh). */
#define QN_CTX_MAX_POINTS (1u << 26)
int  qn_ctx_create(int device, uint32_t max_points, qn_ctx** out);
void qn_ctx_destroy(qn_ctx* ctx);
const char* qn_status_str(int status);
const char* qn_last_error(const qn_ctx* ctx);
/* The context's primary hipStream_t.  NOT an ordering guarantee for inputs: the engine also works on a private second stream (the target
 * cloud of a pair is prepared there while the source's k-NN runs), so device buffers handed to a *_device entry point must be COMPLETE
 * before the call (synchronise the producer, or make it wait on an event of yours); outputs are complete when the call returns.     */
void* qn_ctx_stream(qn_ctx* ctx);
int  qn_ctx_synchronize(qn_ctx* ctx);

/* ---- Nano-GICP ------------------------------------------------------------------------ */
void qn_gicp_default_params(qn_gicp_params* p);                       /* NanoGICP()/LsqRegistration() ctor defaults */
/* loop_closure.cpp:9-16.  QN_ERR_INVALID_ARG, and the context keeps its previous parameters, unless 1 <= k_correspondences <= 32, max_iterations >= 0,
 * lm_max_iterations >= 1, max_corr_dist > 0 and lm_init_lambda_factor >= 0 (a negative factor makes H + lambda I indefinite: no defined step).
 * Both epsilons are taken as they are, NaN and 0 included, with the reference's stopping rule max(mr / rotation_epsilon, mt / transformation_epsilon) < 1
 * and std::max's (a < b) ? b : a: a NaN rotation ratio (epsilon NaN, or 0 with an exact-identity rotation step) never converges, a NaN translation
 * ratio leaves the decision to the rotation's, and an epsilon of 0 never converges on a non-zero step.  max_iterations = 0: T = the guess, iterations 0,
 * not converged, H = identity, fitness at the guess. */
int  qn_gicp_set_params(qn_ctx*, const qn_gicp_params*);
int  qn_gicp_get_params(const qn_ctx*, qn_gicp_params* out);          /* what the setters above last stored (the getters of pcl::Registration / NanoGICP) */
/* setInputSource / setInputTarget do not wait for the GPU: upload, packing and the grid build (its numbers are derived from the bounding box ON the
 * device) are enqueued and the call returns.  Consequences at this boundary: (1) a cloud with non-finite coordinates is refused by the first call that
 * synchronises (align, fitness, a read-back) with QN_ERR_INVALID_ARG, not by the setter; (2) pageable host buffers are consumed when the setter returns
 * (hipMemcpyAsync stages them before returning); PAGE-LOCKED host buffers and the device buffers of the *_device variants are read asynchronously and
 * must stay unchanged until the next synchronising call of this context (qn_gicp_align, qn_ctx_synchronize, ...).                                  */
int  qn_gicp_set_source(qn_ctx*, const float* xyz, uint32_t n, uint32_t stride_bytes);          /* setInputSource, loop_closure.cpp:120 */
int  qn_gicp_set_target(qn_ctx*, const float* xyz, uint32_t n, uint32_t stride_bytes);          /* setInputTarget, loop_closure.cpp:122 */
int  qn_gicp_set_source_device(qn_ctx*, const float* d_xyz, uint32_t n, uint32_t stride_bytes);
int  qn_gicp_set_target_device(qn_ctx*, const float* d_xyz, uint32_t n, uint32_t stride_bytes);
int  qn_gicp_compute_covariances(qn_ctx*, int which);                 /* calculateSource/TargetCovariances, loop_closure.cpp:121,123 */
int  qn_gicp_align(qn_ctx*, const float guess[16], qn_gicp_result* out);  /* align(), loop_closure.cpp:124 (guess NULL = identity); also fills fitness */
int  qn_gicp_fitness(qn_ctx*, double max_range, double* score);       /* getFitnessScore(), loop_closure.cpp:127 */
int  qn_gicp_transformed_source(qn_ctx*, float* xyz_out, uint32_t stride_bytes);  /* the `aligned_` cloud align() fills, loop_closure.cpp:124 */
int  qn_gicp_get_trace(qn_ctx*, qn_iter_trace* out, uint32_t cap, uint32_t* n);
/* the same for lane `lane` of the latest qn_gicp_align_batch run on this context (lane l of a run carries the l-th pair of that run) */
int  qn_gicp_get_lane_trace(qn_ctx*, uint32_t lane, qn_iter_trace* out, uint32_t cap, uint32_t* n);
/* The k-NN index table cloud `which` (QN_SOURCE / QN_TARGET) of lane `lane` was last given its covariances from - the table the registration used, not a
 * fresh search: n x k int32 in the cloud's original point order, row i = the k nearest of point i in ascending (squared distance, index) order, -1 for a
 * missing neighbour (a cloud of fewer than k points).  idx_out NULL: only *n and *k.  Indices only (the batched path keeps no distances).  Same lane
 * convention as qn_gicp_get_lane_trace.  QN_ERR_NOT_READY when the table is gone: the cloud was set anew, k changed, or the buffer now holds the other
 * cloud's table (the target's covariances overwrite the source's table unless the target was prepared on the second stream); also for a lane that borrowed
 * its source from another lane of the run (the lending lane's table is the one to read). */
int  qn_gicp_get_lane_knn(qn_ctx*, uint32_t lane, int which, int32_t* idx_out, uint32_t* n, int* k);
/* qn_gicp_get_covariances of lane `lane` (n x 9 row-major 3x3, rebuilt from the normals the lane holds) */
int  qn_gicp_get_lane_covariances(qn_ctx*, uint32_t lane, int which, double* cov9_out);

/* LoopClosure::icpAlignment in one call (loop_closure.cpp:110-136): set x2, cov x2, align, score,
 * accept test `converged && score < score_thr` (loop_closure.cpp:129).  *valid receives is_valid_. */
int  qn_icp_alignment(qn_ctx*, const float* src, uint32_t ns, const float* dst, uint32_t nt,
                      uint32_t stride_bytes, double score_thr, qn_gicp_result* out, int* valid);
int  qn_icp_alignment_device(qn_ctx*, const float* d_src, uint32_t ns, const float* d_dst, uint32_t nt,
                             uint32_t stride_bytes, double score_thr, qn_gicp_result* out, int* valid);
/* The candidates of ONE loop-closure query share their source cloud: after a qn_icp_alignment[_device] call the context still holds the
   source's grid and covariances; this registers another target against it (the reference rebuilds the source per call,
   loop_closure.cpp:116-123, because it only ever tries one candidate).  QN_ERR_NOT_READY without a prepared source. */
int  qn_icp_alignment_same_source(qn_ctx*, const float* dst, uint32_t nt, uint32_t stride_bytes, int dst_on_device, double score_thr, qn_gicp_result* out, int* valid);

/* ---- batch of independent candidate pairs (BASELINE config "batch of 64 candidate keyframe pairs") ----
 * Every candidate pair of a loop-closure query is an independent icpAlignment (loop_closure.cpp:116-123 rebuilds
 * everything per call), so a batch is spread over several contexts = several hipStreams of one GPU: worker i drives
 * ctxs[i] and pulls the next unprocessed pair.  Parameters are those already set on each context.  status[i] receives
 * the per-pair status code.  Returns QN_OK when every pair ran (individual pairs may still be invalid).          */
typedef struct {
  const float* src; uint32_t ns;
  const float* dst; uint32_t nt;
  uint32_t stride_bytes;
  int32_t  on_device;              /* 1: src/dst are HIP device pointers */
} qn_pair_desc;
int  qn_icp_alignment_batch(qn_ctx* const* ctxs, uint32_t n_ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr,
                            qn_gicp_result* results, int* valid, int* status);
/* The same batch on ONE context with the PAIR AS A GRID DIMENSION (SURVEY.md 8b qn_gicp_align_batch; 7.1 step 8): the pairs are registered `lanes` at a
 * time (default 8; qn_debug_set(ctx, "batch_lanes", B)) in lockstep - every kernel of the chain is launched once for all of them, blockIdx.y selecting the
 * pair's entry of a device-resident argument table - on the context's one stream.  Each pair is an independent icpAlignment (loop_closure.cpp:110-136) with the
 * context's parameters; pairs of ONE call that name the same source buffer (pointer, size, stride) share one preparation of it - grid and covariances - the way the
 * candidates of one loop-closure query share the query cloud (qn_debug_set(ctx, "batch_share_source", 0): every pair rebuilds its source like loop_closure.cpp:120-121).
 * Records are bit-identical to qn_icp_alignment_batch's one-pair-per-stream path.  qn_icp_alignment_batch itself uses this per context.
 * MEMORY: a context that registers batches owns `batch_lanes` - 1 sub-contexts, each with a full max_points slab (~1.2 KB per point of max_points: 119 MB at 100k), created on the
 * first batch call: batch_lanes x in_flight x slab in total (8 x 3 x 119 MB = 2.9 GB at the bench's setting; batch_lanes = 64 at 100k is 7.6 GB per context).  If the lanes cannot be
 * allocated, the ones created so far are freed again and both entry points register the pairs one at a time on the context itself (same records).                        */
int  qn_gicp_align_batch(qn_ctx*, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr, qn_gicp_result* results, int* valid, int* status);
/* The same batch with an initial guess per pair: pair i is align(output, guesses16[16 i .. 16 i + 15]) (NanoGICP::align with a guess, what qn_gicp_align(guess)
 * runs), row-major 4x4 f32, through the same lanes; guesses16 = NULL is qn_gicp_align_batch itself (identity).  Any non-finite guess entry, or a last row other
 * than 0 0 0 1: QN_ERR_INVALID_ARG before anything runs.  The guesses reach the device inside each segment's one argument upload.                        */
int  qn_gicp_align_batch_guess(qn_ctx*, const qn_pair_desc* pairs, const float* guesses16, uint32_t n_pairs, double score_thr,
                               qn_gicp_result* results, int* valid, int* status);

/* ---- candidate pairs sharded over the GPUs of one node (BASELINE "batch of 64 candidate keyframe pairs sharded
 * across 8 MI355X, RCCL gather of best loop").  The reference registers ONE candidate per timer tick
 * (fast_lio_sam_qn.cpp:213-219 -> loop_closure.cpp:168-205); the generalisation keeps every registration independent: pair i runs on
 * GPU i mod N on one of `in_flight` contexts, no data-path collective, then ONE ncclAllGather (RCCL over xGMI) of the fixed-size
 * records below and the host picks the valid record with the smallest score.  Single process, all GPUs (ncclCommInitAll), like the
 * reference's single process.  qn_multi_init fails with QN_ERR_NO_DEVICE when fewer than n_gpus devices are visible.              */
typedef struct qn_multi qn_multi;
typedef struct {            /* 96 bytes */
  int32_t pair_id;          /* index into `pairs`; -1 = padding slot of the gathered table                    */
  int32_t status;           /* qn status of this pair's icpAlignment                                            */
  int32_t valid;            /* is_valid_ (converged && score < score_thr, loop_closure.cpp:129)                 */
  int32_t converged;        /* hasConverged()                                                                   */
  int32_t iterations;
  int32_t reserved;
  double  fitness;          /* getFitnessScore()                                                                */
  float   T[16];            /* getFinalTransformation(), row-major                                              */
} qn_pair_record;
int  qn_multi_init(int n_gpus, const int* device_ids /* NULL: 0 .. n_gpus-1 */, uint32_t max_points, int in_flight, qn_multi** out);
void qn_multi_destroy(qn_multi*);
const char* qn_multi_last_error(const qn_multi*);    /* NULL argument: why the last qn_multi_init on this thread failed */
int  qn_multi_gpu_count(const qn_multi*);
/* ranks of the RCCL communicator as RCCL itself reports them (ncclCommCount on every GPU's communicator; the smallest answer, -1 if a query fails): a caller that
 * asked for N GPUs checks this equals N before it trusts a multi-GPU figure.  qn_multi_verify_gather: after a qn_multi_align_best, QN_OK iff EVERY GPU's receive buffer
 * holds the same gathered record table as GPU 0's (the all-gather delivered every rank's records to every rank, not just to the one the host reads)                     */
int  qn_multi_rccl_ranks(qn_multi*);
int  qn_multi_verify_gather(qn_multi*);
int  qn_multi_set_params(qn_multi*, const qn_gicp_params*);            /* loop_closure.cpp:9-16, on every context */
int  qn_multi_debug_set(qn_multi*, const char* key, double value);     /* qn_debug_set on every context (e.g. "batch_lanes": pairs per kernel launch of each context) */
/* host wall clock of the latest qn_multi_align_best: per GPU from the call's start to its last pair's end [n_gpus], and the gather step */
int  qn_multi_get_timing(const qn_multi*, double* per_gpu_ms, double* gather_ms);
/* pairs[i].src/dst: host buffers, or (on_device) buffers resident on GPU device_ids[i mod n_gpus].  records (optional, n_pairs
 * entries) receives every pair's record as rank 0 holds them after the gather; *best / *best_found the winning loop.             */
int  qn_multi_align_best(qn_multi*, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr,
                         qn_pair_record* records, qn_pair_record* best, int* best_found);

/* ---- Quatro coarse registration ---------------------------------------------------------- */
/* The 10 constructor arguments of quatro<PointType>, in the order LoopClosure passes them
 * (loop_closure.cpp:18-27; struct QuatroConfig, include/loop_closure.h:38-50), plus the seed of the
 * tuple test (the reference seeds rand() from wall-clock and does not reproduce itself).       */
typedef struct {
  double  fpfh_normal_radius;      /* loop_closure.cpp:18 */
  double  fpfh_radius;             /* :19 */
  double  noise_bound;             /* :20  >= 0.  0 = no measurement may deviate: the consistency graph keeps only TIMs of exactly equal length, the rotation's GNC
                                      takes TEASER++'s fallback bound (0.1^2), and each translation axis is the limit of the TLS estimate for a bound going to 0 -
                                      the residual value the most clique members share exactly, the smallest one on a tie (never the NaN the 1 / 0 weights would give) */
  double  rot_gnc_factor;          /* :21 */
  double  rot_cost_diff_thr;       /* :22 */
  int32_t rot_max_iter;            /* :23 */
  int32_t estimate_scale;          /* :24 estimat_scale_ (include/loop_closure.h:44; config.yaml ships false): 1 = TEASER++'s TLS scale solver over the TIM norm ratios runs in front of the
                                      consistency graph; rotation on dst TIMs / scale with the bound x 2 / scale, translation on dst - scale R src.  T stays [R | t] (upstream's quatro::align
                                      returns rotation and translation only); the scale itself: qn_quatro_get_scale */
  int32_t use_optimized_matching;  /* :25  1: Matcher::optimizedMatching (gate + cap), 0: Matcher::advancedMatching */
  double  distance_threshold;      /* :26 */
  int32_t max_num_corres;          /* :27 */
  uint32_t rng_seed;
  double  tuple_scale;             /* Matcher::calculateCorrespondences argument, 0.95 upstream */
} qn_quatro_params;

void qn_quatro_default_params(qn_quatro_params* p);                  /* the reference's effective values */
/* quatro<PointType> ctor, loop_closure.cpp:18-27.  QN_ERR_INVALID_ARG, and the context keeps its previous parameters, unless both radii are > 0 (not NaN),
 * noise_bound >= 0, rot_max_iter >= 1, max_num_corres >= 3 and tuple_scale > 0 */
int  qn_quatro_set_params(qn_ctx*, const qn_quatro_params*);
/* quatro<PointType>::align(src, dst, is_converged), loop_closure.cpp:144: T = 4x4 f64 row-major, *valid = is_converged */
int  qn_quatro_align(qn_ctx*, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride_bytes, double T[16], int* valid);
int  qn_quatro_align_device(qn_ctx*, const float* d_src, uint32_t ns, const float* d_dst, uint32_t nt, uint32_t stride_bytes, double T[16], int* valid);
/* LoopClosure::coarseToFineAlignment, loop_closure.cpp:138-159: Quatro, transformPcd, icpAlignment, T_gicp * T_quatro */
int  qn_coarse_to_fine_alignment(qn_ctx*, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride_bytes, double score_thr,
                                 qn_gicp_result* gicp_out, double T_total[16], double T_quatro[16], int* valid);
/* same with both clouds resident on the device (the output of qn_kf_assemble = setSrcAndDstCloud, loop_closure.cpp:177-192):
 * only the selected correspondences (<= ~6 KB) and the result record cross PCIe                                            */
int  qn_coarse_to_fine_alignment_device(qn_ctx*, const float* d_src, uint32_t ns, const float* d_dst, uint32_t nt, uint32_t stride_bytes, double score_thr,
                                        qn_gicp_result* gicp_out, double T_total[16], double T_quatro[16], int* valid);
/* The reference's DEFAULT per-candidate path for MANY candidates (enable_quatro_ = true, include/loop_closure.h:54 + config.yaml:31; dispatch loop_closure.cpp:188-192 ->
 * coarseToFineAlignment :138-159): n_pairs independent coarse-to-fine registrations over n_ctx contexts (= streams, one pooled host worker each).  Each context takes runs of
 * `batch_lanes` pairs: the Quatro device stages of a run are enqueued back to back (one lane's buffers per pair, ONE synchronisation per run), the host solver runs per pair,
 * transformPcd stays on the device, and the run's accepted pairs go through the GICP lanes (qn_gicp_align_batch's machinery).  Parameters: each context's own
 * (qn_gicp_set_params / qn_quatro_set_params).  results[i] = the fine stage's record, T_total[16 i ..] = T_gicp * T_quatro (row-major f64), T_quatro (optional) = the coarse
 * estimate, valid[i] = Quatro converged && GICP converged && score < score_thr, status[i] = the pair's own status.  Records equal qn_coarse_to_fine_alignment[_device] of
 * the same pair bit for bit.  Pairs of one run that name the same source buffer (the candidates of ONE loop-closure query) share the source's Quatro preparation - grid, normals,
 * SPFH, FPFH are made once per run of lanes and borrowed read-only by the other lanes (qn_debug_set(ctx, "batch_share_source", 0): every pair prepares its own, same records).
 * Memory: every lane allocates its own Quatro buffers on first use (~0.7 KB per point of max_points per lane).                                                          */
int  qn_coarse_to_fine_align_batch(qn_ctx* const* ctxs, uint32_t n_ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr,
                                   qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status);
/* enable_quatro_ (include/loop_closure.h:54): non-NULL = every pair of qn_multi_align_best is a coarseToFineAlignment (qn_coarse_to_fine_align_batch per GPU) with these
 * Quatro parameters, and the records carry T_gicp * T_quatro (cast to f32: the record layout is fixed); NULL = Nano-GICP only (icpAlignment), the default.             */
int  qn_multi_set_quatro_params(qn_multi*, const qn_quatro_params* p);
/* The two stages upstream Quatro exposes on its own:
 *  qn_fpfh            = FPFH descriptors of one cloud (pcl::FPFHEstimationOMP with the context's radii): n x 33 f32, caller order
 *  qn_match_optimized = teaser::Matcher::optimizedMatching(thr_dist, num_max_corres, tuple_scale) on two clouds + their
 *                       descriptors: mutual 33-D NN (GPU), distance gate, tuple test, cap; pairs = (src idx, dst idx)            */
int  qn_fpfh(qn_ctx*, const float* xyz, uint32_t n, uint32_t stride_bytes, float* fpfh33_out);
int  qn_match_optimized(qn_ctx*, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride_bytes,
                        const float* src_fpfh33, const float* dst_fpfh33, float thr_dist, int num_max_corres, float tuple_scale,
                        int32_t* pairs_out, uint32_t cap, uint32_t* n_out);

/* stages, for the parity tests: descriptors of the last qn_quatro_align (original point order; n x 3, n x 33, n x 33),
 * the align with its intermediate products, and the host solver alone (Matcher + TEASER++/Quatro solve)            */
int  qn_quatro_get_features(qn_ctx*, int which, float* normals3, float* spfh33, float* fpfh33);
int  qn_quatro_align_debug(qn_ctx*, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride_bytes, double T[16], int* valid,
                           int32_t* mutual_pairs, uint32_t* n_mutual, int32_t* corres_pairs, uint32_t* n_corres, uint32_t cap,
                           int32_t* clique, uint32_t* n_clique, int32_t* rot_iterations);
int  qn_quatro_solve(const float* src, const float* dst, uint32_t stride_bytes, const int32_t* corres_pairs, uint32_t n_corres,
                     const qn_quatro_params* p, double T[16], int* valid, int32_t* clique, uint32_t* n_clique);
/* the scale TEASER++'s solver estimated (1 unless estimate_scale): of the context's latest qn_quatro_align[_device/_debug] / coarse-to-fine call, and of the host solver alone */
int  qn_quatro_get_scale(qn_ctx*, double* scale);
int  qn_quatro_solve_scaled(const float* src, const float* dst, uint32_t stride_bytes, const int32_t* corres_pairs, uint32_t n_corres,
                            const qn_quatro_params* p, double T[16], int* valid, int32_t* clique, uint32_t* n_clique, double* scale);
/* the same, plus the number of GNC iterations the rotation stage ran (0 when no clique of two or more was found) */
int  qn_quatro_solve_iter(const float* src, const float* dst, uint32_t stride_bytes, const int32_t* corres_pairs, uint32_t n_corres,
                          const qn_quatro_params* p, double T[16], int* valid, int32_t* clique, uint32_t* n_clique, double* scale, int32_t* rot_iterations);

/* ---- feeder of the path, kept on the device -------------------------------
 * Keyframe clouds (PosePcd::pcd_, sensor frame, include/pose_pcd.hpp:7-19) are uploaded once and stay resident;
 * qn_kf_assemble = the inner loops of LoopClosure::setSrcAndDstCloud (loop_closure.cpp:70-107): transformPcd of each
 * listed keyframe with its pose, concatenation, voxelizePcd (pcl::VoxelGrid, include/utilities.hpp:38-51), entirely
 * on the GPU; the returned device pointer (float4, stride 16) feeds qn_icp_alignment_device / the batch API.     */
typedef struct qn_kf_store qn_kf_store;
int  qn_kf_store_create(int device, qn_kf_store** out);
void qn_kf_store_destroy(qn_kf_store*);
const char* qn_kf_last_error(const qn_kf_store*);
int  qn_kf_add(qn_kf_store*, const float* xyz, uint32_t n, uint32_t stride_bytes, int32_t* id_out);
int  qn_kf_assemble(qn_kf_store*, const int32_t* ids, const double* poses16, uint32_t count, double leaf, int slot,
                    const float** d_xyz_out, uint32_t* n_out);
int  qn_kf_download(qn_kf_store*, int slot, float* xyz_out /* n x 3 packed */);
/* S submaps in one pass (setSrcAndDstCloud for one query and its K candidates, loop_closure.cpp:58-108): submap s = transformPcd +
 * concatenation of ids[seg_off[s] .. seg_off[s+1]) with poses16 of the same entries, voxelizePcd at `leaf` - in all 16 bytes of every record
 * what qn_kf_assemble builds for that list (ids may repeat, within and across submaps).  d_xyz_out[s] / n_out[s] / status[s] per submap
 * (float4, stride 16).  Storage is the store's own batch slot: slots 0/1 and the map slot are never touched.  Valid until the next
 * qn_kf_assemble_batch on this store or its destruction.  Returns QN_OK when the call ran; a submap that is empty after dropping non-finite
 * points gets status QN_ERR_EMPTY_CLOUD and n 0 without failing the others.  The overflow guard is applied per submap from the box [min, max] of
 * its own finite points; with inv = 1 / (float)leaf, all in f32, it trips when (1) on any axis floor(min inv) or floor(max inv) is outside
 * [-2^31, 2^31), or (2) on any axis (max - min) inv is not below 2^63 (infinite included), or (3) PCL's own product of int64((max - min) inv) + 1
 * over the axes exceeds INT32_MAX, or (4) the cell count, the product of floor(max inv) - floor(min inv) + 1, exceeds INT32_MAX.  (1), (2) and (4)
 * deviate from pcl::VoxelGrid, which converts out of range and lets its index wrap there; the same rule holds for
 * qn_kf_assemble and qn_kf_build_map.  A tripped submap is its finite points, unfiltered, in concatenation order (qn_kf_last_error carries the warning).  Bad id, non-monotone
 * seg_off, leaf <= 0 or n_seg == 0: QN_ERR_INVALID_ARG before anything runs.  Two host synchronisations per call.                          */
int  qn_kf_assemble_batch(qn_kf_store*, const int32_t* ids, const double* poses16, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                          const float** d_xyz_out, uint32_t* n_out, int* status);
int  qn_kf_download_batch(qn_kf_store*, uint32_t seg, float* xyz_out /* n x 3 packed */);
int  qn_kf_batch_count(const qn_kf_store*, uint32_t seg, uint32_t* n);      /* points of segment `seg` of the batch slot (as n_out of the call that filled it) */
/* Drift-free verification of loop candidates (Scan Context's, typically) of one query: no cloud depends on the accumulated drift of the corrected poses.
 * Store ids are keyframe indices; poses16[i] = keyframe i's corrected pose, n_poses of them.  One qn_kf_assemble_batch into the store's batch slot:
 *   segment 0     = keyframe `query` alone with the exact identity pose (its sensor frame), voxel grid at `leaf` - the one source of every pair;
 *   segment 1 + j = the scan-to-submap window of cand[j] (loop_submap_ids(query, c, submap_range, no Quatro, no submap matching, n_poses)[1]: keyframes
 *                   c - submap_range .. c + submap_range with 0 <= i < n_poses - 1), keyframe i with Q_i = inv(P_c) P_i (inv(P) = [R^T | -R^T t]; every
 *                   entry of each product summed over k = 0..3 in order in f64, no fused multiply-add), voxel grid at `leaf`;
 * then ONE qn_gicp_align_batch_guess on ctx (its parameters) with pair j seeded by Rz(-yaw[j]): c = cos(-yaw), s = sin(-yaw) in f64 (C library), each entry
 * rounded to f32, [c -s 0 0; s c 0 0; 0 0 1 0; 0 0 0 1].  yaw[j] (NULL: all 0) = the candidate's heading minus the query's (qn_kf_sc_query's shift as
 * scancontext.yaw_of_shift).  results[j].T maps query-sensor points into the candidate's sensor frame: an estimate of inv(P_c) P_query; valid[j] follows
 * loop_closure.cpp:129.  status[j]: the candidate submap's assembly status (QN_ERR_EMPTY_CLOUD: valid 0, the others still run), else the registration's.
 * QN_ERR_INVALID_ARG before anything runs (store and context unchanged): a bad or repeated id, a candidate equal to the query, n_cand == 0, n_poses <= the
 * largest id used, a non-finite pose or yaw, leaf <= 0, or store and context on different devices.  Host synchronisations: the assembly's two and the
 * registration's own.                                                                                                                                  */
int  qn_kf_verify_loop_candidates(qn_kf_store*, qn_ctx*, int32_t query, const int32_t* cand, const double* yaw /* per candidate; NULL = 0 */,
                                  uint32_t n_cand, const double* poses16 /* n_poses x 16 */, uint32_t n_poses, uint32_t submap_range, double leaf,
                                  double score_thr, qn_gicp_result* results, int* valid, int* status);
/* The same check for arbitrary (query, candidate) pairs of MANY queries in one call - the keyframes that arrived between two loop-timer ticks
 * (fast_lio_sam_qn.cpp:203-252 checks only keyframes_.back()).  Pair j = (query[j], cand[j], yaw[j]); its record (results[j], valid[j], status[j]) equals
 * qn_kf_verify_loop_candidates(store, ctx, query[j], &cand[j], &yaw[j], 1, poses16, n_poses, submap_range, leaf, score_thr, ...) bit for bit.  Pairs may
 * come in any order; queries and candidates may repeat across pairs.  ONE qn_kf_assemble_batch into the store's batch slot, segments in this order:
 *   segments 0 .. Q - 1     = the distinct queries in order of first appearance, each alone with the identity (the single-query call's segment 0);
 *   segments Q .. Q + C - 1 = the distinct candidates in order of first appearance, each candidate's window relative to it (a window depends on c, the
 *                             poses and submap_range only, so each is built once however many queries name it);
 * then ONE qn_gicp_align_batch_guess over every pair whose two clouds exist, seeded as the single-query call, grouped by query (stable) so that a query's
 * pairs share the source preparation; the records are scattered back into caller order.  status[j]: the assembly status of the pair's query or candidate
 * segment (QN_ERR_EMPTY_CLOUD: valid 0, the other pairs still run), else the registration's.  QN_ERR_INVALID_ARG before anything runs (batch slot, verify
 * record and context unchanged): a null pointer, n_pairs == 0, a bad id, cand[j] == query[j], a repeated (query, cand) pair, an id >= n_poses, a
 * non-finite pose or yaw, leaf <= 0, or store and context on different devices.  Host synchronisations: the assembly's two and the registration's own,
 * whatever n_pairs is.                                                                                                                                */
int  qn_kf_verify_loop_pairs(qn_kf_store*, qn_ctx*, const int32_t* query, const int32_t* cand, const double* yaw /* per pair; NULL = 0 */, uint32_t n_pairs,
                             const double* poses16 /* n_poses x 16 */, uint32_t n_poses, uint32_t submap_range, double leaf,
                             double score_thr, qn_gicp_result* results, int* valid, int* status);
/* Resident Quatro descriptors per keyframe, for the reference's default scan-to-scan check (quatro/enable true, enable_submap_matching false:
 * loop_closure.cpp:85-92, 138-159, 188-192), where each cloud of a pair is one keyframe in its own sensor frame and depends on no pose.
 * qn_kf_quatro_describe: for each listed keyframe, its cloud = qn_kf_assemble({id}, {identity}, leaf) in all 16 bytes of every record (the store's voxel
 *   pipeline as one batch of identity-pose submaps; the assemble, map and batch slots are not touched), and its FPFH rows with ctx's Quatro radii
 *   (fpfh_normal_radius / fpfh_radius): K9 normals, K10 SPFH, K11 FPFH on the grid qn_fpfh builds for that cloud on ctx - the rows equal qn_fpfh's bit for bit.
 *   Both stay resident in a store-owned arena (float4 points; QN_FROW floats per row, original point order); the entry records (leaf, radii, ctx's grid
 *   capacity).  Describing again replaces the entry (an id listed twice: the later one).  status[i] = QN_ERR_EMPTY_CLOUD for a keyframe with no point after
 *   the voxel grid (an entry with no points); the others are still described.  QN_ERR_INVALID_ARG before anything runs: a null pointer, count == 0, a bad id,
 *   leaf <= 0, store and context on different devices.  An allocation failure (QN_ERR_HIP) leaves every earlier entry as it was.  Launches: the voxel
 *   pipeline's, then nine for the grids and K9-K11 of all S keyframes (the keyframe is a grid dimension) - more only when the S grids' scratch (two tables
 *   of max_cells + 1 words per keyframe, ~100 B per point) exceeds 1 GiB.  Host synchronisations: the voxel pipeline's two and one.  Memory per point
 *   resident: 16 B of cloud (x 1.5 growth slack of the voxel output) + 144 B of rows.
 * qn_kf_quatro_cloud: the described cloud of `id` (device pointer, float4, stride 16; NULL and n = 0 for an empty one), valid until `id` is described again
 *   or the store is destroyed.  qn_kf_quatro_features: its n x 33 FPFH rows (one synchronous copy).  Both: QN_ERR_INVALID_ARG for a bad id,
 *   QN_ERR_NOT_READY for a keyframe that was never described.                                                                                       */
int  qn_kf_quatro_describe(qn_kf_store*, qn_ctx*, const int32_t* ids, uint32_t count, double leaf, int* status);
int  qn_kf_quatro_cloud(qn_kf_store*, int32_t id, const float** d_xyz, uint32_t* n);
int  qn_kf_quatro_features(qn_kf_store*, int32_t id, float* fpfh33_out /* n x 33 */);
/* Drift-free coarse-to-fine verification from the described keyframes: pair j = the query's described cloud (source) against cand[j]'s (target), no pose
 * involved.  The Quatro stage of every lane borrows both sides' resident points and rows - no grid, no feature is built - then runs
 * qn_coarse_to_fine_align_batch's own machinery on ctx: matching (K12 / K13), one synchronisation per run of lanes, the host solver, transformPcd on the
 * device, the GICP lanes.  Every record (results, T_total, T_quatro (optional), valid, status) equals qn_coarse_to_fine_align_batch({ctx}) given the two
 * described device clouds bit for bit.  T_total[16 j ..] = T_gicp * T_quatro estimates inv(P_c) P_query; valid[j] = Quatro converged && GICP converged &&
 * score < score_thr (loop_closure.cpp:129, 145-148).  A pair with an empty side: QN_ERR_EMPTY_CLOUD, valid 0, the other pairs still run.
 * QN_ERR_INVALID_ARG before anything runs (store and context unchanged): a null pointer, n_cand == 0, a bad or repeated id, a candidate equal to the query,
 * a keyframe never described, or described with radii other than ctx's current Quatro radii or on a context of another grid capacity (max_points), store
 * and context on different devices.  Memory: the lanes' own, as qn_coarse_to_fine_align_batch; nothing per point beyond it.                        */
int  qn_kf_verify_loop_candidates_c2f(qn_kf_store*, qn_ctx*, int32_t query, const int32_t* cand, uint32_t n_cand, double score_thr,
                                      qn_gicp_result* results, double* T_total /* n_cand x 16 */, double* T_quatro /* n_cand x 16 or NULL */,
                                      int* valid, int* status);
/* The coarse-to-fine check for arbitrary (query, candidate) pairs of many queries: pair j's record (results[j], T_total[16 j ..], T_quatro[16 j ..], valid[j],
 * status[j]) equals qn_kf_verify_loop_candidates_c2f(store, ctx, query[j], &cand[j], 1, ...) bit for bit.  All pairs go through ONE run of the batched
 * coarse-to-fine machinery on ctx, each lane borrowing the described clouds and FPFH rows; the pairs are grouped by query (stable) so that a query's pairs
 * share the source side, and the records come back in caller order.  QN_ERR_INVALID_ARG before anything runs: the single-query call's checks applied
 * to every pair, n_pairs == 0, or a repeated (query, cand) pair.                                                                                     */
int  qn_kf_verify_loop_pairs_c2f(qn_kf_store*, qn_ctx*, const int32_t* query, const int32_t* cand, uint32_t n_pairs, double score_thr,
                                 qn_gicp_result* results, double* T_total /* n_pairs x 16 */, double* T_quatro /* n_pairs x 16 or NULL */,
                                 int* valid, int* status);
/* The debug clouds loopTimerFunc publishes after an attempt (/src, /dst, /coarse_aligned_quatro, /fine_aligned_nano_gicp: fast_lio_sam_qn.cpp:245-248,
 * loop_closure.cpp:207-231) for pair `pair` of the store's latest qn_kf_verify_loop_pairs[_c2f] call, as a device pointer (float4, stride 16) and count:
 *   QN_VERIFY_SRC    the query's segment (GICP path) / the query's described cloud (coarse-to-fine path);
 *   QN_VERIFY_DST    the candidate's segment / the candidate's described cloud;
 *   QN_VERIFY_COARSE coarse-to-fine only: transformPcd(src, T_quatro) in k_transform_cloud_f64's arithmetic (((T0 x + T1 y) + T2 z) + T3 in f64, rounded to f32);
 *   QN_VERIFY_FINAL  the GICP stage's source (src, or COARSE) through the pair's f32 GICP T as align() fills aligned_ (T0 x + (T1 y + (T2 z + T3)) in f32):
 *                    what qn_gicp_transformed_source gives after the equivalent one-pair registration.
 * COARSE and FINAL are computed on demand (one launch, one synchronisation on the store's stream) into a store-owned buffer, one place per pair and cloud.
 * QN_ERR_NOT_READY: no such call yet, its clouds are gone (see below), COARSE on the GICP path, or a pair whose stage did not run (no solved Quatro for
 * COARSE, no registration for FINAL).  QN_ERR_INVALID_ARG: a null pointer, pair >= that call's n_pairs, or a bad `which`.  The pointers stay valid until
 * the next qn_kf_verify_loop_pairs[_c2f] call, the next qn_kf_assemble_batch on the store (any caller: the GICP path's clouds live in its batch slot), a
 * qn_kf_quatro_describe of a keyframe the latest coarse-to-fine call involved, or the store's destruction.  The latest call may also be
 * qn_kf_verify_loop_pairs_submap[_c2f] (below): SRC / DST are then the two resident local submaps, valid until one of them is described again or released;
 * or qn_kf_map_localize[_c2f] (further below): SRC is the scan cloud, DST the map crop, valid until the next crop or localise call.
 * One rule for every verification and localise call above and below: when the batched registration itself returns an error (the call's return value, not a
 * pair's status), the call has written nothing to results / valid / status / T_total / T_quatro and has not replaced the record served here.  */
#define QN_VERIFY_SRC 0
#define QN_VERIFY_DST 1
#define QN_VERIFY_COARSE 2
#define QN_VERIFY_FINAL 3
int  qn_kf_verify_cloud(qn_kf_store*, uint32_t pair, int which, const float** d_xyz /* float4, stride 16 */, uint32_t* n);
/* ---- resident local submaps and the drift-free submap-to-submap check (csrc/qn_kf_submap.inc) ---------------------------------------------------------
 * The reference's third mode (enable_submap_matching true: loop_closure.cpp:70-84, 98-107) registers the submap around the query against the submap around
 * the candidate.  Here the submap around keyframe c lives in c's OWN sensor frame,
 *   voxel_grid( concat_i transformPcd(kf_i, inv(P_c) P_i) ),  i in local_submap_ids(c, r, n) = [i for i in c - r .. c + r if 0 <= i < n],
 * so it depends on the relative poses inside its window only: described from raw odometry it is never invalidated by a pose-graph update; described from
 * corrected poses the caller describes again when it wants to.  NOTE the window rule: it keeps the newest keyframe, unlike loop_submap_ids' `i < n - 1`
 * (qn_kf_verify_loop_candidates, loop_closure.cpp:98-104).  The reference drops the newest keyframe because its only query is keyframes_.back(); with many
 * queries per call there is no such keyframe, and a submap that leaves out its own centre is not what anyone wants.  For c + r < n - 1 both rules give the
 * same list.  An entry is the source when c is a query and the target when c is a candidate; a verified pair (q, c) estimates inv(P_c) P_q.
 * qn_kf_submap_describe: for every listed id c, the cloud = what qn_kf_assemble_batch builds for the list local_submap_ids(c, submap_range, n_poses) with the
 *   poses Q_i = inv(P_c) P_i, in all 16 bytes of every record, Q_i in the arithmetic qn_kf_verify_loop_candidates documents for its candidate segments
 *   (inv(P) = [R^T | -R^T t]; every entry summed over k = 0..3 in order in f64, no fused multiply-add; scancontext.relative_pose) for every i of the window,
 *   i = c included - which is what keeps the entry equal to that call's candidate segment bit for bit wherever the two window rules agree.  All listed windows go
 *   through the store's one voxel-grid pipeline as ONE batch; the assemble, map and batch slots are not touched.  with_features != 0: the FPFH rows of each
 *   cloud with ctx's Quatro radii, equal to qn_fpfh's on that cloud bit for bit, through the launches of qn_kf_quatro_describe (nine for the grids and K9-K11 of
 *   all windows, the window a grid dimension; windows are taken in chunks whose grid scratch - two tables of max_cells + 1 words per window, ~360 B per point -
 *   stays under 1 GiB, one synchronisation per further chunk; the scratch is shared with qn_kf_quatro_describe).  Entries are separate from the scan entries of
 *   qn_kf_quatro_describe: a keyframe may have both.  Each entry records (submap_range, leaf, radii, ctx's grid capacity, whether it has rows).  Describing
 *   again replaces (an id listed twice: the later one).  status[i]: QN_ERR_EMPTY_CLOUD for a window with no point left (an entry with no points),
 *   QN_ERR_CAPACITY for a window whose cloud exceeds ctx's max_points (NO entry, an earlier one of that id is dropped); the others are still described.
 *   QN_ERR_INVALID_ARG before anything runs, store unchanged: a null pointer, count == 0, a bad id, an id >= n_poses, a window member that is no keyframe of the
 *   store (n_poses > the number of keyframes), a non-finite pose, leaf <= 0, store and context on different devices.  An allocation failure (QN_ERR_HIP) leaves
 *   every earlier entry as it was.  Host synchronisations: the voxel pipeline's two and one per chunk.  Memory per point of a window's cloud, resident: 16 B of
 *   cloud (x 1.5 growth slack of the voxel output) + 144 B of rows (with_features); a window holds roughly the points of its 2 r + 1 scans less their overlap.
 * qn_kf_submap_cloud: the entry's cloud (device pointer, float4, stride 16; NULL and n = 0 for an empty one), valid until `id` is described again or released or
 *   the store is destroyed.  qn_kf_submap_features: its n x 33 FPFH rows (one synchronous copy).  Both: QN_ERR_INVALID_ARG for a bad id, QN_ERR_NOT_READY for a
 *   keyframe without an entry (features: or an entry described without rows).
 * qn_kf_submap_release: frees the entries of ids[0 .. count) (never-described ones are skipped), or of every keyframe with ids = NULL and count = 0; device
 *   memory goes back when the last entry of a describe call's block is released.  QN_ERR_INVALID_ARG, nothing released: a bad id, NULL with count > 0 or the reverse. */
int  qn_kf_submap_describe(qn_kf_store*, qn_ctx*, const int32_t* ids, uint32_t count, const double* poses16 /* n_poses x 16 */, uint32_t n_poses,
                           uint32_t submap_range, double leaf, int with_features, int* status);
int  qn_kf_submap_cloud(qn_kf_store*, int32_t id, const float** d_xyz /* float4, stride 16 */, uint32_t* n);
int  qn_kf_submap_features(qn_kf_store*, int32_t id, float* fpfh33_out /* n x 33 */);
int  qn_kf_submap_release(qn_kf_store*, const int32_t* ids, uint32_t count);   /* NULL, 0: all */
/* Submap against submap with Nano-GICP: pair j = query[j]'s entry (source) against cand[j]'s entry (target) through ONE qn_gicp_align_batch_guess on ctx, pair j
 * seeded with Rz(-yaw[j]) built as qn_kf_verify_loop_candidates builds it (yaw NULL: all 0), the pairs grouped by query (stable) so that a query's pairs share
 * the source preparation, the records scattered back to caller order.  Record j (results[j], valid[j], status[j]) equals qn_gicp_align_batch_guess on the two
 * entry clouds with that seed bit for bit.  Rows are not needed.  A pair with an empty side: QN_ERR_EMPTY_CLOUD, valid 0, the other pairs still run.
 * QN_ERR_INVALID_ARG before anything runs (entries, verify record and context unchanged): a null pointer, n_pairs == 0, a bad id, cand[j] == query[j], a
 * repeated (query, cand) pair, a keyframe without an entry, a non-finite yaw, store and context on different devices.  Host synchronisations: the
 * registration's own, whatever n_pairs is.                                                                                                              */
int  qn_kf_verify_loop_pairs_submap(qn_kf_store*, qn_ctx*, const int32_t* query, const int32_t* cand, const double* yaw /* per pair; NULL = 0 */, uint32_t n_pairs,
                                    double score_thr, qn_gicp_result* results, int* valid, int* status);
/* Submap against submap coarse to fine, as qn_kf_verify_loop_pairs_c2f with the lanes borrowing the entries' points and rows: record j equals
 * qn_coarse_to_fine_align_batch({ctx}) on the two entry clouds bit for bit.  QN_ERR_INVALID_ARG before anything runs: that call's checks, with "never
 * described" = no entry, an entry without rows, or rows made with radii or a grid capacity (max_points) other than ctx's; a repeated (query, cand) pair.
 * After either call qn_kf_verify_cloud serves the pair's clouds (SRC / DST = the two entries, COARSE only after this form) until an involved entry is
 * described again or released.                                                                                                                          */
int  qn_kf_verify_loop_pairs_submap_c2f(qn_kf_store*, qn_ctx*, const int32_t* query, const int32_t* cand, uint32_t n_pairs, double score_thr,
                                        qn_gicp_result* results, double* T_total /* n_pairs x 16 */, double* T_quatro /* n_pairs x 16 or NULL */,
                                        int* valid, int* status);
/* ---- the two-way overlap of cloud pairs (csrc/qn_overlap.hip; numpy twin and specification: qn_amd/overlap.py) ----------------------------------------
 * The acceptance rule of every verify call above is the reference's: converged && score < thr, score = the mean squared 1-NN distance of ALL aligned source
 * points, one way.  These calls measure what that number cannot say: how much of each cloud found a partner in the other, and how well those partners fit.
 * For clouds A and B in one frame and a radius r (r2 = float(r * r), the product in f64): d2(a, b) = the f32 squared distance (f32 differences, dx dx + dy dy
 * + dz dz summed left to right, no fused multiply-add).  Per point a of A: nn_d2 = min over the finite b of d2(a, b) if that is <= r2, else +inf; nn_idx =
 * the lowest index b that attains it, else -1.  A non-finite point has +inf / -1 and is nobody's neighbour.  The search is exact (a sorted-key cell index,
 * cell edge >= r; never a dense table, so the clouds' extent costs nothing), the results equal the twin's bit for bit, sum_d2 up to the order of an f64 sum;
 * that order is fixed: a rerun gives the same bits and a pair's record does not depend on which other pairs share the call.
 * qn_overlap_dir (24 bytes) one direction: n points, n_finite finite ones, inliers = points with a partner, sum_d2 = the f64 sum of their nn_d2.
 * qn_overlap (48 bytes): a_to_b (every point of A against B) and b_to_a.  The derived figures are the caller's: overlap = inliers / n_finite, inlier RMSE =
 * sqrt(sum_d2 / inliers), each 0 when its denominator is (qn_amd.overlap.overlap_fraction / inlier_rmse, qn_map::overlapFraction / inlierRmse).
 * qn_kf_overlap_batch: pair j = device clouds d_a[j] (n_a[j] records) and d_b[j], float4 records (stride 16, 16-byte aligned; .w ignored), each inside one
 *   allocation of the store's device (checked), complete when the call is made.  All pairs run in ONE pass on the store's stream, the pair a grid dimension;
 *   two host synchronisations per call whatever n_pairs is.  A pair with an empty side: status[j] = QN_ERR_EMPTY_CLOUD and an all-zero record, the others
 *   still run.  The store's assemble, map and batch slots, its entries and its verify record are not touched (the voxel pipeline's scratch is used).
 * qn_kf_verify_overlap: pair pairs[j] (pairs NULL: pair j, and n_pairs must be that call's n_pairs) of the store's latest qn_kf_verify_loop_pairs[_c2f] /
 *   _submap[_c2f] call with A = its QN_VERIFY_FINAL cloud and B = its QN_VERIFY_DST cloud, as qn_kf_verify_cloud serves them (FINAL is produced on demand in
 *   that call's buffer, without its per-pair synchronisation): the records equal qn_kf_overlap_batch on those two clouds.  The call returns QN_ERR_NOT_READY
 *   when qn_kf_verify_cloud would for every pair (no verify call yet, or its clouds are gone); status[j] = QN_ERR_NOT_READY with a zero record for a pair whose
 *   registration did not run, the others still run.  The verify record and its lifetime rules are unchanged.
 * qn_kf_overlap_points: the per-point results of the store's latest overlap call (either form) for its pair `pair_slot` (the position in that call's list),
 *   dir 0 = A against B (n_a values), 1 = B against A; either output may be NULL, not both.  One synchronous copy.  They live in a buffer of their own until the
 *   next overlap call.  QN_ERR_NOT_READY: no overlap call yet, or a pair that did not run.
 * QN_ERR_INVALID_ARG before anything runs, store unchanged: a null pointer, n_pairs == 0, radius not finite or <= 0, a bad device pointer, a pair index out
 * of range or repeated, a bad dir.  QN_ERR_CAPACITY: more than 32767 pairs, or 2^32 points in one call.                                                   */
typedef struct qn_overlap_dir { uint32_t n, n_finite, inliers, reserved; double sum_d2; } qn_overlap_dir;      /* 24 bytes */
typedef struct qn_overlap { qn_overlap_dir a_to_b, b_to_a; } qn_overlap;                                         /* 48 bytes */
int  qn_kf_overlap_batch(qn_kf_store*, const float* const* d_a, const uint32_t* n_a, const float* const* d_b, const uint32_t* n_b, uint32_t n_pairs,
                         double radius, qn_overlap* out, int* status);
int  qn_kf_verify_overlap(qn_kf_store*, const uint32_t* pairs /* NULL: all */, uint32_t n_pairs, double radius, qn_overlap* out, int* status);
int  qn_kf_overlap_points(qn_kf_store*, uint32_t pair_slot, int dir, float* nn_d2_out, int32_t* nn_idx_out);
/* ---- range images of keyframes and the free-space (see-through) check of loop pairs (csrc/qn_freespace.hip; numpy twin and specification: qn_amd/freespace.py)
 * Score and overlap speak about the points that found a partner.  A point WITHOUT one is either merely out of the other scan's view (occluded, beyond range,
 * outside the field of view: normal in every true revisit) or it contradicts the other scan: under the hypothesised transform it sits where that scan's rays
 * passed on their way to a farther surface.  These calls count the second kind.  Everything happens in a keyframe's SENSOR frame (PosePcd::pcd_), from its raw
 * resident records.  All arithmetic is f64 from the f32 records, no fused multiply-add, no transcendental on the device, the correctly rounded f64 sqrt; every
 * result is an integer or a min / max of f32 values, so images, classes and counts equal the twin's bit for bit and a rerun, or the same pair inside another
 * batch, gives the same record.
 * qn_range_params: n_rows x n_cols pixels (caps: QN_RANGE_MAX_ROWS = 1024, QN_RANGE_MAX_COLS = 8192); el_lo / el_hi [rad] = the lower edge of row 0 and the
 *   upper edge of the last row, -pi/2 < el_lo < el_hi < pi/2; min_range >= 0; window_rows, window_cols (default 1, 1); tol_abs, tol_rel (default 0.3, 0.02).
 *   Host tables from the C library: t[i] = tan(el_lo + i (el_hi - el_lo) / n_rows), i = 0 .. n_rows; (c[j], s[j]) = (cos, sin)(2 pi j / n_cols).
 * Projection of (x, y, z): rho2 = x x + y y, rho = sqrt(rho2), r = sqrt(rho2 + z z); row = #{edges i in 0 .. n_rows : z >= rho t[i]} - 1 (-1 or n_rows: outside
 *   the field of view); column = #{j in 1 .. n_cols - 1 : azimuth >= azimuth of (c[j], s[j])} by Scan Context's half-plane and cross-product test.  Both
 *   counts are defined by the twin's bisection (lo / hi, mid = (lo + hi) >> 1, predicate true -> lo = mid + 1), evaluated at the same indices on both sides.
 *   A point is DROPPED when a coordinate is not finite, r < min_range, or it is outside the field of view.
 * Images of a keyframe: near[row][col] = min, far[row][col] = max over its kept points of (float)r; an empty pixel holds +inf / 0.
 * Check of (q, c, T), T = row-major 4x4 f64 mapping q's sensor frame into c's (results[j].T64 or T_total of the verify calls above): direction 0 (q_in_c) =
 *   every record of q through T, ((T0 x + T1 y) + T2 z) + T3 in f64 and not rounded, against c's images; direction 1 (c_in_q) = every record of c through
 *   inv(T) = [R^T | -R^T t] (the host arithmetic of qn_kf_verify_loop_candidates' relative poses) against q's images.  For a kept point with range r at
 *   (row, col): R_near = min of near and R_far = max of far over the rows row +- window_rows that exist and the columns col +- window_cols, wrapping;
 *   tol = tol_abs + tol_rel r.  One class byte per point: 0 dropped; 1 unobserved (the window holds no return); 2 SEEN THROUGH (r + tol < R_near); 3 occluded
 *   (r > R_far + tol); 4 agree.  qn_freespace_dir (32 bytes): n records, n_finite, in_fov (the kept ones), observed (classes 2 + 3 + 4), seen_through,
 *   occluded, agree, reserved.  qn_freespace (64 bytes): q_in_c, c_in_q.  The derived figure is the caller's: see-through fraction = seen_through / observed,
 *   0 when observed is 0 (qn_amd.freespace.see_through_fraction, qn_map::seeThroughFraction).
 * qn_kf_range_set_params / _get_params: per store (defaults: 64 x 1800, -25 .. 2.2 degrees, min_range 2).  A change of n_rows, n_cols, el_lo, el_hi or
 *   min_range discards every image; the window and the tolerances may change freely.  QN_ERR_INVALID_ARG: a null pointer, a bad range of angles, a zero size
 *   or one above the caps, a non-finite or negative min_range or tolerance, a window that covers a whole dimension (window_rows >= n_rows or
 *   2 window_cols + 1 > n_cols).
 * qn_kf_range_describe: the images of the listed keyframes in ONE pass on the store's stream, the keyframe a grid dimension; they stay resident in a
 *   store-owned block indexed by keyframe id, 8 n_rows n_cols bytes per keyframe (0.92 MB at 64 x 1800).  Describing again replaces.  status[i] =
 *   QN_ERR_EMPTY_CLOUD for a keyframe with no kept point (a valid all-empty image).  One host synchronisation.  QN_ERR_INVALID_ARG: a null pointer,
 *   count == 0, a bad id.
 * qn_kf_range_get: one synchronous copy of the images (either output may be NULL, not both).  QN_ERR_NOT_READY for a keyframe never described.
 * qn_kf_freespace_batch: pair j = (query[j], cand[j], T16[16 j ..]); all pairs and both directions in ONE pass on the store's stream, (pair, direction) a grid
 *   dimension, the counts reduced in a fixed order through per-block slots; one host synchronisation per call whatever n_pairs is.  Pairs may repeat.
 *   status[j] = QN_ERR_EMPTY_CLOUD when one of the keyframes has no record at all (the record is still filled).  QN_ERR_INVALID_ARG before anything runs:
 *   a null pointer, n_pairs == 0, a bad id, query[j] == cand[j], a non-finite T, a keyframe without images.  QN_ERR_CAPACITY: more than 32767 pairs, or 2^32
 *   records in one call.  The store's slots, entries, images and verify record are not touched.
 * qn_kf_freespace_points: the class bytes of the latest qn_kf_freespace_batch for its pair `pair_slot`, dir 0 = q's records (n of q_in_c), 1 = c's.  They live
 *   in a buffer of their own until the next successful call.  QN_ERR_NOT_READY before any call; QN_ERR_INVALID_ARG: a null pointer, a bad slot or dir.
 * A refused call (INVALID_ARG, NOT_READY, CAPACITY) leaves the images and the per-point classes as they were.                                              */
#define QN_RANGE_MAX_ROWS 1024
#define QN_RANGE_MAX_COLS 8192
typedef struct qn_range_params { uint32_t n_rows, n_cols; double el_lo, el_hi, min_range; uint32_t window_rows, window_cols; double tol_abs, tol_rel; } qn_range_params;  /* 56 bytes */
typedef struct qn_freespace_dir { uint32_t n, n_finite, in_fov, observed, seen_through, occluded, agree, reserved; } qn_freespace_dir;      /* 32 bytes */
typedef struct qn_freespace { qn_freespace_dir q_in_c, c_in_q; } qn_freespace;                                                              /* 64 bytes */
int  qn_kf_range_set_params(qn_kf_store*, const qn_range_params*);
int  qn_kf_range_get_params(qn_kf_store*, qn_range_params*);
int  qn_kf_range_describe(qn_kf_store*, const int32_t* ids, uint32_t count, int* status);
int  qn_kf_range_get(qn_kf_store*, int32_t id, float* near_out /* n_rows x n_cols */, float* far_out);
int  qn_kf_freespace_batch(qn_kf_store*, const int32_t* query, const int32_t* cand, const double* T16 /* n_pairs x 16 */, uint32_t n_pairs,
                           qn_freespace* out, int* status);
int  qn_kf_freespace_points(qn_kf_store*, uint32_t pair_slot, int dir, uint8_t* class_out /* one byte per record */);
/* the corrected global map = the three loops of FastLioSamQn that rebuild it from every keyframe with its corrected pose
 * (fast_lio_sam_qn.cpp:302-316 visTimerFunc, :398-411 saveFlagCallback, :435-448 the destructor's result.pcd): transformPcd of each
 * listed keyframe, concatenation in `ids` order (ids may repeat), voxelizePcd at save_voxel_resolution (pcl::VoxelGrid,
 * include/utilities.hpp:38-51) averaging xyz AND intensity.  PointXYZI keyframes come in through qn_kf_add_xyzi (stride 32, intensity
 * at offset 16); keyframes added by qn_kf_add count as intensity 0.  The map has its own slot: building it never touches the
 * qn_kf_assemble slots and assembling never touches it.  When PCL's overflow guard trips (qn_kf_last_error says so) the map is the
 * unfiltered concatenation, non-finite points included, as VoxelGrid::applyFilter's `output = *input_` (qn_kf_assemble drops them first).
 * qn_kf_download_map writes only the 12 xyz bytes and the 4 intensity bytes of each record; the rest of each record is left as it was. */
int  qn_kf_add_xyzi(qn_kf_store*, const float* pts, uint32_t n, uint32_t stride_bytes, uint32_t intensity_offset_bytes, int32_t* id_out);
int  qn_kf_build_map(qn_kf_store*, const int32_t* ids, const double* poses16, uint32_t count, double leaf,
                     const float** d_xyzi_out /* float4: x y z intensity */, uint32_t* n_out);
int  qn_kf_download_map(qn_kf_store*, void* out, uint32_t stride_bytes, uint32_t intensity_offset_bytes);
/* ---- the static map: the corrected map without the records other keyframes saw through (csrc/qn_staticmap.hip; numpy twin and specification:
 * qn_amd/staticmap.py)
 * Whatever moved while the sensor drove past - cars, people - stays in qn_kf_build_map's map as a ghost trail.  The evidence to remove it is resident: a
 * record of one keyframe is transient if, carried with the corrected poses into a neighbouring keyframe's SENSOR frame, it lies where that keyframe's rays
 * passed on their way to a farther surface - class 2, SEEN THROUGH, of the free-space check above, with the same projection, images, window and tolerances
 * (the store's qn_range_params).  These calls take that vote many to many, drop the records voted out and build the map from the rest.  Votes are integers
 * and the map is the one voxel-grid pipeline's, so every byte equals the twin's bit for bit and a rerun gives the same bytes.
 * List: ids[0 .. count) with poses16 (row-major 4x4 f64, sensor -> world), the list qn_kf_build_map takes; ids may repeat; a list position is an ENTRY.
 * Witnesses of entry e: wit[wit_off[e] .. wit_off[e + 1]), entry positions, in the caller's order (qn_map::staticMapWitnesses / staticmap.witnesses make the
 *   default list: the nearest entries of another keyframe).  A witness never has the entry's own keyframe id; at most 255 per entry.
 * Votes of record p of entry e, over its witnesses w in list order: M = inv(P_w) P_e with inv(P) = [R^T | -R^T t] (the host arithmetic of
 *   qn_kf_verify_loop_candidates' relative poses), the point ((M0 x + M1 y) + M2 z) + M3 in f64 and not rounded, its class against the images of keyframe
 *   ids[w].  seen_through[p] = the witnesses giving class 2, agree[p] = those giving class 4, both u8 (exact under the 255 cap).
 * Rule, qn_static_params (8 bytes): min_see_through (>= 1, default 2), agree_weight (default 1).  Record p is REMOVED iff seen_through >= min_see_through and
 *   seen_through > agree_weight * agree, in exact integers.  A record with a non-finite coordinate gets no vote and is never removed.
 * qn_kf_static_classify: ONE vote pass on the store's stream whatever count is (the entry a grid dimension, the witness loop inside the thread: a record is read
 *   once and its three bytes written once), the kept records of every entry compacted in order into a store-owned buffer; one host synchronisation.
 *   removed_per_entry[e] = its removed records; status[e] = QN_ERR_EMPTY_CLOUD for an entry without records.  The store keeps the list, the poses and per record
 *   seen_through, agree and the removed flag until the next successful call.  Refused before anything runs, the state of the previous call left intact:
 *   QN_ERR_INVALID_ARG: a null pointer (wit may be NULL when no entry has a witness), count == 0, a bad id, a non-finite pose, a witness whose keyframe has no
 *   images (qn_kf_range_describe), a witness position >= count, a witness with the entry's own id, a non-monotone wit_off, min_see_through == 0;
 *   QN_ERR_CAPACITY: more than 255 witnesses for an entry, or 2^32 records in the call.
 * qn_kf_static_points: the bytes of entry `entry` of the latest classify, one per record (any output may be NULL, not all).  QN_ERR_NOT_READY before a
 *   classify; QN_ERR_INVALID_ARG: a null store, no output, a bad entry.
 * qn_kf_build_map_static: the static map of the latest classify = by definition qn_kf_build_map of the same list, poses and leaf over keyframes from which the
 *   removed records have been deleted (order and intensity kept, an entry with nothing left contributes nothing; intensity averaging, point order and the
 *   overflow-guard pass-through are qn_kf_build_map's) - into the store's map slot, so qn_kf_download_map serves it.  May be called again with another leaf.
 *   QN_ERR_NOT_READY without a classify, or when a listed keyframe's records are no longer the ones the votes were taken on.  A refused call leaves the map
 *   slot as it was.                                                                                                                                          */
typedef struct qn_static_params { uint32_t min_see_through, agree_weight; } qn_static_params;      /* 8 bytes */
void qn_static_default_params(qn_static_params* p);
int  qn_kf_static_classify(qn_kf_store*, const int32_t* ids, const double* poses16, uint32_t count, const uint32_t* wit_off /* count + 1 */, const uint32_t* wit,
                           const qn_static_params* params, uint32_t* removed_per_entry, int* status);
int  qn_kf_static_points(qn_kf_store*, uint32_t entry, uint8_t* seen_through_out, uint8_t* agree_out, uint8_t* removed_out);
int  qn_kf_build_map_static(qn_kf_store*, double leaf, const float** d_xyzi_out /* float4: x y z intensity */, uint32_t* n_out);
/* ---- normals and curvature of the map (csrc/qn_mapnormals.hip; numpy twin and specification: qn_amd/mapnormals.py)
 * A surface normal and PCL's surface variation for every point of the store's map slot as the latest qn_kf_build_map / qn_kf_build_map_static left it - a
 * passed-through map with its non-finite records included - from the point's fixed-radius neighbourhood, on the GPU.
 * qn_normal_params (16 bytes): radius (finite, > 0, default 0.6), min_neighbors (>= 3, default 5), reserved (0).
 * Neighbours of point p: the finite map points q, p included, with the f32 squared distance (the overlap measure's arithmetic) <= float(radius * radius).
 * Moments: the offsets q - p (f32) times 2^e, e the largest integer with radius * 2^e <= 2^20, rounded half to even to integers di; count, s1[3] = sum di and
 *   s2[6] = sum di dj (xx xy xz yy yz zz) are exact integers (u32, int64), equal to the twin's bit for bit whatever order the neighbours are met in.
 * Covariance (f64, no fused multiply-add): m = s1 / count, C_ij = s2_ij / count - m_i m_j.  normal = the unit eigenvector of the smallest eigenvalue l0 of C,
 *   curvature = l0 / (l0 + l1 + l2) with l0 clamped at 0; both f32.  All four are NaN when count < min_neighbors or the trace of C is <= 0.
 * Orientation: view_idx = the viewpoint (viewpoints_xyz, n_view x 3 f64, the corrected keyframe positions as a rule) nearest to p in f64, the lowest index on
 *   ties, -1 when n_view == 0 or p is non-finite; the normal is turned to face it (negated when n . (v - p) < 0).  With n_view == 0 the normal's component of
 *   largest magnitude is made positive (the lowest axis on a tie).
 * qn_kf_map_normals: one pass on the store's stream over the map indexed by cells of about the radius; two host synchronisations.  *d_normals_out = n float4
 *   records (nx ny nz curvature) at the map's own indices, in store-owned memory good until the next successful call; the results stay resident for the
 *   two downloads.  QN_ERR_NOT_READY without a map.  QN_ERR_INVALID_ARG: a null pointer, a non-finite or non-positive radius, min_neighbors < 3,
 *   reserved != 0, a non-finite viewpoint, n_view > 0 with a null array.  QN_ERR_CAPACITY: 2^21 or more map points in one 3 x 3 x 3 block of cells (the int64
 *   moments would no longer be provably exact), or a map whose extent overflows f32.  A refused call leaves the previous results intact.
 * qn_kf_download_map_normals: normals4_out (n x 4 floats), count_out (n), view_idx_out (n); any may be NULL, not all.  qn_kf_map_moments: s1_out (n x 3),
 *   s2_out (n x 6), for tests; either may be NULL, not both.  QN_ERR_NOT_READY before a successful qn_kf_map_normals and after a later map build replaced
 *   the slot the results were computed from.                                                                                                               */
typedef struct qn_normal_params { double radius; uint32_t min_neighbors, reserved; } qn_normal_params;      /* 16 bytes */
void qn_normal_default_params(qn_normal_params* p);
int  qn_kf_map_normals(qn_kf_store*, const qn_normal_params* params, const double* viewpoints_xyz, uint32_t n_view,
                       const float** d_normals_out /* float4: nx ny nz curvature */, uint32_t* n_out);
int  qn_kf_download_map_normals(qn_kf_store*, float* normals4_out, uint32_t* count_out, int32_t* view_idx_out);
int  qn_kf_map_moments(qn_kf_store*, int64_t* s1_out /* n x 3 */, int64_t* s2_out /* n x 6 */);
/* ---- isolated noise points of the map (csrc/qn_mapoutliers.hip; numpy twin and specification: qn_amd/mapoutliers.py)
 * Stray returns survive the voxel grid and the static vote: mixed pixels off object edges, dust, single hits in mid-air.  These calls find and remove them in
 * the store's map slot as the latest build left it - a passed-through map with its non-finite records included - by PCL's RadiusOutlierRemoval and
 * StatisticalOutlierRemoval rules over one exact bounded-radius k-nearest selection per map point, on the GPU.
 * qn_outlier_params (24 bytes): radius (finite, > 0, default 1.0), std_mul (finite, >= 0, default 2.0), k (1 .. QN_OUTLIER_MAX_K = 32, default 8),
 *   reserved (0).  The defaults are interface choices, not measurements.
 * Neighbours of a finite point p: the finite map points q at ANOTHER INDEX than p with the f32 squared distance d2 (the overlap measure's arithmetic: f32
 *   differences, dx dx + dy dy + dz dz left to right, no fused multiply-add) <= float(radius * radius); a duplicate of p at another index counts.  count =
 *   their number (u32).
 * Sparse: count < k.  The point is an outlier outright (the radius rule with min_neighbors = k), its mean_q is 0xffffffff, it takes no part in the statistics.
 * Dense: count >= k.  The k smallest d2 as a multiset, ascending; s = their correctly rounded f64 roots (of the f32 values widened to f64) summed in that
 *   order in f64; mean_q = (uint32) rint(s / k * 2^e), half to even, e the largest integer with radius * 2^e <= 2^16 (within [-126, 127]); mean_q <= 2^16 + 1.
 * Statistics over the dense points, exact integers: dense = N, sum_q, sum_q2 = the sums of mean_q and of its square (u64).
 * Threshold (host, f64, no contraction): mean = sum_q / N; var = N > 1 ? (sum_q2 - sum_q * sum_q / N) / (N - 1) : 0, clamped at 0; thr_q = mean + std_mul *
 *   sqrt(var); all 0 when N == 0.
 * Removed: a finite point that is sparse or has (double)mean_q > thr_q.  A non-finite record has count 0 and mean_q 0xffffffff and is never removed.
 * count, mean_q, the removed flags and the statistics are integers (the f64 values follow from them), equal to the twin's bit for bit whatever order the
 *   neighbours are met in; a rerun gives the same bytes.
 * qn_outlier_stats (64 bytes): n, n_finite, dense, sparse, removed, quant_exp (e); sum_q, sum_q2; mean_q, std_q, thr_q in units of 2^-e m.
 * qn_kf_map_outliers: classifies the map slot as it stands; the slot itself is not touched.  The per-point results stay resident for the slot's generation
 *   (any later map build, successful or not, ends it).  At most three host synchronisations.  QN_ERR_NOT_READY without a map.  QN_ERR_INVALID_ARG: a null
 *   pointer, a non-finite or non-positive radius, a non-finite or negative std_mul, k outside 1 .. 32, reserved != 0.  QN_ERR_CAPACITY: 2^30 or more map
 *   points (sum_q2 would no longer be provably exact), or a map whose extent overflows f32.  A refused call leaves the previous classification intact.
 * qn_kf_map_outlier_points: count_out, mean_q_out, removed_out (one byte per point), each at the map's own indices; any may be NULL, not all.
 *   QN_ERR_NOT_READY before a successful qn_kf_map_outliers and once the slot's generation has moved on.
 * qn_kf_map_remove_outliers: applies the live classification: the kept records, in order and all 16 bytes each, become the map slot (*d_xyzi_out, *n_out;
 *   NULL and 0 when nothing is left).  The slot's generation advances, so the classification and any map normals go stale; qn_kf_download_map and
 *   qn_kf_map_normals serve the filtered map.  QN_ERR_NOT_READY without a live classification, and the slot is then unchanged.                              */
#define QN_OUTLIER_MAX_K 32
typedef struct qn_outlier_params { double radius; double std_mul; uint32_t k; uint32_t reserved; } qn_outlier_params;      /* 24 bytes */
typedef struct qn_outlier_stats {
  uint32_t n, n_finite, dense, sparse, removed; int32_t quant_exp;
  uint64_t sum_q, sum_q2;
  double mean_q, std_q, thr_q;
} qn_outlier_stats;                                                                                                          /* 64 bytes */
void qn_outlier_default_params(qn_outlier_params* p);
int  qn_kf_map_outliers(qn_kf_store*, const qn_outlier_params* params, qn_outlier_stats* stats_out);
int  qn_kf_map_outlier_points(qn_kf_store*, uint32_t* count_out, uint32_t* mean_q_out, uint8_t* removed_out);
int  qn_kf_map_remove_outliers(qn_kf_store*, const float** d_xyzi_out /* float4: x y z intensity */, uint32_t* n_out);
/* ---- the map's ground and its occupancy grid (csrc/qn_mapground.hip; numpy twin and specification: qn_amd/mapground.py)
 * What a user does with the corrected map next: split the ground from what stands on it, and flatten the result into the 2-D occupancy grid a planner or
 * map_server loads (the "pcd2pgm" step over the saved map).  These calls do it on the GPU for the store's map slot as the latest build or filter left it.
 * Heights are quantised once; everything afterwards is an integer, independent of any order, and equal to the twin's bit for bit.
 * qn_ground_params (40 bytes): cell (grid edge in m; finite, > 0; default 0.5), max_slope (rise over run the ground may have; finite, > 0; default 0.3),
 *   ground_tol (finite, >= 0; default 0.2), clearance (finite, > ground_tol; default 2.0), min_points (>= 1; default 1), reserved (0).  The defaults are
 *   interface choices, not measurements.
 * Units: e = the largest integer with cell * 2^e <= 2^10 (kept within [-126, 127]).  zq = (int32) rint(z * 2^e), half to even, the f32 z widened to f64 first
 *   (the product is exact).  Host f64, no contraction: step_s = max(1, rint(max_slope * cell * 2^e)), step_d = (step_s * 181) >> 7 (a diagonal step, 181 / 128
 *   being sqrt 2 rounded down), tol_q = rint(ground_tol * 2^e), clear_q = rint(clearance * 2^e); QN_ERR_INVALID_ARG when one of them is >= 2^30.
 *   QN_ERR_CAPACITY when a finite point has |zq| >= 2^30.
 * Columns: a finite point is one whose x, y and z are all finite.  Its column, in x and y only, is the voxel grid's arithmetic c = (int)(floorf(x * inv) -
 *   (float)minb) with inv = (float)(1 / cell); minb and the grid W x H (width along x, height along y) come from the finite points' extremes.
 *   QN_ERR_CAPACITY, before any grid-sized allocation, when floorf(x * inv) leaves the int32 range, when W or H exceeds 2^24 (below that the f32 subtraction
 *   is exact) or when W * H > QN_GROUND_MAX_CELLS = 2^26.  Without a finite point the grid is 0 x 0.
 * Seeds: cnt(c) = the finite points of column c; seed(c) = the smallest zq of the column when cnt(c) >= min_points, else INF = INT32_MAX.
 * Ground envelope g: the greatest function on the dense grid with g(c) <= seed(c) and g(c) <= g(n) + step(n, c) for the eight neighbours n (step_s for a
 *   straight one, step_d for a diagonal one; the sum saturates at INF).  It is unique; because step_s <= step_d <= 2 step_s it is g(c) = min over the seeded s of seed(s) + step_d *
 *   min(dx, dy) + step_s * (max(dx, dy) - min(dx, dy)).  Empty columns get a value too; without a seeded column every g is INF.  No relaxation schedule
 *   changes it.
 * Classes, one byte per point, from h = zq - g(column): QN_GROUND_NONE 0 (a non-finite record, or g = INF), QN_GROUND_GROUND 1 (-tol_q <= h <= tol_q),
 *   QN_GROUND_OBSTACLE 2 (tol_q < h <= clear_q), QN_GROUND_OVERHEAD 3 (h > clear_q), QN_GROUND_BELOW 4 (h < -tol_q: only possible in an unseeded column).
 *   height_q = max(h, INT32_MIN + 1) (int32; h < 2^31 always), INT32_MIN for class 0.
 * Occupancy, one byte per column: 0 unknown (no finite point), 2 occupied (at least one OBSTACLE point), 1 free (everything else).  OVERHEAD points do not
 *   occupy: a bridge or a canopy stays drivable.
 * qn_ground_stats (80 bytes): n, n_finite; n_none, n_ground, n_obstacle, n_overhead, n_below (the five class counts); width, height; seeded, occupied, free,
 *   unknown (columns); quant_exp (e), step_s, step_d, tol_q, clear_q; rounds = the relaxation launches the GPU ran - it depends on the schedule and is the only
 *   field the twin does not share; reserved (0).
 * qn_ground_grid (40 bytes): origin_x, origin_y (minb * cell, f64: the corner of column (0, 0)), cell, width, height, quant_exp, reserved (0).
 * qn_kf_map_ground: classifies the map slot as it stands; the slot itself is not touched.  The results stay resident for the slot's generation (any later map
 *   build or filter, successful or not, ends it).  Host synchronisations: 2 + ceil(rounds / 8) - the extent, the envelope's flags every
 *   QN_GROUND_ROUNDS_PER_CHECK = 8 launches, the counts.  The relaxation stops with QN_ERR_INTERNAL after max(W, H) + 2 rounds (a change crosses at most
 *   max(W, H) cells; never seen).  QN_ERR_NOT_READY without a map.  QN_ERR_INVALID_ARG: a null pointer, a parameter outside the ranges above, reserved != 0,
 *   a unit >= 2^30.  QN_ERR_CAPACITY as above.  A refused call leaves the previous results intact.
 * qn_kf_map_ground_points: class_out (one byte per point) and height_q_out at the map's own indices; either may be NULL, not both.  QN_ERR_NOT_READY before a
 *   successful qn_kf_map_ground and once the slot's generation has moved on.
 * qn_kf_map_ground_grid: *info_out and the two arrays, row-major with y the slow axis (column (ix, iy) at iy * width + ix); the arrays may be NULL to fetch
 *   the dimensions first.  ground_q is g in units of 2^-e m.  QN_ERR_NOT_READY as above.
 * qn_kf_map_keep_classes: the records whose class bit (1 << class) is set in class_mask become the map slot, in order and all 16 bytes each (*d_xyzi_out,
 *   *n_out; NULL and 0 when nothing is left).  The generation advances, so normals, outlier and ground results go stale; qn_kf_download_map,
 *   qn_kf_map_normals and qn_kf_map_outliers then serve the kept map.  QN_ERR_NOT_READY without a live classification, and the slot is then unchanged.
 *   QN_ERR_INVALID_ARG: class_mask 0 or with a bit >= 5 set, a null pointer.                                                                          */
#define QN_GROUND_MAX_CELLS (1u << 26)
#define QN_GROUND_ROUNDS_PER_CHECK 8
#define QN_GROUND_NONE 0
#define QN_GROUND_GROUND 1
#define QN_GROUND_OBSTACLE 2
#define QN_GROUND_OVERHEAD 3
#define QN_GROUND_BELOW 4
typedef struct qn_ground_params { double cell, max_slope, ground_tol, clearance; uint32_t min_points; uint32_t reserved; } qn_ground_params;   /* 40 bytes */
typedef struct qn_ground_stats {
  uint32_t n, n_finite;
  uint32_t n_none, n_ground, n_obstacle, n_overhead, n_below;
  uint32_t width, height;
  uint32_t seeded, occupied, free, unknown;
  int32_t quant_exp, step_s, step_d, tol_q, clear_q;
  uint32_t rounds, reserved;
} qn_ground_stats;                                                                                                           /* 80 bytes */
typedef struct qn_ground_grid { double origin_x, origin_y, cell; uint32_t width, height; int32_t quant_exp; uint32_t reserved; } qn_ground_grid;   /* 40 bytes */
void qn_ground_default_params(qn_ground_params* p);
int  qn_kf_map_ground(qn_kf_store*, const qn_ground_params* params, qn_ground_stats* stats_out);
int  qn_kf_map_ground_points(qn_kf_store*, uint8_t* class_out, int32_t* height_q_out);
int  qn_kf_map_ground_grid(qn_kf_store*, qn_ground_grid* info_out, int32_t* ground_q_out, uint8_t* occupancy_out);
int  qn_kf_map_keep_classes(qn_kf_store*, uint32_t class_mask, const float** d_xyzi_out /* float4: x y z intensity */, uint32_t* n_out);
/* ---- a 3-D occupancy map by ray carving (csrc/qn_mapoccupancy.inc, part of csrc/qn_staticmap.hip; numpy twin and specification: qn_amd/mapoccupancy.py)
 * The ground grid above calls a column free when it holds points and no obstacle: a statement about returns, not about space.  Every keyframe record is also a
 * ray from that keyframe's corrected sensor position to a world point; these calls walk the rays of a list of keyframes through a voxel grid on the GPU and
 * leave an OctoMap-style volume in which every voxel is occupied, observed free or never observed.  Both ray ends are quantised once; everything afterwards is
 * an integer, independent of any order, and equal to the twin's bit for bit.
 * Input: the list qn_kf_build_map takes - ids[0 .. count) and poses16 (row-major 4x4 f64, sensor -> world).  Ids may repeat; a list position is an entry.
 * qn_occupancy_params (48 bytes): voxel (edge in m; finite, > 0; default 0.3), min_range (finite, >= 0; default 0.5), max_range (finite, > min_range; default
 *   60), shell (default 1), min_hits (>= 1; default 1), hit_weight (>= 1; default 2), reserved[3] (0).  The defaults are interface choices, not measurements.
 * Accepted records: record p = (x, y, z) of entry e, f32, sensor frame, is skipped and counted n_nonfinite when a coordinate is not finite.  Otherwise
 *   d2 = x x + y y + z z in f32, left to right, no fused multiply-add (the overlap measure's arithmetic); the record is skipped and counted n_near when
 *   d2 < float(min_range * min_range), n_far when d2 > float(max_range * max_range) (the squares in f64, rounded once).  Everything else is a ray.  A far
 *   record is dropped whole instead of having its ray truncated: truncation needs a square root on the path.
 * Ray ends, f64, no contraction: origin O = (P3, P7, P11); end W = ((P0 x + P1 y) + P2 z) + P3 per row (the static vote's arithmetic), the f32 coordinates
 *   widened first; inv = 1.0 / voxel, computed on the host.  Fixed point with S = 10 fractional bits: A_k = (int64) rint((O_k * inv) * 1024.0), B_k likewise
 *   from W, rounded half to even.  QN_ERR_CAPACITY when a ray has |O_k * inv| or |W_k * inv| >= 2^20.
 * Walk, integers only: c = A >> S (an arithmetic shift, so a floor), cend = B >> S.  Per axis k: s_k = sign(B_k - A_k), D_k = |B_k - A_k|, rem_k =
 *   |cend_k - c_k|, r_k = ((c_k + 1) << S) - A_k when s_k > 0, else A_k - (c_k << S) (0 for an origin on a face heading down: it steps at once).
 *   n = rem_x + rem_y + rem_z times: among the axes with rem_k > 0 the one with the smallest r_k / D_k, compared as r_a D_b < r_b D_a in 64 bits; on a tie
 *   the lowest axis; then c_k += s_k, r_k += 1 << S, rem_k -= 1.  The visited voxels are v_0 = c(A), ..., v_n = c(B).
 * Counts, u32 per voxel: hits[v_n] += 1; misses[v_i] += 1 for 0 <= i < n - shell (none when n <= shell).  A ray never carves its own end voxel; shell keeps
 *   the last voxels before a surface out of the carving, so grazing neighbours do not erode it.
 * Grid: minc, maxc per axis from c(A) and c(B) of all rays (the walk is monotone per axis, so it stays inside).  W x H x D, x fastest, z slowest: voxel
 *   (ix, iy, iz) at linear index (iz H + iy) W + ix.  QN_ERR_CAPACITY, before any grid-sized allocation, when a dimension exceeds 2^15 or W H D >
 *   QN_OCC_MAX_CELLS = 2^27.  Without a ray the grid is 0 x 0 x 0.
 * Classes, one byte per voxel: QN_OCC_UNKNOWN 0 (hits = misses = 0), QN_OCC_OCCUPIED 2 (hits >= min_hits and (u64) hits * hit_weight >= misses),
 *   QN_OCC_FREE 1 (everything else).
 * qn_occupancy_stats (64 bytes): n_records, n_rays, n_nonfinite, n_near, n_far; width, height, depth; occupied, free, unknown (voxels); reserved (0);
 *   total_hits, total_misses (u64).  Every field is an integer and is shared with the twin.
 * qn_occupancy_grid (56 bytes): origin[3] (minc * voxel, f64: the corner of voxel (0, 0, 0)), voxel, width, height, depth, minc[3].
 * qn_kf_map_occupancy: QN_ERR_INVALID_ARG, before anything runs and with the previous result intact: a null pointer, count == 0, an id that names no
 *   keyframe, a pose that is not finite, a parameter outside the ranges above, reserved != 0.  QN_ERR_CAPACITY as above (the previous result intact), and at
 *   2^32 records.  The results stay resident until the next successful call; they do not depend on the map slot, and no map build ends them.  Two host
 *   synchronisations: the extent, the counts.
 * qn_kf_map_occupancy_grid: *info_out and the three arrays of W H D elements; the arrays may be NULL to fetch the dimensions first.  QN_ERR_NOT_READY before
 *   a successful qn_kf_map_occupancy.
 * qn_kf_map_occupancy_list: the voxels whose class bit (1 << class) is set in class_mask, in ascending linear index (a stable device compaction): *n_out
 *   their number, ijk_out three grid indices each, hits_out, misses_out; the arrays may be NULL to fetch *n_out first.  QN_ERR_INVALID_ARG: mask 0 or a bit
 *   >= 3.  QN_ERR_NOT_READY as above.
 * qn_kf_map_occupancy_slice: occupancy_out (W x H, row-major with y the slow axis) - per column over the layers iz_lo .. iz_hi inclusive, clipped to the grid:
 *   2 if any voxel is OCCUPIED, else 1 if any is FREE, else 0: the values of qn_kf_map_ground_grid's occupancy, where free here means that a ray passed.
 *   QN_ERR_INVALID_ARG when iz_lo > iz_hi.  QN_ERR_NOT_READY as above.                                                                                  */
#define QN_OCC_MAX_CELLS (1u << 27)
#define QN_OCC_UNKNOWN 0
#define QN_OCC_FREE 1
#define QN_OCC_OCCUPIED 2
typedef struct qn_occupancy_params { double voxel, min_range, max_range; uint32_t shell, min_hits, hit_weight; uint32_t reserved[3]; } qn_occupancy_params;   /* 48 bytes */
typedef struct qn_occupancy_stats {
  uint32_t n_records, n_rays, n_nonfinite, n_near, n_far;
  uint32_t width, height, depth;
  uint32_t occupied, free, unknown, reserved;
  uint64_t total_hits, total_misses;
} qn_occupancy_stats;                                                                                                        /* 64 bytes */
typedef struct qn_occupancy_grid { double origin[3], voxel; uint32_t width, height, depth; int32_t minc[3]; } qn_occupancy_grid;   /* 56 bytes */
void qn_occupancy_default_params(qn_occupancy_params* p);
int  qn_kf_map_occupancy(qn_kf_store*, const int32_t* ids, const double* poses16, uint32_t count, const qn_occupancy_params* params,
                         qn_occupancy_stats* stats_out);
int  qn_kf_map_occupancy_grid(qn_kf_store*, qn_occupancy_grid* info_out, uint32_t* hits_out, uint32_t* misses_out, uint8_t* class_out);
int  qn_kf_map_occupancy_list(qn_kf_store*, uint32_t class_mask, uint32_t* n_out, int32_t* ijk_out, uint32_t* hits_out, uint32_t* misses_out);
int  qn_kf_map_occupancy_slice(qn_kf_store*, int32_t iz_lo, int32_t iz_hi, uint8_t* occupancy_out /* W x H, y slow */);
/* ---- the occupancy map updated in place (csrc/qn_mapoccupancy_update.inc, part of csrc/qn_staticmap.hip; numpy twin and specification: update() of
 * qn_amd/mapoccupancy.py)
 * qn_kf_map_occupancy starts from nothing.  A robot that asks for the volume at every tick has added one keyframe since the last call, or a loop closure has
 * moved some poses; the counts are u32 sums behind one quantisation, so a contribution is taken out again by walking the same rays with -1 (mod 2^32), and the
 * result is the same bytes whatever the order.
 * qn_kf_map_occupancy_update brings the resident volume to this list.  The list, the parameters, the checks and the refusals are those of
 *   qn_kf_map_occupancy.  Afterwards the live result equals, byte for byte, what qn_kf_map_occupancy leaves for the same list and parameters: *stats_out, the
 *   grid info, every voxel's hits, misses and class, so every list and slice.  The grid is the tight box of the list's ray ends again: it also shrinks.  All
 *   getters and qn_kf_map_distance / _route / _frontiers / _view_gain serve the result as they serve a rebuilt one, and a successful update ends the live results
 *   of those four exactly as a successful qn_kf_map_occupancy does.
 * Ledger: for the result it holds the store keeps one row per entry - the id, the 12 pose doubles the carving reads, the five record counts, the box of the
 *   entry's ray ends in voxel coordinates (none without a ray).  A new list is matched against it as a multiset: an entry is kept when its id and the bytes
 *   (memcmp) of its 12 doubles equal an unmatched row; the order of the list does not matter and repeated ids match as often as they occur.  A pose that
 *   differs only in the sign of a zero counts as changed and is walked again.  Unmatched rows are removed - walked with -1 from the ledger's pose -, unmatched
 *   entries are added; the caller never states what to remove, so no count can be driven below zero from outside.  Only a successful update leaves a ledger; a
 *   successful qn_kf_map_occupancy drops it, and the next update then starts from an empty volume (rebuilt = 1), as it does when voxel, min_range, max_range or
 *   shell differ from the ledger's.  When only min_hits or hit_weight differ the counts are kept and the classes formed again.
 * Sequence: the diff on the host; the extent of the added entries only (their counts and boxes; one host read, none when nothing is added); the new box, the
 *   union of the rows' boxes, where QN_ERR_CAPACITY (a ray end at 2^20 voxels, 2^15 a side, 2^27 voxels, 2^32 records) is decided with the previous result
 *   intact, its ledger and the fields over it too; the removed rows' rays subtracted in the old grid; the counts moved into the new box when it differs (a
 *   second pair of count buffers, kept for the next move); the added entries' rays; the classes of the whole grid and the sums (the second and last host read).
 *   A HIP error after the first subtraction leaves no live result and no ledger.
 * qn_occupancy_update (64 bytes): entries_kept, entries_added, entries_removed; rebuilt (1: no ledger to start from, or other ray parameters: every entry was
 *   added to an empty volume); regridded (1: the box changed and the counts were moved); records_walked (the records of the added and the removed entries: what
 *   the walks read); dirty_lo[3], dirty_hi[3] (the union of the boxes of the added and removed rows as indices of the NEW grid, clipped to it: every voxel of
 *   the new grid whose hits or misses changed lies inside; lo = 0 > hi = -1 on every axis when it is empty); rays_added, rays_removed (u64).  Nothing in the
 *   library consumes the dirty box yet.
 * Cost on one MI355X (tools/gpu_map_occupancy_update_time.py, medians of 5; profiles/EXPERIMENTS.md), 500 keyframes x 60 000 records, 1 554 x 346 x 20
 *   voxels, beside 203.6 ms for qn_kf_map_occupancy and 1.07 ms for qn_kf_map_frontiers in the same run: one keyframe added 1.41 ms, nothing changed 0.19 ms,
 *   the last 50 poses moved 41.8 ms, every pose moved 327.6 ms (everything is walked twice), no ledger to start from 172.4 ms.                              */
typedef struct qn_occupancy_update {
  uint32_t entries_kept, entries_added, entries_removed;
  uint32_t rebuilt, regridded, records_walked;
  int32_t  dirty_lo[3], dirty_hi[3];
  uint64_t rays_added, rays_removed;
} qn_occupancy_update;                                                                                                       /* 64 bytes */
int  qn_kf_map_occupancy_update(qn_kf_store*, const int32_t* ids, const double* poses16, uint32_t count, const qn_occupancy_params* params,
                                qn_occupancy_stats* stats_out, qn_occupancy_update* update_out);
/* ---- the occupancy map's Euclidean distance field (csrc/qn_mapdistance.inc, part of csrc/qn_staticmap.hip; numpy twin and specification: qn_amd/mapdistance.py)
 * What a planner asks of an occupancy map first: how far is this place from the nearest obstacle - for the collision check of a trajectory, an inflated
 * costmap, the clearance of a body of some height.  These calls run an exact Euclidean distance transform over the resident class bytes of the live
 * qn_kf_map_occupancy result, W x H x D voxels with x fastest, and keep the field on the device.  Everything is an integer and equal to the twin's bit for bit;
 * only the distance is returned, not the nearest site, so there is no tie to break.
 * Sites: a voxel whose class bit (1 << class) is set in site_mask.  1 << QN_OCC_OCCUPIED is the default; (1 << QN_OCC_OCCUPIED) | (1 << QN_OCC_UNKNOWN) is
 *   the conservative planner's choice, unknown space as an obstacle.  Nothing outside the grid is a site.
 * Field, one uint16_t per voxel: d2[v] = min over sites s of (vx - sx)^2 + (vy - sy)^2 + (vz - sz)^2 in voxel units; a site has d2 = 0; QN_DIST_FAR
 *   (0xffff) when that minimum exceeds max_dist^2 or there is no site.  max_dist <= QN_DIST_MAX_RADIUS = 255, so d2 <= 65025 < QN_DIST_FAR.  The distance in
 *   metres is sqrt(d2) * voxel, host arithmetic.
 * Passes: three, along x, y and z, each a windowed minimum of half-width max_dist that treats an intermediate value above max_dist^2 as infinite.  That is
 *   exact under the cap: a site within max_dist has every per-axis offset <= max_dist.  No atomics, no floating point outside the query's quantisation.
 * qn_distance_params (16 bytes): site_mask (bits 0 .. 2, not 0; default 1 << QN_OCC_OCCUPIED), max_dist (1 .. 255 voxels; default 16), reserved[2] (0).  The
 *   defaults are interface choices, not measurements.
 * qn_distance_stats (32 bytes): sites, reached (the voxels that are no site and have d2 <= max_dist^2), far (the rest): sites + reached + far == W H D;
 *   max_d2 and sum_d2 (u64) over the reached voxels, 0 when there are none; reserved[2] (0).
 * qn_kf_map_distance: QN_ERR_INVALID_ARG, before anything runs and with the previous field intact: a null pointer, site_mask 0 or with a bit >= 3, max_dist
 *   0 or > 255, reserved != 0.  QN_ERR_NOT_READY without a live occupancy result.  A 0 x 0 x 0 grid succeeds with zero statistics.  Device memory: two grids
 *   of at least 2 W H D bytes, the field and one temporary (grown half again as large, kept between calls); when they cannot be allocated QN_ERR_HIP with the previous field intact.  The field stays resident until
 *   the next successful qn_kf_map_distance or the next successful qn_kf_map_occupancy; the latter ends it and the getters answer QN_ERR_NOT_READY again.  A
 *   refused call of either leaves the field intact.  One host synchronisation: the statistics.
 * qn_kf_map_distance_grid: *info_out (the occupancy grid's), *params_out (the parameters used) and d2_out, W H D values of 2 bytes; d2_out may be NULL to
 *   fetch the dimensions first.  QN_ERR_NOT_READY without a live field.  One host synchronisation.
 * qn_kf_map_distance_slice: d2_out (W x H values of 2 bytes, row-major with y the slow axis) - per column the smallest d2 over the layers iz_lo .. iz_hi
 *   inclusive, clipped to the grid: the 3-D clearance of an upright body spanning those layers.  QN_DIST_FAR when the band misses the grid.
 *   QN_ERR_INVALID_ARG when iz_lo > iz_hi or a pointer is null.  QN_ERR_NOT_READY as above.  One host synchronisation.
 * qn_kf_map_distance_query: n world points (xyz, 3 f64 each) go to their voxel by the occupancy map's own arithmetic, c_k = ((int64) rint((x_k * inv) *
 *   1024.0) >> 10) - minc_k with inv = 1.0 / voxel, no contraction, half to even.  d2_out[i] is the field's value there, class_out[i] the voxel's class.  A
 *   point that is not finite, has |x_k * inv| >= 2^20, or falls outside the grid gets QN_DIST_FAR and QN_DIST_OUTSIDE (0xff).  QN_ERR_INVALID_ARG: n == 0 or
 *   a null pointer.  QN_ERR_NOT_READY as above.  One lane per point: an upload of 24 n bytes, one kernel, a download of 3 n bytes; one host synchronisation. */
#define QN_DIST_FAR 0xffffu
#define QN_DIST_MAX_RADIUS 255u
#define QN_DIST_OUTSIDE 0xffu
typedef struct qn_distance_params { uint32_t site_mask, max_dist, reserved[2]; } qn_distance_params;                                    /* 16 bytes */
typedef struct qn_distance_stats  { uint32_t sites, reached, far, max_d2; uint64_t sum_d2; uint32_t reserved[2]; } qn_distance_stats;  /* 32 bytes */
void qn_distance_default_params(qn_distance_params* p);
int  qn_kf_map_distance(qn_kf_store*, const qn_distance_params* params, qn_distance_stats* stats_out);
int  qn_kf_map_distance_grid(qn_kf_store*, qn_occupancy_grid* info_out, qn_distance_params* params_out, uint16_t* d2_out);
int  qn_kf_map_distance_slice(qn_kf_store*, int32_t iz_lo, int32_t iz_hi, uint16_t* d2_out /* W x H, y slow */);
int  qn_kf_map_distance_query(qn_kf_store*, const double* xyz, uint32_t n, uint16_t* d2_out, uint8_t* class_out);
/* ---- planning over the occupancy map: the cost-to-go field and paths (csrc/qn_maproute.inc, part of csrc/qn_staticmap.hip; numpy twin and specification:
 * qn_amd/maproute.py)
 * What a planner asks of the volume second: how far is it from here to there through free space with a given clearance, and along which voxels.  These calls
 * compute, over the resident class bytes of the live qn_kf_map_occupancy result and the live qn_kf_map_distance field, the shortest-path cost from every voxel
 * to the nearest of a set of goals, keep it on the device, and walk paths down it.  Shortest-path costs are unique integers: whatever the schedule of the relaxation,
 * every value equals the twin's bit for bit.
 * qn_route_params (32 bytes): pass_mask (class bits 0 .. 2, not 0; default 1 << QN_OCC_FREE), min_d2 (a voxel passes only if d2 >= min_d2; QN_DIST_FAR passes
 *   any min_d2, 0 switches the test off; default 4), iz_lo, iz_hi (i32: the band of layers, inclusive, clipped to the grid; defaults 0 and INT32_MAX), planar (0
 *   or 1; default 0), reserved[3] (0).  The defaults are interface choices, not measurements.
 * Passable, 3-D (planar 0): voxel v iff its class bit is in pass_mask, d2[v] >= min_d2 and iz_lo <= vz <= iz_hi; the field is W x H x D.  Planar: the field is
 *   W x H x 1; a column is passable iff the clipped band is not empty and every voxel of the column inside it passes the class and d2 tests - an upright body
 *   moving in the plane, the companion of qn_kf_map_distance_slice.
 * Moves: from v to v + o, o in {-1, 0, 1}^3 without 0, both ends inside the field; allowed iff every voxel v + o' is passable, o'_k in {0, o_k} on each axis k:
 *   the 2, 4 or 8 voxels of the block the move spans.  No corner is cut and no diagonal slips between two obstacles; the rule is symmetric, so the graph is
 *   undirected.  Cost 2 + |o|_1: 3 for a face move, 4 for an edge move, 5 for a corner move, the 3-4-5 chamfer metric: cost / 3 * voxel is the length in
 *   metres, in open space between 5.7 % under (a face diagonal) and 10.6 % over (direction (3, 1, 1)) the Euclidean length.
 * Goals: n world points (3 f64 each), 1 .. 2^20, each to its voxel by the occupancy map's own quantisation, exactly as in qn_kf_map_distance_query; in planar
 *   mode only x and y choose the column, z must still be finite with |z * inv| < 2^20.  A goal whose voxel or column is passable has cost 0; every other goal
 *   (not finite, outside, blocked) is ignored and counted in goals_blocked.  With no goal left the call still succeeds and nothing is reached.
 * Field, one uint32_t per voxel (per column in planar mode): the smallest path cost to a goal, QN_ROUTE_BLOCKED (0xfffffffe) where the voxel is not passable,
 *   QN_ROUTE_UNREACHED (0xffffffff) where it is passable but not connected to a goal.  A simple path has at most 2^27 voxels, so a cost is at most 5 * 2^27.
 * qn_route_stats (64 bytes): passable, blocked, reached, unreached (passable = reached + unreached, passable + blocked = the field's cells), goals_used,
 *   goals_blocked, max_cost, reserved0 (0), sum_cost (u64) over the reached cells - these equal the twin's; rounds and tile_visits (u64), diagnostics of the GPU
 *   schedule that the twin does not have: the relaxation launches up to the first that changed nothing and the tiles they loaded; reserved[2] (0).
 * qn_kf_map_route: QN_ERR_INVALID_ARG, before anything runs and with the previous field intact: a null pointer, n == 0 or n > 2^20, pass_mask 0 or with a bit
 *   >= 3, planar > 1, reserved != 0, iz_lo > iz_hi, min_d2 > max_dist^2 of the live distance field (beyond the cap the distance is not known).
 *   QN_ERR_NOT_READY without a live occupancy result and a live distance field.  A 0 x 0 x 0 grid succeeds with zero statistics.  Device memory: 4 bytes per
 *   cell of the field (grown half again as large, kept between calls); when it cannot be allocated QN_ERR_HIP with the previous field intact.  QN_ERR_INTERNAL
 *   if the relaxation has not settled after cells + 2 rounds, which bound it.  The field stays resident until the next successful qn_kf_map_route,
 *   qn_kf_map_distance or qn_kf_map_occupancy; the latter two end it and the getters answer QN_ERR_NOT_READY again.  A refused call of any of the three leaves
 *   the field byte-identical.  Host synchronisations: ceil(rounds / QN_ROUTE_ROUNDS_PER_CHECK) + 1 - one per batch of rounds, then the statistics,
 *   which carry the goals' counts.  Integer arithmetic throughout; the only floating point is the quantisation of goals, starts and query points.
 * qn_kf_map_route_grid: *info_out (the occupancy grid's), *params_out (the parameters used) and cost_out, W H D values of 4 bytes (W H in planar mode);
 *   cost_out may be NULL to fetch the dimensions first.  QN_ERR_NOT_READY without a live field.
 * qn_kf_map_route_query: cost_out[i] = the field's value at world point i, quantised like a goal; QN_ROUTE_BLOCKED for a point that is not finite or outside.
 *   QN_ERR_INVALID_ARG: a null pointer, n == 0 or n > 2^20.
 * qn_kf_map_route_path: S start points (3 f64 each, quantised like goals).  From the start's voxel: at v with cost c > 0 take the first allowed move to n with
 *   cost[n] + w(v, n) == c, the moves enumerated with dz outermost, then dy, then dx, each in the order -1, 0, +1; stop at cost 0.  len_out[S]: the true number
 *   of voxels, start and goal included, 0 for a start that is outside, blocked or unreached.  ijk_out: the first min(len, max_len) voxels of each path at
 *   stride max_len, int32 x 3, the rest 0; in planar mode k = 0.  cost / 3 + 1 bounds len.  QN_ERR_INVALID_ARG: a null pointer, S == 0 or S > 2^20,
 *   max_len == 0. */
#define QN_ROUTE_BLOCKED 0xfffffffeu
#define QN_ROUTE_UNREACHED 0xffffffffu
#define QN_ROUTE_MAX_POINTS (1u << 20)
#define QN_ROUTE_ROUNDS_PER_CHECK 8u                     /* an untuned choice: relaxation launches between two reads of the "anything changed" words */
typedef struct qn_route_params { uint32_t pass_mask, min_d2; int32_t iz_lo, iz_hi; uint32_t planar, reserved[3]; } qn_route_params;     /* 32 bytes */
typedef struct qn_route_stats  { uint32_t passable, blocked, reached, unreached, goals_used, goals_blocked, max_cost, reserved0; uint64_t sum_cost, rounds, tile_visits;
                                 uint32_t reserved[2]; } qn_route_stats;                                                                /* 64 bytes */
void qn_route_default_params(qn_route_params* p);
int  qn_kf_map_route(qn_kf_store*, const double* goals_xyz, uint32_t n, const qn_route_params* params, qn_route_stats* stats_out);
int  qn_kf_map_route_grid(qn_kf_store*, qn_occupancy_grid* info_out, qn_route_params* params_out, uint32_t* cost_out);
int  qn_kf_map_route_query(qn_kf_store*, const double* xyz, uint32_t n, uint32_t* cost_out);
int  qn_kf_map_route_path(qn_kf_store*, const double* starts_xyz, uint32_t n_starts, uint32_t max_len, uint32_t* len_out, int32_t* ijk_out);
/* ---- exploration frontiers of the occupancy map (csrc/qn_mapfrontier.inc, part of csrc/qn_staticmap.hip; numpy twin and specification:
 * qn_amd/mapfrontier.py)
 * What an explorer asks of the volume: where to go next to see more.  The answer is the set of frontiers, the free voxels that border unknown space, grouped
 * into connected regions, each with a size, a box, a centroid and - with a live route field - the cost of reaching it.  These calls compute them over the
 * resident class bytes of the live qn_kf_map_occupancy result and keep them on the device.  Everything is an integer; components are a set property and root,
 * number, box and sums do not depend on any order, so every byte equals the twin's bit for bit whatever the schedule.  They need neither the distance field nor
 * the route field; only qn_kf_map_frontier_costs reads the route field.
 * qn_frontier_params (32 bytes): free_mask (class bits 0 .. 2, not 0; default 1 << QN_OCC_FREE), unknown_mask (class bits 0 .. 2, not 0, no bit of free_mask;
 *   default 1 << QN_OCC_UNKNOWN), edge_unknown (0 or 1; default 1), min_size (>= 1; default 8), iz_lo, iz_hi (i32: the band of layers, inclusive, clipped to the
 *   grid; defaults 0 and INT32_MAX), reserved[2] (0).  The defaults are interface choices, not measurements.
 * Candidate: a voxel whose class bit is in free_mask and whose layer lies in the band.
 * Frontier voxel: a candidate with at least one of its 6 face neighbours unknown.  A neighbour inside the grid is unknown iff its class bit is in unknown_mask;
 *   the band does not apply to neighbours.  A neighbour outside the grid is unknown iff edge_unknown: the grid is the bounding box of the rays, so nothing was
 *   seen beyond it.  faces[v] = the number of unknown face neighbours, 1 .. 6.
 * Components: the connected components of the frontier voxels under 26-connectivity; root = the smallest linear index (iz H + iy) W + ix of the component,
 *   size = its voxel count.  Regions: the components with size >= min_size, numbered 0 .. R - 1 in ascending root.
 * Labels, one int32_t per voxel: the region number, QN_FRONTIER_REJECTED (-1) for the frontier voxels of smaller components, QN_FRONTIER_NONE (-2) elsewhere.
 * qn_frontier_info (64 bytes), one per region: root, size, lo[3], hi[3] (the box of the grid indices ix, iy, iz), faces (the sum of faces[v], the opening's area
 *   in voxel faces), reserved (0), sum[3] (u64: the sums of ix, iy, iz; the centroid is sum / size in grid indices, (minc + c + 0.5) * voxel in metres).
 * qn_frontier_stats (48 bytes): candidates, frontier (voxels), components, regions, too_small (components), region_voxels, rejected_voxels, largest (the size
 *   of the largest component, kept or not), unknown_faces (the sum of faces[v] over all frontier voxels) - these equal the twin's; rounds, a diagnostic of the GPU
 *   schedule that the twin does not have (1: union-find needs no host loop); reserved[2] (0).
 * qn_kf_map_frontiers: QN_ERR_INVALID_ARG, before anything runs and with the previous result intact: a null pointer, a mask that is 0 or has a bit >= 3, masks
 *   that overlap, edge_unknown > 1, min_size == 0, iz_lo > iz_hi, reserved != 0.  QN_ERR_NOT_READY without a live occupancy result.  A 0 x 0 x 0 grid succeeds
 *   with zero statistics.  Device memory: 4 bytes per voxel for the labels and 64 bytes per region (both grown half again as large, kept between calls); when the
 *   labels cannot be allocated QN_ERR_HIP with the previous result intact.  The result stays resident until the next successful qn_kf_map_frontiers or
 *   qn_kf_map_occupancy; the latter ends it and the getters answer QN_ERR_NOT_READY again; qn_kf_map_distance and qn_kf_map_route do not touch it.  A refused
 *   call of either leaves the result byte-identical.  Two host synchronisations: the number of regions, the statistics.
 * qn_kf_map_frontier_grid: *info_out (the occupancy grid's), *params_out (the parameters used) and label_out, W H D values of 4 bytes; label_out may be NULL to
 *   fetch the dimensions first.  QN_ERR_NOT_READY without a live frontier result, here and below.
 * qn_kf_map_frontier_regions: the R rows in region order; *count_out = R.  QN_ERR_CAPACITY, with *count_out set and nothing else written, when capacity < R.
 * qn_kf_map_frontier_list: every frontier voxel (kept or rejected) in ascending linear index by a stable device compaction: ijk_out three grid indices each,
 *   label_out its label; *count_out their number.  QN_ERR_CAPACITY, with *count_out set, when capacity is below it.  With capacity 0 the arrays may be NULL.
 * qn_kf_map_frontier_costs: with the live route field of qn_kf_map_route (3-D or planar: a voxel reads its column's cell), per region the smallest cost
 *   below QN_ROUTE_BLOCKED over its voxels into cost_out[R] and the voxel attaining it, the smallest linear index on a tie, into ijk_out[R x 3];
 *   QN_ROUTE_UNREACHED and voxel (0, 0, 0) when no voxel of the region is reached.  QN_ERR_NOT_READY also without a live route field. */
#define QN_FRONTIER_REJECTED (-1)
#define QN_FRONTIER_NONE (-2)
typedef struct qn_frontier_params { uint32_t free_mask, unknown_mask, edge_unknown, min_size; int32_t iz_lo, iz_hi; uint32_t reserved[2]; } qn_frontier_params;   /* 32 bytes */
typedef struct qn_frontier_stats  { uint32_t candidates, frontier, components, regions, too_small, region_voxels, rejected_voxels, largest, unknown_faces, rounds,
                                    reserved[2]; } qn_frontier_stats;                                                                  /* 48 bytes */
typedef struct qn_frontier_info   { uint32_t root, size; int32_t lo[3], hi[3]; uint32_t faces, reserved; uint64_t sum[3]; } qn_frontier_info;   /* 64 bytes */
void qn_frontier_default_params(qn_frontier_params* p);
int  qn_kf_map_frontiers(qn_kf_store*, const qn_frontier_params* params, qn_frontier_stats* stats_out);
int  qn_kf_map_frontier_grid(qn_kf_store*, qn_occupancy_grid* info_out, qn_frontier_params* params_out, int32_t* label_out /* W H D, may be NULL */);
int  qn_kf_map_frontier_regions(qn_kf_store*, qn_frontier_info* info_out, uint32_t capacity, uint32_t* count_out);
int  qn_kf_map_frontier_list(qn_kf_store*, int32_t* ijk_out, int32_t* label_out, uint32_t capacity, uint32_t* count_out);   /* every frontier voxel, ascending linear index */
int  qn_kf_map_frontier_costs(qn_kf_store*, uint32_t* cost_out /* R */, int32_t* ijk_out /* R x 3 */);
/* ---- view gain over the occupancy map (csrc/qn_mapview.inc, part of csrc/qn_staticmap.hip; numpy twin and specification: qn_amd/mapview.py)
 * What decides between two frontier regions: standing here, how much unknown space would the sensor actually see?  A region's size and faces are the size of
 * an opening, not the volume behind it.  The answer is next-best-view gain: the sensor's rays are cast from each candidate viewpoint through the resident class
 * bytes of the live qn_kf_map_occupancy result, each ray stops at the first occupied voxel, and the distinct unknown voxels the rays pass through are counted.
 * Everything behind the viewpoint's quantisation is an integer; distinct is a set property and the tallies are integer sums, so every byte equals the twin's,
 * bit for bit, whatever the schedule, the pass split or the order of the rays.
 * Input: q viewpoints xyz (world coordinates, f64), 1 <= q <= 2^16; a ray table offsets, r rows of three int32_t, 1 <= r <= 2^20: a ray's end relative to its
 *   start in the occupancy map's fixed point, 1024ths of a voxel, every |component| <= QN_VIEW_MAX_OFFSET (2^25).  The table is the caller's data, so no sine or
 *   cosine is evaluated on the device.
 * qn_view_params (32 bytes): gain_mask (class bits 0 .. 2, not 0; default 1 << QN_OCC_UNKNOWN), stop_mask (class bits 0 .. 2, may be 0, no bit of gain_mask;
 *   default 1 << QN_OCC_OCCUPIED), max_through (0: no limit; default 0), iz_lo, iz_hi (i32: the band of layers, inclusive, clipped to the grid; defaults 0 and
 *   INT32_MAX), reserved[3] (0).  The defaults are interface choices, not measurements.
 * Viewpoint: A_k = int64(rint((x_k * inv) * 1024)), the occupancy map's quantisation (f64, every operation rounded on its own, half to even).  QN_VIEW_OUTSIDE (1)
 *   when a coordinate is not finite, |x_k * inv| >= 2^20 or the voxel c(A) = A >> 10 lies outside the grid, else QN_VIEW_OK (0).  An OUTSIDE viewpoint casts
 *   nothing and its row is zero apart from the status.
 * Ray r of an OK viewpoint: B = A + offsets[r]; the visited voxels v_0 = c(A) .. v_n = c(B) are those of the occupancy walk (the same integer rule, a tie to the
 *   lowest axis, an origin on a face heading down steps at once), examined in order, v_0 included: (1) v_i outside the grid: the ray ESCAPED, it ends and v_i is
 *   not counted in steps; (2) otherwise steps += 1, and if the class bit of v_i is in stop_mask the ray is BLOCKED and ends; (3) otherwise, if its class bit is in
 *   gain_mask, the pair (viewpoint, v_i) is marked when the layer iz lies in the band, through += 1, band or not, and if max_through != 0 and through ==
 *   max_through the ray is SPENT and ends; (4) if v_n has been examined without an end, the ray REACHED.  The four ray ends - blocked, escaped, spent, reached -
 *   exclude each other; a ray with offset (0, 0, 0) examines v_0 only.
 * qn_view_info (48 bytes), one per viewpoint: status, gain (the number of distinct voxels marked for the viewpoint), blocked, escaped, spent, reached (rays),
 *   ijk[3] (the viewpoint's grid voxel, (0, 0, 0) when OUTSIDE), reserved (0), steps (u64).
 * cover: one uint32_t per voxel, W H D, x fastest, linear index (iz H + iy) W + ix: the number of viewpoints that marked the voxel.  Sum cover = sum gain.
 * qn_view_stats (48 bytes): viewpoints (q), outside, rays (r), covered (the voxels with cover >= 1), max_cover, total_gain, steps (the sum of the rows') - these
 *   equal the twin's; passes, a diagnostic of the GPU schedule that the twin does not have; reserved[2] (0).
 * qn_kf_map_view_gain: QN_ERR_INVALID_ARG, before anything runs and with the previous result intact: a null pointer, q or r outside its range, a gain_mask that
 *   is 0 or has a bit >= 3, a stop_mask with a bit >= 3 or one of gain_mask, iz_lo > iz_hi, reserved != 0, an offset beyond the limit.  QN_ERR_NOT_READY without a
 *   live occupancy result.  On a 0 x 0 x 0 grid every viewpoint is OUTSIDE and the call succeeds.  Device memory: 4 bytes per voxel for cover (grown half again as
 *   large beside the previous volume, kept between calls); when it cannot be allocated QN_ERR_HIP with the previous result intact.  The result stays resident
 *   until the next successful qn_kf_map_view_gain or qn_kf_map_occupancy; the latter ends it; qn_kf_map_distance, qn_kf_map_route and qn_kf_map_frontiers do not
 *   touch it.  The kernels: k_mv_origin (the quantisation, one viewpoint per lane), k_mv_cast (one lane per viewpoint and ray; a bitset per viewpoint over its
 *   reach box - the viewpoint's voxel +- ((max |offset component| >> 10) + 1), clipped to the grid - makes a voxel count once: a plain read first, the returning
 *   atomicOr only when the bit looks unset), k_mv_stats (covered, max_cover and the sum in one pass over cover).  The viewpoints go in passes that fit a scratch
 *   budget; the whole call is one synchronisation with the host whatever the number of passes.  Environment, read per call, the same bytes either way:
 *   QN_VIEW_PASS=<n> caps the viewpoints of a pass, QN_VIEW_NO_PEEK=1 always issues the atomicOr (the yardstick of tools/gpu_map_view_time.py).
 *   Time on an MI355X (tools/gpu_map_view_time.py; 57 600 rays of 20 m at voxel 0.3, a volume of 1.08e7 voxels): 0.67 / 0.73 / 1.95 ms for 1 / 16 / 256 viewpoints,
 *   beside 200 ms for qn_kf_map_occupancy and 1.0 ms for qn_kf_map_frontiers on the same store (profiles/EXPERIMENTS.md).
 * qn_kf_map_view_grid: *info_out (the occupancy grid's), *params_out (the parameters used) and cover_out, W H D values of 4 bytes; cover_out may be NULL to
 *   fetch the dimensions first.  QN_ERR_NOT_READY without a live view result. */
#define QN_VIEW_OK 0
#define QN_VIEW_OUTSIDE 1
#define QN_VIEW_MAX_OFFSET (1 << 25)
typedef struct qn_view_params { uint32_t gain_mask, stop_mask, max_through; int32_t iz_lo, iz_hi; uint32_t reserved[3]; } qn_view_params;   /* 32 bytes */
typedef struct qn_view_info   { uint32_t status, gain, blocked, escaped, spent, reached; int32_t ijk[3]; uint32_t reserved; uint64_t steps; } qn_view_info;   /* 48 bytes */
typedef struct qn_view_stats  { uint32_t viewpoints, outside, rays, covered, max_cover, passes, reserved[2]; uint64_t total_gain, steps; } qn_view_stats;   /* 48 bytes */
void qn_view_default_params(qn_view_params* p);
int  qn_kf_map_view_gain(qn_kf_store*, const double* xyz /* Q x 3 */, uint32_t q, const int32_t* offsets /* R x 3 */, uint32_t r, const qn_view_params* params,
                         qn_view_info* info_out /* Q */, qn_view_stats* stats_out);
int  qn_kf_map_view_grid(qn_kf_store*, qn_occupancy_grid* info_out, qn_view_params* params_out, uint32_t* cover_out /* W H D, may be NULL */);
/* ---- the map's points clustered into objects (csrc/qn_mapclusters.inc, part of csrc/qn_mapoutliers.hip; numpy twin and specification: qn_amd/mapclusters.py)
 * After qn_kf_map_ground every point is GROUND, OBSTACLE or OVERHEAD, but the obstacles are an unstructured set.  These calls run PCL's
 * EuclideanClusterExtraction over the store's map slot on the GPU: connected components of the radius graph, each with a size, a box and a centroid, and the
 * clumps too small (or too large) to be anything marked for removal.
 * qn_cluster_params (24 bytes): tolerance (finite, > 0, default 0.5), min_size (>= 1, default 10), max_size (>= min_size, default 0xffffffff), class_mask
 *   (bits 0 .. 4 only, default 0), reserved (0).  The defaults are interface choices, not measurements.
 * Members: with class_mask == 0 every finite point of the map slot (x, y and z all finite); with class_mask != 0 a finite point whose ground class c has its
 *   bit 1 << c set in the mask, the class being the live qn_kf_map_ground classification of the same slot generation.
 *   (1 << QN_GROUND_OBSTACLE) | (1 << QN_GROUND_OVERHEAD) is the intended use.
 * Edges: two members at DIFFERENT map indices are joined when their f32 squared distance (the overlap measure's arithmetic: f32 differences, dx dx + dy dy +
 *   dz dz left to right, no fused multiply-add; symmetric) is <= float(tolerance * tolerance), inclusive.  A duplicate at another index is joined at distance
 *   0.  edges = the number of unordered joined pairs (u64).
 * Components: the connected components of that graph.  root[p] = the smallest map index of p's component, size[p] = its member count; a point that is not a
 *   member has root 0xffffffff and size 0.
 * Clusters: a component with min_size <= size <= max_size, numbered 0 .. C - 1 in ascending order of root.  label[p] (int32) = the number,
 *   QN_CLUSTER_REJECTED -1 for the members of the other components, QN_CLUSTER_NONE -2 for the points that are not members.
 * qn_cluster_info (56 bytes) per cluster: root, size, lo[3], hi[3] - the f32 minimum and maximum of the members' coordinates in the total order of the
 *   sign-magnitude-to-ordered-integer image of the f32, so -0 < +0 - and sum_q[3], the int64 sums of xq = (int64) rint((double)x * 2^e), half to even, e the
 *   largest integer with tolerance * 2^e <= 2^10 (within [-126, 127]; the product is exact).  The centroid is sum_q / size * 2^-e in f64, host arithmetic.
 *   QN_ERR_CAPACITY when a member has |xq| >= 2^31; below that the sums over fewer than 2^32 points are exact.
 * qn_cluster_stats (56 bytes): n, n_finite, members; components, clusters, too_small, too_large (components); clustered_points, rejected_points; largest
 *   (the largest component's size); quant_exp (e), reserved (0); edges.
 * Everything is an integer or an f32 selected by an order-free rule, equal to the twin's bit for bit whatever order neighbours are met in or unions happen; a
 *   rerun gives the same bytes.
 * qn_kf_map_clusters: classifies the map slot as it stands; the slot itself is not touched.  The results stay resident for the slot's generation (any later
 *   map build or filter, successful or not, ends it).  At most four host synchronisations.  QN_ERR_NOT_READY without a map, or with class_mask != 0 and no
 *   live ground classification of this generation.  QN_ERR_INVALID_ARG: a null pointer, a parameter outside the ranges above.  QN_ERR_CAPACITY as above, and
 *   whatever the cell index refuses (a map whose extent overflows f32).  A refused call leaves the previous results intact.
 * qn_kf_map_cluster_points: label_out, root_out, size_out at the map's own indices; any may be NULL, not all.  QN_ERR_NOT_READY before a successful
 *   qn_kf_map_clusters and once the slot's generation has moved on.
 * qn_kf_map_cluster_list: *count_out = C; out NULL: the count only; capacity < C: QN_ERR_CAPACITY and nothing written (*count_out included); else the C
 *   records in cluster order.  QN_ERR_NOT_READY as above.
 * qn_kf_map_drop_rejected_clusters: removes the members of rejected components; points that are not members - non-finite records, excluded ground - stay.
 *   The kept records, in order and all 16 bytes each, become the map slot (*d_xyzi_out, *n_out; NULL and 0 when nothing is left).  The generation advances,
 *   so normals, outlier, ground and cluster results go stale.  QN_ERR_NOT_READY without a live classification, and the slot is then unchanged.          */
#define QN_CLUSTER_REJECTED (-1)
#define QN_CLUSTER_NONE (-2)
typedef struct qn_cluster_params { double tolerance; uint32_t min_size, max_size, class_mask, reserved; } qn_cluster_params;    /* 24 bytes */
typedef struct qn_cluster_info { uint32_t root, size; float lo[3], hi[3]; int64_t sum_q[3]; } qn_cluster_info;                 /* 56 bytes */
typedef struct qn_cluster_stats {
  uint32_t n, n_finite, members;
  uint32_t components, clusters, too_small, too_large;
  uint32_t clustered_points, rejected_points, largest;
  int32_t quant_exp; uint32_t reserved;
  uint64_t edges;
} qn_cluster_stats;                                                                                                          /* 56 bytes */
void qn_cluster_default_params(qn_cluster_params* p);
int  qn_kf_map_clusters(qn_kf_store*, const qn_cluster_params* params, qn_cluster_stats* stats_out);
int  qn_kf_map_cluster_points(qn_kf_store*, int32_t* label_out, uint32_t* root_out, uint32_t* size_out);
int  qn_kf_map_cluster_list(qn_kf_store*, qn_cluster_info* out, uint32_t capacity, uint32_t* count_out);
int  qn_kf_map_drop_rejected_clusters(qn_kf_store*, const float** d_xyzi_out /* float4: x y z intensity */, uint32_t* n_out);
/* ---- scans localised in the corrected map: crop and register (csrc/qn_maplocalize.inc, part of csrc/qn_verify.hip; numpy twin and specification of the crop:
 * qn_amd/maplocalize.py).  The reference saves its map "for FAST-LIO-Localization-QN" (config.yaml, save_map_bag): Quatro + Nano-GICP of a scan against the
 * neighbourhood of a pose guess in the saved map.  Here the map slot never leaves the device: the neighbourhoods are cut out by one streaming pass and handed to
 * the batch registration as device pairs.
 * Membership: a map record p (the float4 of the map slot) is a member of the crop (c, R, shape) iff x, y and z are finite and d2 <= r2, inclusive, with c three
 *   f32 values (the caller's f64 centre rounded to f32), r2 = float(R * R), the product taken in f64, dx = p.x - c.x (dy, dz likewise) in f32 and
 *   d2 = (dx dx + dy dy) + dz dz summed left to right with no fused multiply-add.  QN_LOCALIZE_CYLINDER leaves dz dz out (an upright cylinder without ends; z must
 *   still be finite); QN_LOCALIZE_SPHERE is the default.  Non-finite records are never members.
 * A crop holds its members' full 16-byte records in ascending map index, and a uint32 map index goes with every record.  Crops, indices and counts equal the twin's
 *   bit for bit and a rerun gives the same bytes: brute force over the slot, 64 centres per pass (more centres: further passes), a record loaded once per kernel per
 *   pass, no atomics.  Limits: 32767 centres per call and fewer than 2^32 crop records in all, else QN_ERR_CAPACITY.
 * qn_kf_map_crop: counts_out[c] = the members of crop c.  Two host synchronisations.  QN_ERR_INVALID_ARG before anything runs: a null pointer, n_crops == 0, a
 *   non-finite centre, a radius that is not finite or <= 0, a bad shape.  QN_ERR_NOT_READY without a map.  The crops are COPIES in a buffer of their own (not the
 *   voxel pipeline's scratch): a later map build or filter does not touch them.
 * qn_kf_map_crop_get: crop `crop` of the latest crop (or localise) call as a device pointer (float4: x y z intensity; NULL when empty) and count; idx_out (host,
 *   may be NULL) receives the n map indices (one host synchronisation).  The pointer is valid until the next crop or localise call or the store's destruction.
 *   QN_ERR_NOT_READY before such a call, QN_ERR_INVALID_ARG for a null pointer or crop >= that call's crops.
 * qn_localize_params (32 bytes): radius (35.0), leaf (0.3), score_thr (1.5), shape (sphere), reserved (0) - config.yaml's radius, voxel and score.
 * qn_kf_map_localize: pair j registers keyframe query[j] - alone in its sensor frame, voxel grid at `leaf`, each distinct query once - against the crop around the
 *   translation of g_j, where g_j is guess16[16 j ..] (row-major 4x4, map <- sensor) with every entry rounded to f32: one rounding, the same numbers for the crop
 *   centre and for the seed.  Pairs whose centres have the same f32 bits share one crop (heading hypotheses at one position).  The pairs are grouped by query
 *   (stable) into ONE qn_gicp_align_batch_guess and the records scattered back to caller order: record j equals qn_gicp_align_batch_guess on (scan cloud, crop,
 *   g_j) bit for bit, and its T / T64 is the scan's pose in the map.
 * qn_kf_map_localize_c2f: the same clouds coarse to fine; the centre comes from the guess, its rotation is ignored.  Record j, T_total (the pose) and T_quatro
 *   (may be NULL) equal qn_coarse_to_fine_align_batch({ctx}) on the same two clouds bit for bit.
 * status[j]: QN_ERR_EMPTY_CLOUD for an empty scan or an empty crop, QN_ERR_CAPACITY for a scan or crop above the context's max_points; the other pairs still run.
 *   Whole call: QN_ERR_NOT_READY without a map; QN_ERR_INVALID_ARG before anything runs, with store, record and context unchanged - a null pointer, n_pairs == 0,
 *   a bad id, a non-finite guess or a last row other than 0 0 0 1, bad params, store and context on different devices.
 *   Four host synchronisations (two for the crops, two for the scans' voxel grids) besides the batch registration's own.
 * qn_localize_stats (40 bytes): n_map, n_pairs, n_scans (distinct queries), n_crops (distinct centres), passes, reserved; crop_points (all crops), generation
 *   (the map slot's generation the crops were cut from).
 * Verify record: each localise call leaves the record qn_kf_verify_cloud and qn_kf_verify_overlap serve, pair j with SRC = the scan cloud, DST = the crop,
 *   COARSE (coarse-to-fine only) and FINAL as for a verified loop pair.  The a_to_b overlap of FINAL against the crop is the share of the scan that the map
 *   explains; b_to_a is small by construction (the crop is a whole neighbourhood, the scan sees part of it).  The record goes stale at the next crop or
 *   localise call, or at the next verify call; a rebuilt or filtered map does NOT invalidate it.                                                          */
#define QN_LOCALIZE_SPHERE 0
#define QN_LOCALIZE_CYLINDER 1
typedef struct qn_localize_params { double radius, leaf, score_thr; uint32_t shape, reserved; } qn_localize_params;                     /* 32 bytes */
typedef struct qn_localize_stats { uint32_t n_map, n_pairs, n_scans, n_crops, passes, reserved; uint64_t crop_points, generation; } qn_localize_stats;   /* 40 bytes */
void qn_localize_default_params(qn_localize_params* p);
int  qn_kf_map_crop(qn_kf_store*, const double* centres_xyz /* n_crops x 3 */, uint32_t n_crops, double radius, uint32_t shape, uint32_t* counts_out);
int  qn_kf_map_crop_get(qn_kf_store*, uint32_t crop, const float** d_xyzi /* float4: x y z intensity */, uint32_t* n, uint32_t* idx_out /* may be NULL */);
int  qn_kf_map_localize(qn_kf_store*, qn_ctx*, const qn_localize_params* params, const int32_t* query, const double* guess16 /* n_pairs x 16, map <- sensor */,
                        uint32_t n_pairs, qn_gicp_result* results, int* valid, int* status, qn_localize_stats* stats_out /* may be NULL */);
int  qn_kf_map_localize_c2f(qn_kf_store*, qn_ctx*, const qn_localize_params* params, const int32_t* query, const double* guess16 /* n_pairs x 16 */,
                            uint32_t n_pairs, qn_gicp_result* results, double* T_total, double* T_quatro /* may be NULL */, int* valid, int* status,
                            qn_localize_stats* stats_out /* may be NULL */);
/* LoopClosure::fetchClosestKeyframeIdx (loop_closure.cpp:34-56) generalised to the max_k nearest admissible keyframes,
 * ascending distance; out[0] is the reference's single choice.  Host code (O(#keyframes)).                        */
int  qn_loop_candidates(const double* pos_xyz, const double* stamps, uint32_t n, uint32_t query, double radius, double tdiff,
                        uint32_t max_k, int32_t* out, uint32_t* n_out);

/* ---- keyframes from device memory, and back ----------------------------------------------------------------------------------
 * qn_kf_add_device: a keyframe from a DEVICE buffer (a GPU front end, a torch tensor) with no host staging.  Record i is at
 * d_pts + i * stride_bytes: xyz at byte 0, intensity at intensity_offset_bytes (< 0: none, as qn_kf_add; else the qn_kf_add_xyzi layout
 * rules).  The resident keyframe is byte-identical to qn_kf_add / qn_kf_add_xyzi of the same bytes.  The records must lie inside one
 * device allocation on the store's device (checked: QN_ERR_INVALID_ARG otherwise) and be complete when the call is made (synchronise their
 * producer's stream first); the call returns once they have been copied, so the caller may reuse the buffer.
 * qn_kf_download_keyframe: the resident float4 records of keyframe `id` (n x 4 floats: x y z and .w = intensity for qn_kf_add_xyzi /
 * qn_kf_add_device with intensity / simulated keyframes, 1 for xyz-only ones), for tests and visualisation.                        */
int  qn_kf_add_device(qn_kf_store*, const float* d_pts, uint32_t n, uint32_t stride_bytes, int32_t intensity_offset_bytes, int32_t* id_out);
int  qn_kf_download_keyframe(qn_kf_store*, int32_t id, float* xyzi_out /* n x 4 */);

/* ---- spinning-LiDAR scans ray-cast into the keyframe store (csrc/qn_sim.hip; numpy twin: qn_amd/synth.lidar_scan) -----------
 * The scene is a flat array of analytic primitives:
 *   QN_SIM_GROUND p = (x0, y0, x1, y1, -, -)   plane z = 0 over [x0, x1] x [y0, y1]
 *   QN_SIM_WALL   p = (x0, y0, dx, dy, H, -)   vertical rectangle: dy == 0 -> plane y = y0, x in [x0, x0 + dx]; else plane x = x0,
 *                                              y in [y0, y0 + dy]; z in [0, H]
 *   QN_SIM_POLE   p = (cx, cy, r, H, -, -)     side surface of a vertical cylinder, z in [0, H]
 *   QN_SIM_BOX    p = (cx, cy, sx, sy, H, -)   four sides and the top of an axis-aligned box standing on z = 0
 * The sensor casts n_beams x n_cols rays; the host computes every transcendental (cos / sin of each elevation and azimuth).  Ray (beam,
 * col) of scan s starts at the translation of poses16[s] (sensor -> world, row-major) along R u, u = (cos el cos az, cos el sin az,
 * sin el); primitives are tested in index order and a hit is kept only when strictly nearer (ties go to the lowest index).  The range
 * noise is sigma * sqrt(3) * (u0 + u1 + u2 + u3 - 2), u_i from a counter-based hash of (seeds[s], beam, col, i); the noisy range t' is
 * kept when min_range <= t' <= max_range, and the record is (t' u, intensity) in the SENSOR frame, intensity = a function of the kind and
 * |n . d|.  All arithmetic is f64 (no fused multiply-add), rounded to f32 once: the records equal the numpy twin's bit for bit.
 * Each scan becomes one keyframe (float4 x y z intensity, counted as a qn_kf_add_xyzi keyframe by qn_kf_build_map), hits in (beam, col)
 * order; ids_out[s] are consecutive and n_out[s] is the scan's count (0 allowed).  Every argument is checked before anything runs
 * (QN_ERR_INVALID_ARG, store unchanged): kinds, finite parameters and poses, tables in [-1, 1], 0 <= min_range < max_range,
 * sigma >= 0, and the caps below.  Device scratch is about 40 bytes per ray of the call, kept by the store.  Two host synchronisations
 * per call, whatever n_scans is.                                                                                                     */
enum { QN_SIM_GROUND = 0, QN_SIM_WALL = 1, QN_SIM_POLE = 2, QN_SIM_BOX = 3 };
#define QN_SIM_MAX_PRIMS 4096u                     /* primitives per scene (each ray tests all of them)              */
#define QN_SIM_MAX_RAYS (1u << 20)                 /* n_beams x n_cols per scan                                      */
#define QN_SIM_MAX_SCANS 65535u                    /* scans per call (grid dimension y)                              */
#define QN_SIM_MAX_TOTAL_RAYS (1ull << 27)         /* n_beams x n_cols x n_scans per call (~1160 default 64 x 1800 scans) */
typedef struct {
  uint32_t kind;                                   /* QN_SIM_GROUND / WALL / POLE / BOX */
  uint32_t pad_;
  double p[6];
} qn_sim_prim;
typedef struct {
  uint32_t n_beams, n_cols;
  const double *cos_el, *sin_el;                   /* [n_beams] */
  const double *cos_az, *sin_az;                   /* [n_cols]  */
  double min_range, max_range, sigma;              /* blind radius, detection range, range noise [m] */
} qn_sim_sensor;
int  qn_sim_lidar_to_store(qn_kf_store*, const qn_sim_prim* prims, uint32_t n_prims, const qn_sim_sensor* sensor, const double* poses16,
                           const uint32_t* seeds, uint32_t n_scans, int32_t* ids_out, uint32_t* n_out);

/* ---- loop candidates by Scan Context on the resident keyframes (csrc/qn_sc.hip; numpy twin: qn_amd/scancontext.py) ------------
 * LoopClosure::fetchClosestKeyframeIdx (loop_closure.cpp:34-56, qn_loop_candidates) keeps keyframes within loop_detection_radius of the
 * query's drifted, corrected position; these calls produce the candidate list from a place descriptor instead (Scan Context, Kim & Kim 2018,
 * as in the reference's sibling projects SC-A-LOAM / FAST_LIO_SLAM), independent of the pose estimate.  Opt-in: nothing else uses them.
 * Descriptor of keyframe id: Nr x Ns (n_rings x n_sectors) f32, row-major by ring, from its resident float4 records in the SENSOR frame
 * (PosePcd::pcd_, include/pose_pcd.hpp:7-19), no pose applied.  A point is dropped when x, y or z is not finite, x == y == 0, or
 * r2 = x*x + y*y >= max_radius^2 (f64 from the f32 inputs).  Ring i holds r in [i R / Nr, (i + 1) R / Nr): ring = #{i in 1..Nr-1 : r2 >=
 * (i R / Nr)^2}, edges squared in f64 on the host.  Sector j holds the azimuth [2 pi j / Ns, 2 pi (j + 1) / Ns), counter-clockwise from +x
 * in [0, 2 pi): sector = #{j in 1..Ns-1 : p at or past b_j}, b_j = (cos, sin)(2 pi j / Ns) from the C library on the host; "at or past"
 * = p in the lower half plane [pi, 2 pi) and b_j in the upper, or both in the same half and b_j.x * y - b_j.y * x >= 0 (f64, no fused
 * multiply-add): no transcendental on the device, and a point exactly on an edge goes to the upper bin.  A bin's value is the max over its
 * points of (float)((double)z + lidar_height); a bin with no point is 0 (the original's NO_POINT).
 * Ring key rk[i] = (sum over j in order of d[i][j]) / Ns; column sums of squares ss[j] = sum over i in order of d[i][j]^2; column norm
 * cn[j] = sqrt(ss[j]) (all f64).  Distance of query q to candidate c: for each shift s in [0, Ns), over the columns j in order whose ss_q[j]
 * and ss_c[k] (k = (j + s) mod Ns) are both non-zero, D_s = mean of 1 - (sum over i in order of q[i][j] c[i][k]) / sqrt(ss_q[j] ss_c[k]),
 * D_s = 1 when there is no such column; D = min over s, shift = the lowest s reaching it.  (sqrt of the product rather than the product of
 * the norms: a scan against itself, or turned by whole sectors, is at exactly 0.)  Candidate column j + shift matches query column j: the
 * candidate's heading minus the query's is -shift * 2 pi / Ns.  f64 throughout with IEEE division and the correctly rounded sqrt, in the
 * stated orders, so the engine equals the twin bit for bit.
 * qn_kf_sc_set_params: QN_ERR_INVALID_ARG, previous parameters kept, unless 1 <= n_rings <= QN_SC_MAX_RINGS, 1 <= n_sectors <=
 *   QN_SC_MAX_SECTORS, n_rings * n_sectors <= QN_SC_MAX_BINS, 0 < max_radius <= 1e6, |lidar_height| <= 1e4 (finite; every bin value is
 *   then finite) and ringkey_prefilter <= QN_SC_MAX_PREFILTER.  Changing n_rings, n_sectors, max_radius or lidar_height discards every
 *   descriptor; the prefilter alone does not.  A store starts with n_rings 20, n_sectors 60, max_radius 80, lidar_height 2, no prefilter (qn_kf_sc_get_params).
 * qn_kf_sc_describe: computes the descriptors of `ids` (repeats allowed; an id already described under the current parameters is left as it
 *   is - describing again gives the same bits).  A bad id or count == 0: QN_ERR_INVALID_ARG, nothing described.  One synchronisation (plus
 *   one when the descriptor storage grows).
 * qn_kf_sc_get: desc (Nr x Ns), ringkey (Nr), colnorm (Ns); NULL outputs are skipped.  QN_ERR_NOT_READY when id is not described.
 * qn_kf_sc_query: for each of the nq queries, the candidates c with c != q, stamps[q] - stamps[c] > tdiff (the strict time test of
 *   loop_closure.cpp:45) and c described - an undescribed keyframe is not a candidate.  With ringkey_prefilter = P > 0 only the P of them with
 *   the smallest sum over i in order of (rk_q[i] - rk_c[i])^2 (ties: the lower id) get the full distance (the original's KD-tree search,
 *   made exact).  Row k of the outputs (top_k entries from k * top_k) holds the n_out[k] <= top_k candidates with the smallest D, ties to
 *   the lower id: ids_out, dist_out = D, shift_out = shift; entries past n_out[k] are -1, NaN, -1.  QN_ERR_INVALID_ARG before anything runs,
 *   store unchanged: a null pointer, nq == 0, a query id outside the store, n_stamps < the number of keyframes, NaN tdiff, top_k == 0 or
 *   > QN_SC_MAX_TOP_K, nq * top_k > QN_SC_MAX_RESULTS.  QN_ERR_NOT_READY when a query is not described.  Queries run in chunks whose device
 *   scratch stays under 256 MB; one host synchronisation per call, whatever nq is.                                                 */
#define QN_SC_MAX_RINGS 64u
#define QN_SC_MAX_SECTORS 360u
#define QN_SC_MAX_BINS 8192u                       /* n_rings x n_sectors                              */
#define QN_SC_MAX_PREFILTER 1024u
#define QN_SC_MAX_TOP_K 1024u
#define QN_SC_MAX_RESULTS (1u << 26)               /* nq x top_k per call                               */
typedef struct {
  uint32_t n_rings;                                /* PC_NUM_RING, default 20                           */
  uint32_t n_sectors;                              /* PC_NUM_SECTOR, default 60                         */
  double max_radius;                               /* PC_MAX_RADIUS [m], default 80                     */
  double lidar_height;                             /* LIDAR_HEIGHT [m], added to z, default 2           */
  uint32_t ringkey_prefilter;                      /* 0 = exhaustive (default); P = only the P nearest by ring key */
  uint32_t pad_;
} qn_sc_params;
int  qn_kf_sc_set_params(qn_kf_store*, const qn_sc_params* p);
int  qn_kf_sc_get_params(qn_kf_store*, qn_sc_params* p);
int  qn_kf_sc_describe(qn_kf_store*, const int32_t* ids, uint32_t count);
int  qn_kf_sc_get(qn_kf_store*, int32_t id, float* desc /* Nr x Ns */, double* ringkey /* Nr */, double* colnorm /* Ns */);
int  qn_kf_sc_query(qn_kf_store*, const int32_t* query_ids, uint32_t nq, const double* stamps, uint32_t n_stamps, double tdiff, uint32_t top_k,
                    int32_t* ids_out, double* dist_out, int32_t* shift_out, uint32_t* n_out);

/* ---- per-stage read-backs used by the parity tests (not needed by the shims) ------------ */
int  qn_gicp_get_covariances(qn_ctx*, int which, double* cov9_out);   /* n x 9 f64, original point order */
int  qn_gicp_knn(qn_ctx*, int which, int k, int32_t* idx_out, float* d2_out);   /* self k-NN of a cloud, n x k */
int  qn_gicp_linearize(qn_ctx*, const double T[16], double H[36], double b[6], double* err,
                       int32_t* corr_out, float* sqd_out);            /* one update_correspondences + linearize */
int  qn_gicp_compute_error(qn_ctx*, const double T[16], double* err); /* cached correspondences (LM trial)   */

/* ---- profiling hooks (bench.py roofline leg) -------------------------------------------- */
int  qn_prof_enable(qn_ctx*, int on);                /* records a hipEvent pair around every kernel family launch */
int  qn_prof_reset(qn_ctx*);
int  qn_prof_get(qn_ctx*, int kernel_family, qn_kernel_stat* out);
/* developer knobs (cell size, regime switches, probes, debug counters: the sub-structs LaneKnobs / FeatKnobs / OwnKnobs of csrc/qn_context.h list them); an unknown key is
 * QN_ERR_INVALID_ARG.  Not part of the reference surface */
int  qn_debug_set(qn_ctx*, const char* key, double value);
int  qn_debug_get_counters(qn_ctx*, uint32_t out[16]);
int  qn_debug_selftest(qn_ctx*, uint32_t n_waves, uint32_t seed, uint32_t* mismatches);      /* developer / tests: the device's wave-level search primitives against plain restatements (csrc/qn_selftest.cuh) */
/* developer / tests: the device builds of the two 3 x 3 symmetric eigen solvers (csrc/qn_eig3.cuh) on n caller-supplied matrices, one per lane.  which = 0:
 * qn_eig3_jacobi (the map normals' solver, w unsorted), 1: sym_eig3 (the GICP covariances' and the Quatro normals', w descending).  a6 = (xx, xy, xz, yy, yz, zz)
 * per matrix; w_out 3 n, v_out 9 n row major with the eigenvector of w[k] in column k.  A null pointer, which outside 0 .. 1 or n > QN_DEBUG_EIG3_MAX is
 * QN_ERR_INVALID_ARG; n == 0 succeeds and writes nothing.  Nothing on the product path calls it. */
#define QN_DEBUG_EIG3_MAX (1u << 24)
int  qn_debug_eig3(qn_ctx*, int which, const double* a6, uint32_t n, double* w_out, double* v_out);
/* developer / tests: the device builds of the Gauss-Newton step's small dense f64 routines (csrc/qn_step_math.cuh; d_propose of csrc/qn_gicp_kernels.cuh) on n
 * caller-supplied problems, one per lane.  Records of f64 at a fixed stride per which, in[stride_in * i ..] -> out[stride_out * i ..]; matrices row major:
 *   which  routine              in (stride)                                              out (stride)
 *   0      d_ldlt_solve6_fast   A (36, full symmetric), lambda, b (6)            (43)    x (6), ok (1.0 / 0.0)                                         (7)
 *   1      d_ldlt_solve6        the same; the right-hand side is -b              (43)    x (6)                                                         (6)
 *   2      d_propose            H (36), b (6), lambda, x0 (16)                   (59)    d (6), delta (16), xi (16), path (0.0 fast, 1.0 pivoted)      (39)
 *   3      d_so3_exp            om (3)                                           (3)     R (9)                                                         (9)
 *   4      m3_inverse           M (9)                                            (9)     the inverse (9)                                               (9)
 *   5      d_is_converged       delta (16), rotation_epsilon, transformation_epsilon (18)   converged (1.0 / 0.0), mr, mt                              (3)
 * Every solve is of (A + lambda I) x = -b.  A null pointer, which outside 0 .. 5 or n > QN_DEBUG_STEP_MATH_MAX is QN_ERR_INVALID_ARG with nothing written;
 * n == 0 succeeds and writes nothing.  Nothing on the product path calls it. */
#define QN_DEBUG_STEP_MATH_WHICH 6
#define QN_DEBUG_STEP_MATH_MAX (1u << 20)
int  qn_debug_step_math(qn_ctx*, int which, const double* in, uint32_t n, double* out);
/* developer / tests: what stands between a correspondence and the 6 x 6 system of a registration tick, on caller-supplied inputs (csrc/qn_linearize_debug.hip).
 * Packed f64 throughout; poses are 3 x 4 row major (rotation | translation); points are f64 values that are exactly f32 (they are converted with a cast);
 * normals stand for the covariance I - 0.999 n n^T; lin and have are 0.0 or anything else; the 28 sums are the 21 upper entries of H = J^T M J row major,
 * the 6 of b = J^T M e, then e^T M e.
 *   0  accumulate_point_n (csrc/qn_linearize.cuh), one correspondence per lane, the accumulators starting at zero.  n = correspondences, arg = 0.
 *      in per correspondence (37): Rx (12), Tx (12), pa (3), pb (3), na (3), nb (3), lin.  out per correspondence: the 28 sums.
 *   1  emit_point as the kernels call it (csrc/qn_tick.cuh): blocks of 256 lanes = 4 waves, the block's pose pair in LDS with G = Rx Rx^T from pose_gram, the
 *      transpose buffers and wave rows in LDS of AccumulateK::run's sizes.  n = blocks, arg = trips per lane, 1 .. 4; `first` is true on the first trip only.
 *      in per block (25 + arg x 256 x 13): Rx (12), Tx (12), lin, then per trip and lane, lane fastest: have, pa (3), pb (3), na (3), nb (3) - a lane with
 *      have = 0 hands its record over as it is.  out per block (5 x 28): the four wave rows as emit_point left them, then their sum in wave order.
 *   2  reduce_rows (csrc/qn_gicp_kernels.cuh).  n = rows, arg = NT + COHERENT: 256, 257, 512 or 513.  in: n x 28.  out: the 28 sums.
 * QN_ERR_INVALID_ARG with nothing launched and nothing written: a null pointer, which outside 0 .. 2, an arg other than the above, n above
 * QN_DEBUG_LINEARIZE_MAX_POINTS / _MAX_BLOCKS / _MAX_ROWS.  n == 0 succeeds and writes nothing.  Nothing on a product path calls it. */
#define QN_DEBUG_LINEARIZE_WHICH 3
#define QN_DEBUG_LINEARIZE_MAX_POINTS (1u << 20)
#define QN_DEBUG_LINEARIZE_MAX_BLOCKS (1u << 11)
#define QN_DEBUG_LINEARIZE_MAX_ROWS (1u << 16)
int  qn_debug_linearize(qn_ctx*, int which, const double* in, uint32_t n, uint32_t arg, double* out);
/* developer / tests: the result sinks, pruning bounds, candidate streams and cooperative searches of csrc/qn_device.cuh, called as they are on caller-supplied
 * records (csrc/qn_search_debug.hip).  grid: 0 / 1, the source / target grid the context built for the cloud last set (fix the cell edge with the knob "cell");
 * which 1 and 3 need none.  Host arrays of packed 32-bit words, floats as their bits; one wave of 64 lanes per block.
 *   0  the grid as the device built it.  n = its points, arg = its padded cell count (tiles x 128).  out: cell_start (arg + 1), then per sorted point x, y, z and
 *      the original index.
 *   1  Best1.  n = waves, arg = S | UNIQUE << 8 | L << 16: L consider<UNIQUE> steps, then finish<S>, S one of 1, 2, 4.  in per wave: L x 64 x (on, d2, idx), lane
 *      fastest, then the 64 `on` of finish.  out per lane: key low, key high, second, bd.
 *   2  the bounds.  n = records, arg = 0.  in (8): tile tx, ty, tz, query x, y, z, radius r, face offset f.  out (16): tile_box_d2 | cap_of's o2 x, y, z and S |
 *      cap_extent(r) axis 0, 1, 2 | cap_face_dist(f) axis 0, 1, 2 | cell_coord x, y, z | cell_key of that cell | 0.
 *   3  divmod_small against / and % on the device: every n < 2^22 for d <= 128, and for every d < 2^22 the values 0, d - 1, d, 2^22 - 1, the largest multiple of d
 *      below 2^22 and that +- 1.  n = arg = 0.  out: three 64-bit words - mismatches, pairs compared, the smallest mismatching n << 22 | d (all ones: none).
 *   4  stream_box.  n = waves, arg = recorded candidates a wave at most.  in per wave (12): x0, x1, y0, y1, z0, z1 (cells, inclusive), mode (0 rows, 1 tiles, 2
 *      tiles pruned by the ball), ball centre x, y, z, ball_r2, 0.  out per wave (4 + arg): candidates delivered, overflow (1: more than arg, the rest dropped),
 *      the stream's return value, 0, then the original index of every candidate in delivery order.
 *   5  wave_search<4, Best1>.  n = queries, 16 a wave, arg = max_rounds.  in per query (8): x, y, z, first radius, r_cap (+inf: none), active, 0, 0.  out per
 *      query (8): key low, key high, second, d_unseen, certified, the radius left in r, 0, 0.
 *   6  wave_search_single.  n = queries, one a wave, arg = 0.  in per query (8): x, y, z, first radius, r_cap (+inf, or finite and >= the first radius), 0, 0,
 *      0.  out (8): key low, key high, second, d_unseen, then its SingleStats: rounds, candidates scanned, segments enumerated, the last radius.
 *   7  wave_search_far16.  n = slots, a multiple of 16, 16 a wave, arg = 0.  in per slot (8): x, y, z, radius, member, 0, 0, 0.  out (8): key low, key high, second,
 *      d_unseen, member, 0 ...
 *   8  BestK<KMAX>.  n = waves, arg = KMAX | k << 8 | S << 14 | L << 17: KMAX one of 16, 20, 24, 32 (the four the product instantiates), 1 <= k <= KMAX, L
 *      consider steps (the lazy queue: the whole wave flushes when one lane's queue holds QN_PEND_CAP), then finish<S>, S 1 or 4.  in: as 1.  out per lane
 *      (2 k + 4): the k real entries ascending (key low, key high; all ones: none), w low, w high, found(), 0.
 *   9  wave_search<4, BestK<KMAX>>.  n = queries, 16 a wave, arg = max_rounds | KMAX << 8 | k << 16.  in: as 5.  out per query (2 k + 4): the k entries
 *      ascending, d_unseen, certified, the radius left in r, found().
 *  10  lane_ball_knn<KMAX>, one query per lane.  n = queries, arg = KMAX | k << 8.  in per query (8): x, y, z, first radius, 0 ...  out per query (2 k + 4): the
 *      k entries ascending, found(), 0, 0, 0.
 *  11  build_clusters<S> with stream_clusters<S>: a first walk, then a REUSE second walk of the same clusters.  n = waves, arg = cap | S << 24, S 1 or 4.  in
 *      per lane (8): x, y, z, r, todo, 0 .. (S = 4: the lanes l, l + 16, l + 32, l + 48 hold the same record).  out per wave: header (8): clusters, segments, the
 *      first and the second walk's return value, overflow, 0 ..; then per lane (4 + 2 cap): cluster id, its box's tile mode, accepted in walk 1, in walk 2, then
 *      the original indices the lane accepted under the callers' predicate `mine && in_tile && ccid == cid`, in delivery order: walk 1 (cap), walk 2 (cap).
 *  12  the ball walks of csrc/qn_quatro_kernels.cuh.  n = queries, arg = cap | variant << 24: 0 for_each_in_ball_cells (a query per lane), 1
 *      for_each_in_ball_cells_group<8>, 2 / 3 for_each_in_ball_cells_group_pre<8 | 16> (8 / 16 lanes a query, the group's QN_SEG_CAP table in LDS).  in per
 *      query (8): x, y, z, r, on, 0 ..  out per lane, whole waves (2 + cap): delivered, overflow, then the sorted position of every point body() saw, in order.
 * Everything is checked on the host before any launch; QN_ERR_INVALID_ARG with nothing launched and nothing written: a null pointer, which or grid out of range,
 * a count of 0 or above QN_DEBUG_SEARCH_MAX_WAVES / _MAX_QUERIES / _MAX_STEPS (L) / _MAX_RECORDED (arg of 4), more than _MAX_WORDS words in and out together,
 * a non-finite coordinate, a radius that is not finite and > 0, max_rounds outside 1 .. 64, a KMAX other than the four, k outside 1 .. KMAX, a tile or box outside the grid, a tile-mode box not widened to
 * whole tiles, n or arg of 0 other than the grid's.  QN_ERR_NOT_READY: the context has no grid for that cloud; QN_ERR_EMPTY_CLOUD: the grid is empty (non-finite
 * cloud).  Non-finite queries are refused.  By grep for finite_q, the product callers that screen them before they search are k_nn_search's grouped list
 * pass (wave_search_far16) and k_tick; the queries of the k-NN kernels are the cloud's own points, finite because the grid build empties a cloud
 * that holds another.  NOT screened: k_nn_search's first pass (wave_search<4>) and its one-entry-per-wave list pass (wave_search_single) hand a query over as
 * the pose made it and rely on the searches' own `r == r` exits - those exits are not reached through this entry point.  Nothing on a product path calls it. */
#define QN_DEBUG_SEARCH_WHICH 13
#define QN_DS_DUMP 0
#define QN_DS_BEST1 1
#define QN_DS_BOUNDS 2
#define QN_DS_DIVMOD 3
#define QN_DS_STREAM_BOX 4
#define QN_DS_WAVE_SEARCH1 5
#define QN_DS_WAVE_SEARCH_SINGLE 6
#define QN_DS_WAVE_SEARCH_FAR16 7
#define QN_DS_BESTK 8
#define QN_DS_WAVE_SEARCH_K 9
#define QN_DS_LANE_BALL_KNN 10
#define QN_DS_STREAM_CLUSTERS 11
#define QN_DS_BALL_CELLS 12
#define QN_DEBUG_SEARCH_MAX_WAVES (1u << 12)
#define QN_DEBUG_SEARCH_MAX_QUERIES (1u << 16)
#define QN_DEBUG_SEARCH_MAX_STEPS 64u
#define QN_DEBUG_SEARCH_MAX_RECORDED (1u << 16)
#define QN_DEBUG_SEARCH_MAX_WORDS (1u << 26)
int  qn_debug_search(qn_ctx*, int which, int grid, const void* in, uint32_t n, uint32_t arg, void* out);
/* developer / tests: the device builds of what the map units share (csrc/qn_map_compact.cuh: the wave and block folds, the key walk, the slot folds, the row
 * scan, the block rank; csrc/qn_union_find.cuh: the two linkers; csrc/qn_dense_grid.cuh: the dense grid's index, tile and rim arithmetic) on caller-supplied inputs, on the store's stream with the store's scratch
 * (csrc/qn_map_selftest.hip).  Host arrays, packed, little endian; a block is 256 lanes = 4 waves of 64; u64 / i64 fields are 8-byte aligned in their records:
 *   0  wave_sum / wave_min / wave_max.  n = blocks, arg = 0.  in per lane (32 B): {i32 i; u32 u; f32 f; u32 0; u64 q; i64 s}.  out per wave (64 B), what lane 0
 *      holds: {i32 min i, max i; u32 sum u, min u, max u; f32 min f, max f; u32 0; u64 sum q, min q; i64 sum s; u64 0}.
 *   1  wave_each_key.  n = blocks, arg = 0: the keys as uint32_t, 1: as int32_t.  in per lane (8 B): {u32 has; u32 key}.  out per lane (24 B): {u32 trip, lead,
 *      key, served; u64 same} - the trip (from 0) that had the lane in its mask with the key, lead and mask the callable was handed there, served = the number
 *      of such trips; trip = lead = 0xffffffff for a lane no trip had - then, after all lanes, a u32 per wave: its trips.
 *   2  block_count / block_sum / block_max.  n = blocks, arg = 0.  in per lane (40 B): {u32 pred (bits 0 .. 4); u32 a[3]; u64 b[3]}.  out per block (232 B):
 *      {u32 count[15], sum32[6], max32[6], again32; u64 sum64[6], max64[6], again64, wide[2]}.  count: block_count of the first K predicates, the results of
 *      K = 1, 2, 3, 4, 5 one after the other; sum32 / max32: block_sum / block_max of the first K of a, K = 1, 2, 3 one after the other; sum64 / max64: the
 *      same of b; again32 / again64: the one-value sum called a second time in the kernel, on a[1] / b[1], behind the __syncthreads() its header asks for;
 *      wide: a[0] and a[1] summed in u64.
 *   3  k_slot_fold / k_slot_max.  n = nb slots.  arg = K: uint32_t sums, K one of 1, 2, 3, 5, 10; 0x100 | K: unsigned long long sums, K one of 1, 2, 3; 0x200:
 *      the uint32_t maximum (K = 1).  in: K nb words, slot b at K b.  out: K words.
 *   4  k_scan_rows.  n = nb, arg = rows, | 0x80000000: in place (cnt == off).  in: rows x nb u32 counts.  out: rows x nb u32 exclusive offsets, then rows u32 totals.
 *   5  block_rank.  n = blocks, arg = 0.  in: 256 keep bytes a block, then a u32 base a block.  out: a u32 per lane.
 *   6  uf_unite, 7 uf_unite_min.  n = nodes, arg = the consecutive edges a lane takes, 1 .. 13 (lane t of 256 a block: the edges [t arg, (t + 1) arg)).  in: u32 m,
 *      u32 forest (0 / 1), the n u32 parents of the starting forest when forest is 1 (else the identity), then m edges {u32 a, b}.  out: the n u32 parents as
 *      the unite launch left them, then the n u32 roots after the flatten by plain loads.
 *   8  the dense grid's geometry (dg_index, oc_ijk, dg_tile_of, dg_in_tile, dg_lane_pos, dg_tile_origin, dg_each_neighbour).  n = W H D voxels, arg = 0.  in: u32
 *      W, H, D, none of them 0.  out per linear index (32 B): {u32 x, y, z of the split; the index rebuilt from them; the voxel's tile; its place in the tile
 *      (the lane that holds it); the LDS position of that place in a tile kept with a one-voxel rim; 0}, then per tile (16 B): {i32 x, y, z of its first voxel;
 *      0}, then the 26 offsets {i32 dx, dy, dz} in the order the neighbourhood walk hands them over.
 * Three launches for 6 and 7: init, unite, flatten.  A second call may start from the parents the first one returned.  QN_ERR_INVALID_ARG with nothing
 * launched and nothing written: a null pointer, which outside 0 .. 8, an arg other than the above, more than QN_DEBUG_MAP_PRIMS_MAX_BLOCKS blocks or rows,
 * more than _MAX_NODES nodes, slots or rows x nb counts, more than _MAX_EDGES edges, an edge with an end >= n, a starting parent[x] > x, (8) a side of 0 or
 * W H D != n.  n == 0 succeeds and writes nothing (6, 7: the two header words are still read).  Nothing on a product path calls it. */
#define QN_DEBUG_MAP_PRIMS_WHICH 9
#define QN_DEBUG_MAP_PRIMS_MAX_BLOCKS (1u << 16)
#define QN_DEBUG_MAP_PRIMS_MAX_NODES (1u << 20)
#define QN_DEBUG_MAP_PRIMS_MAX_EDGES (1u << 20)
int  qn_kf_debug_map_prims(qn_kf_store*, int which, const void* in, uint32_t n, uint32_t arg, void* out);
int  qn_debug_get(qn_ctx*, const char* key, double* value);   /* "verify_mismatches" / "verify_passes" / "verify_first" after qn_debug_set("verify_track", 1); "feat_survivors" / "feat_fallbacks" (matrix-core feature matching) */
int  qn_debug_get_grid(qn_ctx*, int which, double out[8]);
int  qn_debug_get_partials(qn_ctx*, double* out, uint32_t* rows_per_buffer, double* state);   /* developer: both partial-row buffers and both state buffers after an align */
int  qn_debug_get_list_probe(qn_ctx*, unsigned long long* out /* [4 * 16384]: per wave of the last unseeded list pass: slowest entry << 32 | entries, busy time (100 MHz ticks), and of that slowest entry rounds << 48 | segments << 24 | candidates, first radius | neighbour distance as f32 bits (knob list_probe) */);
int  qn_debug_get_persist_clk(qn_ctx*, unsigned long long* out /* 64 x 16 + 16 wall-clock stamps of the latest persistent align */);   /* after qn_debug_set("persist_probe", 1) */
int  qn_debug_get_clk(qn_ctx*, unsigned long long* out /* 256 x 8 + 1024 x 12 device-clock stamps / counters */, uint32_t* n);   /* after qn_debug_set("clk_probe", 1) */

#ifdef __cplusplus
}
#endif
#endif /* QN_ENGINE_H */
