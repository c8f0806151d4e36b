// qn_kf_internal.h - what another translation unit may do with a qn_kf_store (its struct lives in qn_cloud.hip).
// Used by the ray-caster (qn_sim.hip), which writes keyframes straight into the store without host staging, and by the Scan Context
// descriptors (qn_sc.hip), which read the resident keyframes and keep per-store state.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "../../include/qn_engine.h"

// the owned buffers of the store and of every unit around it (qn_kf_buf.h, with the error macro and the get-or-create of a unit's state)
template <typename T, bool kPinned> struct KfBuf;
template <typename T> using DevBuf = KfBuf<T, false>;                            // device memory
template <typename T> using PinBuf = KfBuf<T, true>;                             // pinned host memory

int  qn_kf_int_device(const qn_kf_store* s);
hipStream_t qn_kf_int_stream(const qn_kf_store* s);
size_t qn_kf_int_count(const qn_kf_store* s);                                    // keyframes stored so far
void qn_kf_int_set_error(qn_kf_store* s, const char* msg);
// per-store scratch buffer `which` (0 .. QN_KF_INT_SCRATCH - 1) of at least `bytes`; grown only, freed with the store.  nullptr on failure.
#define QN_KF_INT_SCRATCH 8
void* qn_kf_int_scratch(qn_kf_store* s, int which, size_t bytes);
void* qn_kf_int_pinned(qn_kf_store* s, size_t bytes);                           // one pinned host buffer, same rules
// the adopt path of qn_kf_add_device without its final synchronisation: allocates the keyframe's float4 buffer and enqueues the copy of
// n records (xyz at 0, intensity at ioff, ioff < 0: none) on the store's stream; *out = the new buffer (nullptr when n == 0).
int  qn_kf_int_copy_async(qn_kf_store* s, const void* d_pts, uint32_t n, uint32_t stride, int32_t ioff, float4** out);
// append keyframes whose buffers were made by qn_kf_int_copy_async (after the stream has been synchronised); ids are consecutive.
void qn_kf_int_append(qn_kf_store* s, float4* const* bufs, const uint32_t* n, uint32_t count, bool has_i, int32_t* ids_out);
// the resident float4 records of keyframe `id` (0 <= id < qn_kf_int_count; not checked) and their number (nullptr when n == 0)
const float4* qn_kf_int_keyframe(const qn_kf_store* s, int32_t id, uint32_t* n);
bool qn_kf_int_has_intensity(const qn_kf_store* s, int32_t id);                  // added by qn_kf_add_xyzi / with an intensity offset: .w is the intensity
// per-store state of another translation unit (slot QN_KF_INT_EXT_SC: qn_sc.hip's descriptors, QN_KF_INT_EXT_QUATRO: the resident Quatro features of
// qn_kf_quatro.inc, QN_KF_INT_EXT_VERIFY: qn_verify.hip's record of the latest multi-pair verification, QN_KF_INT_EXT_SUBMAP: the resident local submaps of
// qn_kf_submap.inc): nullptr until set; the store owns it from qn_kf_int_set_ext on and calls `release` from qn_kf_store_destroy once its stream has drained.
// Units reach their state through qn_kf_ext_state (qn_kf_buf.h), which makes it on first use.
#define QN_KF_INT_EXT 10
#define QN_KF_INT_EXT_SC 0
#define QN_KF_INT_EXT_QUATRO 1
#define QN_KF_INT_EXT_VERIFY 2
#define QN_KF_INT_EXT_SUBMAP 3
#define QN_KF_INT_EXT_OVERLAP 4                                                  // qn_overlap.hip: the per-point results of the latest overlap call
#define QN_KF_INT_EXT_RANGE 5                                                    // qn_freespace.hip: range images and the classes of the latest check
#define QN_KF_INT_EXT_STATIC 6                                                   // qn_staticmap.hip: the list, votes and kept records of the latest static classify
#define QN_KF_INT_EXT_NORMALS 7                                                  // qn_mapnormals.hip: the normals and moments of the map slot
#define QN_KF_INT_EXT_OUTLIERS 8                                                 // qn_mapoutliers.hip: the classification of the map slot's points, and the clusters of qn_mapclusters.inc
#define QN_KF_INT_EXT_GROUND 9                                                   // qn_mapground.hip: the ground classes and the occupancy grid of the map slot
typedef void (*qn_kf_int_release_fn)(void*);
void* qn_kf_int_ext(const qn_kf_store* s, int which);
void qn_kf_int_set_ext(qn_kf_store* s, int which, void* p, qn_kf_int_release_fn release);
// keyframes ids[0 .. count) each alone in its sensor frame (the identity pose), voxel grid at `leaf`: what qn_kf_assemble({id}, {identity}, leaf) builds,
// through the one voxel-grid pipeline as a batch of `count` submaps.  Every cloud lands in ONE new device allocation (block, the caller's; empty when all clouds are,
// or on an error return); ptr / n / status per keyframe as qn_kf_assemble_batch's.  The store's assemble, map and batch slots are
// not touched.  Two host synchronisations.  ids are not checked.
int qn_kf_int_voxel_each(qn_kf_store* s, const int32_t* ids, uint32_t count, double leaf, DevBuf<float4>& block, const float4** ptr, uint32_t* n, int* status);
// the general form: submap t = keyframes ids[seg_off[t] .. seg_off[t + 1]) with the poses of the same entries (row-major 4x4 f64), what qn_kf_assemble_batch builds
// for those lists - the same pipeline, the same bytes - but into ONE new allocation the caller owns (as above) instead of the store's batch slot.
int qn_kf_int_voxel_windows(qn_kf_store* s, const int32_t* ids, const double* poses, const uint32_t* seg_off, uint32_t n_seg, double leaf,
                            DevBuf<float4>& block, const float4** ptr, uint32_t* n, int* status);
// qn_verify.hip: what qn_kf_verify_cloud serves for pair j of the latest multi-pair verification.  src / dst: the pair's two clouds (batch segments on the
// GICP path, described clouds on the coarse-to-fine path, resident local submaps on the two submap paths); stage: 0 nothing registered, 1 T_quatro solved
// (coarse-to-fine only), 2 the GICP stage ran (Tg = its f32 T).  qn_kf_int_verify_record replaces the store's record; `kind` says which call made it.
// qn_kf_int_verify_stale drops it when the clouds it names go away.  from = where those clouds live: QN_KF_VERIFY_FROM_BATCH, the batch slot is rebuilt (ids
// ignored); _FROM_SCANS / _FROM_SUBMAPS, the scan / local-submap entries of keyframes ids[0 .. count) are replaced or released (ids == nullptr: all of them).
#define QN_KF_VERIFY_GICP 0
#define QN_KF_VERIFY_C2F 1
#define QN_KF_VERIFY_SUBMAP 2
#define QN_KF_VERIFY_SUBMAP_C2F 3
#define QN_KF_VERIFY_MAP 4                                                       // qn_kf_map_localize (qn_maplocalize.inc): cand = -1, src = the scan cloud, dst = the crop
#define QN_KF_VERIFY_MAP_C2F 5
#define QN_KF_VERIFY_FROM_BATCH 0
#define QN_KF_VERIFY_FROM_SCANS 1
#define QN_KF_VERIFY_FROM_SUBMAPS 2
#define QN_KF_VERIFY_FROM_MAP 3                                                  // copies the verify unit owns itself: only the next crop or localise call ends them
struct qn_kf_int_verify_pair { const float4* src; uint32_t ns; const float4* dst; uint32_t nt; int32_t query, cand; int stage; double Tq[16]; float Tg[16]; };
int  qn_kf_int_verify_record(qn_kf_store* s, int kind, const qn_kf_int_verify_pair* p, uint32_t n);
void qn_kf_int_verify_stale(qn_kf_store* s, int from, const int32_t* ids, uint32_t count);
// a pair of the coarse-to-fine batch whose clouds and FPFH rows are resident already: the lane borrows both sides and builds no grid and no feature
struct C2fCached { float4* src_pts; float* src_rows; float4* dst_pts; float* dst_rows; };
// qn_coarse_to_fine_align_batch on one context (qn_quatro_host.inc) that also says how far each pair got (stage 0, 1 = T_quatro solved, 2 = the fine stage
// ran); cached (or null): per pair, the resident points and rows its lane borrows
int qn_ctx_int_c2f_batch_stage(qn_ctx* ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr, qn_gicp_result* results, double* T_total, double* T_quatro,
                               int* valid, int* status, const C2fCached* cached, int* stage);
// The one pair driver behind every loop-verification entry point (qn_verify.hip).  A job = one pair whose clouds exist: src / dst (device float4, nullptr when
// empty), query / cand for the record, group = the query's place among the call's distinct queries, pre = QN_OK "give it to the batch" or the status the pair
// reports without running, guess = the f32 seed of the GICP form, src_rows / dst_rows = the resident FPFH rows of the coarse-to-fine form (nullptr: the lanes
// make their own; when any job of a call has rows, every job's are lent).  qn_kf_int_verify_run fills every output with what a registration that did not run
// reports, submits the QN_OK jobs stable-sorted by group (caller order within a query) to ONE qn_gicp_align_batch_guess or ONE coarse-to-fine batch, scatters
// the records back to caller order and replaces the store's verify record with one of `kind` (QN_KF_VERIFY_KEEP: the store's record is left alone).
// T_total (coarse-to-fine: required) / T_quatro may be nullptr.  When the batched run itself fails, nothing has been written and the record is not replaced.
#define QN_KF_VERIFY_KEEP (-1)
struct qn_kf_int_verify_job {
  const float4* src; uint32_t ns; const float4* dst; uint32_t nt; int32_t query, cand; uint32_t group; int pre;
  float guess[16]; float* src_rows; float* dst_rows;
};
int qn_kf_int_verify_run(qn_kf_store* s, qn_ctx* ctx, const qn_kf_int_verify_job* jobs, uint32_t n, double score_thr, bool c2f, int kind,
                         qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status);
// the distinct ids of ids[0 .. n) in order of first appearance (appended to u) and each entry's place in that list
inline void qn_kf_int_distinct(const int32_t* ids, uint32_t n, std::vector<int32_t>& u, std::vector<uint32_t>& place) {
  place.resize(n);
  for (uint32_t j = 0; j < n; j++) {
    uint32_t k = 0;
    while (k < u.size() && u[k] != ids[j]) k++;
    if (k == u.size()) u.push_back(ids[j]);
    place[j] = k;
  }
}
// the window lists of `count` centres, appended to ids / rel / seg (seg gets one end offset per centre): window of c = keyframes c - range .. c + range
// inside the poses, keyframe i with inv(P_c) P_i (qn_kf_int_relative_pose).  keep_newest = false is the reference's `i < keyframes.size() - 1`
// (loop_closure.cpp:98-104), true the local submap's `i < n_poses`.  QN_ERR_INVALID_ARG for a window member that is no keyframe (i >= n_kf).
int qn_kf_int_windows(const int32_t* centres, uint32_t count, const double* poses, uint32_t n_poses, size_t n_kf, uint32_t range, bool keep_newest,
                      std::vector<int32_t>& ids, std::vector<double>& rel, std::vector<uint32_t>& seg);
// the pose and seed arithmetic qn_kf_verify_loop_candidates documents (include/qn_engine.h): Q = inv(Pc) Pi with inv(P) = [R^T | -R^T t], every entry summed
// in order in f64; g = Rz(-yaw) from the C library's cos / sin in f64, each entry rounded to f32.  Twins: scancontext.relative_pose / seed_from_yaw.
void qn_kf_int_relative_pose(const double* Pc, const double* Pi, double* Q);
void qn_kf_int_seed_from_yaw(double yaw, float* g);
// qn_kf_verify_cloud(pair, QN_VERIFY_FINAL) without its synchronisation: the launch is enqueued on the store's stream and the pointer is good for work
// enqueued there afterwards (qn_overlap.hip measures many pairs per call and may not synchronise once per pair).  Same statuses, same buffer, same lifetime.
int qn_kf_int_verify_final_async(qn_kf_store* s, uint32_t pair, const float4** d_xyz, uint32_t* n);
uint32_t qn_kf_int_verify_pairs(const qn_kf_store* s);                            // pairs of the live verify record, 0 when there is none
// A sorted-key cell index over `count` device clouds (float4; clouds[k] may be nullptr when n[k] == 0), built by the front half of the store's voxel-grid
// pipeline (qn_cloud.hip) with every cloud as its own segment: *points = the clouds concatenated (cloud k at grids[k].p0), *keys = one 64-bit key per point,
// ((prefix | cell) << 32 | position in *points), sorted inside every cloud's range [p0, p0 + n) by cell, a cell's points in ascending original order, the
// non-finite points behind the n_finite finite ones.  cell = cx + cy div[0] + cz div[0] div[1] with c = (int)(floorf(x * inv) - (float)minb); the cell edge
// is >= radius with the margin that makes the 3 x 3 x 3 block around a query's cell hold every point within radius (argument: qn_cloud.hip).  Enqueued on the
// store's stream after one host synchronisation; the buffers are the pipeline's scratch, good until the next call that runs the pipeline.
struct qn_kf_int_cell_grid { uint32_t p0, n, n_finite, prefix; float inv; int minb[3]; int div[3]; };
int qn_kf_int_cell_index(qn_kf_store* s, const float4* const* clouds, const uint32_t* n, uint32_t count, double radius,
                         qn_kf_int_cell_grid* grids, const float4** points, const unsigned long long** keys);
// the map slot as the latest qn_kf_build_map / qn_kf_build_map_static left it (nullptr and *n = 0 without a map) and its generation, which every attempt to
// build a map advances: what was computed from the slot at another generation is stale.
const float4* qn_kf_int_map(const qn_kf_store* s, uint32_t* n, uint64_t* generation);
// shrinks the map slot to a compacted prefix: its first n_kept records become the n_kept records at d_kept (device memory other than the slot; n_kept <= the
// slot's points, else QN_ERR_INVALID_ARG), copied on the store's stream without a synchronisation, and the generation advances as after a build.  n_kept == 0
// leaves the store without a map.
int qn_kf_int_map_shrink(qn_kf_store* s, const float4* d_kept, uint32_t n_kept);
// qn_kf_build_map with its sources given directly instead of by keyframe id: entry k = n[k] float4 records at pts[k] (device memory of this store's device,
// nullptr when n[k] == 0), has_i[k] = their .w is an intensity (else the map counts it as 0), transformed with poses[16 k ..].  The same pipeline, the same map
// slot, the same statuses and notes: for pts / n / has_i of resident keyframes it IS qn_kf_build_map of their ids.  Arguments are not checked.
int qn_kf_int_build_map_from(qn_kf_store* s, const float4* const* pts, const uint32_t* n, const uint8_t* has_i, const double* poses, uint32_t count, double leaf,
                             const float** d_xyzi_out, uint32_t* n_out);
// qn_mapground.hip: the resident class bytes (one per map point, device memory) of the live qn_kf_map_ground classification if it is that of the map slot as
// it stands, else nullptr (qn_mapclusters.inc reads them for its class mask)
const uint8_t* qn_kf_int_ground_classes(qn_kf_store* s);
