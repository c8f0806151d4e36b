// qn_kf_internal.h - what another translation unit may do with a qn_kf_store (its struct lives in qn_cloud.hip).
// Used by the ray-caster (qn_sim.hip), which writes keyframes straight into the store without host staging, and by the Scan Context
// descriptors (qn_sc.hip), which read the resident keyframes and keep per-store state.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include "../../include/qn_engine.h"

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
// per-store state of another translation unit (slot QN_KF_INT_EXT_SC: qn_sc.hip's descriptors, QN_KF_INT_EXT_QUATRO: the resident Quatro features of
// qn_kf_quatro.inc, QN_KF_INT_EXT_VERIFY: qn_verify.hip's record of the latest multi-pair verification): nullptr until set; the store owns it from
// qn_kf_int_set_ext on and calls `release` from qn_kf_store_destroy once its stream has drained.
#define QN_KF_INT_EXT 3
#define QN_KF_INT_EXT_SC 0
#define QN_KF_INT_EXT_QUATRO 1
#define QN_KF_INT_EXT_VERIFY 2
typedef void (*qn_kf_int_release_fn)(void*);
void* qn_kf_int_ext(const qn_kf_store* s, int which);
void qn_kf_int_set_ext(qn_kf_store* s, int which, void* p, qn_kf_int_release_fn release);
// keyframes ids[0 .. count) each alone in its sensor frame (the identity pose), voxel grid at `leaf`: what qn_kf_assemble({id}, {identity}, leaf) builds,
// through the one voxel-grid pipeline as a batch of `count` submaps.  Every cloud lands in ONE new device allocation (*block, nullptr when all are empty)
// that the caller owns from here on (hipFree); ptr / n / status per keyframe as qn_kf_assemble_batch's.  The store's assemble, map and batch slots are
// not touched.  Two host synchronisations.  ids are not checked.
int qn_kf_int_voxel_each(qn_kf_store* s, const int32_t* ids, uint32_t count, double leaf, float4** block, const float4** ptr, uint32_t* n, int* status);
// qn_verify.hip: what qn_kf_verify_cloud serves for pair j of the latest qn_kf_verify_loop_pairs[_c2f] call.  src / dst: the pair's two clouds (batch segments
// on the GICP path, described clouds on the coarse-to-fine path); stage: 0 nothing registered, 1 T_quatro solved (coarse-to-fine only), 2 the GICP stage ran
// (Tg = its f32 T).  qn_kf_int_verify_record replaces the store's record; qn_kf_int_verify_stale drops it when the clouds it names go away: c2f = 0, the batch
// slot is rebuilt (ids ignored); c2f = 1, keyframes ids[0 .. count) are described again.
struct qn_kf_int_verify_pair { const float4* src; uint32_t ns; const float4* dst; uint32_t nt; int32_t query, cand; int stage; double Tq[16]; float Tg[16]; };
int  qn_kf_int_verify_record(qn_kf_store* s, int c2f, const qn_kf_int_verify_pair* p, uint32_t n);
void qn_kf_int_verify_stale(qn_kf_store* s, int c2f, const int32_t* ids, uint32_t count);
