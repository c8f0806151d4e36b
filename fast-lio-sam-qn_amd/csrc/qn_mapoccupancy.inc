// qn_mapoccupancy.inc - a 3-D occupancy map (occupied, free, unknown) by ray carving on the GPU (qn_kf_map_occupancy, qn_kf_map_occupancy_grid,
// qn_kf_map_occupancy_list, qn_kf_map_occupancy_slice: include/qn_engine.h).  The numpy twin qn_amd/mapoccupancy.py is the specification: every record of a
// listed keyframe is a ray from that entry's corrected sensor position O to the world point W; both ends are quantised once (f64, no contraction, half to even,
// 10 fractional bits of a voxel), and everything behind that is an integer: the voxel walk, the u32 hit and miss counts, the class rule.  Integer adds commute,
// so every byte equals the twin's whatever the order of the atomics.
//   extent    k_oc_extent, grid (tiles of the largest entry of the launch, entries) as k_static_vote's, one record per lane: the record is accepted or skipped
//             (oc_ray: non-finite, near, far - f32, left to right, no fused multiply-add), A and B are formed, a ray end of 2^20 voxels or more raises the
//             capacity flag; the per-axis extremes of c(A) and c(B) by wave_min / wave_max and one integer atomicMin / atomicMax per wave; the five record counts by
//             block_count into the block's slot, k_slot_fold adds the slots up.  One host read: the host derives the grid and refuses before anything grid-sized
//             is allocated.
//   carve     k_oc_carve, the same grid, one ray per lane: oc_ray again (nothing is stored between the passes), then oc_walk, which names no floating-point
//             type: hits[v_n] += 1 and misses[v_i] += 1 for i < n - shell by integer atomicAdd.  All rays of a block belong to one entry and start in the same
//             voxel v_0, the hottest address there is: a wave folds its adds to v_0 into one add of the popcount (one atomic a wave instead of one a lane).  The
//             voxels further out are added to lane by lane; a lane stops after its last miss, n - shell steps, since the end voxel is known without walking.
//   classify  k_oc_classify, one voxel per lane: the class byte, the three class counts (block_count) and the block's hit and miss sums (u64, block_sum) into
//             slots, k_slot_fold adds them up.  One host read.
//   list      OcList, the predicate and the payload of the stable voxel list of qn_dense_grid.cuh (k_dg_list_flag / k_scan_rows / k_dg_list_pick).
//   slice     the largest class over a band of layers: k_dg_slice<uint8_t, op_max> of qn_dense_grid.cuh, one column per lane.
// The grid itself - OcGrid, the index arithmetic, the fixed point's OC_S and OC_COORD_LIMIT, the lookup of the live results - is qn_dense_grid.cuh's, shared with
// the fields over it (qn_mapdistance.inc, qn_maproute.inc, qn_mapfrontier.inc, included behind this file).  qn_mapoccupancy_update.inc, right behind this file,
// brings the resident volume to another list in place with the same walk, classify pass and argument checks (qn_kf_map_occupancy_update).
// Host synchronisations of qn_kf_map_occupancy: two - the extent, the counts.  Integer atomics only, no scratch memory, no dynamically indexed private array.
// Part of qn_staticmap.hip's translation unit (included at its end), the unit that turns a list with poses into per-record ray evidence: the results hang on
// that unit's StaticState and take no slot of their own.  They do not depend on the map slot.
#include <climits>
#include <cstdlib>

namespace {

#define OC_BLOCK MO_BLOCK
#define OC_ONE (1 << OC_S)                               // (OC_S, OC_COORD_LIMIT: qn_dense_grid.cuh)
#define OC_MAX_SIDE (1u << 15)
#define OC_RAY 0
#define OC_NONFINITE 1
#define OC_NEAR 2
#define OC_FAR 3
#define OC_CAPACITY 4

struct OcEntry { const float4* pts; uint32_t n, b0; double P[12]; };          // records, first block slot, the pose's three rows; 112 bytes
// the quantisation, shared by the two passes: the status of record p under pose rows P, and for a ray its fixed-point ends
__device__ __forceinline__ int oc_ray(const float4 p, const double* __restrict__ P, double inv, float lo2, float hi2, int32_t (&A)[3], int32_t (&B)[3]) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return OC_NONFINITE;
  const float d2 = (p.x * p.x + p.y * p.y) + p.z * p.z;
  if (d2 < lo2) return OC_NEAR;
  if (d2 > hi2) return OC_FAR;
  const double x = p.x, y = p.y, z = p.z;
  double o[3], w[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    o[k] = P[4 * k + 3] * inv;
    w[k] = (((P[4 * k] * x + P[4 * k + 1] * y) + P[4 * k + 2] * z) + P[4 * k + 3]) * inv;
    ok = ok && fabs(o[k]) < OC_COORD_LIMIT && fabs(w[k]) < OC_COORD_LIMIT;      // (a NaN fails the comparison)
  }
  if (!ok) return OC_CAPACITY;
#pragma unroll
  for (int k = 0; k < 3; k++) { A[k] = (int32_t)rint(o[k] * 1024.0); B[k] = (int32_t)rint(w[k] * 1024.0); }      // |.| <= 2^30
  return OC_RAY;
}

// ext[0 .. 3) / ext[3 .. 6): the smallest / largest voxel coordinate of a ray end, ext[6]: 1 when a ray end is out of range; slots[5 b ..]: the block's records,
// rays, non-finite, near and far records
__global__ void __launch_bounds__(OC_BLOCK) k_oc_extent(const OcEntry* __restrict__ ents, double inv, float lo2, float hi2, int32_t* __restrict__ ext,
                                                        uint32_t* __restrict__ slots) {
  const OcEntry* E = ents + blockIdx.y;
  const uint32_t n = E->n;
  if (blockIdx.x * OC_BLOCK >= n) return;                            // uniform over the block
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  int st = -1;                                                       // (past the end: counted nowhere)
  int32_t lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < n) {
    int32_t A[3], B[3];
    st = oc_ray(E->pts[i], E->P, inv, lo2, hi2, A, B);
    if (st == OC_RAY) {
#pragma unroll
      for (int k = 0; k < 3; k++) { const int32_t a = A[k] >> OC_S, b = B[k] >> OC_S; lo[k] = min(a, b); hi[k] = max(a, b); }
    }
    if (st == OC_CAPACITY) ext[6] = 1;                               // (a plain store of the same value by whoever finds one)
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { lo[k] = wave_min(lo[k]); hi[k] = wave_max(hi[k]); }
  if ((threadIdx.x & 63) == 0 && lo[0] != INT_MAX) {
#pragma unroll
    for (int k = 0; k < 3; k++) { atomicMin(&ext[k], lo[k]); atomicMax(&ext[3 + k], hi[k]); }
  }
  block_count(slots + 5 * (size_t)(E->b0 + blockIdx.x), st >= 0, st == OC_RAY, st == OC_NONFINITE, st == OC_NEAR, st == OC_FAR);
}

// The walk of one ray a lane, integers only.  Every lane of the wave calls it (ray: this lane has one); all rays of the wave start in the same voxel.
// c, r, D, rem and the step are kept per axis in scalars; D <= 2^31 and r <= D + 2^10 fit 32 bits, their products 64.  FOLD: the wave's adds to v_0 as one
// add of the popcount (false: one a lane like every other voxel - the yardstick of tools/gpu_map_occupancy_time.py --no-fold; the same bytes).  SUB: the
// same walk takes the ray's counts out again (qn_mapoccupancy_update.inc) - every add is 0xFFFFFFFF, -1 mod 2^32, the wave's folded one the popcount times that.
template <bool FOLD, bool SUB = false>
__device__ __forceinline__ void oc_walk(bool ray, const int32_t (&A)[3], const int32_t (&B)[3], const OcGrid G, uint32_t shell, uint32_t* __restrict__ hits,
                                        uint32_t* __restrict__ misses) {
  const int32_t stride[3] = {1, (int32_t)G.W, (int32_t)(G.W * G.H)};
  uint32_t r[3], D[3], rem[3]; int32_t step[3];
  uint32_t n = 0; int32_t lin = 0, lend = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int32_t c = A[k] >> OC_S, e = B[k] >> OC_S;                 // arithmetic shifts: floors
    const bool up = B[k] > A[k];
    D[k] = up ? (uint32_t)B[k] - (uint32_t)A[k] : (uint32_t)A[k] - (uint32_t)B[k];
    rem[k] = (uint32_t)(e > c ? e - c : c - e);
    r[k] = (uint32_t)(up ? (c + 1) * OC_ONE - A[k] : A[k] - c * OC_ONE);
    step[k] = up ? stride[k] : -stride[k];
    lin += (c - G.minc[k]) * stride[k]; lend += (e - G.minc[k]) * stride[k];
    n += rem[k];
  }
  const uint32_t carve = ray && n > shell ? n - shell : 0;           // the voxels v_0 .. v_(carve - 1) get a miss
  constexpr uint32_t one = SUB ? 0xFFFFFFFFu : 1u;
  // v_0 is the same voxel in every lane: one add of the popcount for the wave
  if (FOLD) {
    const unsigned long long first = __ballot(carve > 0);
    if (carve > 0 && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)first) - 1) && (uint32_t)lin < G.cells) atomicAdd(&misses[lin], (uint32_t)__popcll(first) * one);
  }
  if (!ray) return;
  if ((uint32_t)lend < G.cells) atomicAdd(&hits[lend], one);         // (always inside: the extremes made the grid; kept as a guard)
  uint32_t r0 = r[0], r1 = r[1], r2 = r[2], m0 = rem[0], m1 = rem[1], m2 = rem[2];
  const uint32_t D0 = D[0], D1 = D[1], D2 = D[2];
  for (uint32_t i = 0; i < carve; i++) {
    if ((!FOLD || i != 0) && (uint32_t)lin < G.cells) { if (SUB) atomicAdd(&misses[lin], 0xFFFFFFFFu); else atomicAdd(&misses[lin], 1u); }
    // among the axes that still have a step to make, the smallest r / D; a tie goes to the lowest axis
    int b; uint32_t rb, Db;
    if (m0 > 0) { b = 0; rb = r0; Db = D0; } else if (m1 > 0) { b = 1; rb = r1; Db = D1; } else { b = 2; rb = r2; Db = D2; }
    if (m1 > 0 && b < 1 && (unsigned long long)r1 * Db < (unsigned long long)rb * D1) { b = 1; rb = r1; Db = D1; }
    if (m2 > 0 && b < 2 && (unsigned long long)r2 * Db < (unsigned long long)rb * D2) b = 2;
    if (b == 0) { lin += step[0]; r0 += OC_ONE; m0--; }
    else if (b == 1) { lin += step[1]; r1 += OC_ONE; m1--; }
    else { lin += step[2]; r2 += OC_ONE; m2--; }
  }
}

// the grid of k_oc_extent: every ray's hit and misses
template <bool FOLD>
__global__ void __launch_bounds__(OC_BLOCK) k_oc_carve(const OcEntry* __restrict__ ents, double inv, float lo2, float hi2, const OcGrid G, uint32_t shell,
                                                       uint32_t* __restrict__ hits, uint32_t* __restrict__ misses) {
  const OcEntry* E = ents + blockIdx.y;
  const uint32_t n = E->n;
  if (blockIdx.x * OC_BLOCK >= n) return;                            // uniform over the block
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  int32_t A[3] = {0, 0, 0}, B[3] = {0, 0, 0};
  bool ray = false;
  if (i < n) ray = oc_ray(E->pts[i], E->P, inv, lo2, hi2, A, B) == OC_RAY;
  oc_walk<FOLD>(ray, A, B, G, shell, hits, misses);
}

// one voxel per lane: the class byte; cslots[3 b ..] = the block's occupied, free and unknown voxels, tslots[2 b ..] = its hits and misses
__global__ void __launch_bounds__(OC_BLOCK) k_oc_classify(uint32_t cells, const uint32_t* __restrict__ hits, const uint32_t* __restrict__ misses, uint32_t min_hits,
                                                          uint32_t hit_weight, uint8_t* __restrict__ cls, uint32_t* __restrict__ cslots,
                                                          unsigned long long* __restrict__ tslots) {
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  int c = -1;                                                        // (past the end: counted nowhere)
  uint32_t h = 0, m = 0;
  if (i < cells) {
    h = hits[i]; m = misses[i];
    c = (h | m) == 0 ? QN_OCC_UNKNOWN : (h >= min_hits && (unsigned long long)h * hit_weight >= (unsigned long long)m) ? QN_OCC_OCCUPIED : QN_OCC_FREE;
    cls[i] = (uint8_t)c;
  }
  block_count(cslots + 3 * (size_t)blockIdx.x, c == QN_OCC_OCCUPIED, c == QN_OCC_FREE, c == QN_OCC_UNKNOWN);
  block_sum(tslots + 2 * (size_t)blockIdx.x, h, m);
}

// the voxel list (k_dg_list_flag / k_dg_list_pick: qn_dense_grid.cuh): the voxels whose class bit is in the mask, to ijk / h_out / m_out
struct OcList {
  const uint8_t* cls; uint32_t mask; const uint32_t *hits, *misses; uint32_t W, H; DgIjk* ijk; uint32_t *h_out, *m_out;
  __device__ bool keep(uint32_t i) const { return ((mask >> cls[i]) & 1u) != 0; }
  __device__ void put(uint32_t i, size_t j) const { ijk[j] = oc_ijk(i, W, H); h_out[j] = hits[i]; m_out[j] = misses[i]; }
};

// ---------------------------------------------------------------------------------------------------------------- host side
// The occupancy results of the latest successful call (a member of the unit's StaticState)
struct OccState {
  bool live = false;
  DevBuf<uint32_t> hits, misses;
  DevBuf<uint8_t> cls;
  qn_occupancy_grid info;
  std::shared_ptr<struct DistState> dist;                // the distance field of qn_mapdistance.inc (included behind this file, where the type is completed)
  std::shared_ptr<struct FrontierState> frontier;        // the frontier regions of qn_mapfrontier.inc (included last), beside the field: they need only the classes
  std::shared_ptr<struct ViewState> view;                // the view gain of qn_mapview.inc (included behind it), beside them: it needs only the classes too
  std::shared_ptr<struct OccLedger> ledger;              // who contributed what to the counts (qn_mapoccupancy_update.inc, included behind this file); only
};                                                       // qn_kf_map_occupancy_update leaves one, a successful qn_kf_map_occupancy drops it
void md_end(DistState*);                                 // (qn_mapdistance.inc) a new occupancy result ends the field of the previous one; its buffers stay
void mf_end(FrontierState*);                             // (qn_mapfrontier.inc) and the frontier regions of the previous one
void mv_end(ViewState*);                                 // (qn_mapview.inc) and its view gain

// Every argument of qn_kf_map_occupancy and qn_kf_map_occupancy_update (but the outputs), checked before anything runs: QN_ERR_INVALID_ARG, or QN_ERR_CAPACITY
// at 2^32 records; QN_OK: ent[e] = the records and the pose rows of entry e, b0 its first block, *tiles the blocks of all
int oc_check_list(qn_kf_store* s, const int32_t* ids, const double* poses16, uint32_t count, const qn_occupancy_params* params, std::vector<OcEntry>& ent,
                  uint64_t* tiles) {
  if (!s || !ids || !poses16 || count == 0 || !params) return QN_ERR_INVALID_ARG;
  const qn_occupancy_params& P = *params;
  if (!std::isfinite(P.voxel) || !(P.voxel > 0.0) || !std::isfinite(P.min_range) || !(P.min_range >= 0.0) || !std::isfinite(P.max_range) ||
      !(P.max_range > P.min_range) || P.min_hits < 1 || P.hit_weight < 1 || P.reserved[0] != 0 || P.reserved[1] != 0 || P.reserved[2] != 0)
    return QN_ERR_INVALID_ARG;
  const size_t n_kf = qn_kf_int_count(s);
  for (uint32_t e = 0; e < count; e++) {
    if (ids[e] < 0 || (size_t)ids[e] >= n_kf) return QN_ERR_INVALID_ARG;
    for (int k = 0; k < 16; k++) if (!std::isfinite(poses16[16 * (size_t)e + k])) return QN_ERR_INVALID_ARG;
  }
  uint64_t total = 0;
  *tiles = 0;
  ent.resize(count);
  for (uint32_t e = 0; e < count; e++) {
    uint32_t n = 0;
    const float4* pts = qn_kf_int_keyframe(s, ids[e], &n);
    ent[e].pts = pts; ent[e].n = n; ent[e].b0 = (uint32_t)*tiles;
    memcpy(ent[e].P, poses16 + 16 * (size_t)e, sizeof(double) * 12);
    total += n; *tiles += dg_blocks(n);
    if (total > 0xFFFFFFFFull) return QN_ERR_CAPACITY;
  }
  return QN_OK;
}

}  // namespace

extern "C" void qn_occupancy_default_params(qn_occupancy_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->voxel = 0.3; p->min_range = 0.5; p->max_range = 60.0; p->shell = 1; p->min_hits = 1; p->hit_weight = 2;      // interface choices, not measurements
}

extern "C" int qn_kf_map_occupancy(qn_kf_store* s, const int32_t* ids, const double* poses16, uint32_t count, const qn_occupancy_params* params,
                                   qn_occupancy_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!stats_out) return QN_ERR_INVALID_ARG;
  uint64_t tiles = 0;
  std::vector<OcEntry> ent;
  const int ok = oc_check_list(s, ids, poses16, count, params, ent, &tiles);
  if (ok != QN_OK) return ok;
  const qn_occupancy_params P = *params;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  StaticState* unit = nullptr;
  const int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_STATIC, &unit);
  if (rc != QN_OK) return rc;
  if (!unit->occ) unit->occ.reset(new (std::nothrow) OccState());
  if (!unit->occ) return qn_kf_fail(s, "qn_kf_map_occupancy: out of memory");
  OccState* st = unit->occ.get();
  const hipStream_t str = qn_kf_int_stream(s);
  const uint32_t nt = (uint32_t)tiles;
  const double inv = 1.0 / P.voxel;
  const float lo2 = (float)(P.min_range * P.min_range), hi2 = (float)(P.max_range * P.max_range);
  // ---- scratch (0: the entries, 3: the blocks' count slots, 4: the blocks' u64 sums, 5: the extent and every folded sum) and the pinned mirror of 0 and 5.
  // The small block: ext[8] (int32), the five record sums, the three class sums (u32), the two totals (u64 at byte 64)
  const size_t ent_bytes = qn_up16(sizeof(OcEntry) * count), small_bytes = 80;
  OcEntry* d_ent = (OcEntry*)qn_kf_int_scratch(s, 0, ent_bytes);
  uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 5 * std::max<size_t>(nt, 1));
  char* d_small = (char*)qn_kf_int_scratch(s, 5, small_bytes);
  char* h = (char*)qn_kf_int_pinned(s, ent_bytes + 2 * small_bytes);
  if (!d_ent || !d_slots || !d_small || !h) return qn_kf_fail(s, "qn_kf_map_occupancy: scratch allocation failed");
  int32_t* d_ext = (int32_t*)d_small; uint32_t* d_sums = (uint32_t*)(d_small + 32); unsigned long long* d_tot = (unsigned long long*)(d_small + 64);
  memcpy(h, ent.data(), sizeof(OcEntry) * count);
  int32_t* h_init = (int32_t*)(h + ent_bytes);
  memset(h_init, 0, small_bytes);
  for (int k = 0; k < 3; k++) { h_init[k] = INT_MAX; h_init[3 + k] = INT_MIN; }
  char* h_small = h + ent_bytes + small_bytes;
  QN_KFCHK(s, hipMemcpyAsync(d_ent, h, sizeof(OcEntry) * count, hipMemcpyHostToDevice, str));
  QN_KFCHK(s, hipMemcpyAsync(d_small, h_init, small_bytes, hipMemcpyHostToDevice, str));
  // ---- the extent
  if (nt) {
    sv_each_chunk(ent.data(), count, OC_BLOCK, [&](uint32_t a, dim3 grid) {
      hipLaunchKernelGGL(k_oc_extent, grid, dim3(OC_BLOCK), 0, str, (const OcEntry*)(d_ent + a), inv, lo2, hi2, d_ext, d_slots);
    });
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 5>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, nt, d_sums);
    QN_KFCHK(s, hipGetLastError());
  }
  QN_KFCHK(s, hipMemcpyAsync(h_small, d_small, small_bytes, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));                   // sync 1: the extent
  const int32_t* ext = (const int32_t*)h_small; const uint32_t* sums = (const uint32_t*)(h_small + 32);
  if (ext[6]) {
    qn_kf_int_set_error(s, "qn_kf_map_occupancy: a ray end of 2^20 voxels or more from the origin");
    return QN_ERR_CAPACITY;
  }
  qn_occupancy_stats r;
  memset(&r, 0, sizeof(r));
  r.n_records = sums[0]; r.n_rays = sums[1]; r.n_nonfinite = sums[2]; r.n_near = sums[3]; r.n_far = sums[4];
  qn_occupancy_grid info;
  memset(&info, 0, sizeof(info));
  info.voxel = P.voxel;
  if (r.n_rays) {
    uint64_t side[3];
    for (int k = 0; k < 3; k++) side[k] = (uint64_t)((int64_t)ext[3 + k] - (int64_t)ext[k] + 1);
    if (side[0] > OC_MAX_SIDE || side[1] > OC_MAX_SIDE || side[2] > OC_MAX_SIDE || side[0] * side[1] * side[2] > (uint64_t)QN_OCC_MAX_CELLS) {
      qn_kf_int_set_error(s, "qn_kf_map_occupancy: a grid of more than 2^27 voxels (or 2^15 a side)");
      return QN_ERR_CAPACITY;
    }
    for (int k = 0; k < 3; k++) { info.minc[k] = ext[k]; info.origin[k] = (double)ext[k] * P.voxel; }
    info.width = (uint32_t)side[0]; info.height = (uint32_t)side[1]; info.depth = (uint32_t)side[2];
  }
  const OcGrid G = oc_grid(info);
  r.width = info.width; r.height = info.height; r.depth = info.depth;
  const uint32_t cells = G.cells, cb = dg_blocks(cells);
  // ---- from here on the previous result is gone
  st->live = false;
  if (cells) {
    if (!st->hits.grow(s, cells) || !st->misses.grow(s, cells) || !st->cls.grow(s, cells)) return QN_ERR_HIP;
    d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * std::max<size_t>(5 * (size_t)nt, 3 * (size_t)cb));      // (unchanged when it fits: nothing reads the old slots any more)
    unsigned long long* d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * 2 * (size_t)cb);
    if (!d_slots || !d_tslots) return qn_kf_fail(s, "qn_kf_map_occupancy: scratch allocation failed");
    QN_KFCHK(s, hipMemsetAsync(st->hits.p, 0, sizeof(uint32_t) * (size_t)cells, str));
    QN_KFCHK(s, hipMemsetAsync(st->misses.p, 0, sizeof(uint32_t) * (size_t)cells, str));
    // ---- carve, classify and count
    const bool fold = getenv("QN_OCC_NO_FOLD") == nullptr;  // (a measuring switch: the results are the same bytes either way)
    sv_each_chunk(ent.data(), count, OC_BLOCK, [&](uint32_t a, dim3 grid) {
      if (fold) hipLaunchKernelGGL(k_oc_carve<true>, grid, dim3(OC_BLOCK), 0, str, (const OcEntry*)(d_ent + a), inv, lo2, hi2, G, P.shell, st->hits.p, st->misses.p);
      else hipLaunchKernelGGL(k_oc_carve<false>, grid, dim3(OC_BLOCK), 0, str, (const OcEntry*)(d_ent + a), inv, lo2, hi2, G, P.shell, st->hits.p, st->misses.p);
    });
    hipLaunchKernelGGL(k_oc_classify, dim3(cb), dim3(OC_BLOCK), 0, str, cells, (const uint32_t*)st->hits.p, (const uint32_t*)st->misses.p, P.min_hits, P.hit_weight,
                       st->cls.p, d_slots, d_tslots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums + 5);
    hipLaunchKernelGGL((k_slot_fold<unsigned long long, 2>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const unsigned long long*)d_tslots, cb, d_tot);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h_small, d_small, small_bytes, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                 // sync 2: the counts
    const unsigned long long* tot = (const unsigned long long*)(h_small + 64);
    r.occupied = sums[5]; r.free = sums[6]; r.unknown = sums[7];
    r.total_hits = tot[0]; r.total_misses = tot[1];
  }
  st->info = info;
  st->live = true;
  st->ledger.reset();                                       // (the counts are no longer those of an update: the next one starts from nothing)
  md_end(st->dist.get());
  mf_end(st->frontier.get());
  mv_end(st->view.get());
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_occupancy_grid(qn_kf_store* s, qn_occupancy_grid* info_out, uint32_t* hits_out, uint32_t* misses_out, uint8_t* class_out) {
  if (!s || !info_out) return QN_ERR_INVALID_ARG;
  const OccState* o = dg_live(s).occ;
  if (!o) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const size_t cells = dg_cells(g);
  *info_out = g;
  if (!cells || (!hits_out && !misses_out && !class_out)) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  if (hits_out) QN_KFCHK(s, hipMemcpyAsync(hits_out, o->hits.p, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, str));
  if (misses_out) QN_KFCHK(s, hipMemcpyAsync(misses_out, o->misses.p, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, str));
  if (class_out) QN_KFCHK(s, hipMemcpyAsync(class_out, o->cls.p, cells, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_map_occupancy_list(qn_kf_store* s, uint32_t class_mask, uint32_t* n_out, int32_t* ijk_out, uint32_t* hits_out, uint32_t* misses_out) {
  if (!s || !n_out || class_mask == 0 || (class_mask & ~7u)) return QN_ERR_INVALID_ARG;
  const OccState* o = dg_live(s).occ;
  if (!o) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t cells = dg_cells(g);
  *n_out = 0;
  if (!cells) return QN_OK;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  OcList L = {o->cls.p, class_mask, o->hits.p, o->misses.p, g.width, g.height, nullptr, nullptr, nullptr};
  uint32_t* h = (uint32_t*)qn_kf_int_pinned(s, 64);
  const uint32_t* d_off = h ? dg_list_count(s, cells, L) : nullptr;
  if (!d_off) return qn_kf_fail(s, "qn_kf_map_occupancy_list: scratch allocation failed");
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_off + dg_blocks(cells), sizeof(uint32_t), hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  const uint32_t n = h[0];
  *n_out = n;
  if (!n || (!ijk_out && !hits_out && !misses_out)) return QN_OK;
  L.ijk = (DgIjk*)qn_kf_int_scratch(s, 1, sizeof(DgIjk) * (size_t)n);
  L.h_out = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * 2 * (size_t)n);
  if (!L.ijk || !L.h_out) return qn_kf_fail(s, "qn_kf_map_occupancy_list: scratch allocation failed");
  L.m_out = L.h_out + n;
  dg_list_pick(s, cells, L, d_off);
  QN_KFCHK(s, hipGetLastError());
  if (ijk_out) QN_KFCHK(s, hipMemcpyAsync(ijk_out, L.ijk, sizeof(DgIjk) * (size_t)n, hipMemcpyDeviceToHost, str));
  if (hits_out) QN_KFCHK(s, hipMemcpyAsync(hits_out, L.h_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  if (misses_out) QN_KFCHK(s, hipMemcpyAsync(misses_out, L.m_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_map_occupancy_slice(qn_kf_store* s, int32_t iz_lo, int32_t iz_hi, uint8_t* occupancy_out) {
  if (!s || !occupancy_out || iz_lo > iz_hi) return QN_ERR_INVALID_ARG;
  const OccState* o = dg_live(s).occ;
  if (!o) return QN_ERR_NOT_READY;
  return dg_slice<uint8_t, op_max>(s, "qn_kf_map_occupancy_slice", o->info, o->cls.p, iz_lo, iz_hi, (uint8_t)0, occupancy_out);
}
