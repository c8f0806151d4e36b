// qn_mapview.inc - view gain over the 3-D occupancy map on the GPU: the distinct unknown voxels a sensor's rays would pass through from each candidate viewpoint
// (qn_view_default_params, qn_kf_map_view_gain, qn_kf_map_view_grid: include/qn_engine.h).  The numpy twin qn_amd/mapview.py is the specification:
//   viewpoint  A = the occupancy map's fixed point of the world position (f64, every operation rounded on its own, half to even, 10 fractional bits of a voxel);
//              OUTSIDE when a coordinate is not finite, 2^20 voxels or more from the origin, or its voxel c(A) is not in the grid: it casts nothing.
//   ray        B = A + offsets[r], the table being the caller's data (no sine or cosine here); the voxels v_0 = c(A) .. v_n = c(B) of the occupancy walk (a tie to
//              the lowest axis, an origin on a face heading down steps at once) examined in order: outside the grid ESCAPED; steps += 1; class bit in stop_mask
//              BLOCKED; class bit in gain_mask: marked when the layer lies in the band iz_lo .. iz_hi, through += 1 band or not, through == max_through != 0
//              SPENT; v_n examined without an end REACHED.  The four ray ends exclude each other.
//   results    gain[q] = the distinct voxels marked for viewpoint q, cover[v] = the viewpoints that marked voxel v (u32 per voxel, resident), sum cover = sum gain.
// Distinct is a set property and the tallies are integer sums, so every byte equals the twin's whatever the schedule, the pass split or the order of the rays.
// The kernels:
//   origin     k_mv_origin, one viewpoint per lane: the quantisation (oc_voxel of qn_dense_grid.cuh, which also hands out the fixed point itself), the row's
//              status and voxel, the corner of the viewpoint's reach box.  The only floating point of the unit.
//   cast       k_mv_cast, one lane per (viewpoint, ray): the viewpoint is blockIdx.y, the rays run along blockIdx.x, MO_BLOCK a block.  Adjacent rows of the table
//              are adjacent directions, so a wave's rays start in one voxel and diverge slowly.  The step loop is the occupancy walk's, written again: r, D and
//              rem per axis in 32-bit scalars, compared in 64 bits, and per axis the steps left before the grid's face - what detects an escape, which the
//              linear index alone cannot.  A voxel counts once through a bitset per viewpoint of the pass over its reach box - the viewpoint's voxel
//              +- ((max |offset component| >> 10) + 1), clipped to the grid: a sensor's reach, which stays in L2, not the whole volume.  A lane first reads
//              the word plainly: bits are only ever set during a launch and the bitsets are cleared in stream order before it, so a stale read can only say
//              "unset".  Only then does it issue the returning atomicOr, and the lane whose returned word lacks the bit counts the voxel: exactly one lane per
//              (viewpoint, voxel) adds to the viewpoint's gain and 1 to cover[v].  Returned atomics drop the line from L2 and cost a round trip, and repeat
//              visits near the viewpoint are the common case: they stay off the atomic path (PEEK false: always the atomicOr, the yardstick of
//              tools/gpu_map_view_time.py; the same bytes).  The rays' tallies are folded per block (block_count, block_sum) and added to the viewpoint's row
//              by one set of integer atomics a block.
//   stats      k_mv_stats, one voxel per lane: covered, max_cover and the sum in one pass over cover (dg_block_stats / dg_fold_stats of qn_dense_grid.cuh).
// The viewpoints go in passes whose bitsets fit MV_BUDGET bytes of scratch (an untuned constant; at least one viewpoint a pass; QN_VIEW_PASS=<n> in the
// environment caps the viewpoints of a pass, read per call like QN_OCC_NO_FOLD, so that a test can put a pass seam anywhere).  Nothing on the host depends on
// a pass's result: the whole call is one host synchronisation whatever the number of passes.  Integer atomics only, no scratch memory, no dynamically indexed
// private array; plain vector stores and vector atomics only.
// Part of qn_staticmap.hip's translation unit (included after qn_mapfrontier.inc, the last): the result hangs on OccState beside the frontier regions and takes
// no slot of its own; the lookup of the live results, dg_live, is defined here, where every state is complete.
#include <cstdlib>

namespace {

#define MV_BLOCK MO_BLOCK
#define MV_BUDGET ((size_t)32 << 20)                     // bytes of bitsets a pass may hold: an untuned choice
#define MV_MAX_PASS 32768u                               // viewpoints a pass at most: the launch grid's y dimension
#define MV_MAX_VIEWS (1u << 16)
#define MV_MAX_RAYS (1u << 20)
static_assert(sizeof(qn_view_info) == 48 && sizeof(qn_view_params) == 32 && sizeof(qn_view_stats) == 48, "the records of include/qn_engine.h");

// a viewpoint as the cast kernel takes it: its fixed point, whether it casts, and the first voxel of its reach box in grid indices
struct MvView { int32_t A[3]; uint32_t ok; int32_t lo[3]; uint32_t pad; };      // 32 bytes
// the reach and the bitset's shape, the same for every viewpoint: reach voxels each way, a box of sx x sy x sz voxels at most, `words` words a viewpoint
struct MvBox { uint32_t reach, sx, sy, sz, words; };

// one viewpoint per lane: the map's own quantisation of the world position, the row with its status and voxel (everything else zero), the reach box's corner
__global__ void __launch_bounds__(MV_BLOCK) k_mv_origin(uint32_t nq, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t Dd, uint32_t reach,
                                                        MvView* __restrict__ views, qn_view_info* __restrict__ info) {
  const uint32_t q = blockIdx.x * MV_BLOCK + threadIdx.x;
  if (q >= nq) return;
  MvView v; qn_view_info r;
  uint32_t c[3];
  const bool ok = oc_voxel(xyz, q, inv, G, Dd, 0u, &c[0], &c[1], &c[2], v.A);      // (qn_dense_grid.cuh: the one quantisation of a world point)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.ijk[k] = ok ? (int32_t)c[k] : 0;
    v.lo[k] = ok ? max(r.ijk[k] - (int32_t)reach, 0) : 0;            // (reach <= 2^15 + 1)
  }
  v.ok = ok ? 1u : 0u; v.pad = 0;
  r.status = ok ? QN_VIEW_OK : QN_VIEW_OUTSIDE;
  r.gain = r.blocked = r.escaped = r.spent = r.reached = 0; r.reserved = 0; r.steps = 0;
  views[q] = v; info[q] = r;
}

// ---- behind the quantisation: integers only
#define MV_BLOCKED 0
#define MV_ESCAPED 1
#define MV_SPENT 2
#define MV_REACHED 3

// Grid (blocks of rays, viewpoints of the pass), one ray a lane: the walk from the viewpoint's voxel, which lies inside the grid.  c, r, D, rem and the steps
// left before the grid's face (room) are kept per axis in scalars; D <= 2^26 and r <= D + 2^10 fit 32 bits, their products 64.  bits: the pass's bitsets, B.words
// words a viewpoint; a voxel's bit is its place in the viewpoint's reach box, x fastest.
template <bool PEEK>
__global__ void __launch_bounds__(MV_BLOCK) k_mv_cast(const MvView* __restrict__ views, const int32_t* __restrict__ offsets, uint32_t R, const OcGrid G, uint32_t Dd,
                                                      const uint8_t* __restrict__ cls, const MvBox B, uint32_t gmask, uint32_t smask, uint32_t max_through, int32_t band_lo,
                                                      int32_t band_hi, uint32_t* bits, uint32_t* __restrict__ cover, qn_view_info* info) {
  __shared__ uint32_t ends[4];
  __shared__ uint32_t sums[2];
  const MvView V = views[blockIdx.y];
  if (!V.ok) return;                                                 // uniform over the block
  const uint32_t i = blockIdx.x * MV_BLOCK + threadIdx.x;
  const bool ray = i < R;
  int end = -1;                                                      // (past the end of the table: counted nowhere)
  uint32_t steps = 0, gain = 0;
  if (ray) {
    const int32_t o0 = offsets[3 * (size_t)i], o1 = offsets[3 * (size_t)i + 1], o2 = offsets[3 * (size_t)i + 2];
    const int32_t off[3] = {o0, o1, o2};
    const uint32_t side[3] = {G.W, G.H, Dd};
    const int32_t gstride[3] = {1, (int32_t)G.W, (int32_t)(G.W * G.H)}, bstride[3] = {1, (int32_t)B.sx, (int32_t)(B.sx * B.sy)};
    uint32_t r[3], D[3], rem[3], room[3]; int32_t gstep[3], bstep[3];
    int32_t lin = 0, bit = 0, z = 0, zstep = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int32_t a = V.A[k], b = a + off[k];                      // |b| <= 2^30 + 2^25
      const int32_t c = a >> OC_S, e = b >> OC_S;                     // arithmetic shifts: floors
      const bool up = b > a;
      const int32_t g = c - G.minc[k];                                // the grid index, inside the grid
      D[k] = up ? (uint32_t)b - (uint32_t)a : (uint32_t)a - (uint32_t)b;
      rem[k] = (uint32_t)(e > c ? e - c : c - e);
      r[k] = (uint32_t)(up ? (c + 1) * OC_ONE - a : a - c * OC_ONE);
      room[k] = up ? side[k] - 1u - (uint32_t)g : (uint32_t)g;
      gstep[k] = up ? gstride[k] : -gstride[k];
      bstep[k] = up ? bstride[k] : -bstride[k];
      lin += g * gstride[k]; bit += (g - V.lo[k]) * bstride[k];
      if (k == 2) { z = g; zstep = up ? 1 : -1; }
    }
    uint32_t* mine = bits + (size_t)blockIdx.y * B.words;
    uint32_t r0 = r[0], r1 = r[1], r2 = r[2], m0 = rem[0], m1 = rem[1], m2 = rem[2], w0 = room[0], w1 = room[1], w2 = room[2];
    const uint32_t D0 = D[0], D1 = D[1], D2 = D[2];
    uint32_t through = 0;
    for (;;) {
      steps++;
      const uint32_t cb = 1u << cls[lin];
      if (cb & smask) { end = MV_BLOCKED; break; }
      if (cb & gmask) {
        if (z >= band_lo && z <= band_hi) {
          uint32_t* word = mine + ((uint32_t)bit >> 5);
          const uint32_t m = 1u << ((uint32_t)bit & 31u);
          if (!PEEK || (*word & m) == 0) {
            if ((atomicOr(word, m) & m) == 0) { gain++; atomicAdd(&cover[lin], 1u); }
          }
        }
        through++;
        if (through == max_through) { end = MV_SPENT; break; }       // (max_through 0: never, through >= 1 here)
      }
      if ((m0 | m1 | m2) == 0) { end = MV_REACHED; break; }
      // among the axes that still have a step to make, the smallest r / D; a tie goes to the lowest axis
      int b; uint32_t rb, Db;
      if (m0 > 0) { b = 0; rb = r0; Db = D0; } else if (m1 > 0) { b = 1; rb = r1; Db = D1; } else { b = 2; rb = r2; Db = D2; }
      if (m1 > 0 && b < 1 && (unsigned long long)r1 * Db < (unsigned long long)rb * D1) { b = 1; rb = r1; Db = D1; }
      if (m2 > 0 && b < 2 && (unsigned long long)r2 * Db < (unsigned long long)rb * D2) b = 2;
      if (b == 0) { if (w0 == 0) { end = MV_ESCAPED; break; } lin += gstep[0]; bit += bstep[0]; r0 += OC_ONE; m0--; w0--; }
      else if (b == 1) { if (w1 == 0) { end = MV_ESCAPED; break; } lin += gstep[1]; bit += bstep[1]; r1 += OC_ONE; m1--; w1--; }
      else { if (w2 == 0) { end = MV_ESCAPED; break; } lin += gstep[2]; bit += bstep[2]; z += zstep; r2 += OC_ONE; m2--; w2--; }
    }
  }
  // ---- the block's tallies into the viewpoint's row: one set of integer atomics a block
  block_count(ends, end == MV_BLOCKED, end == MV_ESCAPED, end == MV_SPENT, end == MV_REACHED);
  block_sum(sums, steps, gain);
  __syncthreads();
  qn_view_info* row = info + blockIdx.y;
  if (threadIdx.x < 4) { if (ends[threadIdx.x]) atomicAdd(&row->blocked + threadIdx.x, ends[threadIdx.x]); }
  else if (threadIdx.x == 4) { if (sums[1]) atomicAdd(&row->gain, sums[1]); }
  else if (threadIdx.x == 5) atomicAdd((unsigned long long*)&row->steps, (unsigned long long)sums[0]);
}

// one voxel per lane: cslots[3 b ..] = the block's covered voxels (and two unused counts), mslots[b] = its largest cover, tslots[b] = the sum of its covers
__global__ void __launch_bounds__(MV_BLOCK) k_mv_stats(uint32_t cells, const uint32_t* __restrict__ cover, uint32_t* __restrict__ cslots, uint32_t* __restrict__ mslots,
                                                       unsigned long long* __restrict__ tslots) {
  const uint32_t i = blockIdx.x * MV_BLOCK + threadIdx.x;
  const uint32_t c = i < cells ? cover[i] : 0u;
  dg_block_stats(c != 0, false, false, c, cslots, mslots, tslots);
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The view result of the latest successful call (a member of OccState, beside the frontier regions); `live` ends with the occupancy result it was computed from
struct ViewState {
  bool live = false;
  DevBuf<uint32_t> cover;
  qn_view_params params;
};

void mv_end(ViewState* v) { if (v) v->live = false; }

// the lookup every entry point behind qn_kf_map_occupancy starts with (declared in qn_dense_grid.cuh; here all five states are complete)
DgLive dg_live(qn_kf_store* s) {
  DgLive L = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const StaticState* st = (const StaticState*)qn_kf_int_ext(s, QN_KF_INT_EXT_STATIC);
  if (st && st->occ && st->occ->live) L.occ = st->occ.get();
  if (L.occ && L.occ->dist && L.occ->dist->live) L.dist = L.occ->dist.get();
  if (L.dist && L.dist->route && L.dist->route->live) L.route = L.dist->route.get();
  if (L.occ && L.occ->frontier && L.occ->frontier->live) L.frontier = L.occ->frontier.get();
  if (L.occ && L.occ->view && L.occ->view->live) L.view = L.occ->view.get();
  return L;
}

}  // namespace

extern "C" void qn_view_default_params(qn_view_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->gain_mask = 1u << QN_OCC_UNKNOWN; p->stop_mask = 1u << QN_OCC_OCCUPIED; p->max_through = 0; p->iz_lo = 0; p->iz_hi = INT32_MAX;      // interface choices, not measurements
}

extern "C" int qn_kf_map_view_gain(qn_kf_store* s, const double* xyz, uint32_t q, const int32_t* offsets, uint32_t r, const qn_view_params* params,
                                   qn_view_info* info_out, qn_view_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !xyz || !offsets || !params || !info_out || !stats_out || q == 0 || q > MV_MAX_VIEWS || r == 0 || r > MV_MAX_RAYS) return QN_ERR_INVALID_ARG;
  const qn_view_params P = *params;
  if (P.gain_mask == 0 || (P.gain_mask & ~7u) || (P.stop_mask & ~7u) || (P.gain_mask & P.stop_mask) || P.iz_lo > P.iz_hi || P.reserved[0] != 0 || P.reserved[1] != 0 ||
      P.reserved[2] != 0)
    return QN_ERR_INVALID_ARG;
  uint32_t far = 0;                                                  // the largest |offset component|
  for (size_t k = 0; k < 3 * (size_t)r; k++) {
    const int64_t v = offsets[k];
    if (v > QN_VIEW_MAX_OFFSET || v < -(int64_t)QN_VIEW_MAX_OFFSET) return QN_ERR_INVALID_ARG;
    far = std::max(far, (uint32_t)(v < 0 ? -v : v));
  }
  OccState* o = dg_mut(dg_live(s).occ);
  if (!o) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t cells = dg_cells(g), cb = dg_blocks(cells);
  qn_view_stats st_out;
  memset(&st_out, 0, sizeof(st_out));
  st_out.viewpoints = q; st_out.rays = r;
  if (!o->view) o->view.reset(new (std::nothrow) ViewState());
  if (!o->view) return qn_kf_fail(s, "qn_kf_map_view_gain: out of memory");
  ViewState* st = o->view.get();
  if (!cells) {                                                      // no voxel: every viewpoint is OUTSIDE
    memset(info_out, 0, sizeof(qn_view_info) * (size_t)q);
    for (uint32_t k = 0; k < q; k++) info_out[k].status = QN_VIEW_OUTSIDE;
    st_out.outside = q;
  } else {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    const hipStream_t str = qn_kf_int_stream(s);
    // ---- the bitset's shape and the passes
    MvBox B;
    B.reach = (far >> OC_S) + 1;
    B.sx = (uint32_t)std::min<uint64_t>(2 * (uint64_t)B.reach + 1, g.width); B.sy = (uint32_t)std::min<uint64_t>(2 * (uint64_t)B.reach + 1, g.height);
    B.sz = (uint32_t)std::min<uint64_t>(2 * (uint64_t)B.reach + 1, g.depth);
    B.words = (uint32_t)(((uint64_t)B.sx * B.sy * B.sz + 31) / 32);      // at most 2^27 bits: the grid's
    const size_t vbytes = sizeof(uint32_t) * (size_t)B.words;
    uint32_t per = (uint32_t)std::min<size_t>(std::max<size_t>(MV_BUDGET / vbytes, 1), std::min<uint32_t>(q, MV_MAX_PASS));
    if (const char* cap = getenv("QN_VIEW_PASS")) {                  // (a testing switch: the results are the same bytes whatever the split)
      const long n = atol(cap);
      if (n >= 1) per = (uint32_t)std::min<long>(n, (long)per);
    }
    const bool peek = getenv("QN_VIEW_NO_PEEK") == nullptr;         // (a measuring switch: the same bytes either way)
    // ---- a larger cover volume is allocated beside the previous one, which goes only once the new one is there
    DevBuf<uint32_t> nc;
    if (!st->cover.grow_beside(s, cells, nc)) return QN_ERR_HIP;
    // ---- scratch (0: the viewpoints' positions; 1: the ray table; 2: the viewpoints as the cast kernel takes them; 3: the blocks' three counts, then their
    //      largest cover; 4: their u64 sums; 5: the folded sums - covered, two unused, max_cover and total_gain at byte 16; 6: the pass's bitsets; 7: the rows)
    DgPoints pts;
    const int rc = dg_points(s, "qn_kf_map_view_gain", xyz, q, &pts);
    if (rc != QN_OK) return rc;
    int32_t* d_off = (int32_t*)qn_kf_int_scratch(s, 1, sizeof(int32_t) * 3 * (size_t)r);
    MvView* d_views = (MvView*)qn_kf_int_scratch(s, 2, sizeof(MvView) * (size_t)q);
    uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 4 * (size_t)cb);
    unsigned long long* d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * (size_t)cb);
    char* d_small = (char*)qn_kf_int_scratch(s, 5, 32);
    uint32_t* d_bits = (uint32_t*)qn_kf_int_scratch(s, 6, vbytes * per);
    qn_view_info* d_info = (qn_view_info*)qn_kf_int_scratch(s, 7, sizeof(qn_view_info) * (size_t)q);
    char* h = (char*)qn_kf_int_pinned(s, 32);
    if (!d_off || !d_views || !d_slots || !d_tslots || !d_small || !d_bits || !d_info || !h) return qn_kf_fail(s, "qn_kf_map_view_gain: scratch allocation failed");
    // ---- from here on the previous result is gone
    st->live = false;
    st->cover.adopt(nc);
    const OcGrid G = oc_grid(g);
    const DgBand band = dg_band(P.iz_lo, P.iz_hi, g.depth);
    QN_KFCHK(s, hipMemcpyAsync(d_off, offsets, sizeof(int32_t) * 3 * (size_t)r, hipMemcpyHostToDevice, str));
    QN_KFCHK(s, hipMemsetAsync(st->cover.p, 0, sizeof(uint32_t) * (size_t)cells, str));
    hipLaunchKernelGGL(k_mv_origin, pts.grid, dim3(MV_BLOCK), 0, str, q, pts.xyz, 1.0 / g.voxel, G, g.depth, B.reach, d_views, d_info);
    // ---- the passes: clear the bitsets, cast
    for (uint32_t q0 = 0; q0 < q; q0 += per) {
      const uint32_t nq = std::min(per, q - q0);
      QN_KFCHK(s, hipMemsetAsync(d_bits, 0, vbytes * nq, str));
      const dim3 grid(dg_blocks(r), nq);
      if (peek) hipLaunchKernelGGL(k_mv_cast<true>, grid, dim3(MV_BLOCK), 0, str, (const MvView*)(d_views + q0), (const int32_t*)d_off, r, G, g.depth, (const uint8_t*)o->cls.p, B,
                                   P.gain_mask, P.stop_mask, P.max_through, band.lo, band.hi, d_bits, st->cover.p, d_info + q0);
      else hipLaunchKernelGGL(k_mv_cast<false>, grid, dim3(MV_BLOCK), 0, str, (const MvView*)(d_views + q0), (const int32_t*)d_off, r, G, g.depth, (const uint8_t*)o->cls.p, B,
                              P.gain_mask, P.stop_mask, P.max_through, band.lo, band.hi, d_bits, st->cover.p, d_info + q0);
      st_out.passes++;
    }
    // ---- the statistics of the cover volume
    hipLaunchKernelGGL(k_mv_stats, dim3(cb), dim3(MV_BLOCK), 0, str, cells, (const uint32_t*)st->cover.p, d_slots, d_slots + 3 * (size_t)cb, d_tslots);
    dg_fold_stats(str, d_slots, d_tslots, cb, d_small);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(info_out, d_info, sizeof(qn_view_info) * (size_t)q, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipMemcpyAsync(h, d_small, 32, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                   // the one sync: the rows and the statistics
    const uint32_t* sums = (const uint32_t*)h;
    st_out.covered = sums[0]; st_out.max_cover = sums[3];
    memcpy(&st_out.total_gain, h + 16, sizeof(st_out.total_gain));
    for (uint32_t k = 0; k < q; k++) { st_out.outside += info_out[k].status == QN_VIEW_OUTSIDE; st_out.steps += info_out[k].steps; }
  }
  st->params = P;
  st->live = true;
  *stats_out = st_out;
  return QN_OK;
}

extern "C" int qn_kf_map_view_grid(qn_kf_store* s, qn_occupancy_grid* info_out, qn_view_params* params_out, uint32_t* cover_out) {
  if (!s || !info_out || !params_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.view) return QN_ERR_NOT_READY;
  const size_t cells = dg_cells(L.occ->info);
  *info_out = L.occ->info; *params_out = L.view->params;
  if (!cells || !cover_out) return QN_OK;
  return qn_kf_download(s, cover_out, L.view->cover.p, sizeof(uint32_t) * cells);
}
