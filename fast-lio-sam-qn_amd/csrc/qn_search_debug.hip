// qn_search_debug.hip - the kernels of qn_debug_search (include/qn_engine.h): the sinks, pruning bounds, candidate streams and cooperative searches of
// qn_device.cuh and the ball walks of qn_ball_walk.cuh, called as they are on the caller's records against a grid the context built.  One wave per block; every record is a row of 32-bit words
// (floats as their bits).  A translation unit of its own: the product kernels are compiled without a line of this.  Test infrastructure
// (tests/test_gpu_search.py): nothing on the registration path calls it.  qn_engine.hip has validated every record before a launch: coordinates and radii
// finite, boxes and tiles inside the grid, counts within the maxima - a kernel here never forms an index from an unchecked word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qn_ball_walk.cuh"

namespace qn {

#define QN_DS_INF __int_as_float(0x7f800000)
__device__ __forceinline__ float dsf(uint32_t w) { return __uint_as_float(w); }
__device__ __forceinline__ uint32_t dsu(float f) { return __float_as_uint(f); }

// ------------------------------------------------------------------ which 0: the grid as the device built it
static __global__ void __launch_bounds__(256) k_dbg_dump(GridView g0, uint32_t ncells, uint32_t npts, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i <= ncells) out[i] = g0.cell_start[i];
  if (i < npts) { const float4 p = g0.pts[i]; uint32_t* o = out + (ncells + 1) + 4 * (size_t)i; o[0] = dsu(p.x); o[1] = dsu(p.y); o[2] = dsu(p.z); o[3] = dsu(p.w); }
}

// ------------------------------------------------------------------ which 1: Best1
// per wave: L steps of 64 x (on, d2, idx), then 64 x the `on` of finish<S>; out per lane: key low, key high, second, bd
static __global__ void __launch_bounds__(64) k_dbg_best1(const uint32_t* __restrict__ in, int L, int unique, int S, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  const uint32_t* w = in + (size_t)blockIdx.x * ((size_t)L * 192 + 64);
  Best1 s; s.init();
  for (int e = 0; e < L; e++) {
    const uint32_t* r = w + ((size_t)e * 64 + lane) * 3;
    if (unique) s.consider<true>(r[0] != 0u, dsf(r[1]), r[2]); else s.consider<false>(r[0] != 0u, dsf(r[1]), r[2]);
  }
  const bool on = w[(size_t)L * 192 + lane] != 0u;
  if (S == 1) s.finish<1>(on); else if (S == 2) s.finish<2>(on); else s.finish<4>(on);
  uint32_t* o = out + ((size_t)blockIdx.x * 64 + lane) * 4;
  o[0] = (uint32_t)s.key; o[1] = (uint32_t)(s.key >> 32); o[2] = dsu(s.second); o[3] = dsu(s.bd);
}

// ------------------------------------------------------------------ which 2: the bounds
// in: tx, ty, tz, qx, qy, qz, r, f; out: tile_box_d2 | cap o2[3], S | cap_extent axis 0..2 (radius r) | cap_face_dist axis 0..2 (offset f) | cell_coord x, y, z | cell_key
static __global__ void __launch_bounds__(64) k_dbg_bounds(GridView g0, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
  const GridView g = grid_resolve(g0);
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* r = in + 8 * (size_t)i;
  uint32_t* o = out + 16 * (size_t)i;
  const float qx = dsf(r[3]), qy = dsf(r[4]), qz = dsf(r[5]), rad = dsf(r[6]), f = dsf(r[7]);
  o[0] = dsu(tile_box_d2(g, (int)r[0], (int)r[1], (int)r[2], qx, qy, qz));
  const CapBox c = cap_of(g, qx, qy, qz);
  o[1] = dsu(c.o2[0]); o[2] = dsu(c.o2[1]); o[3] = dsu(c.o2[2]); o[4] = dsu(c.S);
  o[5] = dsu(cap_extent(g, c, rad, 0)); o[6] = dsu(cap_extent(g, c, rad, 1)); o[7] = dsu(cap_extent(g, c, rad, 2));
  o[8] = dsu(cap_face_dist(c, f, 0)); o[9] = dsu(cap_face_dist(c, f, 1)); o[10] = dsu(cap_face_dist(c, f, 2));
  const int cx = cell_coord(qx, g.ox, g.inv_cell, g.nx), cy = cell_coord(qy, g.oy, g.inv_cell, g.ny), cz = cell_coord(qz, g.oz, g.inv_cell, g.nz);
  o[11] = (uint32_t)cx; o[12] = (uint32_t)cy; o[13] = (uint32_t)cz; o[14] = cell_key(g, cx, cy, cz); o[15] = 0u;
}

// ------------------------------------------------------------------ which 3: divmod_small against / and %
// every n < 2^22 for d <= 128; for every d < 2^22 the values 0, d - 1, d, 2^22 - 1, the largest multiple of d below 2^22 and that +- 1.
// out (64-bit words): mismatches, pairs compared, the smallest mismatching n * 2^22 + d (all ones: none)
#define QN_DS_DM_LIM (1 << 22)
__device__ __forceinline__ bool dm_differs(int n, int d) { int q, r; divmod_small(n, d, q, r); return q != n / d || r != n % d; }
static __global__ void __launch_bounds__(256) k_dbg_divmod(unsigned long long* __restrict__ out) {
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, nth = gridDim.x * 256u;
  unsigned long long bad = 0, done = 0, first = ~0ull;
  for (int d = 1; d <= 128; d++)
    for (uint32_t n = tid; n < (uint32_t)QN_DS_DM_LIM; n += nth) {
      done++;
      if (dm_differs((int)n, d)) { bad++; const unsigned long long p = ((unsigned long long)n << 22) | (uint32_t)d; first = p < first ? p : first; }
    }
  for (uint32_t d = tid + 1u; d < (uint32_t)QN_DS_DM_LIM; d += nth) {
    const int top = ((QN_DS_DM_LIM - 1) / (int)d) * (int)d;               // the largest multiple of d below 2^22
    const int v[7] = {0, (int)d - 1, (int)d, QN_DS_DM_LIM - 1, top, top - 1, top + 1};
#pragma unroll
    for (int u = 0; u < 7; u++) {
      if (v[u] < 0 || v[u] >= QN_DS_DM_LIM) continue;
      done++;
      if (dm_differs(v[u], (int)d)) { bad++; const unsigned long long p = ((unsigned long long)v[u] << 22) | d; first = p < first ? p : first; }
    }
  }
  if (bad) atomicAdd(&out[0], bad);
  atomicAdd(&out[1], done);
  if (first != ~0ull) atomicMin(&out[2], first);
}

// ------------------------------------------------------------------ which 4: stream_box
// in per wave: x0, x1, y0, y1, z0, z1, mode (0 rows, 1 tiles, 2 tiles pruned by the ball), qx, qy, qz, ball_r2, -; out per wave: delivered, overflow, the
// stream's return value, -, then `cap` slots: the original index of every candidate in delivery order (chunk by chunk, lane by lane)
static __global__ void __launch_bounds__(64) k_dbg_stream_box(GridView g0, const uint32_t* __restrict__ in, uint32_t cap, uint32_t* __restrict__ out) {
  __shared__ WaveLds lds;
  const GridView g = grid_resolve(g0);
  const int lane = threadIdx.x;
  const uint32_t* r = in + 12 * (size_t)blockIdx.x;
  uint32_t* o = out + (size_t)blockIdx.x * (4 + (size_t)cap);
  const int x0 = rfl((int)r[0]), x1 = rfl((int)r[1]), y0 = rfl((int)r[2]), y1 = rfl((int)r[3]), z0 = rfl((int)r[4]), z1 = rfl((int)r[5]);
  const uint32_t mode = rflu(r[6]);
  uint32_t base = 0, over = 0;
  const uint32_t ret = stream_box(g, x0, x1, y0, y1, z0, z1, mode != 0u, &lds, [&](const float4& p, bool valid, uint32_t cnt) __attribute__((always_inline)) {
    const uint32_t pos = base + (uint32_t)lane;
    if (valid) { if (pos < cap) o[4 + pos] = dsu(p.w); else over = 1u; }      // (written only below the capacity the host allocated)
    base += cnt;
  }, dsf(r[7]), dsf(r[8]), dsf(r[9]), mode == 2u ? dsf(r[10]) : -1.f);
  const bool any_over = __any(over != 0u);
  if (lane == 0) { o[0] = base; o[1] = any_over ? 1u : 0u; o[2] = ret; o[3] = 0u; }
}

// ------------------------------------------------------------------ which 5: wave_search<4, Best1>
// in per query: qx, qy, qz, r, r_cap, active, -, -; 16 queries a wave (lane l: query l & 15, sub-slot l >> 4); out per query: key low, key high, second,
// d_unseen, certified, the radius left in r, -, -
static __global__ void __launch_bounds__(64) k_dbg_wave_search1(GridView g0, const uint32_t* __restrict__ in, uint32_t n, int max_rounds, uint32_t* __restrict__ out) {
  __shared__ WaveLds lds;
  const GridView g = grid_resolve(g0);
  const int lane = threadIdx.x;
  const uint32_t qi = blockIdx.x * 16u + (uint32_t)(lane & 15);
  const bool have = qi < n;
  const uint32_t* r = in + 8 * (size_t)(have ? qi : 0u);
  const float qx = dsf(r[0]), qy = dsf(r[1]), qz = dsf(r[2]);
  float rad = dsf(r[3]); const float r_cap = dsf(r[4]);
  const bool active = have && r[5] != 0u;
  Best1 sink; sink.init();
  float du = QN_DS_INF;
  const bool cert = wave_search<4>(g, qx, qy, qz, active, rad, r_cap, max_rounds, sink, &lds, du);
  if (have && lane < 16) {
    uint32_t* o = out + 8 * (size_t)qi;
    o[0] = (uint32_t)sink.key; o[1] = (uint32_t)(sink.key >> 32); o[2] = dsu(sink.second); o[3] = dsu(du); o[4] = cert ? 1u : 0u; o[5] = dsu(rad); o[6] = 0u; o[7] = 0u;
  }
}

// ------------------------------------------------------------------ which 6: wave_search_single, one query a wave
// in per query: qx, qy, qz, r, r_cap, -, -, -; out per query: key low, key high, second, d_unseen, rounds, candidates scanned, segments enumerated, last radius
static __global__ void __launch_bounds__(64) k_dbg_wave_search_single(GridView g0, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ WaveLds lds;
  const GridView g = grid_resolve(g0);
  const uint32_t* r = in + 8 * (size_t)blockIdx.x;
  const float qx = uni(dsf(r[0])), qy = uni(dsf(r[1])), qz = uni(dsf(r[2])), rad = uni(dsf(r[3])), r_cap = uni(dsf(r[4]));
  unsigned long long key = QN_INF_KEY; float second = QN_DS_INF, du = QN_DS_INF;
  SingleStats st;                                                    // (the overload k_nn_search's probe uses: what the search did)
  wave_search_single(g, qx, qy, qz, rad, r_cap, key, second, du, &lds, st, true);
  if (threadIdx.x == 0) {
    uint32_t* o = out + 8 * (size_t)blockIdx.x;
    o[0] = (uint32_t)key; o[1] = (uint32_t)(key >> 32); o[2] = dsu(second); o[3] = dsu(du); o[4] = st.rounds; o[5] = st.cand; o[6] = st.segs; o[7] = dsu(st.r_last);
  }
}

// ------------------------------------------------------------------ which 7: wave_search_far16, 16 query slots a wave
// in per slot: qx, qy, qz, r, member, -, -, -  (the caller's layout: slot l & 15 in lanes l, l + 16, l + 32, l + 48); out per slot: key low, key high, second,
// d_unseen, member, -, -, -
static __global__ void __launch_bounds__(64) k_dbg_wave_search_far16(GridView g0, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ WaveLds lds;
  const GridView g = grid_resolve(g0);
  const int lane = threadIdx.x;
  const uint32_t qi = blockIdx.x * 16u + (uint32_t)(lane & 15);
  const uint32_t* r = in + 8 * (size_t)qi;
  const bool member = r[4] != 0u;
  unsigned long long key = QN_INF_KEY; float second = QN_DS_INF, du = QN_DS_INF;
  wave_search_far16(g, dsf(r[0]), dsf(r[1]), dsf(r[2]), member, dsf(r[3]), key, second, du, &lds);
  if (lane < 16) {
    uint32_t* o = out + 8 * (size_t)qi;
    o[0] = (uint32_t)key; o[1] = (uint32_t)(key >> 32); o[2] = dsu(second); o[3] = dsu(du); o[4] = member ? 1u : 0u; o[5] = 0u; o[6] = 0u; o[7] = 0u;
  }
}

// ------------------------------------------------------------------ which 8: BestK<KMAX>
// per wave: L steps of 64 x (on, d2, idx) through consider (the lazy queue: a flush of the whole wave when one lane's queue is full), then finish<S> with the 64 `on`
// behind them; out per lane (2 k + 4): the k real entries ascending (key low, key high), w low, w high, found(), 0
template <int KMAX>
__device__ __forceinline__ void store_bestk(const BestK<KMAX>& s, uint32_t* __restrict__ o) {
#pragma unroll
  for (int j = 0; j < KMAX; j++) if (j >= KMAX - s.k) { o[2 * (j - (KMAX - s.k))] = (uint32_t)s.a[j]; o[2 * (j - (KMAX - s.k)) + 1] = (uint32_t)(s.a[j] >> 32); }
}
template <int KMAX>
static __global__ void __launch_bounds__(64) k_dbg_bestk(const uint32_t* __restrict__ in, int L, int k, int S, uint32_t* __restrict__ out) {
  __shared__ WaveLdsK lds;
  const int lane = threadIdx.x;
  const uint32_t* w = in + (size_t)blockIdx.x * ((size_t)L * 192 + 64);
  BestK<KMAX> s; s.init(k, lds.pend);
  for (int e = 0; e < L; e++) {
    const uint32_t* r = w + ((size_t)e * 64 + lane) * 3;
    s.consider(r[0] != 0u, dsf(r[1]), r[2]);
  }
  const bool on = w[(size_t)L * 192 + lane] != 0u;
  if (S == 1) s.template finish<1>(on); else s.template finish<4>(on);
  uint32_t* o = out + ((size_t)blockIdx.x * 64 + lane) * (size_t)(2 * k + 4);
  store_bestk<KMAX>(s, o);
  o[2 * k] = (uint32_t)s.w; o[2 * k + 1] = (uint32_t)(s.w >> 32); o[2 * k + 2] = (uint32_t)s.found(); o[2 * k + 3] = 0u;
}

// ------------------------------------------------------------------ which 9: wave_search<4, BestK<KMAX>>
// in per query as which 5; out per query (2 k + 4): the k entries ascending (all ones: none), d_unseen, certified, the radius left in r, found()
template <int KMAX>
static __global__ void __launch_bounds__(64) k_dbg_wave_search_k(GridView g0, const uint32_t* __restrict__ in, uint32_t n, int max_rounds, int k, uint32_t* __restrict__ out) {
  __shared__ WaveLdsK lds;
  const GridView g = grid_resolve(g0);
  const int lane = threadIdx.x;
  const uint32_t qi = blockIdx.x * 16u + (uint32_t)(lane & 15);
  const bool have = qi < n;
  const uint32_t* r = in + 8 * (size_t)(have ? qi : 0u);
  const float qx = dsf(r[0]), qy = dsf(r[1]), qz = dsf(r[2]);
  float rad = dsf(r[3]); const float r_cap = dsf(r[4]);
  const bool active = have && r[5] != 0u;
  BestK<KMAX> sink; sink.init(k, lds.pend);
  float du = QN_DS_INF;
  const bool cert = wave_search<4>(g, qx, qy, qz, active, rad, r_cap, max_rounds, sink, &lds.s, du);
  if (have && lane < 16) {
    uint32_t* o = out + (size_t)qi * (size_t)(2 * k + 4);
    store_bestk<KMAX>(sink, o);
    o[2 * k] = dsu(du); o[2 * k + 1] = cert ? 1u : 0u; o[2 * k + 2] = dsu(rad); o[2 * k + 3] = (uint32_t)sink.found();
  }
}

// ------------------------------------------------------------------ which 10: lane_ball_knn<KMAX>, one query per lane
// in per query: x, y, z, r, -; out per query (2 k + 4): the k entries ascending, found(), 0, 0, 0
template <int KMAX>
static __global__ void __launch_bounds__(64) k_dbg_lane_ball_knn(GridView g0, const uint32_t* __restrict__ in, uint32_t n, int k, uint32_t* __restrict__ out) {
  __shared__ WaveLdsK lds;
  const GridView g = grid_resolve(g0);
  const uint32_t qi = blockIdx.x * 64u + threadIdx.x;
  BestK<KMAX> sink; sink.init(k, lds.pend);
  const uint32_t* r = in + 8 * (size_t)(qi < n ? qi : n - 1u);       // (a lane past the end walks the last query with the rest of its wave and writes nothing)
  lane_ball_knn<KMAX>(g, dsf(r[0]), dsf(r[1]), dsf(r[2]), dsf(r[3]), sink);
  if (qi >= n) return;
  uint32_t* o = out + (size_t)qi * (size_t)(2 * k + 4);
  store_bestk<KMAX>(sink, o);
  o[2 * k] = (uint32_t)sink.found(); o[2 * k + 1] = 0u; o[2 * k + 2] = 0u; o[2 * k + 3] = 0u;
}

// ------------------------------------------------------------------ which 11: build_clusters<S> with stream_clusters<S>, a first walk and a REUSE second walk
// in per lane (8): x, y, z, r, todo, - (S = 4: the lanes l, l + 16, l + 32, l + 48 hold one query).  out per wave: header (8): clusters, segments, first walk's
// return, second walk's return, overflow, 0 ..; then per lane (4 + 2 cap): cluster id, box tile mode, accepted in walk 1, accepted in walk 2, then the original indices
// the lane accepted under the callers' predicate `mine && in_tile && ccid == cid` in delivery order, walk 1 (cap slots) and walk 2 (cap slots)
template <int S>
static __global__ void __launch_bounds__(64) k_dbg_stream_clusters(GridView g0, const uint32_t* __restrict__ in, uint32_t cap, uint32_t* __restrict__ out) {
  __shared__ WaveLds lds;
  const GridView g = grid_resolve(g0);
  const int lane = threadIdx.x;
  const uint32_t* r = in + ((size_t)blockIdx.x * 64 + lane) * 8;
  uint32_t* hdr = out + (size_t)blockIdx.x * (8 + 64 * (4 + 2 * (size_t)cap));
  uint32_t* o = hdr + 8 + (size_t)lane * (4 + 2 * (size_t)cap);
  const float qx = dsf(r[0]), qy = dsf(r[1]), qz = dsf(r[2]), rad = dsf(r[3]);
  const unsigned long long todo = __ballot(r[4] != 0u);
  const bool mine = (todo >> lane) & 1ull;
  const int cx = cell_coord(qx, g.ox, g.inv_cell, g.nx), cy = cell_coord(qy, g.oy, g.inv_cell, g.ny), cz = cell_coord(qz, g.oz, g.inv_cell, g.nz);
  uint32_t cid; int ncl; uint32_t nseg_all;
  build_clusters<S>(g, &lds, todo, cx, cy, cz, qx, qy, qz, rad, cid, ncl, nseg_all);
  const uint32_t tmode = mine ? lds.cl_tile_mode[cid & 63u] : 0u;
  uint32_t n1 = 0, n2 = 0, over = 0;
  const uint32_t ret1 = stream_clusters<S>(g, &lds, ncl, nseg_all, [&](const float4& cp, bool in_tile, uint32_t ccid) __attribute__((always_inline)) {
    if (mine && in_tile && ccid == cid) { if (n1 < cap) o[4 + n1] = dsu(cp.w); else over = 1u; n1++; }
  });
  const uint32_t ret2 = stream_clusters<S, true>(g, &lds, ncl, nseg_all, [&](const float4& cp, bool in_tile, uint32_t ccid) __attribute__((always_inline)) {
    if (mine && in_tile && ccid == cid) { if (n2 < cap) o[4 + cap + n2] = dsu(cp.w); else over = 1u; n2++; }
  }, ret1);
  o[0] = cid; o[1] = tmode; o[2] = n1; o[3] = n2;
  const bool any_over = __any(over != 0u);
  if (lane == 0) { hdr[0] = (uint32_t)ncl; hdr[1] = nseg_all; hdr[2] = ret1; hdr[3] = ret2; hdr[4] = any_over ? 1u : 0u; hdr[5] = 0u; hdr[6] = 0u; hdr[7] = 0u; }
}

// ------------------------------------------------------------------ which 12: the ball walks of qn_quatro_kernels.cuh
// in per query (8): x, y, z, r, on, -.  VARIANT 0: for_each_in_ball_cells, one query per lane; 1: for_each_in_ball_cells_group<8>; 2 / 3:
// for_each_in_ball_cells_group_pre<8 | 16> with the group's table in LDS as the kernels give it (a query that is not `on` is skipped by the caller in 0 and 1, handed
// over with on = false in 2 and 3).  out per lane (2 + cap): delivered, overflow, then the sorted position u of every point body() saw, in order
template <int VARIANT>
static __global__ void __launch_bounds__(64) k_dbg_ball_cells(GridView g0, const uint32_t* __restrict__ in, uint32_t n, uint32_t cap, uint32_t* __restrict__ out) {
  constexpr int FG = VARIANT == 0 ? 1 : (VARIANT == 3 ? 16 : 8);
  __shared__ uint2 seg_tab[VARIANT == 0 ? 1 : 64 / FG][QN_SEG_CAP];
  const GridView g = grid_resolve(g0);
  const uint32_t lane_all = blockIdx.x * 64u + threadIdx.x;
  const uint32_t qi = lane_all / FG;
  const int gl = (int)(threadIdx.x % FG);
  const bool have = qi < n;
  const uint32_t* r = in + 8 * (size_t)(have ? qi : 0u);
  const bool on = have && r[4] != 0u;
  uint32_t* o = out + (size_t)lane_all * (2 + (size_t)cap);           // (the host sized `out` for whole waves)
  uint32_t cnt = 0, over = 0;
  auto body = [&](uint32_t u, float4) __attribute__((always_inline)) { if (cnt < cap) o[2 + cnt] = u; else over = 1u; cnt++; };
  const float qx = dsf(r[0]), qy = dsf(r[1]), qz = dsf(r[2]), rad = dsf(r[3]);
  if (VARIANT == 0) { if (on) for_each_in_ball_cells(g, qx, qy, qz, rad, body); }
  else if (VARIANT == 1) { if (on) for_each_in_ball_cells_group<8>(g, qx, qy, qz, rad, gl, body); }
  else for_each_in_ball_cells_group_pre<FG>(g, on, qx, qy, qz, rad, gl, seg_tab[VARIANT == 0 ? 0 : threadIdx.x / FG], body);
  o[0] = cnt; o[1] = over;
}

// KMAX: the four the product instantiates (qn_instances_knn.h: k_knn_cov<16 | 20 | 24 | 32, LIST, 4>)
#define QN_DS_BY_KMAX(KM, CALL) do { if ((KM) == 16) { CALL(16); } else if ((KM) == 20) { CALL(20); } else if ((KM) == 24) { CALL(24); } else { CALL(32); } } while (0)

// launched for qn_debug_search (qn_engine.hip, which has validated which, the records, n and arg) on its stream; in / out are device pointers, `g` a grid of the context
// with dbg cleared.  n: waves (1, 4), records (2), queries (5, 6), slots (7: a multiple of 16)
hipError_t debug_launch_search(int which, const GridView& g, uint32_t ncells, const uint32_t* in, uint32_t n, uint32_t arg, uint32_t* out, hipStream_t stream) {
  switch (which) {
    case 0: { const uint32_t m = (ncells + 1 > n ? ncells + 1 : n); hipLaunchKernelGGL(k_dbg_dump, dim3((m + 255) / 256), dim3(256), 0, stream, g, ncells, n, out); break; }
    case 1: hipLaunchKernelGGL(k_dbg_best1, dim3(n), dim3(64), 0, stream, in, (int)(arg >> 16), (int)((arg >> 8) & 1u), (int)(arg & 7u), out); break;
    case 2: hipLaunchKernelGGL(k_dbg_bounds, dim3((n + 63) / 64), dim3(64), 0, stream, g, in, n, out); break;
    case 3: hipLaunchKernelGGL(k_dbg_divmod, dim3(2048), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(out)); break;
    case 4: hipLaunchKernelGGL(k_dbg_stream_box, dim3(n), dim3(64), 0, stream, g, in, arg, out); break;
    case 5: hipLaunchKernelGGL(k_dbg_wave_search1, dim3((n + 15) / 16), dim3(64), 0, stream, g, in, n, (int)arg, out); break;
    case 6: hipLaunchKernelGGL(k_dbg_wave_search_single, dim3(n), dim3(64), 0, stream, g, in, out); break;
    case 7: hipLaunchKernelGGL(k_dbg_wave_search_far16, dim3(n / 16), dim3(64), 0, stream, g, in, out); break;
    case 8: {                                                         // arg = KMAX | k << 8 | S << 14 | L << 17
      const int KM = (int)(arg & 63u), k = (int)((arg >> 8) & 63u), S = (int)((arg >> 14) & 7u), L = (int)(arg >> 17);
#define QN_DS_CALL(K_) hipLaunchKernelGGL(k_dbg_bestk<K_>, dim3(n), dim3(64), 0, stream, in, L, k, S, out)
      QN_DS_BY_KMAX(KM, QN_DS_CALL);
#undef QN_DS_CALL
      break; }
    case 9: {                                                         // arg = max_rounds | KMAX << 8 | k << 16
      const int rounds = (int)(arg & 255u), KM = (int)((arg >> 8) & 63u), k = (int)((arg >> 16) & 63u);
#define QN_DS_CALL(K_) hipLaunchKernelGGL(k_dbg_wave_search_k<K_>, dim3((n + 15) / 16), dim3(64), 0, stream, g, in, n, rounds, k, out)
      QN_DS_BY_KMAX(KM, QN_DS_CALL);
#undef QN_DS_CALL
      break; }
    case 10: {                                                        // arg = KMAX | k << 8
      const int KM = (int)(arg & 63u), k = (int)((arg >> 8) & 63u);
#define QN_DS_CALL(K_) hipLaunchKernelGGL(k_dbg_lane_ball_knn<K_>, dim3((n + 63) / 64), dim3(64), 0, stream, g, in, n, k, out)
      QN_DS_BY_KMAX(KM, QN_DS_CALL);
#undef QN_DS_CALL
      break; }
    case 11:                                                          // arg = cap | S << 24; n = waves
      if ((arg >> 24) == 1u) hipLaunchKernelGGL(k_dbg_stream_clusters<1>, dim3(n), dim3(64), 0, stream, g, in, arg & 0xffffffu, out);
      else hipLaunchKernelGGL(k_dbg_stream_clusters<4>, dim3(n), dim3(64), 0, stream, g, in, arg & 0xffffffu, out);
      break;
    default: {                                                        // 12: arg = cap | variant << 24; n = queries
      const uint32_t v = arg >> 24, cap = arg & 0xffffffu, fg = v == 0u ? 1u : (v == 3u ? 16u : 8u);
      const dim3 grid((unsigned)(((size_t)n * fg + 63) / 64));
      if (v == 0u) hipLaunchKernelGGL(k_dbg_ball_cells<0>, grid, dim3(64), 0, stream, g, in, n, cap, out);
      else if (v == 1u) hipLaunchKernelGGL(k_dbg_ball_cells<1>, grid, dim3(64), 0, stream, g, in, n, cap, out);
      else if (v == 2u) hipLaunchKernelGGL(k_dbg_ball_cells<2>, grid, dim3(64), 0, stream, g, in, n, cap, out);
      else hipLaunchKernelGGL(k_dbg_ball_cells<3>, grid, dim3(64), 0, stream, g, in, n, cap, out);
      break; }
  }
  return hipGetLastError();
}

}  // namespace qn
