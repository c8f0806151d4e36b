// qn_maproute.inc - planning over the 3-D occupancy map on the GPU: the cost-to-go field to a set of goals and the paths down it (qn_kf_map_route,
// qn_kf_map_route_grid, qn_kf_map_route_query, qn_kf_map_route_path: include/qn_engine.h).  The numpy twin qn_amd/maproute.py is the specification:
//   passable  3-D (planar 0): voxel v iff its class bit is in pass_mask, d2[v] >= min_d2 (QN_DIST_FAR passes any min_d2) and iz_lo <= vz <= iz_hi, the field
//             W x H x D; planar: the field is W x H x 1, a column is passable iff the clipped band is not empty and every voxel of the column inside it passes
//             the class and d2 tests.
//   moves     from v to v + o, o in {-1, 0, 1}^3 without 0, both ends inside the field, allowed iff every voxel v + o' is passable, o'_k in {0, o_k} on each axis:
//             the 2, 4 or 8 voxels of the block the move spans, so no corner is cut; cost 2 + |o|_1, the 3-4-5 chamfer metric.
//   field     one u32 per cell: the smallest path cost to a goal (a passable goal voxel has 0), QN_ROUTE_BLOCKED where the cell is not passable,
//             QN_ROUTE_UNREACHED where it is passable but not connected to a goal.  At most 5 * 2^27, below QN_ROUTE_BLOCKED.
//   paths     at v with cost c > 0 the first allowed move to n with cost[n] + w == c, dz outermost, then dy, then dx, each -1, 0, +1; stop at cost 0.
// Shortest-path costs are unique integers, so every byte equals the twin's whatever the schedule.  The kernels:
//   init      k_mr_init, one cell per lane in linear order: class and d2 -> BLOCKED or UNREACHED (planar: the AND over the column's band).  The field's
//             != BLOCKED is the passable bit from here on; no extra volume is kept.
//   goals     k_mr_goals, one goal per lane: a plain store of 0 into a passable goal cell (duplicate writers all write the same value), the goal's tile marked
//             dirty, used and ignored goals counted by block_count.
//   relax     k_mr_relax, one MR_T^3 tile per block, one voxel per lane: the tile and its one-voxel halo in LDS (1000 costs, 4 KB), a 27-bit word per lane of
//             the moves its block rule allows, then the 26-move relaxation over LDS alone, in place, until the tile stops changing (__syncthreads_or).  Only
//             the tile's own voxels that fell are written back.  Relaxing in place on one buffer, in LDS and in memory, is sound: costs only fall, every value
//             ever stored is the cost of a real path, and a 32-bit load sees some stored value.  A block returns at once unless its tile or one of its 26
//             neighbour tiles changed in the previous launch (or received a goal before the first): the dirty-tile words are double-buffered, every block
//             writes its own word of the next buffer, so a stale halo is re-read one launch later.  At a launch that changed nothing every tile is at its
//             fixed point under the halo memory holds, and the fixed point of values that are costs of real paths is the shortest-path field.  The host
//             launches QN_ROUTE_ROUNDS_PER_CHECK rounds, reads the rounds' "any tile changed" words and visit counts, and stops at the first round that
//             changed nothing.  After k rounds every voxel whose shortest path crosses at most k - 1 tile faces is final: cells + 2 rounds bound the loop.
//   stats     k_mr_stats: reached, unreached and blocked cells by block_count, the blocks' largest and summed cost by wave_max, wave_sum and block_count's barrier; k_slot_fold
//             and k_slot_max fold them.
//   path      k_mr_path, one start per lane: a serial walk in global memory (S is small).     query  k_mr_query, one point per lane.
// MR_T = 8 and QN_ROUTE_ROUNDS_PER_CHECK = 8 are untuned choices.  No scratch memory, no dynamically indexed private array; no floating point outside the quantisation
// of goals, starts and query points (oc_voxel: qn_mapoccupancy.inc); plain vector stores; the one integer atomic is the count of visited tiles, a diagnostic.
// Host synchronisations of qn_kf_map_route: ceil(rounds / QN_ROUTE_ROUNDS_PER_CHECK) + 1 - one per batch of rounds, then the statistics, which carry the goals' counts.
// Part of qn_staticmap.hip's translation unit (included after qn_mapdistance.inc): the field hangs on that file's DistState and takes no slot of its own.

namespace {

#define MR_T 8                                           // the tile's side: an untuned choice
#define MR_TILE (MR_T * MR_T * MR_T)                     // voxels of a tile = lanes of a block of k_mr_relax
#define MR_H (MR_T + 2)                                  // the side with the halo
#define MR_LDS (MR_H * MR_H * MR_H)
#define MR_BLOCK MO_BLOCK
static_assert(MR_T == 8 && MR_TILE == 512, "k_mr_relax takes a lane's voxel from the bits of threadIdx.x");

// bit (dz + 1) 9 + (dy + 1) 3 + (dx + 1) of a lane's neighbourhood words
__host__ __device__ constexpr uint32_t mr_bit(int dx, int dy, int dz) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
// the voxels that must be passable for the move (dx, dy, dz): the block it spans
__host__ __device__ constexpr uint32_t mr_need(int dx, int dy, int dz) {
  return mr_bit(0, 0, 0) | mr_bit(dx, 0, 0) | mr_bit(0, dy, 0) | mr_bit(0, 0, dz) | mr_bit(dx, dy, 0) | mr_bit(dx, 0, dz) | mr_bit(0, dy, dz) | mr_bit(dx, dy, dz);
}

// one cell per lane, linear order: BLOCKED or UNREACHED.  lo .. hi: the clipped band (lo > hi: it misses the grid); cols = W H
__global__ void __launch_bounds__(MR_BLOCK) k_mr_init(uint32_t cells, uint32_t cols, uint32_t planar, const uint8_t* __restrict__ cls, const uint16_t* __restrict__ d2,
                                                      uint32_t mask, uint32_t min_d2, int32_t lo, int32_t hi, uint32_t* __restrict__ cost) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= cells) return;
  bool pass;
  if (planar) {
    pass = lo <= hi;
    for (int32_t z = lo; z <= hi; z++) {
      const size_t v = (size_t)z * cols + i;
      const uint32_t d = d2[v];
      pass = pass && ((mask >> cls[v]) & 1u) != 0 && (d == QN_DIST_FAR || d >= min_d2);
    }
  } else {
    const int32_t z = (int32_t)(i / cols);
    const uint32_t d = d2[i];
    pass = z >= lo && z <= hi && ((mask >> cls[i]) & 1u) != 0 && (d == QN_DIST_FAR || d >= min_d2);
  }
  cost[i] = pass ? QN_ROUTE_UNREACHED : QN_ROUTE_BLOCKED;
}

// one goal per lane: 0 into its cell if that is passable, the cell's tile dirty; gslots[2 b ..] = the block's used and ignored goals
__global__ void __launch_bounds__(MR_BLOCK) k_mr_goals(uint32_t n, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t Df, uint32_t planar, uint32_t* cost,
                                                       uint32_t tiles_x, uint32_t tiles_y, uint32_t* __restrict__ dirty, uint32_t* __restrict__ gslots) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  bool used = false;
  if (i < n) {
    uint32_t x, y, z;
    if (oc_voxel(xyz, i, inv, G, Df, planar, &x, &y, &z)) {
      const size_t lin = ((size_t)z * G.H + y) * G.W + x;
      if (cost[lin] != QN_ROUTE_BLOCKED) {
        cost[lin] = 0u;
        dirty[((size_t)(z / MR_T) * tiles_y + y / MR_T) * tiles_x + x / MR_T] = 1u;
        used = true;
      }
    }
  }
  block_count(gslots + 2 * (size_t)blockIdx.x, used, i < n && !used);
}

// One tile per block, one voxel per lane: the tile relaxed in place to its fixed point under the halo memory holds (see the file header).  dirty_in: the tiles
// that changed in the previous launch, dirty_out[tile]: whether this one changed now; *round_flag = 1 when a tile changed, *visits counts the tiles loaded.
__global__ void __launch_bounds__(MR_TILE) k_mr_relax(uint32_t* cost, uint32_t W, uint32_t H, uint32_t D, uint32_t tiles_x, uint32_t tiles_y, uint32_t tiles_z,
                                                      const uint32_t* __restrict__ dirty_in, uint32_t* __restrict__ dirty_out, uint32_t* __restrict__ round_flag,
                                                      uint32_t* __restrict__ visits) {
  __shared__ uint32_t c[MR_LDS];
  const uint32_t tile = blockIdx.x;
  const int bx = (int)(tile % tiles_x), by = (int)((tile / tiles_x) % tiles_y), bz = (int)(tile / (tiles_x * tiles_y));
  bool near = false;
  if (threadIdx.x < 27) {
    const int nx = bx + (int)(threadIdx.x % 3) - 1, ny = by + (int)((threadIdx.x / 3) % 3) - 1, nz = bz + (int)(threadIdx.x / 9) - 1;
    if (nx >= 0 && nx < (int)tiles_x && ny >= 0 && ny < (int)tiles_y && nz >= 0 && nz < (int)tiles_z) near = dirty_in[((size_t)nz * tiles_y + ny) * tiles_x + nx] != 0;
  }
  if (!__syncthreads_or(near)) {
    if (threadIdx.x == 0) dirty_out[tile] = 0u;
    return;
  }
  // the tile and its halo; BLOCKED outside the field
  for (uint32_t j = threadIdx.x; j < MR_LDS; j += MR_TILE) {
    const int gx = bx * MR_T + (int)(j % MR_H) - 1, gy = by * MR_T + (int)((j / MR_H) % MR_H) - 1, gz = bz * MR_T + (int)(j / (MR_H * MR_H)) - 1;
    uint32_t v = QN_ROUTE_BLOCKED;
    if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H && gz >= 0 && gz < (int)D) v = cost[((size_t)gz * H + gy) * W + gx];
    c[j] = v;
  }
  __syncthreads();
  const uint32_t lx = threadIdx.x & 7u, ly = (threadIdx.x >> 3) & 7u, lz = threadIdx.x >> 6;
  const int me = (int)((lz + 1) * MR_H * MR_H + (ly + 1) * MR_H + lx + 1);
  // the passable voxels of the lane's neighbourhood, then the moves whose block is passable (none from a voxel that is not); neither changes while costs fall
  uint32_t open = 0;
#pragma unroll
  for (int dz = -1; dz <= 1; dz++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        if (c[me + dz * MR_H * MR_H + dy * MR_H + dx] != QN_ROUTE_BLOCKED) open |= mr_bit(dx, dy, dz);
  uint32_t moves = 0;
#pragma unroll
  for (int dz = -1; dz <= 1; dz++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        if ((dx | dy | dz) != 0 && (open & mr_need(dx, dy, dz)) == mr_need(dx, dy, dz)) moves |= mr_bit(dx, dy, dz);
  const uint32_t c0 = c[me];
  uint32_t cur = c0;
  for (;;) {
    uint32_t best = cur;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++)
          if ((dx | dy | dz) != 0 && (moves & mr_bit(dx, dy, dz))) {
            const uint32_t nb = c[me + dz * MR_H * MR_H + dy * MR_H + dx];
            if (nb < QN_ROUTE_BLOCKED) best = min(best, nb + (uint32_t)(2 + (dx != 0) + (dy != 0) + (dz != 0)));      // (UNREACHED + w would wrap)
          }
    const bool fell = best < cur;
    if (fell) { cur = best; c[me] = cur; }
    if (!__syncthreads_or(fell)) break;
  }
  const bool changed = cur < c0;                           // (a lane outside the field holds BLOCKED throughout)
  if (changed) cost[((size_t)(bz * MR_T + (int)lz) * H + (size_t)(by * MR_T + (int)ly)) * W + (size_t)(bx * MR_T + (int)lx)] = cur;
  const bool any = __syncthreads_or(changed) != 0;
  if (threadIdx.x == 0) {
    dirty_out[tile] = any ? 1u : 0u;
    if (any) *round_flag = 1u;
    atomicAdd(visits, 1u);
  }
}

// one cell per lane: cslots[3 b ..] = the block's reached, unreached and blocked cells, mslots[b] = its largest reached cost, tslots[b] = their sum
__global__ void __launch_bounds__(MR_BLOCK) k_mr_stats(uint32_t cells, const uint32_t* __restrict__ cost, uint32_t* __restrict__ cslots, uint32_t* __restrict__ mslots,
                                                       unsigned long long* __restrict__ tslots) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  const bool in = i < cells;
  const uint32_t v = in ? cost[i] : QN_ROUTE_BLOCKED;
  const bool reached = v < QN_ROUTE_BLOCKED;
  const uint32_t m = reached ? v : 0u;
  __shared__ unsigned long long wt[MO_WAVES];
  __shared__ uint32_t wm[MO_WAVES];
  const unsigned long long t = wave_sum((unsigned long long)m);
  const uint32_t mm = wave_max(m);
  if ((threadIdx.x & 63) == 0) { wt[threadIdx.x >> 6] = t; wm[threadIdx.x >> 6] = mm; }
  // its barrier is the one the sums wait for, as in k_md_axis<true>, where block_max and block_sum measured slower (profiles/EXPERIMENTS.md)
  block_count(cslots + 3 * (size_t)blockIdx.x, reached, v == QN_ROUTE_UNREACHED, in && v == QN_ROUTE_BLOCKED);
  if (threadIdx.x == 0) {
    unsigned long long acc = 0; uint32_t top = 0;
    for (int w = 0; w < MO_WAVES; w++) { acc += wt[w]; top = max(top, wm[w]); }
    tslots[blockIdx.x] = acc; mslots[blockIdx.x] = top;
  }
}

// one start per lane: the walk down the field, len_out[i] voxels of which the first max_len go to ijk_out[3 max_len i ..]
__global__ void __launch_bounds__(MR_BLOCK) k_mr_path(uint32_t n, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t Df, uint32_t planar,
                                                      const uint32_t* __restrict__ cost, uint32_t max_len, uint32_t* __restrict__ len_out, int32_t* __restrict__ ijk_out) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int W = (int)G.W, H = (int)G.H, D = (int)Df;
  uint32_t sx, sy, sz, len = 0;
  if (oc_voxel(xyz, i, inv, G, Df, planar, &sx, &sy, &sz)) {
    int x = (int)sx, y = (int)sy, z = (int)sz;
    uint32_t cur = cost[((size_t)z * H + y) * W + x];
    int32_t* out = ijk_out + 3 * (size_t)max_len * i;
    while (cur < QN_ROUTE_BLOCKED) {
      if (len < max_len) { out[3 * (size_t)len] = x; out[3 * (size_t)len + 1] = y; out[3 * (size_t)len + 2] = z; }
      len++;
      if (cur == 0) break;
      bool moved = false;
      for (int dz = -1; dz <= 1 && !moved; dz++)
        for (int dy = -1; dy <= 1 && !moved; dy++)
          for (int dx = -1; dx <= 1 && !moved; dx++) {
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            if ((dx | dy | dz) == 0 || nx < 0 || nx >= W || ny < 0 || ny >= H || nz < 0 || nz >= D) continue;
            const uint32_t nc = cost[((size_t)nz * H + ny) * W + nx];
            if (nc >= QN_ROUTE_BLOCKED || nc + (uint32_t)(2 + (dx != 0) + (dy != 0) + (dz != 0)) != cur) continue;
            bool open = true;                              // the other voxels of the block (between the two ends, so inside the field)
            for (int a = 0; a < 8; a++) {
              const int ox = (a & 1) ? dx : 0, oy = (a & 2) ? dy : 0, oz = (a & 4) ? dz : 0;
              open = open && cost[((size_t)(z + oz) * H + (y + oy)) * W + (x + ox)] != QN_ROUTE_BLOCKED;
            }
            if (!open) continue;
            x = nx; y = ny; z = nz; cur = nc; moved = true;
          }
      if (!moved) break;                                   // (not at a fixed point of the relaxation: every reached voxel with c > 0 has such a move)
    }
  }
  len_out[i] = len;
}

// one point per lane: the field's value at its cell, BLOCKED outside
__global__ void __launch_bounds__(MR_BLOCK) k_mr_query(uint32_t n, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t Df, uint32_t planar,
                                                       const uint32_t* __restrict__ cost, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t x, y, z;
  out[i] = oc_voxel(xyz, i, inv, G, Df, planar, &x, &y, &z) ? cost[((size_t)z * G.H + y) * G.W + x] : QN_ROUTE_BLOCKED;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The route field of the latest successful call (a member of DistState); `live` ends with the distance field it was computed from
struct RouteState {
  bool live = false;
  DevBuf<uint32_t> cost;
  qn_route_params params;
};

void mr_end(RouteState* r) { if (r) r->live = false; }

// the occupancy result, its distance field and the live route field, or nullptr
const RouteState* mr_live(qn_kf_store* s, const OccState** occ) {
  const DistState* d = md_live(s, occ);
  return d && d->route && d->route->live ? d->route.get() : nullptr;
}

// the field's depth: the grid's, or one layer of columns in planar mode
uint32_t mr_depth(const qn_occupancy_grid& g, const qn_route_params& p) { return p.planar ? (g.width * g.height ? 1u : 0u) : g.depth; }

}  // namespace

extern "C" void qn_route_default_params(qn_route_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->pass_mask = 1u << QN_OCC_FREE; p->min_d2 = 4; p->iz_lo = 0; p->iz_hi = INT32_MAX;      // interface choices, not measurements
}

extern "C" int qn_kf_map_route(qn_kf_store* s, const double* goals_xyz, uint32_t n, const qn_route_params* params, qn_route_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !goals_xyz || !params || !stats_out || n == 0 || n > QN_ROUTE_MAX_POINTS) return QN_ERR_INVALID_ARG;
  const qn_route_params P = *params;
  if (P.pass_mask == 0 || (P.pass_mask & ~7u) || P.planar > 1 || P.iz_lo > P.iz_hi || P.reserved[0] != 0 || P.reserved[1] != 0 || P.reserved[2] != 0) return QN_ERR_INVALID_ARG;
  OccState* o = oc_live_mut(s);
  DistState* d = o && o->dist && o->dist->live ? o->dist.get() : nullptr;
  if (!d) return QN_ERR_NOT_READY;
  if (P.min_d2 > d->params.max_dist * d->params.max_dist) return QN_ERR_INVALID_ARG;      // beyond the cap the distance is not known
  const qn_occupancy_grid& g = o->info;
  const uint32_t Df = mr_depth(g, P), cols = g.width * g.height, cells = cols * Df, cb = (cells + MR_BLOCK - 1) / MR_BLOCK, gb = (n + MR_BLOCK - 1) / MR_BLOCK;
  qn_route_stats r;
  memset(&r, 0, sizeof(r));
  if (!d->route) d->route.reset(new (std::nothrow) RouteState());
  if (!d->route) return qn_kf_fail(s, "qn_kf_map_route: out of memory");
  RouteState* st = d->route.get();
  if (cells) {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    const hipStream_t str = qn_kf_int_stream(s);
    const uint32_t tx = (g.width + MR_T - 1) / MR_T, ty = (g.height + MR_T - 1) / MR_T, tz = (Df + MR_T - 1) / MR_T, tiles = tx * ty * tz;
    // ---- a larger field is allocated beside the previous one, which goes only once the new one is there
    DevBuf<uint32_t> nc;
    if (cells > st->cost.cap && !nc.grow(s, cells)) return QN_ERR_HIP;
    // ---- scratch (0: the goals; 1: the two buffers of dirty-tile words; 2: a batch's "any tile changed" words, then its visit counts; 3: the blocks' three
    //      counts, then their largest cost; 4: their u64 sums; 5: the folded sums - reached, unreached, blocked, max_cost, sum_cost at byte 16, the goals' two
    //      counts at byte 24; 6: the goal blocks' two counts)
    double* d_xyz = (double*)qn_kf_int_scratch(s, 0, sizeof(double) * 3 * (size_t)n);
    uint32_t* d_dirty = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * 2 * (size_t)tiles);
    uint32_t* d_words = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK);
    uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 4 * (size_t)cb);
    unsigned long long* d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * (size_t)cb);
    char* d_small = (char*)qn_kf_int_scratch(s, 5, 32);
    uint32_t* d_gslots = (uint32_t*)qn_kf_int_scratch(s, 6, sizeof(uint32_t) * 2 * (size_t)gb);
    char* h = (char*)qn_kf_int_pinned(s, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK);
    if (!d_xyz || !d_dirty || !d_words || !d_slots || !d_tslots || !d_small || !d_gslots || !h) return qn_kf_fail(s, "qn_kf_map_route: scratch allocation failed");
    // ---- from here on the previous field is gone
    st->live = false;
    if (nc.p) st->cost.swap(nc);
    uint32_t* cost = st->cost.p;
    const OcGrid G = oc_grid(g);
    const int32_t lo = std::max<int32_t>(P.iz_lo, 0), hi = (int32_t)std::min<int64_t>(P.iz_hi, (int64_t)g.depth - 1);
    QN_KFCHK(s, hipMemcpyAsync(d_xyz, goals_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, str));
    QN_KFCHK(s, hipMemsetAsync(d_dirty, 0, sizeof(uint32_t) * 2 * (size_t)tiles, str));
    hipLaunchKernelGGL(k_mr_init, dim3(cb), dim3(MR_BLOCK), 0, str, cells, cols, P.planar, (const uint8_t*)o->cls.p, (const uint16_t*)d->d2.p, P.pass_mask, P.min_d2, lo, hi, cost);
    hipLaunchKernelGGL(k_mr_goals, dim3(gb), dim3(MR_BLOCK), 0, str, n, (const double*)d_xyz, 1.0 / g.voxel, G, Df, P.planar, cost, tx, ty, d_dirty, d_gslots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 2>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_gslots, gb, (uint32_t*)(d_small + 24));
    QN_KFCHK(s, hipGetLastError());
    // ---- the relaxation: rounds in batches, the words read once a batch; cells + 2 rounds bound the loop
    const uint64_t limit = (uint64_t)cells + 2;
    uint64_t launched = 0;
    bool settled = false;
    while (!settled && launched < limit) {
      const uint32_t batch = (uint32_t)std::min<uint64_t>(QN_ROUTE_ROUNDS_PER_CHECK, limit - launched);
      QN_KFCHK(s, hipMemsetAsync(d_words, 0, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK, str));
      for (uint32_t b = 0; b < batch; b++, launched++)
        hipLaunchKernelGGL(k_mr_relax, dim3(tiles), dim3(MR_TILE), 0, str, cost, g.width, g.height, Df, tx, ty, tz, (const uint32_t*)(d_dirty + (launched & 1) * (size_t)tiles),
                           d_dirty + ((launched + 1) & 1) * (size_t)tiles, d_words + b, d_words + QN_ROUTE_ROUNDS_PER_CHECK + b);
      QN_KFCHK(s, hipGetLastError());
      QN_KFCHK(s, hipMemcpyAsync(h, d_words, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK, hipMemcpyDeviceToHost, str));
      QN_KFCHK(s, hipStreamSynchronize(str));                // one sync a batch of rounds
      const uint32_t* w = (const uint32_t*)h;
      for (uint32_t b = 0; b < batch && !settled; b++) {     // (the rounds behind the first that changed nothing found no dirty tile)
        r.rounds++; r.tile_visits += w[QN_ROUTE_ROUNDS_PER_CHECK + b];
        settled = w[b] == 0;
      }
    }
    if (!settled) {
      qn_kf_int_set_error(s, "qn_kf_map_route: the relaxation did not settle within cells + 2 rounds");
      return QN_ERR_INTERNAL;
    }
    uint32_t* d_sums = (uint32_t*)d_small; uint32_t* d_mslots = d_slots + 3 * (size_t)cb;
    hipLaunchKernelGGL(k_mr_stats, dim3(cb), dim3(MR_BLOCK), 0, str, cells, (const uint32_t*)cost, d_slots, d_mslots, d_tslots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums);
    hipLaunchKernelGGL(k_slot_max<uint32_t>, dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_mslots, cb, d_sums + 3);
    hipLaunchKernelGGL((k_slot_fold<unsigned long long, 1>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const unsigned long long*)d_tslots, cb, (unsigned long long*)(d_small + 16));
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h, d_small, 32, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                  // the last sync: the statistics
    const uint32_t* sums = (const uint32_t*)h;
    r.reached = sums[0]; r.unreached = sums[1]; r.blocked = sums[2]; r.max_cost = sums[3];
    r.passable = r.reached + r.unreached;
    memcpy(&r.sum_cost, h + 16, sizeof(r.sum_cost));
    r.goals_used = sums[6]; r.goals_blocked = sums[7];
  } else {
    r.goals_blocked = n;                                     // an empty grid holds no goal
  }
  st->params = P;
  st->live = true;
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_route_grid(qn_kf_store* s, qn_occupancy_grid* info_out, qn_route_params* params_out, uint32_t* cost_out) {
  if (!s || !info_out || !params_out) return QN_ERR_INVALID_ARG;
  const OccState* o = nullptr;
  const RouteState* r = mr_live(s, &o);
  if (!r) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const size_t cells = (size_t)g.width * g.height * mr_depth(g, r->params);
  *info_out = g; *params_out = r->params;
  if (!cells || !cost_out) return QN_OK;
  return qn_kf_download(s, cost_out, r->cost.p, sizeof(uint32_t) * cells);
}

extern "C" int qn_kf_map_route_query(qn_kf_store* s, const double* xyz, uint32_t n, uint32_t* cost_out) {
  if (!s || !xyz || n == 0 || n > QN_ROUTE_MAX_POINTS || !cost_out) return QN_ERR_INVALID_ARG;
  const OccState* o = nullptr;
  const RouteState* r = mr_live(s, &o);
  if (!r) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t Df = mr_depth(g, r->params);
  if (!((size_t)g.width * g.height * Df)) {                          // an empty grid: every point is outside
    std::fill(cost_out, cost_out + n, (uint32_t)QN_ROUTE_BLOCKED);
    return QN_OK;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (0: the points, 1: their costs)
  double* d_xyz = (double*)qn_kf_int_scratch(s, 0, sizeof(double) * 3 * (size_t)n);
  uint32_t* d_out = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)n);
  if (!d_xyz || !d_out) return qn_kf_fail(s, "qn_kf_map_route_query: scratch allocation failed");
  QN_KFCHK(s, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, str));
  hipLaunchKernelGGL(k_mr_query, dim3((n + MR_BLOCK - 1) / MR_BLOCK), dim3(MR_BLOCK), 0, str, n, (const double*)d_xyz, 1.0 / g.voxel, oc_grid(g), Df, r->params.planar,
                     (const uint32_t*)r->cost.p, d_out);
  QN_KFCHK(s, hipGetLastError());
  return qn_kf_download(s, cost_out, d_out, sizeof(uint32_t) * (size_t)n);
}

extern "C" int qn_kf_map_route_path(qn_kf_store* s, const double* starts_xyz, uint32_t n_starts, uint32_t max_len, uint32_t* len_out, int32_t* ijk_out) {
  if (!s || !starts_xyz || n_starts == 0 || n_starts > QN_ROUTE_MAX_POINTS || max_len == 0 || !len_out || !ijk_out) return QN_ERR_INVALID_ARG;
  const OccState* o = nullptr;
  const RouteState* r = mr_live(s, &o);
  if (!r) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t Df = mr_depth(g, r->params), n = n_starts;
  const size_t words = 3 * (size_t)max_len * n;
  if (!((size_t)g.width * g.height * Df)) {                          // an empty grid: every start is outside
    std::fill(len_out, len_out + n, 0u); std::fill(ijk_out, ijk_out + words, 0);
    return QN_OK;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (0: the starts, 1: the lengths, 2: the voxels, zeroed so that what lies behind a path's end reads 0)
  double* d_xyz = (double*)qn_kf_int_scratch(s, 0, sizeof(double) * 3 * (size_t)n);
  uint32_t* d_len = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)n);
  int32_t* d_ijk = (int32_t*)qn_kf_int_scratch(s, 2, sizeof(int32_t) * words);
  if (!d_xyz || !d_len || !d_ijk) return qn_kf_fail(s, "qn_kf_map_route_path: scratch allocation failed");
  QN_KFCHK(s, hipMemcpyAsync(d_xyz, starts_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, str));
  QN_KFCHK(s, hipMemsetAsync(d_ijk, 0, sizeof(int32_t) * words, str));
  hipLaunchKernelGGL(k_mr_path, dim3((n + MR_BLOCK - 1) / MR_BLOCK), dim3(MR_BLOCK), 0, str, n, (const double*)d_xyz, 1.0 / g.voxel, oc_grid(g), Df, r->params.planar,
                     (const uint32_t*)r->cost.p, max_len, d_len, d_ijk);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(len_out, d_len, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipMemcpyAsync(ijk_out, d_ijk, sizeof(int32_t) * words, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}
