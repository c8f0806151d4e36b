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
//   relax     k_mr_relax, one DG_T^3 tile per block, one voxel per lane: the tile and its one-voxel halo in LDS (1000 costs, 4 KB), a 27-bit word per lane of
//             the moves its block rule allows, then the 26-move relaxation over LDS alone, in place, until the tile stops changing (__syncthreads_or).  Only
//             the tile's own voxels that fell are written back.  Relaxing in place on one buffer, in LDS and in memory, is sound: costs only fall, every value
//             ever stored is the cost of a real path, and a 32-bit load sees some stored value.  A block returns at once unless its tile or one of its 26
//             neighbour tiles changed in the previous launch (or received a goal before the first): the dirty-tile words are double-buffered, every block
//             writes its own word of the next buffer, so a stale halo is re-read one launch later.  At a launch that changed nothing every tile is at its
//             fixed point under the halo memory holds, and the fixed point of values that are costs of real paths is the shortest-path field.  The host
//             launches QN_ROUTE_ROUNDS_PER_CHECK rounds, reads the rounds' "any tile changed" words and visit counts, and stops at the first round that
//             changed nothing.  After k rounds every voxel whose shortest path crosses at most k - 1 tile faces is final: cells + 2 rounds bound the loop.
//   stats     k_mr_stats: reached, unreached and blocked cells, the blocks' largest and summed cost (dg_block_stats); dg_fold_stats folds them.
//   path      k_mr_path, one start per lane: a serial walk in global memory (S is small).     query  k_mr_query, one point per lane.
// DG_T = 8 (the tile, its rim in LDS, the 26-neighbour walk and the index arithmetic: qn_dense_grid.cuh) and QN_ROUTE_ROUNDS_PER_CHECK = 8 are untuned choices.  No scratch memory, no dynamically indexed private array; no floating point outside the quantisation
// of goals, starts and query points (oc_voxel: qn_dense_grid.cuh); plain vector stores; the one integer atomic is the count of visited tiles, a diagnostic.
// Host synchronisations of qn_kf_map_route: ceil(rounds / QN_ROUTE_ROUNDS_PER_CHECK) + 1 - one per batch of rounds, then the statistics, which carry the goals' counts.
// Part of qn_staticmap.hip's translation unit (included after qn_mapdistance.inc): the field hangs on that file's DistState and takes no slot of its own.

namespace {

#define MR_BLOCK MO_BLOCK

// bit (dz + 1) 9 + (dy + 1) 3 + (dx + 1) of a lane's neighbourhood words
__host__ __device__ constexpr uint32_t mr_bit(int dx, int dy, int dz) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }
// the voxels that must be passable for the move (dx, dy, dz): the block it spans
__host__ __device__ constexpr uint32_t mr_need(int dx, int dy, int dz) {
  return mr_bit(0, 0, 0) | mr_bit(dx, 0, 0) | mr_bit(0, dy, 0) | mr_bit(0, 0, dz) | mr_bit(dx, dy, 0) | mr_bit(dx, 0, dz) | mr_bit(0, dy, dz) | mr_bit(dx, dy, dz);
}

// one cell per lane, linear order: BLOCKED or UNREACHED.  lo .. hi: the clipped band (lo > hi: it misses the grid)
__global__ void __launch_bounds__(MR_BLOCK) k_mr_init(uint32_t cells, uint32_t W, uint32_t H, uint32_t planar, const uint8_t* __restrict__ cls, const uint16_t* __restrict__ d2,
                                                      uint32_t mask, uint32_t min_d2, int32_t lo, int32_t hi, uint32_t* __restrict__ cost) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= cells) return;
  bool pass;
  if (planar) {
    pass = lo <= hi;
    for (int32_t z = lo; z <= hi; z++) {
      const size_t v = (size_t)z * W * H + i;
      const uint32_t d = d2[v];
      pass = pass && ((mask >> cls[v]) & 1u) != 0 && (d == QN_DIST_FAR || d >= min_d2);
    }
  } else {
    const int32_t z = oc_ijk(i, W, H).z;
    const uint32_t d = d2[i];
    pass = z >= lo && z <= hi && ((mask >> cls[i]) & 1u) != 0 && (d == QN_DIST_FAR || d >= min_d2);
  }
  cost[i] = pass ? QN_ROUTE_UNREACHED : QN_ROUTE_BLOCKED;
}

// one goal per lane: 0 into its cell if that is passable, the cell's tile dirty; gslots[2 b ..] = the block's used and ignored goals
__global__ void __launch_bounds__(MR_BLOCK) k_mr_goals(uint32_t n, const double* __restrict__ xyz, double inv, const OcGrid G, uint32_t Df, uint32_t planar, uint32_t* cost,
                                                       const DgTiles tiles, uint32_t* __restrict__ dirty, uint32_t* __restrict__ gslots) {
  const uint32_t i = blockIdx.x * MR_BLOCK + threadIdx.x;
  bool used = false;
  if (i < n) {
    uint32_t x, y, z;
    if (oc_voxel(xyz, i, inv, G, Df, planar, &x, &y, &z)) {
      const uint32_t lin = dg_index(x, y, z, G.W, G.H);
      if (cost[lin] != QN_ROUTE_BLOCKED) {
        cost[lin] = 0u;
        dirty[dg_tile_of(x, y, z, tiles)] = 1u;
        used = true;
      }
    }
  }
  block_count(gslots + 2 * (size_t)blockIdx.x, used, i < n && !used);
}

// One tile per block, one voxel per lane: the tile relaxed in place to its fixed point under the halo memory holds (see the file header).  dirty_in: the tiles
// that changed in the previous launch, dirty_out[tile]: whether this one changed now; *round_flag = 1 when a tile changed, *visits counts the tiles loaded.
__global__ void __launch_bounds__(DG_TILE) k_mr_relax(uint32_t* cost, uint32_t W, uint32_t H, uint32_t D, const DgTiles tiles, const uint32_t* __restrict__ dirty_in,
                                                      uint32_t* __restrict__ dirty_out, uint32_t* __restrict__ round_flag, uint32_t* __restrict__ visits) {
  __shared__ uint32_t c[DG_LDS];
  const uint32_t tile = blockIdx.x;
  const DgIjk o = dg_tile_origin(tile, tiles);                       // the tile's first voxel
  bool near = false;
  if (threadIdx.x < 27) {                                            // the tile itself and its 26 neighbours, those inside the field
    const DgIjk d = oc_ijk(threadIdx.x, 3, 3);
    const int nx = o.x + (d.x - 1) * DG_T, ny = o.y + (d.y - 1) * DG_T, nz = o.z + (d.z - 1) * DG_T;
    if (nx >= 0 && nx < (int)W && ny >= 0 && ny < (int)H && nz >= 0 && nz < (int)D) near = dirty_in[dg_tile_of((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, tiles)] != 0;
  }
  if (!__syncthreads_or(near)) {
    if (threadIdx.x == 0) dirty_out[tile] = 0u;
    return;
  }
  // the tile and its halo; BLOCKED outside the field
  for (uint32_t j = threadIdx.x; j < DG_LDS; j += DG_TILE) {
    const DgIjk h = oc_ijk(j, DG_H, DG_H);
    const int gx = o.x + h.x - 1, gy = o.y + h.y - 1, gz = o.z + h.z - 1;
    uint32_t v = QN_ROUTE_BLOCKED;
    if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H && gz >= 0 && gz < (int)D) v = cost[dg_index((uint32_t)gx, (uint32_t)gy, (uint32_t)gz, W, H)];
    c[j] = v;
  }
  __syncthreads();
  const int me = (int)dg_lane_pos(threadIdx.x);
  // the passable voxels of the lane's neighbourhood, then the moves whose block is passable (none from a voxel that is not); neither changes while costs fall
  uint32_t open = c[me] != QN_ROUTE_BLOCKED ? mr_bit(0, 0, 0) : 0u;
  dg_each_neighbour([&](int dx, int dy, int dz) { if (c[me + dg_step(dx, dy, dz)] != QN_ROUTE_BLOCKED) open |= mr_bit(dx, dy, dz); });
  uint32_t moves = 0;
  dg_each_neighbour([&](int dx, int dy, int dz) { if ((open & mr_need(dx, dy, dz)) == mr_need(dx, dy, dz)) moves |= mr_bit(dx, dy, dz); });
  const uint32_t c0 = c[me];
  uint32_t cur = c0;
  for (;;) {
    uint32_t best = cur;
    dg_each_neighbour([&](int dx, int dy, int dz) {
      if (moves & mr_bit(dx, dy, dz)) {
        const uint32_t nb = c[me + dg_step(dx, dy, dz)];
        if (nb < QN_ROUTE_BLOCKED) best = min(best, nb + (uint32_t)(2 + (dx != 0) + (dy != 0) + (dz != 0)));      // (UNREACHED + w would wrap)
      }
    });
    const bool fell = best < cur;
    if (fell) { cur = best; c[me] = cur; }
    if (!__syncthreads_or(fell)) break;
  }
  const bool changed = cur < c0;                           // (a lane outside the field holds BLOCKED throughout)
  if (changed) cost[dg_index(o + dg_local(threadIdx.x), W, H)] = cur;
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
  dg_block_stats(reached, v == QN_ROUTE_UNREACHED, in && v == QN_ROUTE_BLOCKED, reached ? v : 0u, cslots, mslots, tslots);
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
    uint32_t cur = cost[dg_index(sx, sy, sz, G.W, G.H)];
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
            const uint32_t nc = cost[dg_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, G.W, G.H)];
            if (nc >= QN_ROUTE_BLOCKED || nc + (uint32_t)(2 + (dx != 0) + (dy != 0) + (dz != 0)) != cur) continue;
            bool open = true;                              // the other voxels of the block (between the two ends, so inside the field)
            for (int a = 0; a < 8; a++) {
              const int ox = (a & 1) ? dx : 0, oy = (a & 2) ? dy : 0, oz = (a & 4) ? dz : 0;
              open = open && cost[dg_index((uint32_t)(x + ox), (uint32_t)(y + oy), (uint32_t)(z + oz), G.W, G.H)] != QN_ROUTE_BLOCKED;
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
  out[i] = oc_voxel(xyz, i, inv, G, Df, planar, &x, &y, &z) ? cost[dg_index(x, y, z, G.W, G.H)] : QN_ROUTE_BLOCKED;
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The route field of the latest successful call (a member of DistState); `live` ends with the distance field it was computed from
struct RouteState {
  bool live = false;
  DevBuf<uint32_t> cost;
  qn_route_params params;
};

void mr_end(RouteState* r) { if (r) r->live = false; }

// the field's depth: the grid's, or one layer of columns in planar mode
uint32_t mr_depth(const qn_occupancy_grid& g, const qn_route_params& p) { return p.planar ? (dg_cols(g) ? 1u : 0u) : g.depth; }

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
  const DgLive L = dg_live(s);
  const OccState* o = L.occ; DistState* d = dg_mut(L.dist);
  if (!d) return QN_ERR_NOT_READY;
  if (P.min_d2 > d->params.max_dist * d->params.max_dist) return QN_ERR_INVALID_ARG;      // beyond the cap the distance is not known
  const qn_occupancy_grid& g = o->info;
  const uint32_t Df = mr_depth(g, P), cells = dg_cols(g) * Df, cb = dg_blocks(cells), gb = dg_blocks(n);
  qn_route_stats r;
  memset(&r, 0, sizeof(r));
  if (!d->route) d->route.reset(new (std::nothrow) RouteState());
  if (!d->route) return qn_kf_fail(s, "qn_kf_map_route: out of memory");
  RouteState* st = d->route.get();
  if (cells) {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    const hipStream_t str = qn_kf_int_stream(s);
    const DgTiles T = dg_tiles(g.width, g.height, Df);
    // ---- a larger field is allocated beside the previous one, which goes only once the new one is there
    DevBuf<uint32_t> nc;
    if (!st->cost.grow_beside(s, cells, nc)) return QN_ERR_HIP;
    // ---- scratch (0: the goals; 1: the two buffers of dirty-tile words; 2: a batch's "any tile changed" words, then its visit counts; 3: the blocks' three
    //      counts, then their largest cost; 4: their u64 sums; 5: the folded sums - reached, unreached, blocked, max_cost, sum_cost at byte 16, the goals' two
    //      counts at byte 24; 6: the goal blocks' two counts)
    uint32_t* d_dirty = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * 2 * (size_t)T.n);
    uint32_t* d_words = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK);
    uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 4 * (size_t)cb);
    unsigned long long* d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * (size_t)cb);
    char* d_small = (char*)qn_kf_int_scratch(s, 5, 32);
    uint32_t* d_gslots = (uint32_t*)qn_kf_int_scratch(s, 6, sizeof(uint32_t) * 2 * (size_t)gb);
    char* h = (char*)qn_kf_int_pinned(s, sizeof(uint32_t) * 2 * QN_ROUTE_ROUNDS_PER_CHECK);
    if (!d_dirty || !d_words || !d_slots || !d_tslots || !d_small || !d_gslots || !h) return qn_kf_fail(s, "qn_kf_map_route: scratch allocation failed");
    DgPoints goals;
    if (dg_points(s, "qn_kf_map_route", goals_xyz, n, &goals) != QN_OK) return QN_ERR_HIP;
    // ---- from here on the previous field is gone
    st->live = false;
    st->cost.adopt(nc);
    uint32_t* cost = st->cost.p;
    const DgBand band = dg_band(P.iz_lo, P.iz_hi, g.depth);
    QN_KFCHK(s, hipMemsetAsync(d_dirty, 0, sizeof(uint32_t) * 2 * (size_t)T.n, str));
    hipLaunchKernelGGL(k_mr_init, dim3(cb), dim3(MR_BLOCK), 0, str, cells, g.width, g.height, P.planar, (const uint8_t*)o->cls.p, (const uint16_t*)d->d2.p, P.pass_mask, P.min_d2,
                       band.lo, band.hi, cost);
    hipLaunchKernelGGL(k_mr_goals, goals.grid, dim3(MR_BLOCK), 0, str, n, goals.xyz, 1.0 / g.voxel, oc_grid(g), Df, P.planar, cost, T, d_dirty, d_gslots);
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
        hipLaunchKernelGGL(k_mr_relax, dim3(T.n), dim3(DG_TILE), 0, str, cost, g.width, g.height, Df, T, (const uint32_t*)(d_dirty + (launched & 1) * (size_t)T.n),
                           d_dirty + ((launched + 1) & 1) * (size_t)T.n, d_words + b, d_words + QN_ROUTE_ROUNDS_PER_CHECK + b);
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
    hipLaunchKernelGGL(k_mr_stats, dim3(cb), dim3(MR_BLOCK), 0, str, cells, (const uint32_t*)cost, d_slots, d_slots + 3 * (size_t)cb, d_tslots);
    dg_fold_stats(str, d_slots, d_tslots, cb, d_small);
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
  const DgLive L = dg_live(s);
  if (!L.route) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = L.occ->info;
  const size_t cells = (size_t)dg_cols(g) * mr_depth(g, L.route->params);
  *info_out = g; *params_out = L.route->params;
  if (!cells || !cost_out) return QN_OK;
  return qn_kf_download(s, cost_out, L.route->cost.p, sizeof(uint32_t) * cells);
}

extern "C" int qn_kf_map_route_query(qn_kf_store* s, const double* xyz, uint32_t n, uint32_t* cost_out) {
  if (!s || !xyz || n == 0 || n > QN_ROUTE_MAX_POINTS || !cost_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.route) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = L.occ->info;
  const uint32_t Df = mr_depth(g, L.route->params);
  if (!(dg_cols(g) * Df)) {                                          // an empty grid: every point is outside
    std::fill(cost_out, cost_out + n, (uint32_t)QN_ROUTE_BLOCKED);
    return QN_OK;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (0: the points, 1: their costs)
  uint32_t* d_out = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)n);
  if (!d_out) return qn_kf_fail(s, "qn_kf_map_route_query: scratch allocation failed");
  DgPoints pts;
  if (dg_points(s, "qn_kf_map_route_query", xyz, n, &pts) != QN_OK) return QN_ERR_HIP;
  hipLaunchKernelGGL(k_mr_query, pts.grid, dim3(MR_BLOCK), 0, str, n, pts.xyz, 1.0 / g.voxel, oc_grid(g), Df, L.route->params.planar,
                     (const uint32_t*)L.route->cost.p, d_out);
  QN_KFCHK(s, hipGetLastError());
  return qn_kf_download(s, cost_out, d_out, sizeof(uint32_t) * (size_t)n);
}

extern "C" int qn_kf_map_route_path(qn_kf_store* s, const double* starts_xyz, uint32_t n_starts, uint32_t max_len, uint32_t* len_out, int32_t* ijk_out) {
  if (!s || !starts_xyz || n_starts == 0 || n_starts > QN_ROUTE_MAX_POINTS || max_len == 0 || !len_out || !ijk_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.route) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = L.occ->info;
  const uint32_t Df = mr_depth(g, L.route->params), n = n_starts;
  const size_t words = 3 * (size_t)max_len * n;
  if (!(dg_cols(g) * Df)) {                                          // an empty grid: every start is outside
    std::fill(len_out, len_out + n, 0u); std::fill(ijk_out, ijk_out + words, 0);
    return QN_OK;
  }
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (0: the starts, 1: the lengths, 2: the voxels, zeroed so that what lies behind a path's end reads 0)
  uint32_t* d_len = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)n);
  int32_t* d_ijk = (int32_t*)qn_kf_int_scratch(s, 2, sizeof(int32_t) * words);
  if (!d_len || !d_ijk) return qn_kf_fail(s, "qn_kf_map_route_path: scratch allocation failed");
  DgPoints pts;
  if (dg_points(s, "qn_kf_map_route_path", starts_xyz, n, &pts) != QN_OK) return QN_ERR_HIP;
  QN_KFCHK(s, hipMemsetAsync(d_ijk, 0, sizeof(int32_t) * words, str));
  hipLaunchKernelGGL(k_mr_path, pts.grid, dim3(MR_BLOCK), 0, str, n, pts.xyz, 1.0 / g.voxel, oc_grid(g), Df, L.route->params.planar,
                     (const uint32_t*)L.route->cost.p, max_len, d_len, d_ijk);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(len_out, d_len, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipMemcpyAsync(ijk_out, d_ijk, sizeof(int32_t) * words, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}
