// qn_mapfrontier.inc - exploration frontiers of the 3-D occupancy map on the GPU: the free voxels that border unknown space, grouped into connected regions
// (qn_kf_map_frontiers, qn_kf_map_frontier_grid, qn_kf_map_frontier_regions, qn_kf_map_frontier_list, qn_kf_map_frontier_costs: include/qn_engine.h).  The
// numpy twin qn_amd/mapfrontier.py is the specification:
//   candidate  a voxel whose class bit is in free_mask and whose layer lies in iz_lo .. iz_hi, clipped to the grid.
//   frontier   a candidate with at least one of its 6 face neighbours unknown: inside the grid a neighbour is unknown iff its class bit is in unknown_mask
//              (the band does not apply to it), outside iff edge_unknown.  faces[v] = the number of unknown face neighbours, 1 .. 6.
//   regions    the connected components of the frontier voxels under 26-connectivity, root = the smallest linear index, size = the count; those with
//              size >= min_size numbered 0 .. R - 1 in ascending root (the numbering of qn_mapclusters.inc).
//   labels     one int32 per voxel: the region number, QN_FRONTIER_REJECTED for frontier voxels of smaller components, QN_FRONTIER_NONE elsewhere.
// Components are a set property and root, number, box and sums are order-free integers, so every byte equals the twin's whatever the schedule.  Built: the
// union-find scheme, not the route's relaxation - a frontier is a thin surface that runs through many tiles, so label relaxation would need a launch per
// tile it crosses, while union-find settles any shape in three launches and no host loop (rounds = 1).  The kernels:
//   mark      k_mf_mark, one voxel per lane in linear order: the class byte, and for a candidate its six neighbours by plain global loads - the x neighbours lie
//             in the cache lines the block reads anyway, the y and z neighbours are other blocks' rows, served by L2; nothing is staged in LDS.  label = the own
//             linear index for a frontier voxel, MF_NOLABEL otherwise; the voxel's tile flagged (a plain store of 1, every writer the same value); candidates
//             and frontier voxels counted by block_count, the faces summed by block_sum.
//   tile      k_mf_tile, one DG_T^3 tile per block, one voxel per lane; a block whose tile holds no frontier voxel returns after one load.  The tile's voxels
//             carry their place in the tile in LDS (a one-voxel rim of MF_NOLABEL spares the bounds tests) and fall to the smallest place among their 26
//             neighbours and then to that voxel's own value (a pointer jump), in place, until nothing falls (__syncthreads_or).  Places order like linear
//             indices, so every voxel ends at the smallest linear index of its component within the tile, and writes that.
//   merge     k_mf_merge, one voxel per lane: a frontier voxel on a tile's rim unites, for each of its 13 neighbours at a smaller linear index that lie in
//             another tile and are frontier voxels, the two roots by uf_unite_min, label[] the parent array (qn_union_find.cuh: the lock-free union-find the
//             clusters use, with the safety and termination argument; the link here is its atomic-min entry point, measured faster on this call).
//   flatten   k_mf_flatten: every label becomes its root; the root's size by atomicAdd in a transient word per voxel (scratch, not kept).
//   number    k_mf_roots counts the roots (components), those below min_size and the largest, and the kept roots per block; k_scan_rows gives their offsets
//             and R (the first host synchronisation).  k_mf_pick writes a region's row at its block_rank and the number (or REJECTED) into the root's transient
//             word; k_mf_relabel rewrites the label volume and adds a region voxel's indices and faces into a partial row by integer atomic min, max and add -
//             the voxels of a wave that share a region folded first, and each block into one of up to MF_COPIES copies of the table (k_mf_rows_init), which
//             k_mf_rows folds into the rows: a region that holds most of the frontier would otherwise serialise every wave on one cache line (measured: 6 ms
//             of 12.6 on 1.08e7 voxels).  k_mf_flatten and k_mf_costs fold a wave's voxels of one root or region the same way (wave_each_key).
//             k_slot_fold and k_slot_max fold the statistics (the second and last synchronisation).
//   getters   MfList, the predicate and the payload of the stable voxel list of qn_dense_grid.cuh (as qn_kf_map_occupancy_list).  k_mf_costs: one voxel per lane, a 64-bit atomicMin of
//             (cost << 32) | linear index per region; the host unpacks it.
// DG_T = 8 (the tile, its rim in LDS, the 26-neighbour walk and the index arithmetic: qn_dense_grid.cuh) and MF_COPIES = 32 are untuned choices.  No scratch memory, no dynamically indexed private array, no floating point; plain vector stores and vector atomics only.
// Part of qn_staticmap.hip's translation unit (included after qn_maproute.inc): the result hangs on OccState beside the distance field and takes no slot.

namespace {

#define MF_BLOCK MO_BLOCK
#define MF_NOLABEL 0xffffffffu
#define MF_COPIES 32u                                    // copies of the regions' partial rows, a power of two: an untuned choice
#define MF_PART_ROWS (1u << 18)                          // partial rows at most (16 MB of scratch), one copy of the table at least
static_assert((MF_COPIES & (MF_COPIES - 1)) == 0 && MF_COPIES <= MF_PART_ROWS, "a block chooses its copy by a mask");
static_assert(sizeof(qn_frontier_info) == 64 && sizeof(qn_frontier_params) == 32 && sizeof(qn_frontier_stats) == 48, "the records of include/qn_engine.h");

// the unknown face neighbours of voxel (x, y, z) at linear index i
__device__ __forceinline__ uint32_t mf_faces(const uint8_t* __restrict__ cls, uint32_t i, uint32_t x, uint32_t y, uint32_t z, uint32_t W, uint32_t H, uint32_t D,
                                             uint32_t umask, uint32_t edge) {
  const uint32_t WH = W * H;
  uint32_t f = 0;
  f += x > 0 ? (umask >> cls[i - 1]) & 1u : edge;
  f += x + 1 < W ? (umask >> cls[i + 1]) & 1u : edge;
  f += y > 0 ? (umask >> cls[i - W]) & 1u : edge;
  f += y + 1 < H ? (umask >> cls[i + W]) & 1u : edge;
  f += z > 0 ? (umask >> cls[i - WH]) & 1u : edge;
  f += z + 1 < D ? (umask >> cls[i + WH]) & 1u : edge;
  return f;
}

// one voxel per lane, linear order: label, the tile's flag; slots[3 b ..] = the block's candidates, frontier voxels and unknown faces
__global__ void __launch_bounds__(MF_BLOCK) k_mf_mark(uint32_t cells, uint32_t W, uint32_t H, uint32_t D, const uint8_t* __restrict__ cls, uint32_t fmask, uint32_t umask,
                                                      uint32_t edge, int32_t lo, int32_t hi, const DgTiles tiles, uint32_t* __restrict__ label,
                                                      uint32_t* __restrict__ tflag, uint32_t* __restrict__ slots) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  bool cand = false;
  uint32_t f = 0;
  if (i < cells) {
    const DgIjk v = oc_ijk(i, W, H);
    const uint32_t x = (uint32_t)v.x, y = (uint32_t)v.y, z = (uint32_t)v.z;
    cand = ((fmask >> cls[i]) & 1u) != 0 && v.z >= lo && v.z <= hi;
    if (cand) f = mf_faces(cls, i, x, y, z, W, H, D, umask, edge);
    label[i] = f ? i : MF_NOLABEL;
    if (f) tflag[dg_tile_of(x, y, z, tiles)] = 1u;
  }
  block_count(slots + 3 * (size_t)blockIdx.x, cand, f != 0);
  block_sum(slots + 3 * (size_t)blockIdx.x + 2, f);
}

// One tile per block, one voxel per lane: every frontier voxel of the tile to the smallest linear index of its component within the tile (see the file header)
__global__ void __launch_bounds__(DG_TILE) k_mf_tile(uint32_t* __restrict__ label, uint32_t W, uint32_t H, uint32_t D, const DgTiles tiles, const uint32_t* __restrict__ tflag) {
  __shared__ uint32_t c[DG_LDS];
  const uint32_t tile = blockIdx.x;
  if (tflag[tile] == 0) return;                                      // uniform over the block
  const DgIjk o = dg_tile_origin(tile, tiles);                       // the tile's first voxel
  for (uint32_t j = threadIdx.x; j < DG_LDS; j += DG_TILE) c[j] = MF_NOLABEL;
  __syncthreads();
  const DgIjk v = o + dg_local(threadIdx.x);
  const bool in = (uint32_t)v.x < W && (uint32_t)v.y < H && (uint32_t)v.z < D;
  const uint32_t g = in ? dg_index(v, W, H) : 0u;
  const int me = (int)dg_lane_pos(threadIdx.x);
  const bool front = in && label[g] != MF_NOLABEL;
  if (front) c[me] = threadIdx.x;
  __syncthreads();
  uint32_t cur = front ? threadIdx.x : MF_NOLABEL;
  for (;;) {
    bool fell = false;
    if (front) {
      uint32_t best = cur;
      dg_each_neighbour([&](int dx, int dy, int dz) { best = min(best, c[me + dg_step(dx, dy, dz)]); });
      best = c[dg_lane_pos(best)];                                        // (a value names a voxel of the same component, whose own value is no larger)
      fell = best < cur;
      if (fell) { cur = best; c[me] = cur; }
    }
    if (!__syncthreads_or(fell)) break;
  }
  if (front && cur != threadIdx.x) label[g] = dg_index(o + dg_local(cur), W, H);
}

// one voxel per lane: a frontier voxel on its tile's rim and its frontier neighbours in other tiles at smaller linear indices (every touching pair once); label[]
// is the parent array of uf_unite_min (qn_union_find.cuh, with the safety and termination argument): k_mf_tile left every word at most its own index
__global__ void __launch_bounds__(MF_BLOCK) k_mf_merge(uint32_t cells, uint32_t W, uint32_t H, uint32_t D, uint32_t* label) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  if (i >= cells || uf_load(label + i) == MF_NOLABEL) return;
  const DgIjk v = oc_ijk(i, W, H);
  const int x = v.x, y = v.y, z = v.z;
  const uint32_t lx = dg_in_tile((uint32_t)x), ly = dg_in_tile((uint32_t)y), lz = dg_in_tile((uint32_t)z), last = DG_T - 1;
  if (lx != 0 && lx != last && ly != 0 && ly != last && lz != 0 && lz != last) return;
  dg_each_neighbour([&](int dx, int dy, int dz) {
    if (!(dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))))) return;        // the 13 neighbours at smaller linear indices
    const int nx = x + dx, ny = y + dy, nz = z + dz;
    if (nx < 0 || nx >= (int)W || ny < 0 || ny >= (int)H || nz < 0 || nz >= (int)D) return;
    if (dg_tile_coord(nx) == dg_tile_coord(x) && dg_tile_coord(ny) == dg_tile_coord(y) && dg_tile_coord(nz) == dg_tile_coord(z)) return;      // the same tile: k_mf_tile joined them
    const uint32_t j = dg_index((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, W, H);
    if (uf_load(label + j) != MF_NOLABEL) uf_unite_min(label, i, j);
  });
}

// one voxel per lane: label = the root; aux[root] counts the component's voxels, the voxels of a wave that share a root in one atomicAdd
__global__ void __launch_bounds__(MF_BLOCK) k_mf_flatten(uint32_t cells, uint32_t* label, uint32_t* __restrict__ aux) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  uint32_t r = MF_NOLABEL;
  if (i < cells) {
    uint32_t p = uf_load(label + i);
    if (p != MF_NOLABEL) {
      r = i;
      while (p != r) { r = p; p = uf_load(label + r); }              // (a root's word is never written here, a voxel's word only with its root)
      if (r != i) label[i] = r;
    }
  }
  wave_each_key(r != MF_NOLABEL, r, [&](uint32_t r0, int lead, unsigned long long same) {
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(aux + r0, (uint32_t)__popcll(same));
  });
}

// one voxel per lane: kept[b] = the block's roots with size >= min_size, slots[2 b ..] = its roots and those below min_size, mslots[b] = its largest size
__global__ void __launch_bounds__(MF_BLOCK) k_mf_roots(uint32_t cells, const uint32_t* __restrict__ label, const uint32_t* __restrict__ aux, uint32_t min_size,
                                                       uint32_t* __restrict__ kept, uint32_t* __restrict__ slots, uint32_t* __restrict__ mslots) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  const bool root = i < cells && label[i] == i;
  const uint32_t size = root ? aux[i] : 0u;
  block_count(kept + blockIdx.x, root && size >= min_size);
  block_count(slots + 2 * (size_t)blockIdx.x, root, root && size < min_size);      // (another instance, with LDS words of its own)
  block_max(mslots + blockIdx.x, size);
}

// one voxel per lane: a kept root's row at its rank, in ascending root; aux[root] = the region number, or QN_FRONTIER_REJECTED
__global__ void __launch_bounds__(MF_BLOCK) k_mf_pick(uint32_t cells, const uint32_t* __restrict__ label, uint32_t* __restrict__ aux, uint32_t min_size,
                                                      const uint32_t* __restrict__ off, qn_frontier_info* __restrict__ info) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  const bool root = i < cells && label[i] == i;
  const uint32_t size = root ? aux[i] : 0u;
  const bool keep = root && size >= min_size;
  const uint32_t j = block_rank(keep, off[blockIdx.x]);
  if (keep) {
    info[j].root = i; info[j].size = size;                           // (the rest of the row: k_mf_rows)
    aux[i] = j;
  } else if (root) {
    aux[i] = (uint32_t)QN_FRONTIER_REJECTED;
  }
}

// n partial rows: the neutral elements of the box, zero faces and sums
__global__ void __launch_bounds__(MF_BLOCK) k_mf_rows_init(uint32_t n, qn_frontier_info* __restrict__ part) {
  const uint32_t j = blockIdx.x * MF_BLOCK + threadIdx.x;
  if (j >= n) return;
  qn_frontier_info r;
  r.root = 0; r.size = 0; r.faces = 0; r.reserved = 0;
  for (int k = 0; k < 3; k++) { r.lo[k] = INT_MAX; r.hi[k] = INT_MIN; r.sum[k] = 0; }
  part[j] = r;
}

// one voxel per lane: label = the region number, REJECTED or NONE; a region voxel's indices and faces into the block's copy (block & pmask) of the region's
// partial row - the voxels of a wave that share a region folded first, one set of atomics for them; slots[2 b ..] = the block's region and rejected voxels
__global__ void __launch_bounds__(MF_BLOCK) k_mf_relabel(uint32_t cells, uint32_t W, uint32_t H, uint32_t D, const uint8_t* __restrict__ cls, uint32_t umask, uint32_t edge,
                                                         int32_t* label, const uint32_t* __restrict__ aux, uint32_t R, uint32_t pmask, qn_frontier_info* part,
                                                         uint32_t* __restrict__ slots) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  int32_t k = QN_FRONTIER_NONE;
  bool in = false;
  if (i < cells) {
    const uint32_t l = (uint32_t)label[i];
    if (l != MF_NOLABEL) k = (int32_t)aux[l];
    label[i] = k;
    in = k >= 0;
  }
  int x = 0, y = 0, z = 0, f = 0;
  if (in) {
    const DgIjk v = oc_ijk(i, W, H);
    x = v.x; y = v.y; z = v.z;
    f = (int)mf_faces(cls, i, (uint32_t)x, (uint32_t)y, (uint32_t)z, W, H, D, umask, edge);
  }
  wave_each_key(in, k, [&](int32_t k0, int, unsigned long long same) {      // one trip per region the wave holds
    const bool mine = (same >> (threadIdx.x & 63)) & 1ull;
    const int x0 = wave_min(mine ? x : INT_MAX), y0 = wave_min(mine ? y : INT_MAX), z0 = wave_min(mine ? z : INT_MAX);
    const int x1 = wave_max(mine ? x : INT_MIN), y1 = wave_max(mine ? y : INT_MIN), z1 = wave_max(mine ? z : INT_MIN);
    const uint32_t sx = wave_sum(mine ? (uint32_t)x : 0u), sy = wave_sum(mine ? (uint32_t)y : 0u), sz = wave_sum(mine ? (uint32_t)z : 0u), sf = wave_sum(mine ? (uint32_t)f : 0u);
    if ((threadIdx.x & 63) == 0) {                                   // (lane 0 holds the results)
      qn_frontier_info* r = part + (size_t)(blockIdx.x & pmask) * R + (uint32_t)k0;
      atomicMin(&r->lo[0], x0); atomicMin(&r->lo[1], y0); atomicMin(&r->lo[2], z0);
      atomicMax(&r->hi[0], x1); atomicMax(&r->hi[1], y1); atomicMax(&r->hi[2], z1);
      atomicAdd(&r->faces, sf);
      atomicAdd((unsigned long long*)&r->sum[0], (unsigned long long)sx); atomicAdd((unsigned long long*)&r->sum[1], (unsigned long long)sy);
      atomicAdd((unsigned long long*)&r->sum[2], (unsigned long long)sz);
    }
  });
  block_count(slots + 2 * (size_t)blockIdx.x, in, k == QN_FRONTIER_REJECTED);
}

// one region per lane: its copies = pmask + 1 partial rows folded into its row (root and size are k_mf_pick's)
__global__ void __launch_bounds__(MF_BLOCK) k_mf_rows(uint32_t R, uint32_t copies, const qn_frontier_info* __restrict__ part, qn_frontier_info* __restrict__ info) {
  const uint32_t k = blockIdx.x * MF_BLOCK + threadIdx.x;
  if (k >= R) return;
  int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN;
  uint32_t faces = 0;
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (uint32_t c = 0; c < copies; c++) {
    const qn_frontier_info* r = part + (size_t)c * R + k;
    lo0 = min(lo0, r->lo[0]); lo1 = min(lo1, r->lo[1]); lo2 = min(lo2, r->lo[2]);
    hi0 = max(hi0, r->hi[0]); hi1 = max(hi1, r->hi[1]); hi2 = max(hi2, r->hi[2]);
    faces += r->faces; s0 += r->sum[0]; s1 += r->sum[1]; s2 += r->sum[2];
  }
  qn_frontier_info* o = info + k;
  o->lo[0] = lo0; o->lo[1] = lo1; o->lo[2] = lo2; o->hi[0] = hi0; o->hi[1] = hi1; o->hi[2] = hi2;
  o->faces = faces; o->reserved = 0; o->sum[0] = s0; o->sum[1] = s1; o->sum[2] = s2;
}

// the voxel list (k_dg_list_flag / k_dg_list_pick: qn_dense_grid.cuh): the frontier voxels, to ijk / lab
struct MfList {
  const int32_t* label; uint32_t W, H; DgIjk* ijk; int32_t* lab;
  __device__ bool keep(uint32_t i) const { return label[i] != QN_FRONTIER_NONE; }
  __device__ void put(uint32_t i, size_t j) const { ijk[j] = oc_ijk(i, W, H); lab[j] = label[i]; }
};

// one voxel per lane: a region voxel the route field reaches offers (cost << 32) | linear index to its region; cols = W H, planar: a voxel reads its column
__global__ void __launch_bounds__(MF_BLOCK) k_mf_costs(uint32_t cells, uint32_t cols, uint32_t planar, const int32_t* __restrict__ label, const uint32_t* __restrict__ cost,
                                                       unsigned long long* __restrict__ key) {
  const uint32_t i = blockIdx.x * MF_BLOCK + threadIdx.x;
  int32_t k = QN_FRONTIER_NONE;
  unsigned long long mine = ~0ull;
  if (i < cells && label[i] >= 0) {
    const uint32_t c = cost[planar ? i % cols : i];
    if (c < QN_ROUTE_BLOCKED) { k = label[i]; mine = ((unsigned long long)c << 32) | i; }
  }
  wave_each_key(k >= 0, k, [&](int32_t k0, int, unsigned long long same) {      // one trip and one atomicMin per region the wave holds
    const unsigned long long v = wave_min((same >> (threadIdx.x & 63)) & 1ull ? mine : ~0ull);
    if ((threadIdx.x & 63) == 0) atomicMin(key + k0, v);             // (lane 0 holds the smallest)
  });
}

// ---------------------------------------------------------------------------------------------------------------- host side
// The frontier result of the latest successful call (a member of OccState, beside the distance field); `live` ends with the occupancy result it was computed from
struct FrontierState {
  bool live = false;
  DevBuf<int32_t> label;
  DevBuf<qn_frontier_info> info;
  qn_frontier_params params;
  qn_frontier_stats stats;
};

void mf_end(FrontierState* f) { if (f) f->live = false; }

// (dg_live, the lookup every entry point behind qn_kf_map_occupancy starts with: qn_mapview.inc, included last, where every state is complete)

}  // namespace

extern "C" void qn_frontier_default_params(qn_frontier_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->free_mask = 1u << QN_OCC_FREE; p->unknown_mask = 1u << QN_OCC_UNKNOWN; p->edge_unknown = 1; p->min_size = 8; p->iz_lo = 0; p->iz_hi = INT32_MAX;      // interface choices, not measurements
}

extern "C" int qn_kf_map_frontiers(qn_kf_store* s, const qn_frontier_params* params, qn_frontier_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !stats_out) return QN_ERR_INVALID_ARG;
  const qn_frontier_params P = *params;
  if (P.free_mask == 0 || (P.free_mask & ~7u) || P.unknown_mask == 0 || (P.unknown_mask & ~7u) || (P.free_mask & P.unknown_mask) || P.edge_unknown > 1 || P.min_size == 0 ||
      P.iz_lo > P.iz_hi || P.reserved[0] != 0 || P.reserved[1] != 0)
    return QN_ERR_INVALID_ARG;
  OccState* o = dg_mut(dg_live(s).occ);
  if (!o) return QN_ERR_NOT_READY;
  const qn_occupancy_grid& g = o->info;
  const uint32_t W = g.width, H = g.height, D = g.depth, cells = dg_cells(g), cb = dg_blocks(cells);
  qn_frontier_stats r;
  memset(&r, 0, sizeof(r));
  if (!o->frontier) o->frontier.reset(new (std::nothrow) FrontierState());
  if (!o->frontier) return qn_kf_fail(s, "qn_kf_map_frontiers: out of memory");
  FrontierState* st = o->frontier.get();
  if (cells) {
    QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
    const hipStream_t str = qn_kf_int_stream(s);
    const DgTiles T = dg_tiles(W, H, D);
    // ---- a larger label volume is allocated beside the previous one, which goes only once the new one is there
    DevBuf<int32_t> nl;
    if (!st->label.grow_beside(s, cells, nl)) return QN_ERR_HIP;
    // ---- scratch (1: the transient word per voxel - a root's size, then its number; 2: the tiles' flags; 3: the blocks' count slots, three words each; 4: the
    //      blocks' kept roots, their offsets and the total, then the blocks' largest sizes; 5: the folded sums - candidates, frontier, faces, components,
    //      too small, largest, region voxels, rejected voxels)
    uint32_t* d_aux = (uint32_t*)qn_kf_int_scratch(s, 1, sizeof(uint32_t) * (size_t)cells);
    uint32_t* d_tflag = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (size_t)T.n);
    uint32_t* d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 3 * (size_t)cb);
    uint32_t* d_blk = (uint32_t*)qn_kf_int_scratch(s, 4, sizeof(uint32_t) * (3 * (size_t)cb + 1));
    uint32_t* d_sums = (uint32_t*)qn_kf_int_scratch(s, 5, 32);
    uint32_t* h = (uint32_t*)qn_kf_int_pinned(s, 64);
    if (!d_aux || !d_tflag || !d_slots || !d_blk || !d_sums || !h) return qn_kf_fail(s, "qn_kf_map_frontiers: scratch allocation failed");
    uint32_t* d_off = d_blk + cb; uint32_t* d_mslots = d_blk + 2 * (size_t)cb + 1;
    // ---- from here on the previous result is gone
    st->live = false;
    st->label.adopt(nl);
    uint32_t* lab = (uint32_t*)st->label.p;
    const uint8_t* cls = (const uint8_t*)o->cls.p;
    const DgBand band = dg_band(P.iz_lo, P.iz_hi, D);
    QN_KFCHK(s, hipMemsetAsync(d_aux, 0, sizeof(uint32_t) * (size_t)cells, str));
    QN_KFCHK(s, hipMemsetAsync(d_tflag, 0, sizeof(uint32_t) * (size_t)T.n, str));
    // ---- mark, label: tile, merge, flatten
    hipLaunchKernelGGL(k_mf_mark, dim3(cb), dim3(MF_BLOCK), 0, str, cells, W, H, D, cls, P.free_mask, P.unknown_mask, P.edge_unknown, band.lo, band.hi, T, lab, d_tflag, d_slots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums);
    hipLaunchKernelGGL(k_mf_tile, dim3(T.n), dim3(DG_TILE), 0, str, lab, W, H, D, T, (const uint32_t*)d_tflag);
    hipLaunchKernelGGL(k_mf_merge, dim3(cb), dim3(MF_BLOCK), 0, str, cells, W, H, D, lab);
    hipLaunchKernelGGL(k_mf_flatten, dim3(cb), dim3(MF_BLOCK), 0, str, cells, lab, d_aux);
    // ---- number: the kept roots ranked in ascending index
    hipLaunchKernelGGL(k_mf_roots, dim3(cb), dim3(MF_BLOCK), 0, str, cells, (const uint32_t*)lab, (const uint32_t*)d_aux, P.min_size, d_blk, d_slots, d_mslots);
    hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_blk, cb, d_off, d_off + cb);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 2>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums + 3);
    hipLaunchKernelGGL(k_slot_max<uint32_t>, dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_mslots, cb, d_sums + 5);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h, d_off + cb, sizeof(uint32_t), hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                  // sync 1: the number of regions
    const uint32_t R = h[0];
    if (!st->info.grow(s, std::max<uint32_t>(R, 1))) return QN_ERR_HIP;
    // the regions' partial rows (scratch 6): up to MF_COPIES copies of the table, a block adding into copy block % copies, so that a region that holds most of the
    // frontier does not serialise every wave on one cache line; fewer copies for a long table
    uint32_t copies = MF_COPIES;
    while (copies > 1 && (uint64_t)copies * R > MF_PART_ROWS) copies >>= 1;
    const uint32_t rows = copies * std::max<uint32_t>(R, 1);
    qn_frontier_info* d_part = (qn_frontier_info*)qn_kf_int_scratch(s, 6, sizeof(qn_frontier_info) * (size_t)rows);
    if (!d_part) return qn_kf_fail(s, "qn_kf_map_frontiers: scratch allocation failed");
    hipLaunchKernelGGL(k_mf_rows_init, dim3(dg_blocks(rows)), dim3(MF_BLOCK), 0, str, rows, d_part);
    hipLaunchKernelGGL(k_mf_pick, dim3(cb), dim3(MF_BLOCK), 0, str, cells, (const uint32_t*)lab, d_aux, P.min_size, (const uint32_t*)d_off, st->info.p);
    hipLaunchKernelGGL(k_mf_relabel, dim3(cb), dim3(MF_BLOCK), 0, str, cells, W, H, D, cls, P.unknown_mask, P.edge_unknown, st->label.p, (const uint32_t*)d_aux, R, copies - 1,
                       d_part, d_slots);
    if (R) hipLaunchKernelGGL(k_mf_rows, dim3(dg_blocks(R)), dim3(MF_BLOCK), 0, str, R, copies, (const qn_frontier_info*)d_part, st->info.p);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 2>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums + 6);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h, d_sums, 32, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                  // sync 2, the last: the statistics
    r.candidates = h[0]; r.frontier = h[1]; r.unknown_faces = h[2]; r.components = h[3]; r.too_small = h[4]; r.largest = h[5]; r.region_voxels = h[6];
    r.rejected_voxels = h[7]; r.regions = R; r.rounds = 1;
  }
  st->params = P; st->stats = r;
  st->live = true;
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_frontier_grid(qn_kf_store* s, qn_occupancy_grid* info_out, qn_frontier_params* params_out, int32_t* label_out) {
  if (!s || !info_out || !params_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.frontier) return QN_ERR_NOT_READY;
  const size_t cells = dg_cells(L.occ->info);
  *info_out = L.occ->info; *params_out = L.frontier->params;
  if (!cells || !label_out) return QN_OK;
  return qn_kf_download(s, label_out, L.frontier->label.p, sizeof(int32_t) * cells);
}

extern "C" int qn_kf_map_frontier_regions(qn_kf_store* s, qn_frontier_info* info_out, uint32_t capacity, uint32_t* count_out) {
  if (!s || !count_out || (!info_out && capacity)) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.frontier) return QN_ERR_NOT_READY;
  const uint32_t R = L.frontier->stats.regions;
  *count_out = R;
  if (capacity < R) return QN_ERR_CAPACITY;
  if (!R) return QN_OK;
  return qn_kf_download(s, info_out, L.frontier->info.p, sizeof(qn_frontier_info) * (size_t)R);
}

extern "C" int qn_kf_map_frontier_list(qn_kf_store* s, int32_t* ijk_out, int32_t* label_out, uint32_t capacity, uint32_t* count_out) {
  if (!s || !count_out || ((!ijk_out || !label_out) && capacity)) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.frontier) return QN_ERR_NOT_READY;
  const uint32_t n = L.frontier->stats.frontier;
  *count_out = n;
  if (capacity < n) return QN_ERR_CAPACITY;
  if (!n) return QN_OK;
  const qn_occupancy_grid& g = L.occ->info;
  const uint32_t cells = dg_cells(g);
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (3: dg_list_count's; 1: the voxels; 2: their labels)
  DgIjk* d_ijk = (DgIjk*)qn_kf_int_scratch(s, 1, sizeof(DgIjk) * (size_t)n);
  int32_t* d_lab = (int32_t*)qn_kf_int_scratch(s, 2, sizeof(int32_t) * (size_t)n);
  const MfList list = {L.frontier->label.p, g.width, g.height, d_ijk, d_lab};
  const uint32_t* d_off = d_ijk && d_lab ? dg_list_count(s, cells, list) : nullptr;
  if (!d_off) return qn_kf_fail(s, "qn_kf_map_frontier_list: scratch allocation failed");
  dg_list_pick(s, cells, list, d_off);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(ijk_out, d_ijk, sizeof(DgIjk) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipMemcpyAsync(label_out, d_lab, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  return QN_OK;
}

extern "C" int qn_kf_map_frontier_costs(qn_kf_store* s, uint32_t* cost_out, int32_t* ijk_out) {
  if (!s || !cost_out || !ijk_out) return QN_ERR_INVALID_ARG;
  const DgLive L = dg_live(s);
  if (!L.frontier || !L.route) return QN_ERR_NOT_READY;
  const uint32_t R = L.frontier->stats.regions;
  if (!R) return QN_OK;
  const qn_occupancy_grid& g = L.occ->info;
  const uint32_t cols = dg_cols(g), cells = dg_cells(g);
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t str = qn_kf_int_stream(s);
  // ---- scratch (1: the regions' keys) and their pinned mirror
  unsigned long long* d_key = (unsigned long long*)qn_kf_int_scratch(s, 1, sizeof(unsigned long long) * (size_t)R);
  unsigned long long* h = (unsigned long long*)qn_kf_int_pinned(s, sizeof(unsigned long long) * (size_t)R);
  if (!d_key || !h) return qn_kf_fail(s, "qn_kf_map_frontier_costs: scratch allocation failed");
  QN_KFCHK(s, hipMemsetAsync(d_key, 0xff, sizeof(unsigned long long) * (size_t)R, str));
  hipLaunchKernelGGL(k_mf_costs, dim3(dg_blocks(cells)), dim3(MF_BLOCK), 0, str, cells, cols, L.route->params.planar, (const int32_t*)L.frontier->label.p,
                     (const uint32_t*)L.route->cost.p, d_key);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_key, sizeof(unsigned long long) * (size_t)R, hipMemcpyDeviceToHost, str));
  QN_KFCHK(s, hipStreamSynchronize(str));
  for (uint32_t k = 0; k < R; k++) {
    const bool none = h[k] == ~0ull;
    cost_out[k] = none ? QN_ROUTE_UNREACHED : (uint32_t)(h[k] >> 32);
    const DgIjk v = oc_ijk(none ? 0u : (uint32_t)(h[k] & 0xffffffffull), g.width, g.height);
    ijk_out[3 * (size_t)k] = v.x; ijk_out[3 * (size_t)k + 1] = v.y; ijk_out[3 * (size_t)k + 2] = v.z;
  }
  return QN_OK;
}
