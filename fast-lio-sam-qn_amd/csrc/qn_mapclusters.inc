// qn_mapclusters.inc - the points of the store's map slot clustered into objects on the GPU (qn_kf_map_clusters, qn_kf_map_cluster_points,
// qn_kf_map_cluster_list, qn_kf_map_drop_rejected_clusters: include/qn_engine.h).  The numpy twin qn_amd/mapclusters.py is the specification: the members are
// the finite map points (class_mask == 0) or the finite points whose live ground class has its bit in the mask; two members at different map indices are
// joined when their f32 squared distance - cell_walk's d2, the oracle's sqdist3, symmetric - is <= float(tolerance * tolerance), inclusive; root = the
// smallest map index of a point's connected component, size = its member count; a component with min_size <= size <= max_size is a cluster, numbered in
// ascending order of root; per cluster the box (f32 extremes in the order of the ordered-integer image, -0 < +0) and the int64 sums of xq = rint(x 2^e),
// e = qn_quant_exponent(tolerance, 10), the product exact as the ground unit's zq.  The components of a graph depend on no schedule, the extremes and the
// integer sums on no order: every byte equals the twin's whatever order the neighbours are met in or the unions happen, and a rerun gives the same bytes.
//   members   class_mask != 0 only: k_mc_member / k_scan_rows / k_mc_pick compact the members stably into a scratch cloud with orig[] = their map indices, so
//             the walk never gathers a class byte per candidate; stable, so "smaller cloud index <=> smaller map index" and the root rule survives.  With
//             class_mask == 0 the cloud is the slot itself (the index puts the non-finite records behind the finite ones).
//   index     qn_kf_int_cell_index (qn_cloud.hip) at radius = tolerance over that one cloud, k_cell_gather (qn_cell_walk.cuh, with the exactness argument).
//   hook      k_mc_hook, one point per lane, 256 lanes a block, in the sorted order: the walk's candidates with d2 <= r2 at a LOWER cloud index (each edge is
//             met once, by its higher end; block_sum puts the lanes' counts into the block's slot, k_slot_fold adds the slots up), and a
//             lock-free union in parent[] over cloud indices (uf_unite: qn_union_find.cuh, with the safety and termination argument).
//   flatten   k_mc_flatten, a launch of its own, so the kernel boundary makes parent[] coherent: root = the end of the parent chain, by plain loads, written at
//             the map's own index; size by integer atomicAdd on the root's counter, one add per wave when its active lanes share a root (in cell-sorted order
//             the common case), else one per lane.
//   number    k_mc_number, one point per lane in the map's own order: ten counts a block (two five-predicate block_counts, k_slot_fold), the kept roots
//             (root == own index, size in range) of every block for k_scan_rows, the largest size by wave_max and one atomicMax; k_mc_root_label gives
//             every kept root its rank - the cluster number - and every other root REJECTED; k_mc_finish copies label and size from the root to its members,
//             writes NONE and the removed byte, and counts the records a drop keeps (k_scan_rows again: the offsets of the shared compaction).
//   info      after the counts are on the host (the list is sized from C): k_mc_info, one member per lane in the sorted order: atomicMin / atomicMax on the
//             ordered-integer images of x, y, z and 64-bit integer atomicAdd of xq on the cluster's record, once per wave when its active lanes share a
//             cluster, else per lane; k_mc_info_fin turns the images back into f32.  Integer atomics only.
//   drop      qn_kf_map_drop_rejected_clusters: the shared end of the map's filters (qn_map_compact.cuh).
// Host synchronisations of a classify: the member count (class_mask != 0 only), the index's, the counts, the end (only when there is a cluster).  Results
// are committed only on success (KfMapResults, qn_kf_buf.h), so a refused call leaves the previous results as they were.  No float atomics, no scratch, no
// dynamically indexed private array.
// Part of qn_mapoutliers.hip's translation unit (included at its end): the two point filters of the map slot share one instantiation of the gather, the
// scan and the compaction, and one slot of the store - the results here hang on that unit's MoUnit.

namespace {

#define MC_NO_ROOT 0xffffffffu
#define MC_STATS 10                                      // the counts of k_mc_number per block

static_assert(sizeof(qn_cluster_params) == 24 && sizeof(qn_cluster_info) == 56 && sizeof(qn_cluster_stats) == 56, "the records of include/qn_engine.h");

__device__ __forceinline__ bool mc_finite(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
// the ordered-integer image of an f32: ascending with the value, -0 below +0; and back
__device__ __forceinline__ uint32_t mc_ord(float x) { const uint32_t b = __float_as_uint(x); return (b >> 31) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t mc_unord(uint32_t u) { return (u >> 31) ? (u & 0x7fffffffu) : ~u; }

// one record per lane in the map's own order: is it a member under the class mask; the block's members into its slot
__global__ void __launch_bounds__(MO_BLOCK) k_mc_member(uint32_t n, const float4* __restrict__ map, const uint8_t* __restrict__ cls, uint32_t mask,
                                                        uint32_t* __restrict__ blk) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool mem = false;
  if (i < n) mem = mc_finite(map[i]) && ((mask >> (cls[i] & 31u)) & 1u) != 0;
  block_count(blk + blockIdx.x, mem);
}

// the block's members, in order, to cloud[off[block] ..] with their map indices in orig
__global__ void __launch_bounds__(MO_BLOCK) k_mc_pick(uint32_t n, const float4* __restrict__ map, const uint8_t* __restrict__ cls, uint32_t mask,
                                                      const uint32_t* __restrict__ off, float4* __restrict__ cloud, uint32_t* __restrict__ orig) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  const float4 p = i < n ? map[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const bool mem = i < n && mc_finite(p) && ((mask >> (cls[i] & 31u)) & 1u) != 0;
  const uint32_t d = block_rank(mem, off[blockIdx.x]);
  if (mem) { cloud[d] = p; orig[d] = i; }
}

__global__ void __launch_bounds__(MO_BLOCK) k_mc_init(uint32_t nc, uint32_t* __restrict__ parent) {
  const uint32_t c = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (c < nc) parent[c] = c;
}

// one point per lane in the sorted order: the union of the point with every joined partner at a lower cloud index; the block's edges into its slot
__global__ void __launch_bounds__(MO_BLOCK) k_mc_hook(const CellSeg S, const float4* __restrict__ spts, const uint32_t* __restrict__ cells, float r2,
                                                      uint32_t* parent, unsigned long long* __restrict__ slots) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  unsigned long long e = 0;
  if (t < S.nfin) {                                      // (no early return: every thread of the block meets the barrier of the reduction)
    const float4 q = spts[S.p0 + t];
    const uint32_t qi = __float_as_uint(q.w);
    cell_walk(S, spts, cells, q, [&](uint32_t, const float4& p, float d2) {
      const uint32_t pj = __float_as_uint(p.w);
      if (pj < qi && d2 <= r2) { e++; uf_unite(parent, qi, pj); }       // another index than the query's: a duplicate of it elsewhere is joined
    });
  }
  block_sum(slots + blockIdx.x, e);
}

// one point per lane in the sorted order, after the hook's launch has ended: the root at the map's own index, the root's counter
__global__ void __launch_bounds__(MO_BLOCK) k_mc_flatten(const CellSeg S, const float4* __restrict__ spts, const uint32_t* __restrict__ orig,
                                                         const uint32_t* __restrict__ parent, uint32_t* __restrict__ root, uint32_t* __restrict__ size) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool act = t < S.nfin;
  uint32_t ri = MC_NO_ROOT;
  if (act) {
    const uint32_t c = __float_as_uint(spts[S.p0 + t].w);
    uint32_t r = c;
    for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;       // p < r every trip
    ri = orig ? orig[r] : r;
    root[orig ? orig[c] : c] = ri;
  }
  const unsigned long long bal = __ballot(act);
  if (bal == 0) return;                                  // (wave-uniform)
  const int first = __ffsll((long long)bal) - 1;
  const uint32_t r0 = __shfl(ri, first);
  if (__ballot(act && ri != r0) == 0) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&size[r0], (uint32_t)__popcll(bal));
  } else if (act) {
    atomicAdd(&size[ri], 1u);
  }
}

__device__ __forceinline__ bool mc_too_far(float x, double scale) { return !(fabs(rint((double)x * scale)) < 2147483648.0); }

// one record per lane in the map's own order: slots[10 b ..] = finite, members, components, clusters, too small | too large, clustered points, rejected
// points, members beyond the quantisation's range, 0; blk[b] = the block's kept roots; *largest = the largest size
__global__ void __launch_bounds__(MO_BLOCK) k_mc_number(uint32_t n, const float4* __restrict__ map, const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                                                        uint32_t min_size, uint32_t max_size, double scale, uint32_t* __restrict__ slots, uint32_t* __restrict__ blk,
                                                        uint32_t* __restrict__ largest) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool fin = false, mem = false, isroot = false, bad = false;
  uint32_t sz = 0;
  if (i < n) {
    const float4 p = map[i];
    fin = mc_finite(p);
    const uint32_t r = root[i];
    mem = r != MC_NO_ROOT;
    if (mem) {
      sz = size[r]; isroot = r == i;
      bad = mc_too_far(p.x, scale) || mc_too_far(p.y, scale) || mc_too_far(p.z, scale);
    }
  }
  const bool ok = mem && sz >= min_size && sz <= max_size;
  block_count(slots + MC_STATS * (size_t)blockIdx.x, fin, mem, isroot, isroot && ok, isroot && sz < min_size);
  __syncthreads();                                       // (the second count reuses the first one's words)
  block_count(slots + MC_STATS * (size_t)blockIdx.x + 5, isroot && sz > max_size, ok, mem && !ok, bad, false);
  block_count(blk + blockIdx.x, isroot && ok);
  const uint32_t big = wave_max(isroot ? sz : 0u);
  if ((threadIdx.x & 63) == 0 && big) atomicMax(largest, big);
}

// one record per lane: a kept root's label = its rank among the kept roots, every other root's REJECTED
__global__ void __launch_bounds__(MO_BLOCK) k_mc_root_label(uint32_t n, const uint32_t* __restrict__ root, const uint32_t* __restrict__ size, uint32_t min_size,
                                                            uint32_t max_size, const uint32_t* __restrict__ off, int32_t* __restrict__ label) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  const bool isroot = i < n && root[i] == i;
  const uint32_t sz = isroot ? size[i] : 0u;
  const bool kept = isroot && sz >= min_size && sz <= max_size;
  const uint32_t rank = block_rank(kept, off[blockIdx.x]);
  if (kept) label[i] = (int32_t)rank;
  else if (isroot) label[i] = QN_CLUSTER_REJECTED;
}

// one record per lane: label and size from the root (a root's own words are written by nobody here), NONE for the rest, the removed byte of a drop and the
// block's kept records into its slot
__global__ void __launch_bounds__(MO_BLOCK) k_mc_finish(uint32_t n, const uint32_t* __restrict__ root, uint32_t* size, int32_t* label, uint8_t* __restrict__ removed,
                                                        uint32_t* __restrict__ blk) {
  const uint32_t i = blockIdx.x * MO_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const uint32_t r = root[i];
    int32_t l = QN_CLUSTER_NONE;
    if (r == i) l = label[i];
    else if (r != MC_NO_ROOT) { l = label[r]; size[i] = size[r]; }
    if (r != i) label[i] = l;
    removed[i] = l == QN_CLUSTER_REJECTED ? 1 : 0;
    keep = l != QN_CLUSTER_REJECTED;
  }
  block_count(blk + blockIdx.x, keep);
}

// the cluster records before the members arrive: the images of the extremes at their identities, the sums 0
__global__ void __launch_bounds__(MO_BLOCK) k_mc_info_init(uint32_t C, qn_cluster_info* __restrict__ info) {
  const uint32_t c = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (c >= C) return;
  qn_cluster_info* o = info + c;
  uint32_t* lo = (uint32_t*)o->lo; uint32_t* hi = (uint32_t*)o->hi;
  o->root = 0; o->size = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) { lo[a] = 0xffffffffu; hi[a] = 0u; o->sum_q[a] = 0; }
}

// one point per lane in the sorted order: a cluster's member into the cluster's record
// (the coordinates come from the cloud itself: the index keeps a transformed copy, in which a -0 has become +0)
__global__ void __launch_bounds__(MO_BLOCK) k_mc_info(const CellSeg S, const float4* __restrict__ spts, const float4* __restrict__ cloud, const uint32_t* __restrict__ orig,
                                                      const int32_t* __restrict__ label, const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                                                      double scale, uint32_t C, qn_cluster_info* info) {
  const uint32_t t = blockIdx.x * MO_BLOCK + threadIdx.x;
  int32_t l = QN_CLUSTER_NONE;
  uint32_t ox = 0xffffffffu, oy = 0xffffffffu, oz = 0xffffffffu, hx = 0, hy = 0, hz = 0;
  long long qx = 0, qy = 0, qz = 0;
  if (t < S.nfin) {
    const uint32_t c = __float_as_uint(spts[S.p0 + t].w), i = orig ? orig[c] : c;
    const float4 p = cloud[c];
    l = label[i];
    if (l >= 0 && (uint32_t)l < C) {                     // (always below C: the guard of the store)
      ox = hx = mc_ord(p.x); oy = hy = mc_ord(p.y); oz = hz = mc_ord(p.z);
      qx = (long long)rint((double)p.x * scale); qy = (long long)rint((double)p.y * scale); qz = (long long)rint((double)p.z * scale);      // |.| < 2^31: the host checked
      if (root[i] == i) { info[l].root = i; info[l].size = size[i]; }
    } else {
      l = QN_CLUSTER_NONE;
    }
  }
  const bool act = l >= 0;
  const unsigned long long bal = __ballot(act);
  if (bal == 0) return;                                  // (wave-uniform)
  const int first = __ffsll((long long)bal) - 1;
  const int32_t l0 = __shfl(l, first);
  if (__ballot(act && l != l0) == 0) {                   // one cluster in the wave: the idle lanes carry the identities
    ox = wave_min(ox); oy = wave_min(oy); oz = wave_min(oz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    qx = wave_sum(qx); qy = wave_sum(qy); qz = wave_sum(qz);
    if ((threadIdx.x & 63) != 0) return;                 // (lane 0 holds the wave's results)
    l = l0;
  } else if (!act) {
    return;
  }
  qn_cluster_info* o = info + l;
  uint32_t* lo = (uint32_t*)o->lo; uint32_t* hi = (uint32_t*)o->hi;
  unsigned long long* sq = (unsigned long long*)o->sum_q;
  atomicMin(lo + 0, ox); atomicMin(lo + 1, oy); atomicMin(lo + 2, oz);
  atomicMax(hi + 0, hx); atomicMax(hi + 1, hy); atomicMax(hi + 2, hz);
  atomicAdd(sq + 0, (unsigned long long)qx); atomicAdd(sq + 1, (unsigned long long)qy); atomicAdd(sq + 2, (unsigned long long)qz);
}

__global__ void __launch_bounds__(MO_BLOCK) k_mc_info_fin(uint32_t C, qn_cluster_info* __restrict__ info) {
  const uint32_t c = blockIdx.x * MO_BLOCK + threadIdx.x;
  if (c >= C) return;
  uint32_t* lo = (uint32_t*)info[c].lo; uint32_t* hi = (uint32_t*)info[c].hi;
#pragma unroll
  for (int a = 0; a < 3; a++) { lo[a] = mc_unord(lo[a]); hi[a] = mc_unord(hi[a]); }
}

// the store's cluster state (MoUnit::clusters in slot QN_KF_INT_EXT_OUTLIERS): of the classified map's records a drop keeps `kept`; `clusters` records in info
struct McSet { DevBuf<int32_t> label; DevBuf<uint32_t> root, size, off; DevBuf<uint8_t> removed; DevBuf<qn_cluster_info> info; uint32_t kept = 0, clusters = 0; };
typedef KfMapResults<McSet> ClusterState;

// the live cluster results if they are those of the map slot as it stands (*map its records, *n their number), else nullptr
inline const McSet* mc_lookup(qn_kf_store* s, const float4** map, uint32_t* n) {
  const MoUnit* unit = (const MoUnit*)qn_kf_int_ext(s, QN_KF_INT_EXT_OUTLIERS);
  uint64_t gen = 0;
  *map = qn_kf_int_map(s, n, &gen);
  return unit && unit->clusters ? ((const ClusterState*)unit->clusters)->current(s, map, n) : nullptr;
}

}  // namespace

extern "C" void qn_cluster_default_params(qn_cluster_params* p) {
  if (!p) return;
  p->tolerance = 0.5; p->min_size = 10; p->max_size = 0xffffffffu; p->class_mask = 0; p->reserved = 0;      // interface choices, not measurements
}

extern "C" int qn_kf_map_clusters(qn_kf_store* s, const qn_cluster_params* params, qn_cluster_stats* stats_out) {
  // ---- every argument is checked before anything runs
  if (!s || !params || !stats_out) return QN_ERR_INVALID_ARG;
  const qn_cluster_params P = *params;
  if (!std::isfinite(P.tolerance) || !(P.tolerance > 0.0) || P.min_size < 1 || P.max_size < P.min_size || (P.class_mask & ~31u) || P.reserved != 0)
    return QN_ERR_INVALID_ARG;
  uint32_t n = 0; uint64_t gen = 0;
  const float4* map = qn_kf_int_map(s, &n, &gen);
  if (!map) return QN_ERR_NOT_READY;
  const uint8_t* d_cls = nullptr;
  if (P.class_mask && !(d_cls = qn_kf_int_ground_classes(s))) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  MoUnit* unit = nullptr;
  int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_OUTLIERS, &unit);
  if (rc != QN_OK) return rc;
  if (!unit->clusters) {
    if (!(unit->clusters = new (std::nothrow) ClusterState())) return qn_kf_fail(s, "qn_kf: out of memory");
    unit->release = [](void* p) { delete (ClusterState*)p; };
  }
  ClusterState* st = (ClusterState*)unit->clusters;
  hipStream_t stream = qn_kf_int_stream(s);
  const uint32_t nb = (n + MO_BLOCK - 1) / MO_BLOCK;
  const dim3 grid(nb), block(MO_BLOCK), one(1), wide(MO_SCAN_BLOCK);
  McSet& o = st->spare();
  if (!o.label.grow(s, n) || !o.root.grow(s, n) || !o.size.grow(s, n) || !o.removed.grow(s, n) || !o.off.grow(s, (size_t)nb + 1)) return QN_ERR_HIP;
  // scratch 3, u32: the counts of k_mc_number per block | a count per block (members, kept roots, kept records in turn) | its offsets | the sums and the largest
  const size_t w_blk = MC_STATS * (size_t)nb, w_off = w_blk + nb, w_sum = w_off + nb + 1, w_end = w_sum + 16;
  uint32_t* d_w = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * w_end);
  uint32_t* h = (uint32_t*)qn_kf_int_pinned(s, 128);
  if (!d_w || !h) return qn_kf_fail(s, "qn_kf_map_clusters: scratch allocation failed");
  uint32_t* d_blk = d_w + w_blk; uint32_t* d_off = d_w + w_off; uint32_t* d_sum = d_w + w_sum;
  // ---- the cloud: the slot itself, or the members under the mask, compacted in order
  const float4* cloud = map; const uint32_t* d_orig = nullptr; uint32_t nc = n;
  if (P.class_mask) {
    hipLaunchKernelGGL(k_mc_member, grid, block, 0, stream, n, map, d_cls, P.class_mask, d_blk);
    hipLaunchKernelGGL(k_scan_rows, one, wide, 0, stream, (const uint32_t*)d_blk, nb, d_off, d_off + nb);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h, d_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    QN_KFCHK(s, hipStreamSynchronize(stream));           // the member count sizes the cloud
    nc = h[0];
    if (nc > n) return qn_kf_fail(s, "qn_kf_map_clusters: more members than records");
    float4* d_cloud = (float4*)qn_kf_int_scratch(s, 6, sizeof(float4) * (size_t)std::max<uint32_t>(nc, 1));
    uint32_t* d_o = (uint32_t*)qn_kf_int_scratch(s, 7, sizeof(uint32_t) * (size_t)std::max<uint32_t>(nc, 1));
    if (!d_cloud || !d_o) return qn_kf_fail(s, "qn_kf_map_clusters: scratch allocation failed");
    hipLaunchKernelGGL(k_mc_pick, grid, block, 0, stream, n, map, d_cls, P.class_mask, (const uint32_t*)d_off, d_cloud, d_o);
    QN_KFCHK(s, hipGetLastError());
    cloud = d_cloud; d_orig = d_o;
  }
  const uint32_t ncb = (nc + MO_BLOCK - 1) / MO_BLOCK;
  unsigned long long* d_edges = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * ((size_t)ncb + 1));       // per block, then the sum
  if (!d_edges) return qn_kf_fail(s, "qn_kf_map_clusters: scratch allocation failed");
  QN_KFCHK(s, hipMemsetAsync(d_edges + ncb, 0, sizeof(unsigned long long), stream));
  QN_KFCHK(s, hipMemsetAsync(d_sum, 0, sizeof(uint32_t) * 16, stream));
  QN_KFCHK(s, hipMemsetAsync(o.root.p, 0xff, sizeof(uint32_t) * (size_t)n, stream));
  QN_KFCHK(s, hipMemsetAsync(o.size.p, 0, sizeof(uint32_t) * (size_t)n, stream));
  const int e = qn_quant_exponent(P.tolerance, 10);
  const double scale = std::ldexp(1.0, e);
  CellSeg seg; memset(&seg, 0, sizeof(seg));
  const float4* d_spts = nullptr;
  if (nc) {
    qn_kf_int_cell_grid g;
    const float4* pts = nullptr; const unsigned long long* keys = nullptr;
    rc = qn_kf_int_cell_index(s, &cloud, &nc, 1, P.tolerance, &g, &pts, &keys);      // the index's sync
    if (rc != QN_OK) return rc;
    float4* sp = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)nc);
    uint32_t* d_cells = (uint32_t*)qn_kf_int_scratch(s, 2, sizeof(uint32_t) * (size_t)nc);
    uint32_t* d_parent = (uint32_t*)qn_kf_int_scratch(s, 5, sizeof(uint32_t) * (size_t)nc);
    if (!sp || !d_cells || !d_parent) return qn_kf_fail(s, "qn_kf_map_clusters: scratch allocation failed");
    seg = cell_seg(g); d_spts = sp;
    const double rr = P.tolerance * P.tolerance;
    const dim3 cgrid(ncb);
    hipLaunchKernelGGL(k_cell_gather, cgrid, block, 0, stream, seg, keys, pts, sp, d_cells);
    hipLaunchKernelGGL(k_mc_init, cgrid, block, 0, stream, nc, d_parent);
    hipLaunchKernelGGL(k_mc_hook, cgrid, block, 0, stream, seg, (const float4*)sp, (const uint32_t*)d_cells, (float)rr, d_parent, d_edges);
    hipLaunchKernelGGL((k_slot_fold<unsigned long long, 1>), one, wide, 0, stream, (const unsigned long long*)d_edges, ncb, d_edges + ncb);
    hipLaunchKernelGGL(k_mc_flatten, cgrid, block, 0, stream, seg, (const float4*)sp, d_orig, (const uint32_t*)d_parent, o.root.p, o.size.p);
  }
  // ---- the clusters' numbers, every record's label and size, the counts
  hipLaunchKernelGGL(k_mc_number, grid, block, 0, stream, n, map, (const uint32_t*)o.root.p, (const uint32_t*)o.size.p, P.min_size, P.max_size, scale, d_w, d_blk,
                     d_sum + MC_STATS);
  hipLaunchKernelGGL((k_slot_fold<uint32_t, MC_STATS>), one, wide, 0, stream, (const uint32_t*)d_w, nb, d_sum);
  hipLaunchKernelGGL(k_scan_rows, one, wide, 0, stream, (const uint32_t*)d_blk, nb, d_off, d_off + nb);
  hipLaunchKernelGGL(k_mc_root_label, grid, block, 0, stream, n, (const uint32_t*)o.root.p, (const uint32_t*)o.size.p, P.min_size, P.max_size, (const uint32_t*)d_off,
                     o.label.p);
  hipLaunchKernelGGL(k_mc_finish, grid, block, 0, stream, n, (const uint32_t*)o.root.p, o.size.p, o.label.p, o.removed.p, d_blk);
  hipLaunchKernelGGL(k_scan_rows, one, wide, 0, stream, (const uint32_t*)d_blk, nb, o.off.p, o.off.p + nb);
  QN_KFCHK(s, hipGetLastError());
  QN_KFCHK(s, hipMemcpyAsync(h, d_sum, sizeof(uint32_t) * (MC_STATS + 1), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipMemcpyAsync(h + 12, o.off.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipMemcpyAsync(h + 16, d_edges + ncb, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));             // the counts
  if (h[8]) {
    qn_kf_int_set_error(s, "qn_kf_map_clusters: a member's coordinate is 2^31 units of 2^-e m or more");
    return QN_ERR_CAPACITY;
  }
  qn_cluster_stats r;
  memset(&r, 0, sizeof(r));
  r.n = n; r.n_finite = h[0]; r.members = h[1]; r.components = h[2]; r.clusters = h[3]; r.too_small = h[4]; r.too_large = h[5];
  r.clustered_points = h[6]; r.rejected_points = h[7]; r.largest = h[MC_STATS]; r.quant_exp = e;
  memcpy(&r.edges, h + 16, sizeof(r.edges));
  const uint32_t C = r.clusters, kept = h[12];
  // ---- the clusters' records, sized from C
  if (C) {
    if (!o.info.grow(s, C)) return QN_ERR_HIP;
    const dim3 igrid((C + MO_BLOCK - 1) / MO_BLOCK);
    hipLaunchKernelGGL(k_mc_info_init, igrid, block, 0, stream, C, o.info.p);
    hipLaunchKernelGGL(k_mc_info, dim3(ncb), block, 0, stream, seg, d_spts, cloud, d_orig, (const int32_t*)o.label.p, (const uint32_t*)o.root.p, (const uint32_t*)o.size.p, scale,
                       C, o.info.p);
    hipLaunchKernelGGL(k_mc_info_fin, igrid, block, 0, stream, C, o.info.p);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipStreamSynchronize(stream));           // the end
  }
  o.kept = kept; o.clusters = C;
  st->commit(gen, n);
  *stats_out = r;
  return QN_OK;
}

extern "C" int qn_kf_map_cluster_points(qn_kf_store* s, int32_t* label_out, uint32_t* root_out, uint32_t* size_out) {
  if (!s || (!label_out && !root_out && !size_out)) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const McSet* o = mc_lookup(s, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  hipStream_t stream = qn_kf_int_stream(s);
  if (label_out) QN_KFCHK(s, hipMemcpyAsync(label_out, o->label.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (root_out) QN_KFCHK(s, hipMemcpyAsync(root_out, o->root.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  if (size_out) QN_KFCHK(s, hipMemcpyAsync(size_out, o->size.p, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

extern "C" int qn_kf_map_cluster_list(qn_kf_store* s, qn_cluster_info* out, uint32_t capacity, uint32_t* count_out) {
  if (!s || !count_out) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const McSet* o = mc_lookup(s, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  if (out && capacity < o->clusters) return QN_ERR_CAPACITY;
  *count_out = o->clusters;
  if (!out || !o->clusters) return QN_OK;
  return qn_kf_download(s, out, o->info.p, sizeof(qn_cluster_info) * (size_t)o->clusters);
}

extern "C" int qn_kf_map_drop_rejected_clusters(qn_kf_store* s, const float** d_xyzi_out, uint32_t* n_out) {
  if (!s || !d_xyzi_out || !n_out) return QN_ERR_INVALID_ARG;
  const float4* map = nullptr; uint32_t n = 0;
  const McSet* o = mc_lookup(s, &map, &n);
  if (!o) return QN_ERR_NOT_READY;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  float4* d_kept = (float4*)qn_kf_int_scratch(s, 1, sizeof(float4) * (size_t)std::max<uint32_t>(o->kept, 1));
  if (!d_kept) return qn_kf_fail(s, "qn_kf_map_drop_rejected_clusters: scratch allocation failed");
  return qn_kf_map_compact_shrink(s, map, n, o->removed.p, o->off.p, d_kept, o->kept, d_xyzi_out, n_out);
}
