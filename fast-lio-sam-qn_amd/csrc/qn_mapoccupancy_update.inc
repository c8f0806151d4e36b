// qn_mapoccupancy_update.inc - the resident occupancy volume of qn_mapoccupancy.inc brought to a new list in place (qn_kf_map_occupancy_update: include/qn_engine.h).
// The numpy twin is qn_amd/mapoccupancy.py's update().  Behind the quantisation of the ray ends the volume is u32 sums, so an entry's contribution is taken out
// again by walking the same rays with -1 mod 2^32 (oc_walk<FOLD, true>), and the bytes afterwards are those of a rebuild of the new list whatever the order.
//   ledger    OccLedger, hanging on OccState: per entry of the list the volume holds its id, its 12 pose doubles, its five record counts and the box of its ray
//             ends in voxel coordinates.  A new list is matched against it as a multiset of (id, the bytes of the pose); unmatched rows are removed, unmatched
//             entries added.  Only this call leaves a ledger; qn_kf_map_occupancy drops it.
//   extent    k_oc_extent_entry over the added entries only, k_oc_extent's grid: the extremes by wave_min / wave_max and the counts by block_count as there, then
//             integer atomics on the entry's own row instead of the call's.  One host read; the new box (the union of the rows' boxes) and every refusal follow
//             from it on the host, with the previous result, the ledger and the fields over them untouched.
//   subtract  k_oc_uncarve over the removed rows, in the old grid: k_oc_carve with the other sign.
//   regrid    k_oc_regrid, one voxel of the new grid per lane, x fastest: the counts of the same voxel of the old grid, or 0 outside it, into a second pair of
//             buffers, which then change places with the first.  Nothing is cleared: an old voxel outside the new box holds 0 behind the subtraction, since only
//             removed rows reached it (the twin asserts it).
//   add       k_oc_carve of qn_mapoccupancy.inc over the added entries, in the new grid; then its k_oc_classify over the whole grid.  The second host read.
// Integer atomics only, no scratch memory, no dynamically indexed private array.  Part of qn_staticmap.hip's translation unit, behind qn_mapoccupancy.inc.
#include <unordered_map>

namespace {

struct OuRow { int32_t lo[3], hi[3]; uint32_t cnt[5], pad; };        // an entry's extremes of c(A), c(B) and its records, rays, non-finite, near and far records; 48 bytes
struct OuLedgerRow { int32_t id; double P[12]; OuRow r; };           // (no ray: r.cnt[1] == 0, and lo > hi)
struct OccLedger {
  bool valid = false;                                    // the rows are those of the live counts
  qn_occupancy_params par;
  std::vector<OuLedgerRow> rows;
  DevBuf<uint32_t> hits, misses;                         // where the regrid writes; they change places with OccState's
};

// k_oc_extent with the extremes and the counts kept per entry: rows[e] for entry e of the launch, *flag = 1 when a ray end is out of range
__global__ void __launch_bounds__(OC_BLOCK) k_oc_extent_entry(const OcEntry* __restrict__ ents, double inv, float lo2, float hi2, OuRow* __restrict__ rows,
                                                              int32_t* __restrict__ flag) {
  __shared__ uint32_t cnt[5];
  const OcEntry* E = ents + blockIdx.y;
  const uint32_t n = E->n;
  if (blockIdx.x * OC_BLOCK >= n) return;                            // uniform over the block
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  OuRow* own = rows + blockIdx.y;
  int st = -1;                                                       // (past the end: counted nowhere)
  int32_t lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < n) {
    int32_t A[3], B[3];
    st = oc_ray(E->pts[i], E->P, inv, lo2, hi2, A, B);
    if (st == OC_RAY) {
#pragma unroll
      for (int k = 0; k < 3; k++) { const int32_t a = A[k] >> OC_S, b = B[k] >> OC_S; lo[k] = min(a, b); hi[k] = max(a, b); }
    }
    if (st == OC_CAPACITY) *flag = 1;                                // (a plain store of the same value by whoever finds one)
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { lo[k] = wave_min(lo[k]); hi[k] = wave_max(hi[k]); }
  if ((threadIdx.x & 63) == 0 && lo[0] != INT_MAX) {
#pragma unroll
    for (int k = 0; k < 3; k++) { atomicMin(&own->lo[k], lo[k]); atomicMax(&own->hi[k], hi[k]); }
  }
  block_count(cnt, st >= 0, st == OC_RAY, st == OC_NONFINITE, st == OC_NEAR, st == OC_FAR);
  if (threadIdx.x < 5) atomicAdd(&own->cnt[threadIdx.x], cnt[threadIdx.x]);      // (the lane that wrote the word reads it)
}

// k_oc_carve with the other sign: every ray's hit and misses taken out again
template <bool FOLD>
__global__ void __launch_bounds__(OC_BLOCK) k_oc_uncarve(const OcEntry* __restrict__ ents, double inv, float lo2, float hi2, const OcGrid G, uint32_t shell,
                                                         uint32_t* __restrict__ hits, uint32_t* __restrict__ misses) {
  const OcEntry* E = ents + blockIdx.y;
  const uint32_t n = E->n;
  if (blockIdx.x * OC_BLOCK >= n) return;                            // uniform over the block
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  int32_t A[3] = {0, 0, 0}, B[3] = {0, 0, 0};
  bool ray = false;
  if (i < n) ray = oc_ray(E->pts[i], E->P, inv, lo2, hi2, A, B) == OC_RAY;
  oc_walk<FOLD, true>(ray, A, B, G, shell, hits, misses);
}

// one voxel of the new grid N per lane: its counts in the old grid O (depth layers deep), 0 where O does not reach
__global__ void __launch_bounds__(OC_BLOCK) k_oc_regrid(const OcGrid N, const OcGrid O, uint32_t depth, const uint32_t* __restrict__ old_hits,
                                                        const uint32_t* __restrict__ old_misses, uint32_t* __restrict__ hits, uint32_t* __restrict__ misses) {
  const uint32_t i = blockIdx.x * OC_BLOCK + threadIdx.x;
  if (i >= N.cells) return;
  const DgIjk v = oc_ijk(i, N.W, N.H);
  const uint32_t x = (uint32_t)(v.x + (N.minc[0] - O.minc[0])), y = (uint32_t)(v.y + (N.minc[1] - O.minc[1])), z = (uint32_t)(v.z + (N.minc[2] - O.minc[2]));
  const bool in = x < O.W && y < O.H && z < depth;                   // (a negative coordinate wrapped to a large one)
  const uint32_t j = in ? dg_index(x, y, z, O.W, O.H) : 0;
  hits[i] = in ? old_hits[j] : 0u;
  misses[i] = in ? old_misses[j] : 0u;
}

template <bool SUB> void ou_walk(hipStream_t str, const OcEntry* h_ent, const OcEntry* d_ent, uint32_t count, bool fold, double inv, float lo2, float hi2,
                                 const OcGrid& G, uint32_t shell, uint32_t* hits, uint32_t* misses) {
  sv_each_chunk(h_ent, count, OC_BLOCK, [&](uint32_t a, dim3 grid) {
    if (SUB) {
      if (fold) hipLaunchKernelGGL(k_oc_uncarve<true>, grid, dim3(OC_BLOCK), 0, str, d_ent + a, inv, lo2, hi2, G, shell, hits, misses);
      else hipLaunchKernelGGL(k_oc_uncarve<false>, grid, dim3(OC_BLOCK), 0, str, d_ent + a, inv, lo2, hi2, G, shell, hits, misses);
    } else {
      if (fold) hipLaunchKernelGGL(k_oc_carve<true>, grid, dim3(OC_BLOCK), 0, str, d_ent + a, inv, lo2, hi2, G, shell, hits, misses);
      else hipLaunchKernelGGL(k_oc_carve<false>, grid, dim3(OC_BLOCK), 0, str, d_ent + a, inv, lo2, hi2, G, shell, hits, misses);
    }
  });
}

}  // namespace

extern "C" int qn_kf_map_occupancy_update(qn_kf_store* s, const int32_t* ids, const double* poses16, uint32_t count, const qn_occupancy_params* params,
                                          qn_occupancy_stats* stats_out, qn_occupancy_update* update_out) {
  // ---- 1. the arguments as qn_kf_map_occupancy checks them, then the diff against the ledger on the host
  if (!stats_out || !update_out) return QN_ERR_INVALID_ARG;
  uint64_t tiles = 0;
  std::vector<OcEntry> list;
  const int ok = oc_check_list(s, ids, poses16, count, params, list, &tiles);
  if (ok != QN_OK) return ok;
  const qn_occupancy_params P = *params;
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  StaticState* unit = nullptr;
  const int rc = qn_kf_ext_state(s, QN_KF_INT_EXT_STATIC, &unit);
  if (rc != QN_OK) return rc;
  if (!unit->occ) unit->occ.reset(new (std::nothrow) OccState());
  if (unit->occ && !unit->occ->ledger) unit->occ->ledger.reset(new (std::nothrow) OccLedger());
  if (!unit->occ || !unit->occ->ledger) return qn_kf_fail(s, "qn_kf_map_occupancy_update: out of memory");
  OccState* st = unit->occ.get();
  OccLedger* led = st->ledger.get();
  const bool rebuilt = !(st->live && led->valid && led->par.voxel == P.voxel && led->par.min_range == P.min_range && led->par.max_range == P.max_range &&
                         led->par.shell == P.shell);
  const size_t key_bytes = sizeof(int32_t) + sizeof(double) * 12;
  auto key_of = [&](int32_t id, const double* pose) {
    std::string k(key_bytes, '\0');
    memcpy(&k[0], &id, sizeof(id)); memcpy(&k[sizeof(id)], pose, sizeof(double) * 12);
    return k;
  };
  std::unordered_multimap<std::string, uint32_t> unmatched;          // (id, the bytes of the pose) -> a ledger row; equal rows are interchangeable
  if (!rebuilt) for (uint32_t k = 0; k < led->rows.size(); k++) unmatched.emplace(key_of(led->rows[k].id, led->rows[k].P), k);
  std::vector<OuLedgerRow> rows(count);
  std::vector<uint32_t> added;                                       // list positions
  std::vector<OcEntry> ent;                                          // the added entries, then the removed rows
  for (uint32_t e = 0; e < count; e++) {
    const auto it = unmatched.find(key_of(ids[e], list[e].P));
    if (it != unmatched.end()) { rows[e] = led->rows[it->second]; unmatched.erase(it); continue; }
    rows[e].id = ids[e]; memcpy(rows[e].P, list[e].P, sizeof(rows[e].P));
    added.push_back(e); ent.push_back(list[e]);
  }
  const uint32_t na = (uint32_t)added.size(), nr = (uint32_t)unmatched.size();
  qn_occupancy_update u;
  memset(&u, 0, sizeof(u));
  u.entries_kept = count - na; u.entries_added = na; u.entries_removed = nr; u.rebuilt = rebuilt ? 1 : 0;
  int64_t dlo[3] = {INT_MAX, INT_MAX, INT_MAX}, dhi[3] = {INT_MIN, INT_MIN, INT_MIN};      // the boxes of the added and removed rows together
  auto widen = [](int64_t (&lo)[3], int64_t (&hi)[3], const OuRow& r) {
    if (r.cnt[1]) for (int k = 0; k < 3; k++) { lo[k] = std::min<int64_t>(lo[k], r.lo[k]); hi[k] = std::max<int64_t>(hi[k], r.hi[k]); }
  };
  for (const auto& kv : unmatched) {
    const OuLedgerRow& row = led->rows[kv.second];
    OcEntry E;
    E.pts = qn_kf_int_keyframe(s, row.id, &E.n); E.b0 = 0;
    memcpy(E.P, row.P, sizeof(E.P));
    ent.push_back(E);
    u.records_walked += row.r.cnt[0]; u.rays_removed += row.r.cnt[1];
    widen(dlo, dhi, row.r);
  }
  const hipStream_t str = qn_kf_int_stream(s);
  const double inv = 1.0 / P.voxel;
  const float lo2 = (float)(P.min_range * P.min_range), hi2 = (float)(P.max_range * P.max_range);
  // ---- scratch (0: the entries, 1: the added entries' rows and the flag behind them, 3 and 4: the classify blocks' slots, 5: the folded sums) and the pinned mirror
  const size_t ent_bytes = qn_up16(sizeof(OcEntry) * std::max<size_t>(ent.size(), 1)), row_bytes = sizeof(OuRow) * ((size_t)na + 1), small_bytes = 32;
  OcEntry* d_ent = (OcEntry*)qn_kf_int_scratch(s, 0, ent_bytes);
  OuRow* d_rows = (OuRow*)qn_kf_int_scratch(s, 1, row_bytes);
  char* d_small = (char*)qn_kf_int_scratch(s, 5, small_bytes);
  char* h = (char*)qn_kf_int_pinned(s, ent_bytes + 2 * row_bytes + small_bytes);
  if (!d_ent || !d_rows || !d_small || !h) return qn_kf_fail(s, "qn_kf_map_occupancy_update: scratch allocation failed");
  OuRow* h_init = (OuRow*)(h + ent_bytes); OuRow* h_rows = h_init + na + 1;
  char* h_small = h + ent_bytes + 2 * row_bytes;
  if (!ent.empty()) {
    memcpy(h, ent.data(), sizeof(OcEntry) * ent.size());
    QN_KFCHK(s, hipMemcpyAsync(d_ent, h, sizeof(OcEntry) * ent.size(), hipMemcpyHostToDevice, str));
  }
  // ---- 2. the extent of the added entries
  if (na) {
    memset(h_init, 0, row_bytes);
    for (uint32_t a = 0; a < na; a++) for (int k = 0; k < 3; k++) { h_init[a].lo[k] = INT_MAX; h_init[a].hi[k] = INT_MIN; }
    QN_KFCHK(s, hipMemcpyAsync(d_rows, h_init, row_bytes, hipMemcpyHostToDevice, str));
    sv_each_chunk(ent.data(), na, OC_BLOCK, [&](uint32_t a, dim3 grid) {
      hipLaunchKernelGGL(k_oc_extent_entry, grid, dim3(OC_BLOCK), 0, str, (const OcEntry*)(d_ent + a), inv, lo2, hi2, d_rows + a, &d_rows[na].lo[0]);
    });
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h_rows, d_rows, row_bytes, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                 // sync 1: the extent
    if (h_rows[na].lo[0]) {
      qn_kf_int_set_error(s, "qn_kf_map_occupancy_update: a ray end of 2^20 voxels or more from the origin");
      return QN_ERR_CAPACITY;
    }
    for (uint32_t a = 0; a < na; a++) {
      rows[added[a]].r = h_rows[a];
      u.records_walked += h_rows[a].cnt[0]; u.rays_added += h_rows[a].cnt[1];
      widen(dlo, dhi, h_rows[a]);
    }
  }
  // ---- 3. the new box: the union of the rows' boxes; every capacity refusal
  qn_occupancy_stats r;
  memset(&r, 0, sizeof(r));
  int64_t blo[3] = {INT_MAX, INT_MAX, INT_MAX}, bhi[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (const OuLedgerRow& row : rows) {
    r.n_records += row.r.cnt[0]; r.n_rays += row.r.cnt[1]; r.n_nonfinite += row.r.cnt[2]; r.n_near += row.r.cnt[3]; r.n_far += row.r.cnt[4];
    widen(blo, bhi, row.r);
  }
  qn_occupancy_grid info;
  memset(&info, 0, sizeof(info));
  info.voxel = P.voxel;
  if (r.n_rays) {
    uint64_t side[3];
    for (int k = 0; k < 3; k++) side[k] = (uint64_t)(bhi[k] - blo[k] + 1);
    if (side[0] > OC_MAX_SIDE || side[1] > OC_MAX_SIDE || side[2] > OC_MAX_SIDE || side[0] * side[1] * side[2] > (uint64_t)QN_OCC_MAX_CELLS) {
      qn_kf_int_set_error(s, "qn_kf_map_occupancy_update: a grid of more than 2^27 voxels (or 2^15 a side)");
      return QN_ERR_CAPACITY;
    }
    for (int k = 0; k < 3; k++) { info.minc[k] = (int32_t)blo[k]; info.origin[k] = (double)blo[k] * P.voxel; }
    info.width = (uint32_t)side[0]; info.height = (uint32_t)side[1]; info.depth = (uint32_t)side[2];
  }
  const OcGrid G = oc_grid(info);
  r.width = info.width; r.height = info.height; r.depth = info.depth;
  const uint32_t cells = G.cells, cb = dg_blocks(cells);
  const qn_occupancy_grid was = st->info;                   // (read only when !rebuilt)
  const bool regrid = !rebuilt && (was.width != info.width || was.height != info.height || was.depth != info.depth || was.minc[0] != info.minc[0] ||
                                   was.minc[1] != info.minc[1] || was.minc[2] != info.minc[2]);
  u.regridded = regrid ? 1 : 0;
  for (int k = 0; k < 3; k++) {
    const int64_t side = k == 0 ? info.width : k == 1 ? info.height : info.depth;
    dlo[k] = std::max<int64_t>(dlo[k] - info.minc[k], 0); dhi[k] = std::min<int64_t>(dhi[k] - info.minc[k], side - 1);
  }
  const bool dirty = dlo[0] <= dhi[0] && dlo[1] <= dhi[1] && dlo[2] <= dhi[2];
  for (int k = 0; k < 3; k++) { u.dirty_lo[k] = dirty ? (int32_t)dlo[k] : 0; u.dirty_hi[k] = dirty ? (int32_t)dhi[k] : -1; }
  // ---- what can fail for want of memory while the previous result is intact: the regrid's buffers, the class bytes beside the old ones, the slots
  DevBuf<uint8_t> fresh_cls;
  uint32_t* d_slots = nullptr; unsigned long long* d_tslots = nullptr;
  if (cells) {
    if (regrid && (!led->hits.grow(s, cells) || !led->misses.grow(s, cells))) return QN_ERR_HIP;
    if (!rebuilt && !st->cls.grow_beside(s, cells, fresh_cls)) return QN_ERR_HIP;
    d_slots = (uint32_t*)qn_kf_int_scratch(s, 3, sizeof(uint32_t) * 3 * (size_t)cb);
    d_tslots = (unsigned long long*)qn_kf_int_scratch(s, 4, sizeof(unsigned long long) * 2 * (size_t)cb);
    if (!d_slots || !d_tslots) return qn_kf_fail(s, "qn_kf_map_occupancy_update: scratch allocation failed");
  }
  // ---- from here on the previous result and its ledger are gone
  st->live = false; led->valid = false;
  const bool fold = getenv("QN_OCC_NO_FOLD") == nullptr;    // (a measuring switch: the results are the same bytes either way)
  if (rebuilt) {
    if (cells) {
      if (!st->hits.grow(s, cells) || !st->misses.grow(s, cells) || !st->cls.grow(s, cells)) return QN_ERR_HIP;
      QN_KFCHK(s, hipMemsetAsync(st->hits.p, 0, sizeof(uint32_t) * (size_t)cells, str));
      QN_KFCHK(s, hipMemsetAsync(st->misses.p, 0, sizeof(uint32_t) * (size_t)cells, str));
    }
  } else {
    // ---- 4. the removed rows' rays out of the old grid   5. the counts into the new box
    const OcGrid O = oc_grid(was);
    if (nr && O.cells) ou_walk<true>(str, ent.data() + na, d_ent + na, nr, fold, inv, lo2, hi2, O, P.shell, st->hits.p, st->misses.p);
    if (regrid && cells) {
      hipLaunchKernelGGL(k_oc_regrid, dim3(cb), dim3(OC_BLOCK), 0, str, G, O, was.depth, (const uint32_t*)st->hits.p, (const uint32_t*)st->misses.p, led->hits.p,
                         led->misses.p);
      st->hits.swap(led->hits); st->misses.swap(led->misses);
    }
    st->cls.adopt(fresh_cls);
  }
  if (cells) {
    // ---- 6. the added entries' rays   7. classify and count, as qn_kf_map_occupancy does
    if (na) ou_walk<false>(str, ent.data(), d_ent, na, fold, inv, lo2, hi2, G, P.shell, st->hits.p, st->misses.p);
    uint32_t* d_sums = (uint32_t*)d_small; unsigned long long* d_tot = (unsigned long long*)(d_small + 16);
    hipLaunchKernelGGL(k_oc_classify, dim3(cb), dim3(OC_BLOCK), 0, str, cells, (const uint32_t*)st->hits.p, (const uint32_t*)st->misses.p, P.min_hits, P.hit_weight,
                       st->cls.p, d_slots, d_tslots);
    hipLaunchKernelGGL((k_slot_fold<uint32_t, 3>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const uint32_t*)d_slots, cb, d_sums);
    hipLaunchKernelGGL((k_slot_fold<unsigned long long, 2>), dim3(1), dim3(MO_SCAN_BLOCK), 0, str, (const unsigned long long*)d_tslots, cb, d_tot);
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipMemcpyAsync(h_small, d_small, small_bytes, hipMemcpyDeviceToHost, str));
    QN_KFCHK(s, hipStreamSynchronize(str));                 // sync 2: the counts
    const uint32_t* sums = (const uint32_t*)h_small; const unsigned long long* tot = (const unsigned long long*)(h_small + 16);
    r.occupied = sums[0]; r.free = sums[1]; r.unknown = sums[2];
    r.total_hits = tot[0]; r.total_misses = tot[1];
  } else {
    QN_KFCHK(s, hipGetLastError());
    QN_KFCHK(s, hipStreamSynchronize(str));                 // (a subtraction into a grid that goes: drained before the call returns)
  }
  st->info = info;
  st->live = true;
  led->par = P; led->rows.swap(rows); led->valid = true;
  md_end(st->dist.get());
  mf_end(st->frontier.get());
  mv_end(st->view.get());
  *stats_out = r;
  *update_out = u;
  return QN_OK;
}
