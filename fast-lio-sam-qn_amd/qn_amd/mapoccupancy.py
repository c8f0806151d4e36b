"""A 3-D occupancy map (occupied, free, unknown) by ray carving: the numpy twin of csrc/qn_mapoccupancy.inc (qn_kf_map_occupancy / _grid / _list / _slice) and
its specification.  Pure numpy, no GPU.

Every keyframe record is a ray from that keyframe's corrected sensor position to a world point.  The rays of a list of keyframes with poses (the list build_map
takes: ids may repeat, a list position is an ENTRY) are walked through a voxel grid; the voxel a ray ends in gets a hit, the voxels it crossed get a miss.

  params       OccupancyParams(voxel, min_range, max_range, shell, min_hits, hit_weight): voxel finite > 0 (0.3), min_range finite >= 0 (0.5), max_range finite >
               min_range (60), shell a u32 (1), min_hits >= 1 (1), hit_weight >= 1 (2).  The defaults are interface choices, not measurements.
  records      record p = (x, y, z) of entry e, f32, sensor frame.  Skipped and counted n_nonfinite when a coordinate is not finite.  Otherwise d2 = x x + y y + z z
               in f32, left to right, no fused multiply-add (the overlap measure's arithmetic); skipped and counted n_near when d2 < float32(min_range^2), n_far when
               d2 > float32(max_range^2) (the squares formed in f64, rounded once).  Everything else is a ray.  A far record is dropped whole, not truncated:
               truncation needs a square root on the path.
  ray ends     f64, every operation rounded on its own: origin O = (P3, P7, P11) of the entry's row-major pose, end W = ((P0 x + P1 y) + P2 z) + P3 per row (the
               static vote's arithmetic), the f32 coordinates widened first.  inv = 1.0 / voxel.  Fixed point with S = 10 fractional bits:
               A_k = int64(rint((O_k * inv) * 1024.0)), B_k likewise from W, rounded half to even.  CapacityError when a ray has |O_k * inv| or |W_k * inv| >= 2^20
               (or not a number).
  walk         integers only.  c = A >> S (an arithmetic shift: a floor), cend = B >> S.  Per axis k: s_k = sign(B_k - A_k), D_k = |B_k - A_k|, rem_k = |cend_k - c_k|,
               r_k = ((c_k + 1) << S) - A_k when s_k > 0, else A_k - (c_k << S) (0 for an origin on a face heading down: that axis steps at once).  n = rem_x +
               rem_y + rem_z times: among the axes with rem_k > 0 the one with the smallest r_k / D_k, compared as r_a D_b < r_b D_a in int64, a tie to the lowest
               axis; then c_k += s_k, r_k += 1 << S, rem_k -= 1.  The visited voxels are v_0 = c(A), ..., v_n = c(B).
  counts       u32 per voxel: hits[v_n] += 1; misses[v_i] += 1 for 0 <= i < n - shell (none when n <= shell).  A ray never carves its own end voxel, and `shell`
               keeps the last voxels before a surface out of the carving.
  grid         minc, maxc per axis from c(A) and c(B) of all rays (the walk is monotone per axis, so it stays inside).  W x H x D, x fastest, z slowest: linear
               index (iz H + iy) W + ix; the arrays are (D, H, W).  CapacityError when a dimension exceeds MAX_SIDE = 2^15 or W H D > MAX_CELLS = 2^27.  Without
               a ray the grid is 0 x 0 x 0 and minc (0, 0, 0).
  classes      one byte per voxel: UNKNOWN 0 (hits = misses = 0), OCCUPIED 2 (hits >= min_hits and hits * hit_weight >= misses), FREE 1 (everything else).
Everything after the quantisation is an integer and integer adds commute, so no order of anything changes a byte.
  update       the same volume brought to another list in place (update(), the twin of csrc/qn_mapoccupancy_update.inc, qn_kf_map_occupancy_update): for the same
               reason an entry's counts leave again when its rays are walked with -1, and the result is classify's of the new list in every byte.
"""
import math
from collections import namedtuple
import numpy as np

OccupancyParams = namedtuple("OccupancyParams", "voxel min_range max_range shell min_hits hit_weight", defaults=(0.3, 0.5, 60.0, 1, 1, 2))   # interface choices
OccupancyStats = namedtuple("OccupancyStats", "n_records n_rays n_nonfinite n_near n_far total_hits total_misses width height depth occupied free unknown")
OccupancyGrid = namedtuple("OccupancyGrid", "origin voxel width height depth minc")
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
S = 10
ONE = 1 << S
COORD_LIMIT = float(1 << 20)
MAX_SIDE = 1 << 15
MAX_CELLS = 1 << 27
FLUSH = 1 << 22                                      # classify(): visited voxels held back before they are counted


class CapacityError(ValueError):
    """what the C library answers with QN_ERR_CAPACITY"""


def check_params(p):
    v, lo, hi = (float(x) for x in p[:3])
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("mapoccupancy: voxel must be finite and > 0")
    if not (math.isfinite(lo) and lo >= 0.0):
        raise ValueError("mapoccupancy: min_range must be finite and >= 0")
    if not (math.isfinite(hi) and hi > lo):
        raise ValueError("mapoccupancy: max_range must be finite and > min_range")
    for name, x, least in (("shell", p[3], 0), ("min_hits", p[4], 1), ("hit_weight", p[5], 1)):
        if int(x) != x or not (least <= int(x) <= 0xffffffff):
            raise ValueError("mapoccupancy: %s must be an integer >= %d" % (name, least))


def range_bounds(p):
    """-> (float32(min_range^2), float32(max_range^2)), the squares formed in f64"""
    return np.float32(np.float64(p[1]) * np.float64(p[1])), np.float32(np.float64(p[2]) * np.float64(p[2]))


def quantise(v, inv):
    """world coordinates (f64, any shape) -> their fixed-point integers int64(rint((v * inv) * 1024)); CapacityError when a |v * inv| is not below 2^20"""
    t = np.asarray(v, np.float64) * np.float64(inv)
    if t.size and not (np.abs(t) < COORD_LIMIT).all():
        raise CapacityError("mapoccupancy: a ray end of 2^20 voxels or more from the origin")
    return np.rint(t * np.float64(1024.0)).astype(np.int64)


def walk(A, B):
    """one ray between the fixed-point ends A and B (three Python integers each) -> the list of visited voxels [(cx, cy, cz)], v_0 = c(A) .. v_n = c(B).
    Pure integers."""
    A = [int(a) for a in A]; B = [int(b) for b in B]
    c = [a >> S for a in A]; cend = [b >> S for b in B]
    s = [(b > a) - (b < a) for a, b in zip(A, B)]
    D = [abs(b - a) for a, b in zip(A, B)]
    rem = [abs(e - k) for e, k in zip(cend, c)]
    r = [(((c[k] + 1) << S) - A[k]) if s[k] > 0 else (A[k] - (c[k] << S)) for k in range(3)]
    out = [tuple(c)]
    for _ in range(sum(rem)):
        best = -1
        for k in range(3):
            if rem[k] > 0 and (best < 0 or r[k] * D[best] < r[best] * D[k]):
                best = k
        c[best] += s[best]; r[best] += ONE; rem[best] -= 1
        out.append(tuple(c))
    return out


def rays(keyframes, poses, params=None):
    """the accepted records of every entry as fixed-point rays -> (A (m, 3) int64, B (m, 3) int64, [n_records, n_rays, n_nonfinite, n_near, n_far])"""
    p = OccupancyParams() if params is None else OccupancyParams(*params)
    check_params(p)
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(P) != len(keyframes):
        raise ValueError("mapoccupancy: %d entries but %d poses" % (len(keyframes), len(P)))
    if not np.isfinite(P).all():
        raise ValueError("mapoccupancy: a pose that is not finite")
    lo2, hi2 = range_bounds(p)
    inv = np.float64(1.0) / np.float64(p.voxel)
    As, Bs = [], []
    cnt = [0, 0, 0, 0, 0]
    for cloud, T in zip(keyframes, P):
        a = np.asarray(cloud)
        if a.ndim != 2 or (len(a) and a.shape[1] < 3):
            raise ValueError("mapoccupancy: an (n, >= 3) array of records per entry")
        a = np.ascontiguousarray(a[:, :3], np.float32) if len(a) else np.zeros((0, 3), np.float32)
        cnt[0] += len(a)
        fin = np.isfinite(a).all(axis=1)
        cnt[2] += int((~fin).sum())
        f = a[fin]
        with np.errstate(over="ignore"):
            d2 = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]          # f32, left to right
        near = d2 < lo2
        far = ~near & (d2 > hi2)
        cnt[3] += int(near.sum()); cnt[4] += int(far.sum())
        f = f[~near & ~far].astype(np.float64)
        if not len(f):
            continue
        cnt[1] += len(f)
        W = np.stack([((T[k, 0] * f[:, 0] + T[k, 1] * f[:, 1]) + T[k, 2] * f[:, 2]) + T[k, 3] for k in range(3)], axis=1)
        Bs.append(quantise(W, inv))
        As.append(np.broadcast_to(quantise(T[:3, 3], inv), (len(f), 3)))
    if cnt[0] >= 1 << 32:
        raise CapacityError("mapoccupancy: 2^32 records or more")
    if not As:
        z = np.zeros((0, 3), np.int64)
        return z, z.copy(), cnt
    return np.concatenate(As), np.concatenate(Bs), cnt


def class_of(hits, misses, min_hits=1, hit_weight=2):
    """the class rule on arrays of counts -> uint8"""
    h = np.asarray(hits).astype(np.uint64); m = np.asarray(misses).astype(np.uint64)
    occ = (h >= np.uint64(min_hits)) & (h * np.uint64(hit_weight) >= m)
    return np.where((h == 0) & (m == 0), UNKNOWN, np.where(occ, OCCUPIED, FREE)).astype(np.uint8)


def classify(keyframes, poses, params=None):
    """keyframes[e] = the (n, >= 3) f32 records of entry e, poses[e] its 4x4 f64 pose
    -> dict(hits (D, H, W) u32, misses (D, H, W) u32, classes (D, H, W) u8, stats: an OccupancyStats, grid: an OccupancyGrid).  All rays advance together, one
    walk step a round, so the cost is the longest ray's rounds of numpy work."""
    p = OccupancyParams() if params is None else OccupancyParams(*params)
    A, B, cnt = rays(keyframes, poses, p)
    voxel = float(p.voxel)
    if not len(A):
        z = np.zeros((0, 0, 0), np.uint32)
        return dict(hits=z, misses=z.copy(), classes=z.astype(np.uint8), stats=OccupancyStats(*cnt, 0, 0, 0, 0, 0, 0, 0, 0),
                    grid=OccupancyGrid((0.0, 0.0, 0.0), voxel, 0, 0, 0, (0, 0, 0)))
    c = A >> S; cend = B >> S
    minc = np.minimum(c.min(axis=0), cend.min(axis=0)); maxc = np.maximum(c.max(axis=0), cend.max(axis=0))
    Wd, Hd, Dd = (int(v) for v in maxc - minc + 1)
    if max(Wd, Hd, Dd) > MAX_SIDE or Wd * Hd * Dd > MAX_CELLS:
        raise CapacityError("mapoccupancy: a grid of more than 2^27 voxels (or 2^15 a side)")
    cells = Wd * Hd * Dd
    stride = np.array([1, Wd, Wd * Hd], np.int64)
    s = np.sign(B - A)
    D = np.abs(B - A)
    rem = np.abs(cend - c)
    r = np.where(s > 0, ((c + 1) << S) - A, A - (c << S))
    n = rem.sum(axis=1)
    lin = ((c - minc) * stride).sum(axis=1)
    hits = np.bincount(((cend - minc) * stride).sum(axis=1), minlength=cells).astype(np.int64)
    misses = np.zeros(cells, np.int64)
    carve = n - int(p.shell)                         # the steps i < carve leave a miss
    step = s * stride
    idx = np.arange(len(A))
    pending = []; held = 0

    def flush():                                     # the visited voxels gathered so far into the counts, one bincount for many rounds
        nonlocal held, misses
        if pending:
            misses += np.bincount(np.concatenate(pending), minlength=cells)
        pending.clear(); held = 0

    i = 0
    while True:
        live = n[idx] > i
        if not live.all():
            idx = idx[live]
        if not len(idx):
            break
        m = carve[idx] > i
        if m.any():
            pending.append(lin[idx[m]]); held += int(m.sum())
            if held > FLUSH:
                flush()
        rr = r[idx]; DD = D[idx]; on = rem[idx] > 0
        best = np.where(on[:, 0], 0, np.where(on[:, 1], 1, 2))
        for k in (1, 2):
            rb = np.take_along_axis(rr, best[:, None], 1)[:, 0]; Db = np.take_along_axis(DD, best[:, None], 1)[:, 0]
            better = on[:, k] & (k > best) & (rr[:, k] * Db < rb * DD[:, k])
            best = np.where(better, k, best)
        lin[idx] += step[idx, best]
        r[idx, best] += ONE
        rem[idx, best] -= 1
        i += 1
    flush()
    hits = hits.astype(np.uint32).reshape(Dd, Hd, Wd); misses = misses.astype(np.uint32).reshape(Dd, Hd, Wd)
    cls = class_of(hits, misses, int(p.min_hits), int(p.hit_weight))
    stats = OccupancyStats(*cnt, int(hits.sum(dtype=np.uint64)), int(misses.sum(dtype=np.uint64)), Wd, Hd, Dd, int((cls == OCCUPIED).sum()), int((cls == FREE).sum()),
                           int((cls == UNKNOWN).sum()))
    grid = OccupancyGrid(tuple(float(m) * voxel for m in minc), voxel, Wd, Hd, Dd, tuple(int(m) for m in minc))
    return dict(hits=hits, misses=misses, classes=cls, stats=stats, grid=grid)


def check_mask(mask):
    if int(mask) != mask or int(mask) == 0 or int(mask) & ~7:
        raise ValueError("mapoccupancy: class_mask must have at least one of the bits 0 .. 2 set and no other")
    return int(mask)


def voxel_list(result, mask):
    """-> (ijk (m, 3) int32 grid indices (ix, iy, iz), hits (m,) u32, misses (m,) u32) of the voxels whose class bit (1 << class) is set in mask, in ascending
    linear index (what qn_kf_map_occupancy_list returns)"""
    m = check_mask(mask)
    cls = result["classes"]
    Dd, Hd, Wd = cls.shape
    k = np.flatnonzero(((m >> cls.reshape(-1).astype(np.int64)) & 1) == 1)
    ijk = np.stack([k % Wd, (k // Wd) % Hd, k // (Wd * Hd)], axis=1).astype(np.int32) if Wd else np.zeros((0, 3), np.int32)
    return ijk, result["hits"].reshape(-1)[k], result["misses"].reshape(-1)[k]


def slice2d(classes, iz_lo, iz_hi):
    """per column over the layers iz_lo .. iz_hi inclusive, clipped to the grid: 2 if any voxel is OCCUPIED, else 1 if any is FREE, else 0 -> (H, W) uint8, the
    values of mapground's occupancy (to_pgm / map_yaml serve it); here free means that a ray passed"""
    if int(iz_lo) > int(iz_hi):
        raise ValueError("mapoccupancy: iz_lo > iz_hi")
    cls = np.asarray(classes, np.uint8)
    Dd, Hd, Wd = cls.shape
    lo, hi = max(int(iz_lo), 0), min(int(iz_hi), Dd - 1)
    if lo > hi:
        return np.zeros((Hd, Wd), np.uint8)
    return cls[lo:hi + 1].max(axis=0)


def layer_of(z, grid):
    """the layer index iz of world height z in `grid`, by the quantisation's own arithmetic (it may lie outside 0 .. depth - 1)"""
    g = OccupancyGrid(*grid)
    return int(quantise(float(z), np.float64(1.0) / np.float64(g.voxel)) >> S) - int(g.minc[2])


def centres(ijk, grid):
    """the centres (minc + i + 0.5) * voxel of the voxels ijk -> (m, 3) f64"""
    g = OccupancyGrid(*grid)
    return (np.asarray(ijk, np.float64).reshape(-1, 3) + np.asarray(g.minc, np.float64) + 0.5) * float(g.voxel)


# ---- the volume updated in place: the specification of qn_kf_map_occupancy_update (csrc/qn_mapoccupancy_update.inc)
OccupancyUpdate = namedtuple("OccupancyUpdate", "entries_kept entries_added entries_removed rebuilt regridded records_walked dirty_lo dirty_hi rays_added rays_removed")


def accumulate(A, B, minc, dims, shell, sign, hits, misses):
    """the rays A -> B (fixed point, (m, 3) int64) walked through the grid at voxel minc of dims = (W, H, D): hits[v_n] += sign and misses[v_i] += sign for
    i < n - shell, in place on the flat int64 arrays.  The walk is walk()'s, all rays one step a round."""
    if not len(A):
        return
    Wd, Hd, Dd = (int(v) for v in dims)
    cells = Wd * Hd * Dd
    minc = np.asarray(minc, np.int64)
    stride = np.array([1, Wd, Wd * Hd], np.int64)
    c = A >> S; cend = B >> S
    assert ((c >= minc) & (cend >= minc) & (c < minc + np.array([Wd, Hd, Dd])) & (cend < minc + np.array([Wd, Hd, Dd]))).all(), "a ray end outside the grid"
    s = np.sign(B - A); D = np.abs(B - A); rem = np.abs(cend - c)
    r = np.where(s > 0, ((c + 1) << S) - A, A - (c << S))
    n = rem.sum(axis=1)
    lin = ((c - minc) * stride).sum(axis=1)
    hits += sign * np.bincount(((cend - minc) * stride).sum(axis=1), minlength=cells)
    carve = n - int(shell)
    step = s * stride
    idx = np.arange(len(A))
    i = 0
    while True:
        live = n[idx] > i
        if not live.all():
            idx = idx[live]
        if not len(idx):
            break
        m = carve[idx] > i
        if m.any():
            misses += sign * np.bincount(lin[idx[m]], minlength=cells)
        rr = r[idx]; DD = D[idx]; on = rem[idx] > 0
        best = np.where(on[:, 0], 0, np.where(on[:, 1], 1, 2))
        for k in (1, 2):
            rb = np.take_along_axis(rr, best[:, None], 1)[:, 0]; Db = np.take_along_axis(DD, best[:, None], 1)[:, 0]
            best = np.where(on[:, k] & (k > best) & (rr[:, k] * Db < rb * DD[:, k]), k, best)
        lin[idx] += step[idx, best]
        r[idx, best] += ONE
        rem[idx, best] -= 1
        i += 1


def _pose44(rows34):
    T = np.eye(4)
    T[:3] = rows34
    return T


def update(ledger, clouds, ids, poses, params=None):
    """The volume of `ledger` (None: none yet) brought to the list (ids, poses): clouds[id] = the (n, >= 3) f32 records of keyframe id, poses[e] the 4x4 f64 pose
    of entry e.  -> (result, upd, ledger): result has the form of classify's and equals classify of the list in every array, statistic and the grid; upd is an
    OccupancyUpdate; ledger is the new state (the one passed in is not changed, so a refused call - an exception - leaves it good).
      ledger   ray_params (voxel, min_range, max_range, shell); rows, one per entry: id, the pose's first 12 doubles, the five record counts, the box (lo, hi) of
               the entry's ray ends in voxel coordinates or None without a ray; minc, dims (W, H, D); hits, misses (flat int64); outside: the counts the last
               regrid found in old voxels outside the new box (always 0, asserted).
      match    a multiset: an entry is kept when its id and the bytes of its 12 doubles equal an unmatched row (so -0.0 is not 0.0); the unmatched rows are
               removed, the unmatched entries added.  Without a ledger, or with another voxel, min_range, max_range or shell: rebuilt - every entry is added to
               an empty volume.  min_hits and hit_weight only form the classes.
      box      the union of the boxes of the new rows; without a ray 0 x 0 x 0 at minc (0, 0, 0).  CapacityError as classify raises it, before anything changes.
      order    the removed rows' rays with -1 in the old grid (from clouds[row id] under the row's pose); when the box differs, the counts of the voxels both
               boxes hold move, every other new voxel starts at 0; the added entries' rays with +1; the classes.
      dirty    the union of the boxes of the added and removed rows minus the new minc, clipped to the new grid; (0, 0, 0) > (-1, -1, -1) when that is empty."""
    p = OccupancyParams() if params is None else OccupancyParams(*params)
    check_params(p)
    ids = [int(i) for i in ids]
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if not ids or len(P) != len(ids):
        raise ValueError("mapoccupancy: %d entries but %d poses" % (len(ids), len(P)))
    if not np.isfinite(P).all():
        raise ValueError("mapoccupancy: a pose that is not finite")
    ray_params = (float(p.voxel), float(p.min_range), float(p.max_range), int(p.shell))
    rebuilt = ledger is None or ledger["ray_params"] != ray_params
    old_rows = [] if rebuilt else ledger["rows"]
    unmatched = {}
    for k, row in enumerate(old_rows):
        unmatched.setdefault((row["id"], row["pose"].tobytes()), []).append(k)
    rows, fresh = [], []
    for i, T in zip(ids, P):
        pose = np.ascontiguousarray(T[:3])
        left = unmatched.get((i, pose.tobytes()))
        if left:
            rows.append(old_rows[left.pop()])
            continue
        A, B, cnt = rays([clouds[i]], [T], p)
        c = np.concatenate([A >> S, B >> S])
        row = dict(id=i, pose=pose.copy(), cnt=tuple(cnt), box=(tuple(int(v) for v in c.min(axis=0)), tuple(int(v) for v in c.max(axis=0))) if len(A) else None)
        rows.append(row); fresh.append((row, A, B))
    gone = [old_rows[k] for left in unmatched.values() for k in left]
    if sum(r["cnt"][0] for r in rows) >= 1 << 32:
        raise CapacityError("mapoccupancy: 2^32 records or more")
    boxes = [r["box"] for r in rows if r["box"]]
    voxel = float(p.voxel)
    if boxes:
        minc = np.min([b[0] for b in boxes], axis=0).astype(np.int64); maxc = np.max([b[1] for b in boxes], axis=0).astype(np.int64)
        dims = tuple(int(v) for v in maxc - minc + 1)
        if max(dims) > MAX_SIDE or dims[0] * dims[1] * dims[2] > MAX_CELLS:
            raise CapacityError("mapoccupancy: a grid of more than 2^27 voxels (or 2^15 a side)")
    else:
        minc = np.zeros(3, np.int64); dims = (0, 0, 0)
    cells = dims[0] * dims[1] * dims[2]
    outside = 0
    if rebuilt:
        regridded = False
        hits = np.zeros(cells, np.int64); misses = np.zeros(cells, np.int64)
    else:
        ominc = np.asarray(ledger["minc"], np.int64); odims = tuple(ledger["dims"])
        hits = ledger["hits"].copy(); misses = ledger["misses"].copy()
        for row in gone:
            A, B, _ = rays([clouds[row["id"]]], [_pose44(row["pose"])], p)
            accumulate(A, B, ominc, odims, p.shell, -1, hits, misses)
        assert (hits >= 0).all() and (misses >= 0).all(), "a count below zero"
        regridded = odims != dims or (ominc != minc).any()
        if regridded:
            oh = hits.reshape(odims[::-1]); om = misses.reshape(odims[::-1])
            hits = np.zeros(dims[::-1], np.int64); misses = np.zeros(dims[::-1], np.int64)
            lo = np.maximum(ominc, minc); hi = np.minimum(ominc + odims, minc + dims)             # the voxels both boxes hold, hi exclusive
            moved = 0
            if (lo < hi).all():
                src = tuple(slice(int(lo[k] - ominc[k]), int(hi[k] - ominc[k])) for k in (2, 1, 0))
                dst = tuple(slice(int(lo[k] - minc[k]), int(hi[k] - minc[k])) for k in (2, 1, 0))
                hits[dst] = oh[src]; misses[dst] = om[src]
                moved = int(oh[src].sum() + om[src].sum())
            outside = int(oh.sum() + om.sum()) - moved
            assert outside == 0, "an old voxel outside the new box still held a count"
            hits = hits.reshape(-1); misses = misses.reshape(-1)
    for row, A, B in fresh:
        accumulate(A, B, minc, dims, p.shell, +1, hits, misses)
    walked = [r for r, _, _ in fresh] + gone
    wb = [r["box"] for r in walked if r["box"]]
    dlo, dhi = (0, 0, 0), (-1, -1, -1)
    if wb:
        a = np.maximum(np.min([b[0] for b in wb], axis=0) - minc, 0); b = np.minimum(np.max([b[1] for b in wb], axis=0) - minc, np.array(dims) - 1)
        if (a <= b).all():
            dlo, dhi = tuple(int(v) for v in a), tuple(int(v) for v in b)
    upd = OccupancyUpdate(len(ids) - len(fresh), len(fresh), len(gone), int(rebuilt), int(regridded), sum(r["cnt"][0] for r in walked), dlo, dhi,
                          sum(r["cnt"][1] for r, _, _ in fresh), sum(r["cnt"][1] for r in gone))
    shape = dims[::-1]
    h = hits.astype(np.uint32).reshape(shape); m = misses.astype(np.uint32).reshape(shape)
    cls = class_of(h, m, int(p.min_hits), int(p.hit_weight))
    cnt = [sum(r["cnt"][k] for r in rows) for k in range(5)]
    stats = OccupancyStats(*cnt, int(h.sum(dtype=np.uint64)), int(m.sum(dtype=np.uint64)), dims[0], dims[1], dims[2], int((cls == OCCUPIED).sum()),
                           int((cls == FREE).sum()), int((cls == UNKNOWN).sum()))
    grid = OccupancyGrid(tuple(float(v) * voxel for v in minc), voxel, dims[0], dims[1], dims[2], tuple(int(v) for v in minc))
    new = dict(ray_params=ray_params, rows=rows, minc=tuple(int(v) for v in minc), dims=dims, hits=hits, misses=misses, outside=outside)
    return dict(hits=h, misses=m, classes=cls, stats=stats, grid=grid), upd, new
