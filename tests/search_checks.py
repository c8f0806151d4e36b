"""References for the direct tests of the neighbour search's building blocks (csrc/qn_device.cuh through qn_debug_search; the record layouts are those of
include/qn_engine.h), shared by tests/test_search_cpu.py (the references against each other and against exact arithmetic) and tests/test_gpu_search.py
(the device).  No GPU.

The grid's numbers are restated from grid_dims_from_bbox, the bounds in numpy f32 operation by operation (the library is built without contraction and with
correctly rounded f32 divide and square root, so they are restatable to the bit), the sinks twice - serially, step by step, and from a sort - and the searches as a
brute force whose key is (f32 d2 in sqdist's order (dx^2 + dy^2) + dz^2, original index)."""
import numpy as np

F = np.float32
INF = F(np.inf)
INF_KEY = (1 << 64) - 1
U24 = 2.0 ** -24


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def b1(x):
    """the bits of one f32 as a Python int"""
    return int(np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)[0])


def f1(u):
    """one f32 from its bits"""
    return np.asarray(int(u) & 0xffffffff, dtype=np.uint32).reshape(1).view(np.float32)[0]


def fbits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ the grid
class Grid:
    """grid_dims_from_bbox for a finite cloud under the knob `cell` (the table of the test clouds fits: no coarsening)"""

    def __init__(self, xyz, cell):
        p = np.asarray(xyz, dtype=np.float32)
        mn, mx = p.min(axis=0), p.max(axis=0)
        L = np.maximum(mx.astype(np.float64) - mn.astype(np.float64), 0.0)
        self.o = mn.copy()
        self.cell = F(cell)
        self.inv = F(1.0) / self.cell
        self.dims = (np.floor(L / float(cell)).astype(np.int64) + 1)
        self.tdims = (self.dims + np.array([7, 3, 3])) // np.array([8, 4, 4])
        amax = F(max(np.abs(mn).max(), np.abs(mx).max()))
        self.eps = F(F(1e-3) * self.cell) + F(F(1e-6) * F(amax + F(L.max())))
        self.ncells = int(np.prod(self.tdims)) * 128
        self.n = len(p)

    def cell_coord(self, v, axis):
        """clampi((int)floorf((v - o) * inv), 0, n - 1), f32"""
        t = np.floor((np.asarray(v, dtype=np.float32) - self.o[axis]) * self.inv)
        return np.clip(t, 0, self.dims[axis] - 1).astype(np.int64)

    def cells(self, p):
        p = np.asarray(p, dtype=np.float32)
        return np.stack([self.cell_coord(p[..., a], a) for a in range(3)], axis=-1)

    def cell_key(self, c):
        x, y, z = c[..., 0], c[..., 1], c[..., 2]
        tile = ((z >> 2) * self.tdims[1] + (y >> 2)) * self.tdims[0] + (x >> 3)
        return (tile << 7) | ((z & 3) << 5) | ((y & 3) << 3) | (x & 7)

    def tile_of(self, c):
        return np.stack([c[..., 0] >> 3, c[..., 1] >> 2, c[..., 2] >> 2], axis=-1)

    # ---- the bounds, f32 operation by operation
    def tile_box_d2(self, t, q, shrink=True, factor=F(0.999998)):
        """tile_box_d2(g, tx, ty, tz, qx, qy, qz); t (..., 3) ints, q (..., 3) f32.  shrink=False / factor=1: deliberately wrong variants"""
        t = np.asarray(t); q = np.asarray(q, dtype=np.float32)
        d = []
        for a, w in enumerate((8, 4, 4)):
            lo = self.o[a] + (t[..., a] * w).astype(np.float32) * self.cell
            hi = self.o[a] + np.minimum(t[..., a] * w + w, self.dims[a]).astype(np.float32) * self.cell
            m = np.maximum(lo - q[..., a], q[..., a] - hi)
            d.append(np.maximum(m - self.eps if shrink else m, F(0)))
        return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * factor

    def cap_of(self, q):
        q = np.asarray(q, dtype=np.float32)
        o2 = []
        for a in range(3):
            hi = self.o[a] + F(self.dims[a]) * self.cell
            o = np.maximum(np.maximum(self.o[a] - q[..., a], q[..., a] - hi), F(0))
            o2.append(o * o)
        o2 = np.stack(o2, axis=-1)
        return o2, (o2[..., 0] + o2[..., 1]) + o2[..., 2]

    def cap_extent(self, o2, S, r, axis, up=True):
        r = np.asarray(r, dtype=np.float32)
        rest = S - o2[..., axis]
        v = r * r - rest * (F(0.999999) if up else F(1))
        with np.errstate(invalid="ignore"):
            e = np.where(v > 0, np.sqrt(np.maximum(v, F(0))) * (F(1.000001) if up else F(1)) + (self.eps if up else F(0)), self.eps if up else F(0)).astype(np.float32)
        return np.where(rest <= 0, r, e).astype(np.float32)

    def cap_face_dist(self, o2, S, f, axis, down=True):
        f = np.asarray(f, dtype=np.float32)
        rest = (S - o2[..., axis]) * (F(0.999999) if down else F(1))
        return np.where(rest > 0, np.sqrt(f * f + rest) * (F(0.999999) if down else F(1)), f).astype(np.float32)

    def exact_outside(self, q):
        """the exact distance from q to the grid box [o, o + n cell] per axis, f64 (the f32 inputs are exact in f64; n cell and the sums round at 2^-53)"""
        q = np.asarray(q, dtype=np.float64)
        o = self.o.astype(np.float64)
        hi = o + self.dims * float(self.cell)
        return np.maximum(np.maximum(o - q, q - hi), 0.0)


def sqdist32(q, p):
    """sqdist: (dx^2 + dy^2) + dz^2 in f32; q (Q, 3), p (N, 3) -> (Q, N)"""
    q = np.asarray(q, dtype=np.float32)[:, None, :]; p = np.asarray(p, dtype=np.float32)[None, :, :]
    d = q - p
    d2 = d * d
    return (d2[..., 0] + d2[..., 1]) + d2[..., 2]


def pack_keys(d2, idx):
    return (bits(d2).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.uint64)


def brute_force(q, pts):
    """-> key (Q,) uint64 of the nearest point by (f32 d2, index), and the exact side: i1 (Q,) the index of a nearest point in f64, D1 its distance, D2 the
    distance of the nearest point other than i1 (f64 from the f32 coordinates: exact differences, sums rounded at 2^-53)"""
    d2 = sqdist32(q, pts)
    keys = pack_keys(d2, np.broadcast_to(np.arange(len(pts)), d2.shape))
    best = keys.min(axis=1)
    dd = np.asarray(q, dtype=np.float64)[:, None, :] - np.asarray(pts, dtype=np.float64)[None, :, :]
    ex = np.sqrt((dd * dd).sum(axis=2))
    ar = np.arange(len(ex))
    i1 = ex.argmin(axis=1)
    D1 = ex[ar, i1].copy()
    ex[ar, i1] = np.inf
    return best, i1, D1, ex.min(axis=1)


def distance_to_the_others(truth, idx):
    """D of the bound check: the exact distance from each query to the nearest point other than point idx (idx < 0: no key, the nearest point at all)"""
    _, i1, D1, D2 = truth
    return np.where(np.asarray(idx) == i1, D2, D1)


def box_points(grid, pts, box):
    """the original indices of the points whose restated cell lies in the inclusive cell box (x0, x1, y0, y1, z0, z1)"""
    c = grid.cells(pts)
    m = np.ones(len(c), dtype=bool)
    for a in range(3):
        m &= (c[:, a] >= box[2 * a]) & (c[:, a] <= box[2 * a + 1])
    return np.flatnonzero(m)


def widen(grid, box):
    """a cell box widened to whole tiles, as every tile-mode caller does"""
    b = list(box)
    for a, w in enumerate((8, 4, 4)):
        b[2 * a] = (b[2 * a] // w) * w
        b[2 * a + 1] = min((b[2 * a + 1] // w) * w + w - 1, int(grid.dims[a]) - 1)
    return tuple(b)


# ------------------------------------------------------------------ Best1, twice
def _med3(a, b, c):
    return sorted((a, b, c))[1]


def best1_serial(seq, unique, keep_higher_on_ties=False):
    """one lane of Best1 step by step: seq = [(on, d2 (np.float32), idx)] -> (key, second, bd).  keep_higher_on_ties: a deliberately wrong variant"""
    key, second, bd = INF_KEY, INF, INF
    for on, d2, idx in seq:
        k = (b1(d2) << 32) | int(idx)
        lt = on and (k < key if not keep_higher_on_ties else (k >> 32, -(k & 0xffffffff)) < (key >> 32, -(key & 0xffffffff)))
        d2e = d2 if (on and (unique or k != key)) else INF
        second = _med3(bd, second, d2e)
        if lt:
            bd, key = d2, k
    return key, F(second), F(bd)


def best1_sorted(seq, unique):
    """the same from a sort: the smallest key wins; second = the smallest d2 among the records other than the winner's (not UNIQUE: a record that repeats
    the winner's key is the same point again and does not count; UNIQUE: every record but one of the winner's counts)"""
    recs = sorted(((b1(d2) << 32) | int(idx), d2) for on, d2, idx in seq if on)
    if not recs:
        return INF_KEY, INF, INF
    key = recs[0][0]
    rest = [d2 for k, d2 in recs[1:] if unique or k != key]
    return key, F(min(rest)) if rest else INF, F(recs[0][1])


def best1_finish(lanes, S, on):
    """finish<S> on the 64 (key, second, bd) of a wave: the S sub-slots of a query are the lanes l, l ^ 32 (and ^ 16 for S = 4); a lane with on = false keeps what
    it held.  Stated from the meaning: the winner of the group, and the smallest runner-up candidate among the sub-slots - the loser sub-slots' own best d2, the
    winner sub-slot's second"""
    if S == 1:
        return list(lanes)
    out = []
    for l in range(64):
        grp = [l ^ x for x in ((0, 32) if S == 2 else (0, 16, 32, 48))]
        b = min(lanes[g][0] for g in grp)
        cands = []
        for g in grp:
            k, s, _ = lanes[g]
            cands.append(INF if k == INF_KEY else (s if k == b else f1(k >> 32)))
        c = min(cands)
        out.append((b, F(c), f1(b >> 32) if b != INF_KEY else INF) if on[l] else lanes[l])
    return out


# ------------------------------------------------------------------ build_clusters and the ball walks, restated
def ball_box(grid, q, r):
    """the inclusive cell box cell_coord(q - r) .. cell_coord(q + r) per axis, f32; q (..., 3), r (...) -> (..., 6) as x0, x1, y0, y1, z0, z1"""
    q = np.asarray(q, dtype=np.float32); r = np.asarray(r, dtype=np.float32)
    out = []
    for a in range(3):
        out += [grid.cell_coord(q[..., a] - r, a), grid.cell_coord(q[..., a] + r, a)]
    return np.stack(out, axis=-1)


def clusters_restated(grid, q, r, todo, S):
    """build_clusters<S> for one wave: q (64, 3), r (64,), todo (64,) bool -> cid (64,) (-1: not todo), [(box, tile_mode)] per cluster.  Clusters form around
    the lowest open lane: every open lane whose cell is within 8 x 4 x 4 cells of its cell; the box is the union of the ball boxes of the cluster's lanes below
    64 / S; more than 384 row segments: tile mode, the box widened to whole tiles"""
    c = grid.cells(q); bb = ball_box(grid, q, r)
    cid = np.full(64, -1); rem = [l for l in range(64) if todo[l]]; out = []
    while rem:
        a = c[rem[0]]
        mem = [l for l in rem if abs(c[l][0] - a[0]) <= 8 and abs(c[l][1] - a[1]) <= 4 and abs(c[l][2] - a[2]) <= 4]
        cid[mem] = len(out)
        b = bb[[l for l in mem if l < 64 // S]]
        box = (b[:, 0].min(), b[:, 1].max(), b[:, 2].min(), b[:, 3].max(), b[:, 4].min(), b[:, 5].max())
        nseg = ((box[1] >> 3) - (box[0] >> 3) + 1) * (box[3] - box[2] + 1) * (box[5] - box[4] + 1)
        tm = nseg > 384
        out.append((widen(grid, box) if tm else tuple(int(v) for v in box), bool(tm)))
        rem = [l for l in rem if l not in mem]
    return cid, out


def ball_walk_restated(grid, cell_start, q, r, FG):
    """for_each_in_ball_cells (FG = 1) / _group<FG>: the sorted positions each of the FG lanes of one query sees, in order - rows z-major, then y, then the tiles
    along x; lane gl takes the positions s + gl, s + gl + FG, ... of every segment [s, e) of the device's own cell_start"""
    b = ball_box(grid, q, r)
    lanes = [[] for _ in range(FG)]; nseg = 0
    for rz in range(b[4], b[5] + 1):
        for ry in range(b[2], b[3] + 1):
            for tx in range(b[0] >> 3, (b[1] >> 3) + 1):
                xa, xb = max(b[0], tx << 3), min(b[1], (tx << 3) + 7)
                k0 = int(grid.cell_key(np.array([xa, ry, rz])))
                s, e = int(cell_start[k0]), int(cell_start[k0 + (xb - xa) + 1])
                nseg += 1
                for gl in range(FG):
                    lanes[gl] += list(range(s + gl, e, FG))
    return lanes, nseg


# ------------------------------------------------------------------ BestK, twice
PEND_CAP = 16


def bestk_wave_serial(steps, k, S, on, merge_from=0):
    """one wave of BestK step by step.  steps: [L][64] of (on, key); a lane parks a key below its k-th best AS OF THE LAST FLUSH; when one lane's queue holds
    PEND_CAP the whole wave flushes; finish<S> flushes what is parked, then lanes 0-31 with `on` take in the list of lane ^ 32, then (S = 4) lanes 0-15 that of
    lane ^ 16, and every `on` lane reads the k-th best of its query's sub-slot 0.  -> per lane (list padded to k with INF_KEY, w, found).
    merge_from: a deliberately wrong variant - the merge leaves out the sender's first `merge_from` entries"""
    lists = [[] for _ in range(64)]; w = [INF_KEY] * 64; pend = [[] for _ in range(64)]

    def kth(l):
        return lists[l][k - 1] if len(lists[l]) == k else INF_KEY

    def flush():
        for l in range(64):
            lists[l] = sorted(lists[l] + pend[l])[:k]; pend[l] = []; w[l] = kth(l)
    for row in steps:
        for l, (o, key) in enumerate(row):
            if o and key < w[l]:
                pend[l].append(key)
        if any(len(p) == PEND_CAP for p in pend):
            flush()
    if any(pend):
        flush()
    if S > 1:
        for x, lim in ((32, 32), (16, 16))[:2 if S == 4 else 1]:
            snap = [list(v) for v in lists]
            for l in range(lim):
                if on[l]:
                    lists[l] = sorted(lists[l] + snap[l ^ x][merge_from:])[:k]
        for l in range(64):
            w[l] = kth(l)
        w0 = [w[l & (64 // S - 1)] for l in range(64)]
        w = [w0[l] if on[l] else w[l] for l in range(64)]
    return [(lists[l] + [INF_KEY] * (k - len(lists[l])), w[l], len(lists[l])) for l in range(64)]


def bestk_sorted(keys, k):
    """the first k of the sorted keys (each point is shown once: no two equal keys), padded with INF_KEY"""
    s = sorted(keys)[:k]
    return s + [INF_KEY] * (k - len(s)), len(s)


def brute_force_k(q, pts, kmax=32):
    """-> (Q, kmax) uint64: the kmax smallest (f32 d2, index) keys of every query, ascending"""
    d2 = sqdist32(q, pts)
    keys = pack_keys(d2, np.broadcast_to(np.arange(len(pts)), d2.shape))
    return np.sort(keys, axis=1)[:, :kmax]


# ------------------------------------------------------------------ the row split of for_each_in_ball_cells_group_pre
def row_split_f32(r, ny):
    """(int)(((float)r + 0.5f) * (1.0f / ny))"""
    return ((np.asarray(r, dtype=np.float32) + F(0.5)) * (F(1.0) / np.asarray(ny, dtype=np.float32))).astype(np.int64)
