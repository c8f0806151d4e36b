"""Planning over the occupancy map - the cost-to-go field to a set of goals and the paths down it: the numpy twin of csrc/qn_maproute.inc (qn_kf_map_route /
_grid / _query / _path) and its specification.  Pure numpy, no GPU.

  input        the class bytes of a 3-D occupancy map, (D, H, W) uint8 with x the fastest axis, and the distance field computed from them (mapdistance.transform,
               or KeyframeStore.map_distance_grid): (D, H, W) uint16.
  params       RouteParams(pass_mask, min_d2, iz_lo, iz_hi, planar): pass_mask has at least one of the class bits 0 .. 2 and no other (1 << FREE); a voxel
               passes only if d2 >= min_d2 (4), FAR passes any min_d2 and 0 switches the test off; min_d2 above max_dist^2 of the field is refused - beyond the
               cap the distance is not known, for the reason mapdistance.inflate gives; iz_lo .. iz_hi (0, INT32_MAX) is the band of layers, inclusive, clipped
               to the grid, iz_lo > iz_hi is refused; planar 0 or 1 (0).  The defaults are interface choices, not measurements.
  passable     3-D (planar 0): voxel v is passable iff its class bit is in pass_mask, d2[v] >= min_d2 and iz_lo <= vz <= iz_hi; the field is W x H x D.
               planar: the field is W x H x 1; a column is passable iff the clipped band is not empty and every voxel of the column inside it passes the class
               and d2 tests - an upright body moving in the plane, the companion of mapdistance.slice2d.
  moves        from v to v + o, o in {-1, 0, 1}^3 without 0, both ends inside the field; allowed iff every voxel v + o' is passable, o'_k in {0, o_k} on
               each axis k: the 2, 4 or 8 voxels of the block the move spans.  No corner is cut and no diagonal slips between two obstacles.  The rule is
               symmetric, so the graph is undirected.  Cost 2 + |o|_1: 3 for a face move, 4 for an edge move, 5 for a corner move - the 3-4-5 chamfer metric;
               metres() divides by 3 and multiplies by the voxel: in open space between 5.7 % under (a face diagonal) and 10.6 % over (direction (3, 1, 1)) the Euclidean length.
  goals        n world points (f64 xyz), each to its voxel by the occupancy map's own quantisation (mapdistance.query); in planar mode only x and y choose the
               column, z must still be finite and inside the coordinate limit.  A goal whose voxel or column is passable has cost 0; every other goal (not
               finite, outside, blocked) is ignored and counted.  With no goal left nothing is reached.
  field        one uint32 per voxel, or per column in planar mode: the smallest path cost to a goal, BLOCKED = 0xfffffffe where the voxel is not passable,
               UNREACHED = 0xffffffff where it is passable but not connected to a goal.  A simple path has at most 2^27 voxels, so a cost is at most 5 * 2^27.
  stats        RouteStats(passable, blocked, reached, unreached, goals_used, goals_blocked, max_cost, sum_cost): passable = reached + unreached, passable +
               blocked = the field's cells; max_cost and sum_cost over the reached cells.
  paths        from the start's voxel: at v with cost c > 0 take the first allowed move to n with cost[n] + w(v, n) == c, the moves enumerated with dz
               outermost, then dy, then dx, each in the order -1, 0, +1; stop at cost 0.  len = the true number of voxels, start and goal included, 0 for a
               start that is outside, blocked or unreached; ijk = the first min(len, max_len) voxels, the rest 0; in planar mode k = 0.  cost // 3 + 1 bounds len.
  field()      Dial's buckets over the integer costs, each level's frontier relaxed by 26 vectorised moves; dijkstra() is the definition literally - an
               explicit edge list handed to scipy.sparse.csgraph.dijkstra, or a heap without scipy - the second, independent statement.
Shortest-path costs are unique integers, so any exact algorithm gives the same bytes."""
import heapq
from collections import namedtuple
import numpy as np
from . import mapdistance as md, mapoccupancy as mo

INT32_MAX = 0x7fffffff
RouteParams = namedtuple("RouteParams", "pass_mask min_d2 iz_lo iz_hi planar", defaults=(1 << mo.FREE, 4, 0, INT32_MAX, 0))      # interface choices
RouteStats = namedtuple("RouteStats", "passable blocked reached unreached goals_used goals_blocked max_cost sum_cost")
BLOCKED = 0xfffffffe
UNREACHED = 0xffffffff
MAX_POINTS = 1 << 20
# the 26 moves in the paths' order: dz outermost, then dy, then dx, each -1, 0, +1 -> (dx, dy, dz)
MOVES = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def weight(o):
    return 2 + abs(o[0]) + abs(o[1]) + abs(o[2])


def block_of(o):
    """the offsets o' with o'_k in {0, o_k}, without (0, 0, 0): the other voxels of the block the move o spans"""
    return [(a, b, c) for c in {0, o[2]} for b in {0, o[1]} for a in {0, o[0]} if (a, b, c) != (0, 0, 0)]


def check_params(p, max_dist=None):
    """raises ValueError on a value outside its range; with max_dist (of the live distance field) also on min_d2 > max_dist^2"""
    m, d, lo, hi, planar = p
    if int(m) != m or int(m) == 0 or int(m) & ~7:
        raise ValueError("maproute: pass_mask must have at least one of the bits 0 .. 2 set and no other")
    if int(d) != d or not (0 <= int(d) <= 0xffffffff):
        raise ValueError("maproute: min_d2 must be an integer in 0 .. 2^32 - 1")
    if max_dist is not None and int(d) > int(max_dist) ** 2:
        raise ValueError("maproute: min_d2 above max_dist^2 of the distance field - beyond the cap the distance is not known")
    for v in (lo, hi):
        if int(v) != v or not (-INT32_MAX - 1 <= int(v) <= INT32_MAX):
            raise ValueError("maproute: iz_lo and iz_hi must be 32-bit integers")
    if int(lo) > int(hi):
        raise ValueError("maproute: iz_lo > iz_hi")
    if int(planar) != planar or int(planar) not in (0, 1):
        raise ValueError("maproute: planar must be 0 or 1")


def _params(params, max_dist=None):
    p = RouteParams() if params is None else RouteParams(*params)
    check_params(p, max_dist)
    return RouteParams(*(int(v) for v in p))


def band(depth, p):
    """the clipped band of layers (lo, hi); lo > hi: it misses the grid"""
    return max(int(p.iz_lo), 0), min(int(p.iz_hi), int(depth) - 1)


def passable(classes, d2, params=None):
    """-> the boolean field: (D, H, W) in 3-D mode, (1, H, W) in planar mode"""
    p = _params(params)
    cls = np.asarray(classes, np.uint8); d = np.asarray(d2, np.uint16)
    if cls.ndim != 3 or cls.shape != d.shape:
        raise ValueError("maproute: classes and d2 must be (D, H, W), the same")
    ok = (((p.pass_mask >> cls.astype(np.int64)) & 1) == 1) & ((d == md.FAR) | (d.astype(np.int64) >= p.min_d2))
    lo, hi = band(cls.shape[0], p)
    if p.planar:
        if lo > hi:
            return np.zeros((1,) + cls.shape[1:], bool)
        return ok[lo:hi + 1].all(axis=0)[None]
    z = np.arange(cls.shape[0])
    return ok & ((z >= lo) & (z <= hi))[:, None, None]


def voxels_of(grid, xyz, params=None):
    """world points (n, 3) f64 -> (inside (n,) bool, ijk (n, 3) int64 field indices, rows of points that are not inside meaningless): the occupancy map's
    quantisation; not inside: a point that is not finite, has a |x_k * inv| >= 2^20, or falls outside the field (planar: z is not compared with the grid, k = 0)"""
    p = _params(params)
    g = mo.OccupancyGrid(*grid)
    pts = np.asarray(xyz, np.float64).reshape(-1, 3)
    inv = np.float64(1.0) / np.float64(g.voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(pts * inv) < mo.COORD_LIMIT).all(axis=1)        # (a NaN fails the comparison)
    c = np.zeros((len(pts), 3), np.int64)
    if ok.any():
        c[ok] = (mo.quantise(pts[ok], inv) >> mo.S) - np.asarray(g.minc, np.int64)
    side = np.array([g.width, g.height, g.depth], np.int64)
    if p.planar:
        c[:, 2] = 0
        side[2] = 1 if g.width * g.height else 0
    inside = ok & ((c >= 0) & (c < side)).all(axis=1)
    return inside, c


def stats_of(cost, goals_used, goals_blocked):
    c = np.asarray(cost, np.uint32)
    reached = c < BLOCKED
    return RouteStats(int((c != BLOCKED).sum()), int((c == BLOCKED).sum()), int(reached.sum()), int((c == UNREACHED).sum()), int(goals_used), int(goals_blocked),
                      int(c[reached].max()) if reached.any() else 0, int(c[reached].sum(dtype=np.uint64)))


def _goal_voxels(free, grid, goals, p):
    """-> (the linear indices in `free` of the goals that count, how many count, how many do not)"""
    pts = np.asarray(goals, np.float64).reshape(-1, 3)
    if not (1 <= len(pts) <= MAX_POINTS):
        raise ValueError("maproute: 1 .. 2^20 goals")
    inside, c = voxels_of(grid, pts, p)
    lin = np.zeros(0, np.int64)
    if inside.any():
        c = c[inside]
        c = c[free[c[:, 2], c[:, 1], c[:, 0]]]
        lin = (c[:, 2] * free.shape[1] + c[:, 1]) * free.shape[2] + c[:, 0]
    return lin, len(lin), len(pts) - len(lin)


def field(classes, d2, grid, goals, params=None):
    """-> dict(cost: the (D, H, W) or (1, H, W) uint32 field, stats: a RouteStats), by Dial's buckets"""
    p = _params(params)
    free = passable(classes, d2, p)
    lin, used, ignored = _goal_voxels(free, grid, goals, p)
    Df, H, W = free.shape
    pad = np.zeros((Df + 2, H + 2, W + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = free
    sy, sz = W + 2, (W + 2) * (H + 2)
    P = pad.ravel()
    INF = np.int64(1) << 62
    best = np.full(P.size, INF, np.int64)
    off = lambda o: o[0] + o[1] * sy + o[2] * sz
    moves = [(off(o), weight(o), [off(b) for b in block_of(o)]) for o in MOVES if Df > 1 or o[2] == 0]
    buckets = {}
    if len(lin):
        z, r = np.divmod(lin, H * W); y, x = np.divmod(r, W)
        start = np.unique((z + 1) * sz + (y + 1) * sy + (x + 1))
        best[start] = 0
        buckets[0] = [start]
    level = 0
    while buckets:
        if level not in buckets:
            level = min(buckets)
        f = np.unique(np.concatenate(buckets.pop(level)))
        f = f[best[f] == level]                                       # (an entry improved since it was queued is settled at its lower level)
        for o, w, blk in moves:
            ok = np.ones(len(f), bool)
            for b in blk:
                ok &= P[f + b]
            n = f[ok] + o
            n = n[best[n] > level + w]
            if len(n):
                best[n] = level + w
                buckets.setdefault(level + w, []).append(n)
        level += 1
    b3 = best.reshape(pad.shape)[1:-1, 1:-1, 1:-1]
    cost = np.where(~free, BLOCKED, np.where(b3 >= INF, UNREACHED, b3)).astype(np.uint32)
    return dict(cost=cost, stats=stats_of(cost, used, ignored))


def edges(free):
    """the definition's graph over the boolean field -> (from, to, weight) int64 arrays of linear indices, every allowed move in both directions"""
    Df, H, W = free.shape
    idx = np.arange(free.size, dtype=np.int64).reshape(free.shape)
    src, dst, wgt = [], [], []
    for o in MOVES:
        def view(a, s):
            """the part of a shifted by s for which the cell and the cell + o are both inside"""
            sl = []
            for k, n in ((2, Df), (1, H), (0, W)):
                lo, hi = max(0, -o[k]), n - max(0, o[k])
                if hi <= lo:
                    return None
                sl.append(slice(lo + s[k], hi + s[k]))
            return a[tuple(sl)]
        base = view(free, (0, 0, 0))
        if base is None:
            continue
        ok = base.copy()
        for b in block_of(o):
            ok &= view(free, b)
        src.append(view(idx, (0, 0, 0))[ok]); dst.append(view(idx, o)[ok]); wgt.append(np.full(int(ok.sum()), weight(o), np.int64))
    if not src:
        return (np.zeros(0, np.int64),) * 3
    return np.concatenate(src), np.concatenate(dst), np.concatenate(wgt)


def dijkstra(classes, d2, grid, goals, params=None):
    """the definition literally: the explicit edge list of every allowed move, then Dijkstra from the goals (scipy's, or a heap without scipy)
    -> dict(cost, stats) as field()"""
    p = _params(params)
    free = passable(classes, d2, p)
    lin, used, ignored = _goal_voxels(free, grid, goals, p)
    n = free.size
    dist = np.full(n, np.inf)
    src, dst, wgt = edges(free)
    if len(lin):
        try:
            from scipy.sparse import csr_matrix
            from scipy.sparse.csgraph import dijkstra as sp_dijkstra
        except ImportError:
            sp_dijkstra = None
        if sp_dijkstra is not None:
            dist = sp_dijkstra(csr_matrix((wgt.astype(np.float64), (src, dst)), shape=(n, n)), directed=True, indices=np.unique(lin), min_only=True)
        else:
            order = np.argsort(src, kind="stable")
            dst, wgt = dst[order], wgt[order]
            first = np.searchsorted(src[order], np.arange(n + 1))
            heap = [(0, int(v)) for v in np.unique(lin)]
            for _, v in heap:
                dist[v] = 0
            while heap:
                c, v = heapq.heappop(heap)
                if c > dist[v]:
                    continue
                for e in range(first[v], first[v + 1]):
                    t = c + int(wgt[e])
                    if t < dist[dst[e]]:
                        dist[dst[e]] = t
                        heapq.heappush(heap, (t, int(dst[e])))
    d = dist.reshape(free.shape)
    cost = np.where(~free, BLOCKED, np.where(np.isinf(d), UNREACHED, np.where(np.isinf(d), 0, d))).astype(np.uint32)
    return dict(cost=cost, stats=stats_of(cost, used, ignored))


def allowed(cost, v, o):
    """whether the move o from the field voxel v = (x, y, z) is allowed: the end inside the field and every voxel of the block passable (cost != BLOCKED)"""
    Df, H, W = cost.shape
    for b in [(0, 0, 0)] + block_of(o):
        x, y, z = v[0] + b[0], v[1] + b[1], v[2] + b[2]
        if not (0 <= x < W and 0 <= y < H and 0 <= z < Df) or int(cost[z, y, x]) == BLOCKED:
            return False
    return True


def paths(cost, grid, starts, max_len, params=None):
    """-> (len (S,) uint32, ijk (S, max_len, 3) int32): the walk down the field from every start (see the module text)"""
    p = _params(params)
    cost = np.asarray(cost, np.uint32)
    if int(max_len) < 1:
        raise ValueError("maproute: max_len must be at least 1")
    pts = np.asarray(starts, np.float64).reshape(-1, 3)
    if not (1 <= len(pts) <= MAX_POINTS):
        raise ValueError("maproute: 1 .. 2^20 starts")
    inside, c = voxels_of(grid, pts, p)
    lens = np.zeros(len(pts), np.uint32); ijk = np.zeros((len(pts), int(max_len), 3), np.int32)
    for i in np.flatnonzero(inside):
        v = tuple(int(a) for a in c[i])
        cur = int(cost[v[2], v[1], v[0]])
        if cur >= BLOCKED:
            continue
        n = 0
        while True:
            if n < max_len:
                ijk[i, n] = v
            n += 1
            if cur == 0:
                break
            for o in MOVES:
                t = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
                if allowed(cost, v, o) and int(cost[t[2], t[1], t[0]]) + weight(o) == cur:
                    v, cur = t, cur - weight(o)
                    break
            else:
                raise AssertionError("maproute: the field is no fixed point at %r" % (v,))
        lens[i] = n
    return lens, ijk


def query(cost, grid, xyz, params=None):
    """world points (n, 3) f64 -> the field's value (n,) uint32 at each; BLOCKED for a point that is not finite or outside"""
    p = _params(params)
    cost = np.asarray(cost, np.uint32)
    inside, c = voxels_of(grid, xyz, p)
    out = np.full(len(c), BLOCKED, np.uint32)
    c = c[inside]
    out[inside] = cost[c[:, 2], c[:, 1], c[:, 0]]
    return out


def metres(cost, voxel):
    """costs as metres, f64: cost / 3 * voxel; BLOCKED and UNREACHED -> inf"""
    c = np.asarray(cost, np.uint32)
    return np.where(c >= BLOCKED, np.inf, c.astype(np.float64) / 3.0 * float(voxel))


def centres(grid, ijk, params=None):
    """the centres of the field voxels ijk in world coordinates -> (m, 3) f64; in planar mode z is the middle of the clipped band (NaN when it misses the grid)"""
    p = _params(params)
    g = mo.OccupancyGrid(*grid)
    out = np.ascontiguousarray(mo.centres(ijk, g))
    if p.planar:
        lo, hi = band(g.depth, p)
        out[:, 2] = (float(g.minc[2]) + 0.5 * (lo + hi + 1)) * float(g.voxel) if lo <= hi else np.nan
    return out
