"""The ground of a cloud and its 2-D occupancy grid - what a user does with the corrected map next (the "pcd2pgm" step): the numpy twin of
csrc/qn_mapground.hip (qn_kf_map_ground / qn_kf_map_ground_points / qn_kf_map_ground_grid / qn_kf_map_keep_classes) and its specification.  Pure numpy, no GPU.

For the n records of a cloud (x y z, anything behind carried along) and GroundParams(cell, max_slope, ground_tol, clearance, min_points) - cell finite > 0,
max_slope (rise over run) finite > 0, ground_tol finite >= 0, clearance finite > ground_tol, min_points an integer >= 1:
  units        e = quant_exponent(cell): the largest integer with cell * 2^e <= 2^10 (kept within [-126, 127]).  zq = int32(rint(z * 2^e)), half to even, the
               f32 z widened to f64 first, so the product is exact.  f64, every operation rounded on its own: step_s = max(1, rint(max_slope * cell * 2^e)),
               step_d = (step_s * 181) >> 7, tol_q = rint(ground_tol * 2^e), clear_q = rint(clearance * 2^e); one of them >= 2^30: ValueError.
               A finite point with |zq| >= 2^30: CapacityError.
  columns      a finite point is one whose x, y and z are all finite.  In x and y only, the voxel grid's arithmetic: c = int(floorf(x * inv) - float32(minb)),
               inv = float32(1 / cell), minb = floorf(min x * inv), the grid W x H from the extremes (W along x, H along y).  CapacityError when floorf(x * inv)
               leaves the int32 range (a NaN from 0 * inf included), when W or H > 2^24 (below that the f32 subtraction is exact), or when W * H > MAX_CELLS =
               2^26.  Without a finite point the grid is 0 x 0 and the origin (0, 0).
  seeds        cnt(c) = the finite points of column c; seed(c) = the smallest zq of the column when cnt(c) >= min_points, else INF = 2^31 - 1.
  envelope     g = the greatest function on the dense grid with g(c) <= seed(c) and g(c) <= g(n) + step(n, c) for the eight neighbours n, step_s for a straight
               and step_d for a diagonal one, the sum saturating at INF.  Unique; as step_s <= step_d <= 2 step_s it is envelope_closed_form: g(c) = min(INF,
               min over the seeded s of seed(s) + step_d * min(dx, dy) + step_s * (max(dx, dy) - min(dx, dy))).  Empty columns get a value too; no seeded
               column: every g is INF.  No relaxation schedule changes it; envelope() sweeps the eight directions in place until a cycle changes nothing.
  classes      one byte per point from h = zq - g(column): NONE 0 (a non-finite record, or g = INF), GROUND 1 (-tol_q <= h <= tol_q), OBSTACLE 2 (tol_q < h <=
               clear_q), OVERHEAD 3 (h > clear_q), BELOW 4 (h < -tol_q: only possible in an unseeded column).  height_q = max(h, -2^31 + 1) as int32 (h < 2^31 always;
               the floor binds only where g has all but saturated), INT32_MIN for class 0.
  occupancy    one byte per column: 0 unknown (no finite point), 2 occupied (at least one OBSTACLE point), 1 free (everything else): OVERHEAD does not occupy.
Arrays over the grid are (H, W), row-major with y the slow axis.  Everything after the quantisation is an integer, so no order of anything changes a byte.
"""
import math
from collections import namedtuple
import numpy as np

GroundParams = namedtuple("GroundParams", "cell max_slope ground_tol clearance min_points", defaults=(0.5, 0.3, 0.2, 2.0, 1))      # interface choices, not measurements
GroundStats = namedtuple("GroundStats", "n n_finite n_none n_ground n_obstacle n_overhead n_below width height seeded occupied free unknown "
                                        "quant_exp step_s step_d tol_q clear_q")
GridInfo = namedtuple("GridInfo", "origin_x origin_y cell width height quant_exp")
NONE, GROUND, OBSTACLE, OVERHEAD, BELOW = range(5)
INF = 2 ** 31 - 1
NO_HEIGHT = -2 ** 31
MAX_CELLS = 1 << 26
MAX_SIDE = 1 << 24
LIMIT = 1 << 30
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205                      # map_server's trinary values


class CapacityError(ValueError):
    """what the C library answers with QN_ERR_CAPACITY"""


def check_params(p):
    c, s, t, cl = (float(v) for v in p[:4])
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError("mapground: cell must be finite and > 0")
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError("mapground: max_slope must be finite and > 0")
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError("mapground: ground_tol must be finite and >= 0")
    if not (math.isfinite(cl) and cl > t):
        raise ValueError("mapground: clearance must be finite and > ground_tol")
    if int(p[4]) != p[4] or not (1 <= int(p[4]) <= 0xffffffff):
        raise ValueError("mapground: min_points must be an integer >= 1")


def quant_exponent(cell):
    """the largest e with cell * 2^e <= 2^10 (f64; exact through frexp), clamped to the exponents of normal f32 powers of two"""
    m, x = math.frexp(float(cell))                   # cell = m 2^x, 0.5 <= m < 1
    e = 11 - x if m == 0.5 else 10 - x
    return max(-126, min(127, e))


def units(params):
    """-> (e, step_s, step_d, tol_q, clear_q), Python integers"""
    p = GroundParams(*params)
    check_params(p)
    e = quant_exponent(p.cell)
    scale = np.float64(math.ldexp(1.0, e))
    s = np.rint(np.float64(p.max_slope) * np.float64(p.cell) * scale)
    t = np.rint(np.float64(p.ground_tol) * scale)
    c = np.rint(np.float64(p.clearance) * scale)
    if not (s < LIMIT and t < LIMIT and c < LIMIT):
        raise ValueError("mapground: a quantised parameter is 2^30 or more")
    step_s = max(1, int(s))
    step_d = (step_s * 181) >> 7
    if step_d >= LIMIT:
        raise ValueError("mapground: a quantised parameter is 2^30 or more")
    return e, step_s, step_d, int(t), int(c)


def envelope_closed_form(seed, step_s, step_d):
    """g(c) = min(INF, min over the seeded s of seed(s) + step_d min(dx, dy) + step_s (max(dx, dy) - min(dx, dy))), by brute force: (H, W) int32"""
    seed = np.asarray(seed, np.int64)
    H, W = seed.shape
    g = np.full((H, W), INF, np.int64)
    ys, xs = np.nonzero(seed != INF)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for y, x in zip(ys, xs):
        dx = np.abs(xx - x); dy = np.abs(yy - y)
        lo = np.minimum(dx, dy); hi = np.maximum(dx, dy)
        np.minimum(g, seed[y, x] + step_d * lo + step_s * (hi - lo), out=g)
    return g.astype(np.int32)


def envelope(seed, step_s, step_d):
    """the same by relaxation to the fixed point: the eight directions one after the other, in place, until a whole cycle changes nothing"""
    g = np.asarray(seed, np.int64).copy()
    H, W = g.shape
    if H == 0 or W == 0:
        return g.astype(np.int32)
    dirs = [(0, 1, step_s), (0, -1, step_s), (1, 0, step_s), (-1, 0, step_s), (1, 1, step_d), (1, -1, step_d), (-1, 1, step_d), (-1, -1, step_d)]

    def part(a, d):                                  # the cells that have a neighbour at -d, and that neighbour
        return (slice(max(d, 0), a + min(d, 0)), slice(max(-d, 0), a + min(-d, 0)))

    while True:
        changed = False
        for dy, dx, st in dirs:
            ty, sy = part(H, dy); tx, sx = part(W, dx)
            dst = g[ty, tx]
            cand = np.minimum(g[sy, sx] + st, INF)   # (INF + step stays INF: the sum saturates)
            m = cand < dst
            if m.any():
                dst[m] = cand[m]
                changed = True
        if not changed:
            return g.astype(np.int32)


def _xyz(cloud):
    a = np.asarray(cloud)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("mapground: an (n, >= 3) array of records")
    return np.ascontiguousarray(a[:, :3], np.float32)


def classify(points, params=None, envelope_fn=None):
    """-> dict(classes (n,) u8, height_q (n,) i32, ground_q (H, W) i32, occupancy (H, W) u8, seed (H, W) i32, info: a GridInfo, stats: a GroundStats)"""
    p = GroundParams() if params is None else GroundParams(*params)
    e, step_s, step_d, tol_q, clear_q = units(p)
    a = _xyz(points)
    n = len(a)
    fin = np.isfinite(a).all(axis=1)
    f = a[fin]
    nf = len(f)
    zqf = np.rint(f[:, 2].astype(np.float64) * np.float64(math.ldexp(1.0, e)))
    if nf and not (np.abs(zqf) < LIMIT).all():
        raise CapacityError("mapground: a height of 2^30 units or more")
    classes = np.zeros(n, np.uint8); height = np.full(n, NO_HEIGHT, np.int32)
    if nf == 0:
        z = np.zeros((0, 0), np.int32)
        return dict(classes=classes, height_q=height, ground_q=z, occupancy=z.astype(np.uint8), seed=z.copy(), info=GridInfo(0.0, 0.0, float(p.cell), 0, 0, e),
                    stats=GroundStats(n, 0, n, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, e, step_s, step_d, tol_q, clear_q))
    inv = np.float32(1.0 / float(p.cell))
    minb = []; size = []
    with np.errstate(over="ignore", invalid="ignore"):
        for ax in (0, 1):
            lo = np.floor(f[:, ax].min() * inv); hi = np.floor(f[:, ax].max() * inv)
            if not (-2.0 ** 31 <= lo < 2.0 ** 31 and -2.0 ** 31 <= hi < 2.0 ** 31):
                raise CapacityError("mapground: a column index outside the int32 range")
            minb.append(int(lo)); size.append(int(hi) - int(lo) + 1)
        W, H = size
        if W > MAX_SIDE or H > MAX_SIDE or W * H > MAX_CELLS:
            raise CapacityError("mapground: a grid of more than 2^26 columns")
        cx = (np.floor(f[:, 0] * inv) - np.float32(minb[0])).astype(np.int64)
        cy = (np.floor(f[:, 1] * inv) - np.float32(minb[1])).astype(np.int64)
    col = cy * W + cx
    zq = zqf.astype(np.int64)
    cnt = np.bincount(col, minlength=W * H)
    low = np.full(W * H, INF, np.int64)
    np.minimum.at(low, col, zq)
    seed = np.where(cnt >= int(p.min_points), low, INF).astype(np.int32).reshape(H, W)
    g = (envelope_fn or envelope)(seed, step_s, step_d)
    gc = g.reshape(-1)[col].astype(np.int64)
    h = zq - gc
    cf = np.where(gc == INF, NONE, np.where(h < -tol_q, BELOW, np.where(h <= tol_q, GROUND, np.where(h <= clear_q, OBSTACLE, OVERHEAD)))).astype(np.uint8)
    classes[fin] = cf
    height[fin] = np.where(gc == INF, NO_HEIGHT, np.maximum(h, NO_HEIGHT + 1)).astype(np.int32)
    obst = np.bincount(col[cf == OBSTACLE], minlength=W * H) > 0
    occ = np.where(cnt == 0, 0, np.where(obst, 2, 1)).astype(np.uint8).reshape(H, W)
    k = np.bincount(classes, minlength=5)
    stats = GroundStats(n, nf, int(k[0]), int(k[1]), int(k[2]), int(k[3]), int(k[4]), W, H, int((seed != INF).sum()), int((occ == 2).sum()), int((occ == 1).sum()),
                        int((occ == 0).sum()), e, step_s, step_d, tol_q, clear_q)
    info = GridInfo(float(minb[0]) * float(p.cell), float(minb[1]) * float(p.cell), float(p.cell), W, H, e)
    return dict(classes=classes, height_q=height, ground_q=g, occupancy=occ, seed=seed, info=info, stats=stats)


def check_mask(mask):
    if int(mask) != mask or int(mask) == 0 or int(mask) & ~31:
        raise ValueError("mapground: class_mask must have at least one of the bits 0 .. 4 set and no other")
    return int(mask)


def keep(points, classes, mask):
    """-> the records of `points` whose class bit is set in mask, in order and with every column (what qn_kf_map_keep_classes leaves in the map slot)"""
    m = check_mask(mask)
    c = np.asarray(points)
    return np.ascontiguousarray(c[((m >> np.asarray(classes).astype(np.int64)) & 1) == 1])


def to_pgm(occupancy):
    """the occupancy grid as the bytes of a binary PGM in map_server's conventions: occupied 0, free 254, unknown 205; row 0 of the image is the largest y"""
    occ = np.asarray(occupancy, np.uint8)
    H, W = occ.shape if occ.ndim == 2 else (0, 0)
    lut = np.array([PGM_UNKNOWN, PGM_FREE, PGM_OCCUPIED], np.uint8)
    return b"P5\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(lut[occ][::-1]).tobytes()


def map_yaml(info, image="map.pgm"):
    """the map_server description beside the image: resolution = cell, origin = [origin_x, origin_y, 0] (the lower-left corner of the image)"""
    i = GridInfo(*info)
    return ("image: %s\nresolution: %r\norigin: [%r, %r, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
            % (image, float(i.cell), float(i.origin_x), float(i.origin_y)))
