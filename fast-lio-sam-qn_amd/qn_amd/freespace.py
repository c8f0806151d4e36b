"""Free-space (see-through) consistency of a loop pair: the numpy twin of csrc/qn_freespace.hip (qn_kf_range_* / qn_kf_freespace_*) and its specification.
Pure numpy, no GPU.

Overlap and the fitness score speak about points that found a partner.  This check speaks about the others: a point of one scan that lies, under the
hypothesised transform, where the other scan's rays passed on their way to a farther surface contradicts that scan; a point behind everything the other scan saw,
or in a direction it never measured, does not.  Everything happens in the SENSOR frame of a keyframe (PosePcd::pcd_), the only frame a range image makes sense in.

All arithmetic is f64 from the f32 records, no fused multiply-add, no transcendental per point (the tables come from math.tan / math.cos / math.sin, the C
library's functions the engine's host code calls), the correctly rounded f64 sqrt.  Every result is an integer or a min / max of f32 values, so the GPU equals
this module bit for bit.

  parameters   Params (qn_range_params): n_rows x n_cols pixels; el_lo / el_hi [rad] the lower edge of row 0 and the upper edge of the last row,
               -pi/2 < el_lo < el_hi < pi/2; min_range; window_rows, window_cols (1, 1); tol_abs, tol_rel (0.3, 0.02).
  tables       t[i] = tan(el_lo + i * (el_hi - el_lo) / n_rows), i = 0 .. n_rows;  (c[j], s[j]) = (cos, sin)(2 pi j / n_cols), j = 0 .. n_cols - 1.
  projection   of (x, y, z):  rho2 = x x + y y, rho = sqrt(rho2), r2 = rho2 + z z, r = sqrt(r2).
               row    = #{edges i in 0 .. n_rows : z >= rho t[i]} - 1;  -1 or n_rows is outside the field of view;
               column = #{j in 1 .. n_cols - 1 : azimuth(p) >= azimuth(b_j)}, b_j = (c[j], s[j]), decided as Scan Context decides its sector: by half plane
                        (y > 0, or y == 0 and x > 0, is the upper one), then by c[j] y - s[j] x >= 0.
               Both counts are DEFINED by the bisection of count_rows / count_cols below (lo / hi, mid = (lo + hi) >> 1, predicate true -> lo = mid + 1), which
               equals the plain count wherever the predicate is monotone in the index and stays well defined where rounding next to an edge makes it not.
  dropped      a point with a non-finite coordinate (after the transform, when there is one), with r < min_range, or outside the field of view.
  images       of a keyframe, from its raw records: near[row, col] = min, far[row, col] = max over its kept points of float32(r); an empty pixel holds +inf / 0.
  check        of (q, c, T), T (4x4 f64) mapping q's sensor frame into c's: direction 0 = every record of q through T, ((T0 x + T1 y) + T2 z) + T3 in f64, not
               rounded to f32, against c's images; direction 1 = every record of c through inv(T) = [R^T | -R^T t] (scancontext.relative_pose's arithmetic)
               against q's images.  For a kept point with range r at (row, col): R_near = min of near, R_far = max of far over the rows row +- window_rows that
               exist and the columns col +- window_cols, wrapping; tol = tol_abs + tol_rel r.
  classes      one byte per point: 0 dropped; 1 unobserved (R_near is +inf: the window holds no return); 2 seen through (r + tol < R_near);
               3 occluded (r > R_far + tol); 4 agree (the rest).
  record       per direction (qn_freespace_dir, eight u32): n, n_finite, in_fov (the kept points), observed (classes 2, 3, 4), seen_through, occluded, agree,
               reserved.  see_through_fraction = seen_through / observed, 0 when observed is 0."""
import math
from dataclasses import dataclass
import numpy as np

MAX_ROWS, MAX_COLS = 1024, 8192
DROPPED, UNOBSERVED, SEEN_THROUGH, OCCLUDED, AGREE = range(5)
INF32 = np.float32(np.inf)


@dataclass
class Params:
    n_rows: int = 64
    n_cols: int = 1800
    el_lo: float = math.radians(-25.0)
    el_hi: float = math.radians(2.2)
    min_range: float = 2.0
    window_rows: int = 1
    window_cols: int = 1
    tol_abs: float = 0.3
    tol_rel: float = 0.02

    @classmethod
    def for_sensor(cls, sensor, **kw):
        """The image of a synth.SpinningLidar: one row per beam and one column per azimuth step, the edges half a beam spacing outside el_min / el_max so that
        every simulated beam sits at a row centre."""
        el = sensor.elevations()
        half = 0.5 * (float(el[-1]) - float(el[0])) / (sensor.n_beams - 1) if sensor.n_beams > 1 else math.radians(0.5)
        return cls(n_rows=sensor.n_beams, n_cols=sensor.n_cols, el_lo=float(el[0]) - half, el_hi=float(el[-1]) + half, min_range=sensor.min_range, **kw)


def params_ok(p):
    """the checks of qn_kf_range_set_params"""
    f = [float(p.el_lo), float(p.el_hi), float(p.min_range), float(p.tol_abs), float(p.tol_rel)]
    return (1 <= int(p.n_rows) <= MAX_ROWS and 1 <= int(p.n_cols) <= MAX_COLS and all(math.isfinite(v) for v in f) and
            -0.5 * math.pi < f[0] < f[1] < 0.5 * math.pi and f[2] >= 0.0 and f[3] >= 0.0 and f[4] >= 0.0 and
            0 <= int(p.window_rows) < int(p.n_rows) and int(p.window_cols) >= 0 and 2 * int(p.window_cols) + 1 <= int(p.n_cols))


def tables(p):
    """-> (t [n_rows + 1], cos [n_cols], sin [n_cols]) f64"""
    if not params_ok(p):
        raise ValueError("freespace: bad range-image parameters")
    nr, nc, lo, hi = int(p.n_rows), int(p.n_cols), float(p.el_lo), float(p.el_hi)
    t = np.array([math.tan(lo + float(i) * (hi - lo) / nr) for i in range(nr + 1)])
    c = np.array([math.cos(2.0 * math.pi * j / nc) for j in range(nc)])
    s = np.array([math.sin(2.0 * math.pi * j / nc) for j in range(nc)])
    return t, c, s


def row_predicate(z, rho, t, i):
    """edge i lies at or below the point: z >= rho t[i]"""
    return z >= rho * t[i]


def col_predicate(x, y, c, s, j):
    """azimuth(p) >= azimuth(b_j): Scan Context's half-plane and cross-product test"""
    hp = np.where((y > 0.0) | ((y == 0.0) & (x > 0.0)), 0, 1)
    hb = np.where((s[j] > 0.0) | ((s[j] == 0.0) & (c[j] > 0.0)), 0, 1)
    return (hp > hb) | ((hp == hb) & (c[j] * y - s[j] * x >= 0.0))


def _bisect(pred, lo, hi, n):
    """the count of the definition for n points at once: every point walks its own lo / hi, all for the same number of trips (a finished point stays put)"""
    lo = np.full(n, lo, np.int64); hi = np.full(n, hi, np.int64)
    while True:
        live = lo < hi
        if not live.any():
            return lo
        mid = (lo + hi) >> 1
        ok = pred(np.where(live, mid, 0)) & live
        lo = np.where(ok, mid + 1, lo)
        hi = np.where(live & ~ok, mid, hi)


def count_rows(z, rho, t):
    """the number of edges at or below each point, by bisection over the edges 0 .. n_rows"""
    return _bisect(lambda i: row_predicate(z, rho, t, i), 0, len(t), len(z))


def count_cols(x, y, c, s):
    """the number of boundaries 1 .. n_cols - 1 at or before each point, by bisection"""
    return _bisect(lambda j: col_predicate(x, y, c, s, j), 1, len(c), len(x)) - 1


def project(xyz64, p, tabs=None):
    """(n, 3) f64 points -> (row, col, r f64, finite, keep)"""
    t, c, s = tables(p) if tabs is None else tabs
    a = np.asarray(xyz64, np.float64).reshape(-1, 3)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    with np.errstate(all="ignore"):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        x = np.where(fin, x, 1.0); y = np.where(fin, y, 0.0); z = np.where(fin, z, 0.0)
        rho2 = x * x + y * y
        rho = np.sqrt(rho2)
        r = np.sqrt(rho2 + z * z)
        row = count_rows(z, rho, t) - 1
        col = count_cols(x, y, c, s)
    keep = fin & (r >= float(p.min_range)) & (row >= 0) & (row < int(p.n_rows))
    return row, col, r, fin, keep


def _xyz(cloud):
    a = np.asarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("freespace: a cloud is (n, >= 3) float32")
    return a[:, :3].astype(np.float64)


def range_images(cloud, p, tabs=None):
    """-> (near, far), each (n_rows, n_cols) f32, of a keyframe's records in its sensor frame"""
    nr, nc = int(p.n_rows), int(p.n_cols)
    row, col, r, _, keep = project(_xyz(cloud), p, tabs)
    near = np.full(nr * nc, INF32, np.float32); far = np.zeros(nr * nc, np.float32)
    if keep.any():
        pix = row[keep] * nc + col[keep]
        r32 = r[keep].astype(np.float32)
        np.minimum.at(near, pix, r32); np.maximum.at(far, pix, r32)
    return near.reshape(nr, nc), far.reshape(nr, nc)


def transform(cloud, T):
    """the records through T in the engine's row order, f64, not rounded"""
    a = _xyz(cloud)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def inverse(T):
    """inv(T) = [R^T | -R^T t] in scancontext.relative_pose's arithmetic (each -R^T t entry summed over k = 0 .. 2 in order)"""
    T = [[float(v) for v in row] for row in np.asarray(T, np.float64).reshape(4, 4)]
    A = np.zeros((4, 4))
    for r in range(3):
        acc = 0.0
        for k in range(3):
            A[r, k] = T[k][r]
            acc = acc + T[k][r] * T[k][3]
        A[r, 3] = -acc
    A[3, 3] = 1.0
    return A


def window_extrema(near, far, row, col, p):
    """-> (R_near, R_far) f32 of every (row, col): rows clipped, columns wrapping"""
    nr, nc = near.shape
    rn = np.full(len(row), INF32, np.float32); rf = np.zeros(len(row), np.float32)
    for dr in range(-int(p.window_rows), int(p.window_rows) + 1):
        rr = row + dr
        ok = (rr >= 0) & (rr < nr)
        rc = np.clip(rr, 0, nr - 1)
        for dc in range(-int(p.window_cols), int(p.window_cols) + 1):
            cc = (col + dc) % nc
            rn = np.where(ok, np.minimum(rn, near[rc, cc]), rn)
            rf = np.where(ok, np.maximum(rf, far[rc, cc]), rf)
    return rn, rf


def classify(points64, near, far, p, tabs=None):
    """(n, 3) f64 points in the images' sensor frame -> (classes (n,) uint8, finite (n,) bool)"""
    row, col, r, fin, keep = project(points64, p, tabs)
    cls = np.zeros(len(r), np.uint8)
    if keep.any():
        k = np.flatnonzero(keep)
        rn, rf = window_extrema(near, far, row[k], col[k], p)
        rk = r[k]
        tol = float(p.tol_abs) + float(p.tol_rel) * rk
        c = np.full(len(k), AGREE, np.uint8)
        c[rk > rf.astype(np.float64) + tol] = OCCLUDED
        c[rk + tol < rn.astype(np.float64)] = SEEN_THROUGH
        c[rn == INF32] = UNOBSERVED
        cls[k] = c
    return cls, fin


def record(cls, fin):
    """the direction record from the per-point classes"""
    n = [int((cls == k).sum()) for k in range(5)]
    return dict(n=int(len(cls)), n_finite=int(fin.sum()), in_fov=n[1] + n[2] + n[3] + n[4], observed=n[2] + n[3] + n[4], seen_through=n[2], occluded=n[3], agree=n[4])


def direction(cloud, T, near, far, p, points=False, tabs=None):
    """every record of `cloud` through T against the images (near, far) -> the direction record (points=True: also `classes`)"""
    cls, fin = classify(transform(cloud, T), near, far, p, tabs)
    rec = record(cls, fin)
    if points:
        rec["classes"] = cls
    return rec


def freespace(q_cloud, c_cloud, T, p, points=False, q_images=None, c_images=None):
    """the record of one pair: q_in_c (direction 0) and c_in_q (direction 1).  T maps q's sensor frame into c's."""
    tabs = tables(p)
    qi = range_images(q_cloud, p, tabs) if q_images is None else q_images
    ci = range_images(c_cloud, p, tabs) if c_images is None else c_images
    return dict(q_in_c=direction(q_cloud, T, ci[0], ci[1], p, points, tabs), c_in_q=direction(c_cloud, inverse(T), qi[0], qi[1], p, points, tabs))


def see_through_fraction(d):
    """seen_through / observed of one direction record (0 when nothing was observed)"""
    return d["seen_through"] / d["observed"] if d["observed"] else 0.0
