"""The occupancy map's exact Euclidean distance field: the numpy twin of csrc/qn_mapdistance.inc (qn_kf_map_distance / _grid / _slice / _query) and its
specification.  Pure numpy, no GPU.

  input        the class bytes of a 3-D occupancy map (mapoccupancy.classify, or KeyframeStore.map_occupancy_grid): (D, H, W) uint8, x the fastest axis.
  params       DistanceParams(site_mask, max_dist): site_mask has at least one of the bits 0 .. 2 and no other (1 << OCCUPIED), max_dist 1 .. MAX_RADIUS = 255
               voxels (16).  The defaults are interface choices, not measurements.
  sites        a voxel whose class bit (1 << class) is set in site_mask.  (1 << OCCUPIED) | (1 << UNKNOWN) is the conservative planner's choice, unknown space
               as an obstacle.  Nothing outside the grid is a site.
  field        d2[v] = min over sites s of (vx - sx)^2 + (vy - sy)^2 + (vz - sz)^2, in voxel units, an integer; a site has 0; FAR = 0xffff when the minimum
               exceeds max_dist^2 or there is no site.  max_dist <= 255, so d2 <= 65025 < FAR: one uint16 per voxel.
  transform    three separable passes, x then y then z, each g[i] = min over |d| <= max_dist of f[i + d] + d d inside the axis, a value above max_dist^2 counted
               as infinite afterwards.  Exact under the cap: a site within max_dist has every per-axis offset <= max_dist, so it survives all three windows.
  brute        the definition literally, for small grids.
  stats        DistanceStats(sites, reached, far, max_d2, sum_d2): reached = the voxels that are no site and have d2 <= max_dist^2, far the rest, so that
               sites + reached + far == W H D; max_d2 and sum_d2 run over the reached voxels and are 0 without one.
Integers throughout, so any exact algorithm gives the same bytes; only the distance is returned, not the nearest site, so there is no tie to break.
"""
from collections import namedtuple
import numpy as np
from . import mapoccupancy as mo

DistanceParams = namedtuple("DistanceParams", "site_mask max_dist", defaults=(1 << mo.OCCUPIED, 16))      # interface choices
DistanceStats = namedtuple("DistanceStats", "sites reached far max_d2 sum_d2")
FAR = 0xffff
OUTSIDE = 0xff
MAX_RADIUS = 255
_INF = np.int32(1 << 30)                              # "no site" inside the passes: above every sum of a squared distance and a window term


def check_params(p):
    m, r = p[0], p[1]
    if int(m) != m or int(m) == 0 or int(m) & ~7:
        raise ValueError("mapdistance: site_mask must have at least one of the bits 0 .. 2 set and no other")
    if int(r) != r or not (1 <= int(r) <= MAX_RADIUS):
        raise ValueError("mapdistance: max_dist must be an integer in 1 .. %d" % MAX_RADIUS)


def sites_of(classes, site_mask):
    """-> the boolean array of the voxels whose class bit is in site_mask"""
    return ((int(site_mask) >> np.asarray(classes, np.uint8).astype(np.int64)) & 1) == 1


def stats_of(d2, max_dist):
    """the statistics of a finished field"""
    d = np.asarray(d2, np.uint16)
    reached = (d != 0) & (d != FAR)
    assert not reached.any() or int(d[reached].max()) <= int(max_dist) ** 2
    return DistanceStats(int((d == 0).sum()), int(reached.sum()), int((d == FAR).sum()), int(d[reached].max()) if reached.any() else 0,
                         int(d[reached].sum(dtype=np.uint64)))


def _axis_pass(f, axis, r, r2):
    """g[i] = min over |d| <= r of f[i + d] + d d along `axis`, inside the array; above r2: infinite"""
    n = f.shape[axis]
    g = f.copy()
    for d in range(1, min(r, n - 1) + 1):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[axis] = slice(0, n - d); hi[axis] = slice(d, n)
        lo, hi = tuple(lo), tuple(hi)
        np.minimum(g[lo], f[hi] + d * d, out=g[lo])
        np.minimum(g[hi], f[lo] + d * d, out=g[hi])
    g[g > r2] = _INF
    return g


def _finish(f, p):
    d2 = np.where(f >= _INF, FAR, f).astype(np.uint16)
    return dict(d2=d2, stats=stats_of(d2, p.max_dist))


def transform(classes, params=None):
    """classes (D, H, W) uint8 -> dict(d2 (D, H, W) uint16, stats: a DistanceStats), by the windowed separable passes"""
    p = DistanceParams() if params is None else DistanceParams(*params)
    check_params(p)
    cls = np.asarray(classes, np.uint8)
    if cls.ndim != 3:
        raise ValueError("mapdistance: classes must be (D, H, W)")
    r = int(p.max_dist); r2 = r * r
    f = np.where(sites_of(cls, p.site_mask), np.int32(0), _INF)
    if f.size:
        for axis in (2, 1, 0):                       # x, y, z
            f = _axis_pass(f, axis, r, r2)
    return _finish(f, p)


def brute(classes, params=None, chunk=2048):
    """the definition literally: every voxel against every site.  For small grids."""
    p = DistanceParams() if params is None else DistanceParams(*params)
    check_params(p)
    cls = np.asarray(classes, np.uint8)
    r2 = int(p.max_dist) ** 2
    site = sites_of(cls, p.site_mask)
    s = np.argwhere(site).astype(np.int64)                           # (m, 3): z, y, x
    v = np.argwhere(np.ones(cls.shape, bool)).astype(np.int64)
    best = np.full(len(v), _INF, np.int64)
    for a in range(0, len(s), chunk):
        for b in range(0, len(v), chunk):
            d = ((v[b:b + chunk, None, :] - s[None, a:a + chunk, :]) ** 2).sum(axis=2)
            best[b:b + chunk] = np.minimum(best[b:b + chunk], d.min(axis=1))
    best[best > r2] = _INF
    return _finish(best.reshape(cls.shape), p)


def slice2d(d2, iz_lo, iz_hi):
    """per column the smallest d2 over the layers iz_lo .. iz_hi inclusive, clipped to the grid - the 3-D clearance of an upright body spanning those layers;
    FAR when the band misses the grid -> (H, W) uint16"""
    if int(iz_lo) > int(iz_hi):
        raise ValueError("mapdistance: iz_lo > iz_hi")
    d = np.asarray(d2, np.uint16)
    Dd, Hd, Wd = d.shape
    lo, hi = max(int(iz_lo), 0), min(int(iz_hi), Dd - 1)
    if lo > hi:
        return np.full((Hd, Wd), FAR, np.uint16)
    return d[lo:hi + 1].min(axis=0)


def query(d2, classes, grid, xyz):
    """world points xyz (n, 3) f64 -> (d2 (n,) uint16, class (n,) uint8) of the voxel each falls in, by the occupancy map's own quantisation
    (mapoccupancy.quantise: c_k = (int64(rint((x_k * inv) * 1024)) >> 10) - minc_k, inv = 1.0 / voxel); FAR and OUTSIDE for a point that is not finite, has
    |x_k * inv| >= 2^20, or falls outside the grid"""
    g = mo.OccupancyGrid(*grid)
    d = np.asarray(d2, np.uint16); cls = np.asarray(classes, np.uint8)
    pts = np.asarray(xyz, np.float64).reshape(-1, 3)
    inv = np.float64(1.0) / np.float64(g.voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(pts * inv) < mo.COORD_LIMIT).all(axis=1)        # (a NaN fails the comparison)
    out_d = np.full(len(pts), FAR, np.uint16); out_c = np.full(len(pts), OUTSIDE, np.uint8)
    if ok.any():
        c = (mo.quantise(pts[ok], inv) >> mo.S) - np.asarray(g.minc, np.int64)
        inside = ((c >= 0) & (c < np.array([g.width, g.height, g.depth], np.int64))).all(axis=1)
        k = np.flatnonzero(ok)[inside]
        c = c[inside]
        out_d[k] = d[c[:, 2], c[:, 1], c[:, 0]]; out_c[k] = cls[c[:, 2], c[:, 1], c[:, 0]]
    return out_d, out_c


def metres(d2, voxel):
    """the field in metres, f64: sqrt(d2) * voxel, FAR -> inf"""
    d = np.asarray(d2, np.uint16)
    return np.where(d == FAR, np.inf, np.sqrt(d.astype(np.float64)) * float(voxel))


def inflate(occupancy_slice, d2_slice, r2):
    """a 2-D occupancy slice (mapoccupancy.slice2d: 0 unknown, 1 free, 2 occupied) inflated by a robot's radius: 2 where d2 <= r2, else the slice's value
    -> uint8.  FAR is never inflated: beyond max_dist the distance is not known, so r2 has a meaning only up to max_dist^2."""
    occ = np.asarray(occupancy_slice, np.uint8); d = np.asarray(d2_slice, np.uint16)
    if occ.shape != d.shape:
        raise ValueError("mapdistance: the two slices differ in shape")
    return np.where((d <= min(int(r2), FAR - 1)), np.uint8(2), occ).astype(np.uint8)
