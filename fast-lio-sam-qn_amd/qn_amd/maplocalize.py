"""Neighbourhoods cut out of the corrected map around pose guesses: the numpy twin of the crop kernels in csrc/qn_maplocalize.inc (qn_kf_map_crop /
qn_kf_map_localize[_c2f]) and their specification.  Pure numpy, no GPU.

For the n records of a map (x y z intensity, f32), a centre (three f64 values, each rounded to f32), a radius R (f64, finite, > 0) and a shape:
  r2       float32(R * R), the product taken in f64 (overlap.radius2)
  d2       dx = p.x - c.x, dy, dz likewise in f32; d2 = (dx dx + dy dy) + dz dz, every operation rounded to f32 on its own, summed left to right
           (CYLINDER: d2 = dx dx + dy dy, an upright cylinder without ends)
  member   x, y and z finite and d2 <= r2, inclusive.  A non-finite record is never a member (for the cylinder a non-finite z as well).
  crop     the members' full 16-byte records in ascending map index, and with every record its map index (u32).
The localise calls take the centre from the pose guess: guess_f32(P) rounds every entry of the 4x4 guess to f32 once, and the same numbers are the crop
centre (the translation column) and the registration's seed.
"""
from collections import namedtuple
import numpy as np
from . import overlap

SPHERE, CYLINDER = 0, 1
MAX_CROPS = 32767
PASS = 64                                                            # centres per streaming pass of the kernels (a launch seam, no part of the rule)
LocalizeParams = namedtuple("LocalizeParams", "radius leaf score_thr shape", defaults=(35.0, 0.3, 1.5, SPHERE))      # config.yaml's radius, voxel and score
F = np.float32


def centre_f32(centre):
    """the three f64 values rounded to f32; a centre that is not finite (before or after the rounding) is refused"""
    c64 = np.asarray(centre, dtype=np.float64).reshape(3)
    with np.errstate(over="ignore"):
        c = c64.astype(F)
    if not (np.isfinite(c64).all() and np.isfinite(c).all()):
        raise ValueError("maplocalize: a centre must be finite")
    return c


def crop_indices(map_xyzi, centre, radius, shape=SPHERE):
    """-> the map indices (u32, ascending) of the members of the crop"""
    if shape not in (SPHERE, CYLINDER):
        raise ValueError("maplocalize: shape must be SPHERE or CYLINDER")
    r2 = overlap.radius2(radius)
    c = centre_f32(centre)
    p = np.asarray(map_xyzi, dtype=F)
    if p.ndim != 2 or p.shape[1] < 3:
        raise ValueError("maplocalize: a map is (n, >= 3) float32")
    with np.errstate(invalid="ignore", over="ignore"):
        dx = p[:, 0] - c[0]; dy = p[:, 1] - c[1]; dz = p[:, 2] - c[2]
        d2 = dx * dx + dy * dy                                       # (f32 arrays: every product and sum rounded on its own)
        if shape == SPHERE:
            d2 = d2 + dz * dz
        member = np.isfinite(p[:, :3]).all(axis=1) & (d2 <= r2)
    return np.flatnonzero(member).astype(np.uint32)


def crop(map_xyzi, centre, radius, shape=SPHERE):
    """-> (records (m, 4) f32: the members' own bytes, indices (m,) u32)"""
    p = np.ascontiguousarray(map_xyzi, dtype=F).reshape(-1, 4)
    idx = crop_indices(p, centre, radius, shape)
    return p[idx].copy(), idx


def guess_f32(P):
    """the 4x4 guess (map <- sensor) with every entry rounded to f32 -> (4, 4) f32; its [:3, 3] is the crop centre.  Refused: a non-finite entry, a last row
    other than 0 0 0 1."""
    P64 = np.asarray(P, dtype=np.float64).reshape(4, 4)
    with np.errstate(over="ignore"):
        g = P64.astype(F)
    if not (np.isfinite(P64).all() and np.isfinite(g).all()):
        raise ValueError("maplocalize: a guess must be finite")
    if not np.array_equal(P64[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("maplocalize: the last row of a guess must be 0 0 0 1")
    return g


def transform_final(src_xyz, T):
    """QN_VERIFY_FINAL of a GICP-path pair: the cloud through the f32 T as align() fills aligned_, T0 x + (T1 y + (T2 z + T3)) in f32 -> (n, 3) f32"""
    T = np.asarray(T, dtype=F).reshape(4, 4)
    p = np.asarray(src_xyz, dtype=F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([T[r, 0] * x + (T[r, 1] * y + (T[r, 2] * z + T[r, 3])) for r in range(3)], axis=1).astype(F)
