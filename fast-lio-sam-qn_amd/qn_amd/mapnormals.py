"""Surface normals and curvature of a cloud from fixed-radius neighbourhoods: the numpy twin of csrc/qn_mapnormals.hip (qn_kf_map_normals) and its
specification.  Pure numpy, no GPU.

For the n records of a cloud (x y z, anything behind ignored), a radius r (f64, finite, > 0; r2 = float32(r * r) as overlap.radius2), min_neighbors (>= 3)
and V viewpoints (V x 3 f64, finite; V may be 0):
  neighbours of p   the finite points q, p itself included, with sqdist3(p, q) <= r2 - overlap.sqdist3_block's f32 arithmetic, <= inclusive.  A non-finite p
                    has none.
  moments           e = quant_exponent(r), the largest integer with r * 2^e <= 2^20 (kept within [-126, 127], where 2^e is a normal f32).  Per neighbour
                    d = q - p per axis in f32 and di = int32(rint(d * 2^e)): the product is exact and the rounding is half to even; |di| <= 2^20 + 1.
                    count = the neighbours (u32), s1[3] = sum di, s2[6] = sum di * dj in the order xx xy xz yy yz zz, both int64: exact integers, so no
                    summation order changes them (nothing overflows below 2^21 neighbours).
  covariance        f64, every operation rounded on its own (no fused multiply-add): m = double(s1) / count, C_ij = double(s2_ij) / count - m_i * m_j, in
                    units of 2^-2e m^2; trace = (C_xx + C_yy) + C_zz.
  valid             count >= min_neighbors and trace > 0; otherwise normal and curvature are NaN.
  normal            the unit eigenvector of the smallest eigenvalue l0 <= l1 <= l2 of C (numpy.linalg.eigh), oriented as below, rounded to f32.
  curvature         l0 / ((l0 + l1) + l2) with l0 clamped at 0 first (PCL's surface variation), rounded to f32.
  view_idx          (i32) the viewpoint with the smallest f64 ((dx * dx + dy * dy) + dz * dz), d = v - double(p), the lowest index on ties; -1 when V = 0
                    or p is non-finite.
  orientation       with a viewpoint v: the normal is negated when (n_x * dx + n_y * dy) + n_z * dz < 0 (f64, n the f64 eigenvector, d = v - double(p));
                    with V = 0: when its component of largest magnitude is negative (the lowest axis on a tie).
Where the answer is well conditioned is what `gap` and `view_cos` say: gap = (l1 - l0) / l2, the relative eigen-gap that bounds how far another backward-stable
solve may turn the normal, and view_cos = |n . d| / |d| (with V = 0: the lead of the largest component over the runner-up), how far the sign is from a coin toss.
"""
import math
from collections import namedtuple
import numpy as np
from . import overlap

NormalParams = namedtuple("NormalParams", "radius min_neighbors", defaults=(0.6, 5))
MAX_NEIGHBORS = 1 << 21          # a 3 x 3 x 3 cell block with this many points is refused by the kernel (QN_ERR_CAPACITY)


def check_params(radius, min_neighbors):
    overlap.radius2(radius)
    if int(min_neighbors) != min_neighbors or not (3 <= int(min_neighbors) <= 0xffffffff):
        raise ValueError("mapnormals: min_neighbors must be an integer >= 3")


def quant_exponent(radius):
    """the largest e with r * 2^e <= 2^20 (f64; exact through frexp), clamped to the exponents of normal f32 powers of two"""
    overlap.radius2(radius)
    m, x = math.frexp(float(radius))                 # r = m 2^x, 0.5 <= m < 1
    e = 21 - x if m == 0.5 else 20 - x
    return max(-126, min(127, e))


def _viewpoints(viewpoints):
    v = np.zeros((0, 3)) if viewpoints is None else np.ascontiguousarray(np.asarray(viewpoints, dtype=np.float64).reshape(-1, 3))
    if not np.isfinite(v).all():
        raise ValueError("mapnormals: a viewpoint is not finite")
    return v


def moments(cloud, radius, block=256):
    """-> count (n,) uint32, s1 (n, 3) int64, s2 (n, 6) int64 by brute force in blocks of queries"""
    a = overlap._xyz(cloud)
    r2 = overlap.radius2(radius)
    scale = np.float32(math.ldexp(1.0, quant_exponent(radius)))
    n = len(a)
    count = np.zeros(n, np.uint32); s1 = np.zeros((n, 3), np.int64); s2 = np.zeros((n, 6), np.int64)
    fin = np.isfinite(a).all(axis=1)
    rows = np.flatnonzero(fin)
    b = a[rows]                                      # a non-finite point is nobody's neighbour
    step = max(1, int(block))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(rows), step):
            r = rows[s:s + step]
            p = a[r]
            nb = overlap.sqdist3_block(p, b) <= r2
            d = b[None, :, :] - p[:, None, :]                         # q - p, f32
            di = np.where(nb[:, :, None], np.rint(d * scale), np.float32(0)).astype(np.int64)      # (exact in f32: |d 2^e| <= 2^20 + 1)
            count[r] = nb.sum(axis=1).astype(np.uint32)
            s1[r] = di.sum(axis=1)
            k = 0
            for i in range(3):
                for j in range(i, 3):
                    s2[r, k] = (di[:, :, i] * di[:, :, j]).sum(axis=1); k += 1
    return count, s1, s2


def covariance(count, s1, s2):
    """-> C (n, 3, 3) f64 and trace (n,) by the definition (rows with count 0: zeros)"""
    n = len(count)
    C = np.zeros((n, 3, 3)); tr = np.zeros(n)
    ok = np.flatnonzero(count > 0)
    k = count[ok].astype(np.float64)
    m = s1[ok].astype(np.float64) / k[:, None]
    q = 0
    for i in range(3):
        for j in range(i, 3):
            c = s2[ok, q].astype(np.float64) / k - m[:, i] * m[:, j]
            C[ok, i, j] = c; C[ok, j, i] = c; q += 1
    tr[ok] = (C[ok, 0, 0] + C[ok, 1, 1]) + C[ok, 2, 2]
    return C, tr


def nearest_viewpoint(cloud, viewpoints):
    """-> view_idx (n,) int32"""
    a = overlap._xyz(cloud); v = _viewpoints(viewpoints)
    idx = np.full(len(a), -1, np.int32)
    fin = np.flatnonzero(np.isfinite(a).all(axis=1))
    if len(v) and len(fin):
        p = a[fin].astype(np.float64)
        for s in range(0, len(fin), 4096):
            q = p[s:s + 4096]
            dx = v[None, :, 0] - q[:, None, 0]; dy = v[None, :, 1] - q[:, None, 1]; dz = v[None, :, 2] - q[:, None, 2]
            idx[fin[s:s + 4096]] = np.argmin((dx * dx + dy * dy) + dz * dz, axis=1).astype(np.int32)      # the first minimum: the lowest index
    return idx


def normals(cloud, params=None, viewpoints=None, block=256):
    """-> dict(normals (n, 3) f32, curvature (n,) f32, count (n,) u32, view_idx (n,) i32, s1, s2, and per point gap, view_cos (f64, NaN where not valid))"""
    p = NormalParams() if params is None else NormalParams(*params)
    check_params(p.radius, p.min_neighbors)
    a = overlap._xyz(cloud); v = _viewpoints(viewpoints)
    n = len(a)
    count, s1, s2 = moments(a, p.radius, block)
    C, tr = covariance(count, s1, s2)
    view_idx = nearest_viewpoint(a, v)
    nrm = np.full((n, 3), np.nan, np.float32); curv = np.full(n, np.nan, np.float32)
    gap = np.full(n, np.nan); view_cos = np.full(n, np.nan)
    ok = np.flatnonzero((count >= np.uint32(p.min_neighbors)) & (tr > 0.0))
    if len(ok):
        w, U = np.linalg.eigh(C[ok])
        n0 = U[:, :, 0].copy()
        l0 = np.maximum(w[:, 0], 0.0)
        curv[ok] = (l0 / ((l0 + w[:, 1]) + w[:, 2])).astype(np.float32)
        gap[ok] = (w[:, 1] - w[:, 0]) / w[:, 2]
        if len(v):
            d = v[view_idx[ok]] - a[ok].astype(np.float64)
            dot = (n0[:, 0] * d[:, 0] + n0[:, 1] * d[:, 1]) + n0[:, 2] * d[:, 2]
            flip = dot < 0.0
            with np.errstate(invalid="ignore", divide="ignore"):
                view_cos[ok] = np.abs(dot) / np.sqrt((d * d).sum(axis=1))
        else:
            mag = np.abs(n0)
            lead = np.argmax(mag, axis=1)                             # the first maximum: the lowest axis
            flip = n0[np.arange(len(ok)), lead] < 0.0
            srt = np.sort(mag, axis=1)
            view_cos[ok] = srt[:, 2] - srt[:, 1]
        n0[flip] = -n0[flip]
        nrm[ok] = n0.astype(np.float32)
    return dict(normals=nrm, curvature=curv, count=count, view_idx=view_idx, s1=s1, s2=s2, gap=gap, view_cos=view_cos)
