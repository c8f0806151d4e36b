"""The two-way overlap of two clouds: the numpy twin of csrc/qn_overlap.hip (qn_kf_overlap_batch / qn_kf_verify_overlap) and its specification.
Pure numpy, no GPU.

For clouds A (n_a x 3 f32) and B (n_b x 3 f32) in one frame and a radius r > 0 (f64; r2 = float32(r * r)):
  d2(a, b)   the oracle's sqdist3 (oracle/gicp_oracle.cpp:15-18): f32 differences, dx*dx + dy*dy + dz*dz summed left to right in f32, no fused multiply-add;
  nn_d2[a]   min over the finite b of d2(a, b) if that minimum is <= r2, else +inf; nn_idx[a] the lowest index b that attains it, else -1.
             A non-finite point of A has +inf / -1, a non-finite point of B is nobody's neighbour;
  direction  n (points), n_finite, inliers (points with a finite nn_d2), sum_d2 (the f64 sum of those nn_d2);
  record     both directions, a_to_b and b_to_a (the C struct qn_overlap: two qn_overlap_dir of 24 bytes).
overlap_fraction and inlier_rmse are derived from a direction record alone and are 0 when their denominator is.

direction() computes the definition by brute force in blocks; direction_kdtree() is the scipy form (f64 distances: the same index sets wherever f32 and f64
agree, which tools/gpu_overlap_time.py uses as the host-side yardstick)."""
import math
import numpy as np

INF32 = np.float32(np.inf)


def radius2(radius):
    """float32(r * r), the product in f64"""
    r = float(radius)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("overlap: the radius must be finite and > 0")
    return np.float32(r * r)


def _xyz(cloud):
    a = np.asarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("overlap: a cloud is (n, >= 3) float32")
    return np.ascontiguousarray(a[:, :3])


def sqdist3_block(qa, b):
    """(m, 3) x (n, 3) -> (m, n) f32 squared distances in sqdist3's arithmetic (numpy's f32 ufuncs round every operation; there is no fused form)"""
    dx = qa[:, None, 0] - b[None, :, 0]
    dy = qa[:, None, 1] - b[None, :, 1]
    dz = qa[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest_unbounded(a, b, block=256):
    """-> min_d2 (n_a,) float32, idx (n_a,) int32: the nearest finite point of `b` for every finite point of `a`, whatever its distance (+inf / -1 for a
    non-finite point of `a` or without finite points in `b`).  nearest() is this followed by the radius test, so one pass serves many radii."""
    a = _xyz(a); b = _xyz(b)
    min_d2 = np.full(len(a), INF32, np.float32); idx = np.full(len(a), -1, np.int32)
    fa = np.isfinite(a).all(axis=1); fb = np.flatnonzero(np.isfinite(b).all(axis=1))
    if not len(fb) or not fa.any():
        return min_d2, idx
    bf = b[fb]
    rows = np.flatnonzero(fa)
    step = max(1, int(block))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(rows), step):
            r = rows[s:s + step]
            d = sqdist3_block(a[r], bf)
            j = np.argmin(d, axis=1)                         # the first minimum: fb ascends, so the lowest original index
            min_d2[r] = d[np.arange(len(r)), j]; idx[r] = fb[j].astype(np.int32)
    return min_d2, idx


def apply_radius(min_d2, idx, radius):
    """the radius test of the definition on nearest_unbounded's output -> nn_d2, nn_idx"""
    ok = (idx >= 0) & (min_d2 <= radius2(radius))
    return np.where(ok, min_d2, INF32).astype(np.float32), np.where(ok, idx, -1).astype(np.int32)


def nearest(a, b, radius, block=256):
    """-> nn_d2 (n_a,) float32, nn_idx (n_a,) int32: every point of `a` against `b`, by the definition above"""
    radius2(radius)
    return apply_radius(*nearest_unbounded(a, b, block), radius)


def record(a, nn_d2):
    """the direction record of cloud `a` from its nn_d2"""
    inl = np.isfinite(nn_d2)
    return dict(n=int(len(a)), n_finite=int(np.isfinite(_xyz(a)).all(axis=1).sum()), inliers=int(inl.sum()), sum_d2=float(np.sum(nn_d2[inl].astype(np.float64))))


def direction(a, b, radius, block=256, points=False):
    """-> dict(n, n_finite, inliers, sum_d2) of `a` against `b` (points=True: also nn_d2, nn_idx)"""
    a = _xyz(a)
    nn_d2, nn_idx = nearest(a, b, radius, block)
    rec = record(a, nn_d2)
    if points:
        rec["nn_d2"] = nn_d2; rec["nn_idx"] = nn_idx
    return rec


def overlap(a, b, radius, block=256, points=False):
    """-> dict(a_to_b=direction(a, b), b_to_a=direction(b, a)): the record of one pair"""
    return dict(a_to_b=direction(a, b, radius, block, points), b_to_a=direction(b, a, radius, block, points))


def overlap_fraction(d):
    """inliers / n_finite of one direction record (0 without finite points)"""
    return d["inliers"] / d["n_finite"] if d["n_finite"] else 0.0


def inlier_rmse(d):
    """sqrt(sum_d2 / inliers) of one direction record (0 without inliers)"""
    return math.sqrt(d["sum_d2"] / d["inliers"]) if d["inliers"] else 0.0


def direction_kdtree(a, b, radius):
    """The same record through scipy.spatial.cKDTree (f64 distances: indices and counts agree with direction() wherever the f32 and f64 distances order
    alike, sum_d2 is the f64 one).  The host-side form for timing and for cross-checking the index sets."""
    from scipy.spatial import cKDTree
    a = _xyz(a).astype(np.float64); b = _xyz(b).astype(np.float64)
    fa = np.isfinite(a).all(axis=1); fb = np.flatnonzero(np.isfinite(b).all(axis=1))
    nn_idx = np.full(len(a), -1, np.int32); d = np.full(len(a), np.inf)
    if len(fb) and fa.any():
        dist, j = cKDTree(b[fb]).query(a[fa], k=1, distance_upper_bound=float(np.nextafter(float(radius), np.inf)))     # the bound itself is excluded by scipy
        ok = np.isfinite(dist)
        rows = np.flatnonzero(fa)
        nn_idx[rows[ok]] = fb[j[ok]].astype(np.int32); d[rows[ok]] = dist[ok]
    inl = np.isfinite(d)
    return dict(n=int(len(a)), n_finite=int(fa.sum()), inliers=int(inl.sum()), sum_d2=float(np.sum(d[inl] * d[inl])), nn_idx=nn_idx)
