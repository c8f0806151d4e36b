"""Isolated noise points of a cloud - PCL's RadiusOutlierRemoval and StatisticalOutlierRemoval over one bounded-radius k-nearest selection: the numpy twin of
csrc/qn_mapoutliers.hip (qn_kf_map_outliers / qn_kf_map_remove_outliers) and its specification.  Pure numpy, no GPU.

For the n records of a cloud (x y z, anything behind carried along), a radius r (f64, finite, > 0; r2 = float32(r * r) as overlap.radius2), std_mul (f64,
finite, >= 0) and k (1 .. MAX_K = 32):
  neighbours of p   the finite points q AT ANOTHER INDEX than p with sqdist3(p, q) <= r2 - overlap.sqdist3_block's f32 arithmetic, <= inclusive.  A duplicate
                    of p at another index counts.  count = their number (u32).  A non-finite p has none.
  sparse            a finite p with count < k: an outlier outright (the radius rule with min_neighbors = k); mean_q = 0xffffffff, no part in the statistics.
  dense             count >= k.  The k smallest d2 as a multiset (ties need no tie-break), ascending d2_1 <= ... <= d2_k;
                    s = ((sqrt(d2_1) + sqrt(d2_2)) + ...) + sqrt(d2_k), each sqrt the correctly rounded f64 root of the f32 value widened to f64, summed in
                    that order in f64; mean_q = uint32(rint(s / k * 2^e)), half to even, e = quant_exponent(r), the largest integer with r * 2^e <= 2^16
                    (kept within [-126, 127]).  mean_q <= 2^16 + 1.
  statistics        over the dense points, exact integers: dense = N, sum_q = sum mean_q, sum_q2 = sum mean_q^2 (u64; exact below MAX_POINTS = 2^30 points).
  threshold         f64, every operation rounded on its own: mean = sum_q / N; var = (sum_q2 - sum_q * sum_q / N) / (N - 1) for N > 1, else 0, clamped at 0;
                    thr_q = mean + std_mul * sqrt(var) (PCL's formula on the quantised mean distances).  N == 0: all three 0.
  removed           a finite p that is sparse or has double(mean_q) > thr_q.  A non-finite record has count 0 and mean_q 0xffffffff and is never removed.
Everything per point is an integer, so no order of meeting the neighbours changes it.
"""
import math
from collections import namedtuple
import numpy as np
from . import overlap

OutlierParams = namedtuple("OutlierParams", "radius std_mul k", defaults=(1.0, 2.0, 8))      # interface choices, not measurements
OutlierStats = namedtuple("OutlierStats", "n n_finite dense sparse removed quant_exp sum_q sum_q2 mean_q std_q thr_q")
MAX_K = 32
MAX_POINTS = 1 << 30
NO_MEAN = 0xffffffff


def check_params(radius, std_mul, k):
    overlap.radius2(radius)
    s = float(std_mul)
    if not (math.isfinite(s) and s >= 0.0):
        raise ValueError("mapoutliers: std_mul must be finite and >= 0")
    if int(k) != k or not (1 <= int(k) <= MAX_K):
        raise ValueError("mapoutliers: k must be an integer in 1 .. %d" % MAX_K)


def quant_exponent(radius):
    """the largest e with r * 2^e <= 2^16 (f64; exact through frexp), clamped to the exponents of normal f32 powers of two"""
    overlap.radius2(radius)
    m, x = math.frexp(float(radius))                 # r = m 2^x, 0.5 <= m < 1
    e = 17 - x if m == 0.5 else 16 - x
    return max(-126, min(127, e))


def threshold(dense, sum_q, sum_q2, std_mul):
    """-> (mean_q, std_q, thr_q) f64 from the integer statistics, in the order the C library computes them"""
    if dense == 0:
        return 0.0, 0.0, 0.0
    N = np.float64(dense); s = np.float64(int(sum_q)); s2 = np.float64(int(sum_q2))
    mean = s / N
    var = (s2 - s * s / N) / np.float64(dense - 1) if dense > 1 else np.float64(0.0)
    var = max(var, np.float64(0.0))
    std = np.sqrt(var)
    return float(mean), float(std), float(mean + np.float64(std_mul) * std)


def knn_mean(cloud, radius, k, block=256):
    """-> count (n,) uint32, mean_q (n,) uint32 (NO_MEAN where count < k or the record is non-finite).  Brute force in blocks of queries; the blocks are taken
    in x order and meet only the points within 1.5 r of the block in x, which drops no neighbour (|dx| > 1.5 r gives d2 > r2 wherever r2 is a normal number
    with room below it; for a smaller radius nothing is pruned)."""
    a = overlap._xyz(cloud)
    r2 = overlap.radius2(radius)
    k = int(k)
    scale = np.float64(math.ldexp(1.0, quant_exponent(radius)))
    n = len(a)
    count = np.zeros(n, np.uint32); mean_q = np.full(n, NO_MEAN, np.uint32)
    rows = np.flatnonzero(np.isfinite(a).all(axis=1))
    rows = rows[np.argsort(a[rows, 0], kind="stable")]
    b = a[rows]                                      # a non-finite point is nobody's neighbour
    bx = b[:, 0].astype(np.float64)
    prune = float(r2) >= 2.0 ** -100
    w = 1.5 * float(radius)
    step = max(1, int(block))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(rows), step):
            e = min(s + step, len(rows))
            lo, hi = (int(np.searchsorted(bx, bx[s] - w, "left")), int(np.searchsorted(bx, bx[e - 1] + w, "right"))) if prune else (0, len(rows))
            d2 = overlap.sqdist3_block(b[s:e], b[lo:hi])
            nb = d2 <= r2
            nb[np.arange(e - s), np.arange(s, e) - lo] = False          # the point itself (its own index only: a duplicate elsewhere stays)
            cnt = nb.sum(axis=1)
            count[rows[s:e]] = cnt.astype(np.uint32)
            qi, cj = np.nonzero(nb)
            v = d2[qi, cj]
            o = np.lexsort((v, qi))                                      # by query, ascending d2 inside
            qi = qi[o]; v = v[o]
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            rank = np.arange(len(qi)) - start[qi]
            dense = np.flatnonzero(cnt >= k)
            if not len(dense):
                continue
            slot = np.full(e - s, -1); slot[dense] = np.arange(len(dense))
            take = (rank < k) & (slot[qi] >= 0)
            part = np.zeros((len(dense), k), np.float32)
            part[slot[qi[take]], rank[take]] = v[take]
            root = np.sqrt(part.astype(np.float64))
            acc = root[:, 0].copy()
            for j in range(1, k):
                acc = acc + root[:, j]
            mean_q[rows[s:e][dense]] = np.rint(acc / np.float64(k) * scale).astype(np.uint32)
    return count, mean_q


def classify(cloud, params=None, block=256):
    """-> dict(count (n,) u32, mean_q (n,) u32, removed (n,) u8, stats: an OutlierStats)"""
    p = OutlierParams() if params is None else OutlierParams(*params)
    check_params(p.radius, p.std_mul, p.k)
    a = overlap._xyz(cloud)
    n = len(a)
    if n >= MAX_POINTS:
        raise ValueError("mapoutliers: 2^30 or more points")
    fin = np.isfinite(a).all(axis=1)
    count, mean_q = knn_mean(a, p.radius, p.k, block)
    dense = fin & (count >= np.uint32(p.k))
    N = int(dense.sum())
    mq = [int(v) for v in mean_q[dense]]                                # Python integers: exact whatever the size
    sum_q = sum(mq); sum_q2 = sum(v * v for v in mq)
    mean, std, thr = threshold(N, sum_q, sum_q2, p.std_mul)
    removed = fin & (~dense | (mean_q.astype(np.float64) > thr))
    stats = OutlierStats(n, int(fin.sum()), N, int((fin & ~dense).sum()), int(removed.sum()), quant_exponent(p.radius), sum_q, sum_q2, mean, std, thr)
    return dict(count=count, mean_q=mean_q, removed=removed.astype(np.uint8), stats=stats)


def remove(cloud, params=None, block=256):
    """-> the kept records of `cloud`, in order and with every column (what qn_kf_map_remove_outliers leaves in the map slot)"""
    c = np.asarray(cloud)
    return np.ascontiguousarray(c[classify(c, params, block)["removed"] == 0])
