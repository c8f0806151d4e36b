"""The numpy twin of the map's outlier filter (qn_amd/mapoutliers.py, the specification of qn_kf_map_outliers) against an O(n^2) brute force written from the
definition with Python scalars, and the hand cases whose answers follow from the geometry.  No GPU."""
import math
import numpy as np
import pytest
from qn_amd import mapoutliers as mo

F = np.float32


def brute(cloud, radius, std_mul, k):
    """the definition, one pair at a time"""
    a = np.asarray(cloud, np.float32)[:, :3]
    n = len(a)
    r2 = F(float(radius) * float(radius))
    e = mo.quant_exponent(radius)
    fin = [bool(np.isfinite(a[i]).all()) for i in range(n)]
    count = [0] * n; mean_q = [mo.NO_MEAN] * n
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            if not fin[i]:
                continue
            d = []
            for j in range(n):
                if j == i or not fin[j]:
                    continue
                dx = a[i, 0] - a[j, 0]; dy = a[i, 1] - a[j, 1]; dz = a[i, 2] - a[j, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 <= r2:
                    d.append(d2)
            count[i] = len(d)
            if len(d) >= k:
                s = 0.0
                for v in sorted(d)[:k]:
                    s = s + math.sqrt(float(v))                      # (math.sqrt is the correctly rounded IEEE root)
                mean_q[i] = int(np.rint(s / k * math.ldexp(1.0, e)))
    dense = [i for i in range(n) if fin[i] and count[i] >= k]
    N = len(dense); sq = sum(mean_q[i] for i in dense); sq2 = sum(mean_q[i] ** 2 for i in dense)
    if N:
        mean = float(sq) / N
        var = max((float(sq2) - float(sq) * float(sq) / N) / (N - 1), 0.0) if N > 1 else 0.0
        thr = mean + float(std_mul) * math.sqrt(var)
    else:
        mean = var = thr = 0.0
    removed = [1 if fin[i] and (count[i] < k or float(mean_q[i]) > thr) else 0 for i in range(n)]
    return count, mean_q, removed, (N, sq, sq2, mean, math.sqrt(var), thr)


def same_as_brute(cloud, params):
    got = mo.classify(cloud, params)
    count, mean_q, removed, (N, sq, sq2, mean, std, thr) = brute(cloud, *params)
    assert got["count"].dtype == np.uint32 and got["mean_q"].dtype == np.uint32 and got["removed"].dtype == np.uint8
    assert got["count"].tolist() == count and got["mean_q"].tolist() == mean_q and got["removed"].tolist() == removed
    s = got["stats"]
    assert (s.n, s.dense, s.sum_q, s.sum_q2, s.mean_q, s.std_q, s.thr_q) == (len(cloud), N, sq, sq2, mean, std, thr)
    assert s.sparse == s.n_finite - N and s.removed == sum(removed) and s.quant_exp == mo.quant_exponent(params[0])
    return got


@pytest.mark.parametrize("seed,n,radius,std_mul,k", [(1, 300, 0.25, 1.0, 4), (2, 257, 0.3, 0.0, 1), (3, 400, 0.4, 2.0, 8), (4, 350, 0.6, 0.5, 17), (5, 300, 1.5, 3.0, 32)])
def test_random_clouds_against_the_brute_force(seed, n, radius, std_mul, k):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) * [1.0, 1.0, 0.2]
    c[:, 3] = rng.uniform(0, 255, n)
    c[rng.choice(n, 30, replace=False), :3] = c[rng.choice(n, 30), :3]           # duplicated points, at other indices
    c[[7, 91, 200], :3] = [[np.nan, 0, 0], [0, np.inf, 0.1], [0.2, 0.1, -np.inf]]
    c[15, :3] = [3e38, -3e38, 3e38]                                             # differences that overflow f32
    got = same_as_brute(c, (radius, std_mul, k))
    bad = ~np.isfinite(c[:, :3]).all(axis=1)
    assert (got["count"][bad] == 0).all() and (got["mean_q"][bad] == mo.NO_MEAN).all() and (got["removed"][bad] == 0).all()
    kept = mo.remove(c, (radius, std_mul, k))
    assert kept.dtype == np.float32 and np.array_equal(kept.view(np.uint32), c[got["removed"] == 0].view(np.uint32))
    assert np.array_equal(mo.classify(c, (radius, std_mul, k), block=37)["mean_q"], got["mean_q"])      # the twin's own block size changes nothing


def test_a_tiny_radius_is_not_pruned():
    c = np.zeros((40, 3), np.float32); c[:, 0] = np.arange(40) * F(1e-30)
    same_as_brute(c, (2.5e-30, 1.0, 2))


H = F(0.25)


def lattice(m=9):
    k = np.arange(m).astype(np.float32) * H
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(x.size, np.float32)], axis=1)


def test_planar_lattice_by_hand():
    """spacing h = 2^-2, radius 0.3: the neighbours are the four axis partners at exactly h (the diagonal, h sqrt 2 = 0.354, is outside)"""
    pts = lattice()
    got = same_as_brute(pts, (0.3, 2.0, 4))
    e = mo.quant_exponent(0.3)
    assert e == 17 and got["stats"].quant_exp == 17                  # 0.3 * 2^17 = 39321.6 <= 2^16 < 0.3 * 2^18
    ij = np.rint(pts[:, :2] / H).astype(int)
    inner = ((ij > 0) & (ij < 8)).all(axis=1)
    assert inner.sum() == 49
    assert (got["count"][inner] == 4).all() and (got["mean_q"][inner] == int(0.25 * 2 ** 17)).all()
    assert (got["count"][~inner] < 4).all() and (got["mean_q"][~inner] == mo.NO_MEAN).all()
    # all mean_q equal: var = 0, the threshold is the mean and removes nothing; the border goes by the radius rule alone
    s = got["stats"]
    assert (s.dense, s.sparse, s.std_q, s.thr_q, s.mean_q) == (49, 32, 0.0, 32768.0, 32768.0)
    assert np.array_equal(got["removed"], (~inner).astype(np.uint8)) and s.removed == 32
    assert np.array_equal(mo.classify(pts, (0.3, 0.0, 4))["removed"], got["removed"])       # std_mul = 0: still nothing above the mean


def test_an_isolated_point_is_removed():
    pts = np.concatenate([lattice(), [[1.0, 1.0, 0.9]]]).astype(np.float32)                # 3 r above the lattice's middle
    got = same_as_brute(pts, (0.3, 2.0, 4))
    assert got["count"][-1] == 0 and got["mean_q"][-1] == mo.NO_MEAN and got["removed"][-1] == 1
    assert np.array_equal(got["count"][:-1], mo.classify(lattice(), (0.3, 2.0, 4))["count"])


def test_a_dense_but_far_point_goes_by_the_threshold():
    """a lattice of spacing 0.1 (mean distance of the 4 nearest: 0.1) and a point 0.9 r above its middle, r = 0.5: it has more than k neighbours, all of them at
    0.45 or more"""
    k = np.arange(11).astype(np.float32) * F(0.1)
    x, y = np.meshgrid(k, k, indexing="ij")
    pts = np.concatenate([np.stack([x.ravel(), y.ravel(), np.zeros(x.size, np.float32)], axis=1), [[0.5, 0.5, 0.45]]]).astype(np.float32)
    at0 = same_as_brute(pts, (0.5, 0.0, 4))
    assert at0["count"][-1] >= 4 and at0["mean_q"][-1] != mo.NO_MEAN and at0["mean_q"][-1] >= int(0.45 * 2 ** 17)
    assert at0["removed"][-1] == 1
    wide = same_as_brute(pts, (0.5, 1000.0, 4))
    assert wide["removed"][-1] == 0 and wide["stats"].removed == 0 and np.array_equal(wide["mean_q"], at0["mean_q"])


def test_no_dense_point_and_one_dense_point():
    far = np.array([[0, 0, 0], [5, 0, 0], [0, 5, 0]], np.float32)
    got = same_as_brute(far, (1.0, 2.0, 1))
    s = got["stats"]
    assert (s.dense, s.sum_q, s.sum_q2, s.mean_q, s.std_q, s.thr_q, s.sparse, s.removed) == (0, 0, 0, 0.0, 0.0, 0.0, 3, 3)
    # N = 1: a pair 0.5 apart of which one point also sees a third one; with k = 2 only that one is dense
    three = np.array([[0, 0, 0], [0.5, 0, 0], [-0.75, 0, 0]], np.float32)
    got = same_as_brute(three, (1.0, 0.0, 2))
    s = got["stats"]
    assert got["count"].tolist() == [2, 1, 1] and s.dense == 1 and s.std_q == 0.0
    assert got["mean_q"][0] == int(0.625 * 2 ** 16) == s.sum_q == s.thr_q and s.sum_q2 == s.sum_q ** 2
    assert got["removed"].tolist() == [0, 1, 1]
    assert mo.classify(np.zeros((0, 3), np.float32))["stats"].n == 0
    one = mo.classify(np.zeros((1, 3), np.float32), (1.0, 2.0, 1))
    assert one["count"].tolist() == [0] and one["removed"].tolist() == [1]


def test_more_than_k_neighbours_tied_at_the_kth_distance():
    """six neighbours at exactly 0.5 on the axes and one at 0.25: with k = 3 the third smallest is one of six equal values"""
    pts = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32)
    got = same_as_brute(pts, (0.6, 2.0, 3))
    assert got["count"][0] == 7
    assert got["mean_q"][0] == int(np.rint((0.25 + 0.5 + 0.5) / 3 * 2 ** 16))
    dup = np.concatenate([pts, pts[:1], pts[:1]])                                          # duplicates of the query: neighbours at distance 0
    got = same_as_brute(dup, (0.6, 2.0, 3))
    assert got["count"][0] == 9 and got["mean_q"][0] == int(np.rint(0.25 / 3 * 2 ** 16))


def test_statistics_arithmetic_with_python_integers():
    mean, std, thr = mo.threshold(4, 10, 30, 1.5)
    assert (mean, std, thr) == (2.5, math.sqrt((30.0 - 100.0 / 4.0) / 3.0), 2.5 + 1.5 * math.sqrt(5.0 / 3.0))
    # the largest sums the capacity allows stay exact integers: 2^30 - 1 points of mean_q 2^16 + 1
    N = mo.MAX_POINTS - 1; q = (1 << 16) + 1
    assert N * q * q < 1 << 64
    mean, std, thr = mo.threshold(N, N * q, N * q * q, 2.0)
    assert mean == float(q) and std == 0.0 and thr == float(q)
    assert mo.threshold(0, 0, 0, 2.0) == (0.0, 0.0, 0.0) and mo.threshold(1, 7, 49, 9.0) == (7.0, 0.0, 7.0)
    assert mo.threshold(2, 3, 4, 1.0)[1] == 0.0                      # a negative variance (inconsistent sums) is clamped


def test_quant_exponent_and_params():
    for r, e in [(1.0, 16), (0.5, 17), (0.3, 17), (0.6, 16), (2.0, 15), (1.9999, 15), (65536.0, 0), (1e-45, 127), (1e18, -44)]:
        assert mo.quant_exponent(r) == e, r
        assert r * 2.0 ** e <= 2.0 ** 16 and (e in (-126, 127) or r * 2.0 ** (e + 1) > 2.0 ** 16)
    assert mo.OutlierParams() == (1.0, 2.0, 8) and mo.MAX_K == 32
    c = np.zeros((4, 3), np.float32)
    for bad in [(0.0, 2.0, 8), (-1.0, 2.0, 8), (float("nan"), 2.0, 8), (float("inf"), 2.0, 8), (1.0, -0.1, 8), (1.0, float("nan"), 8), (1.0, float("inf"), 8),
                (1.0, 2.0, 0), (1.0, 2.0, 33), (1.0, 2.0, 2.5)]:
        with pytest.raises(ValueError):
            mo.classify(c, bad)
