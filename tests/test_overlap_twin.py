"""The numpy twin of the two-way overlap (qn_amd/overlap.py), which is the specification of qn_kf_overlap_batch: against a literal double loop, against
scipy's cKDTree on coordinates where f32 and f64 distances agree exactly, and on the cases the definition spells out.  No GPU needed."""
import math
import numpy as np
import pytest
from qn_amd import overlap as ov


def _loop(a, b, r):
    """the definition, one pair of points at a time, every operation a rounded f32 one"""
    f = np.float32
    r2 = f(float(r) * float(r))
    d2 = np.full(len(a), np.inf, np.float32); idx = np.full(len(a), -1, np.int32)
    for i, p in enumerate(a):
        if not np.isfinite(p).all():
            continue
        best, bi = None, -1
        for j, q in enumerate(b):
            if not np.isfinite(q).all():
                continue
            dx, dy, dz = f(p[0] - q[0]), f(p[1] - q[1]), f(p[2] - q[2])
            d = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
            if best is None or d < best:
                best, bi = d, j
        if best is not None and best <= r2:
            d2[i], idx[i] = best, bi
    return d2, idx


def _clouds(seed, na, nb, extent=3.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-extent, extent, (na, 3)).astype(np.float32), rng.uniform(-extent, extent, (nb, 3)).astype(np.float32)


@pytest.mark.parametrize("seed,na,nb,r", [(1, 60, 80, 0.5), (2, 131, 47, 1.0), (3, 40, 40, 0.2), (4, 1, 90, 2.0), (5, 90, 1, 2.0)])
def test_twin_equals_the_double_loop(seed, na, nb, r):
    a, b = _clouds(seed, na, nb)
    a[::17] = np.round(a[::17])                                 # some exact ties and repeated points
    b[:len(a[::17])][: min(len(b), len(a[::17]))] = a[::17][: min(len(b), len(a[::17]))]
    for block in (7, 256):
        rec = ov.overlap(a, b, r, block=block, points=True)
        for d, (x, y) in ((rec["a_to_b"], (a, b)), (rec["b_to_a"], (b, a))):
            d2, idx = _loop(x, y, r)
            assert np.array_equal(d["nn_d2"].view(np.uint32), d2.view(np.uint32)) and np.array_equal(d["nn_idx"], idx)
            inl = np.isfinite(d2)
            assert (d["n"], d["n_finite"], d["inliers"]) == (len(x), len(x), int(inl.sum())) and d["inliers"] > 0
            assert d["sum_d2"] == float(np.sum(d2[inl].astype(np.float64)))


def test_index_sets_equal_ckdtree_on_dyadic_coordinates():
    """coordinates k / 64 with |k| <= 512: differences, squares and their sums are exact in f32 and in f64, so both order the candidates alike; points are
    distinct and r * r is no attainable squared distance, so neither ties nor the bound's inclusiveness can differ"""
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    rng = np.random.default_rng(11)
    for r in (0.3, 1.1, 2.7):
        a = (rng.integers(-512, 513, (700, 3)) / 64.0).astype(np.float32)
        b = (rng.integers(-512, 513, (900, 3)) / 64.0).astype(np.float32)
        a[5] = [np.nan, 0, 0]; b[9] = [0, np.inf, 0]
        d2, idx = ov.nearest(a, b, r)
        fa = np.isfinite(a).all(1); fb = np.flatnonzero(np.isfinite(b).all(1))
        dist, j = cKDTree(b[fb].astype(np.float64)).query(a[fa].astype(np.float64), k=1, distance_upper_bound=r)
        want = np.full(len(a), -1, np.int64); ok = np.isfinite(dist)
        want[np.flatnonzero(fa)[ok]] = fb[j[ok]]
        # a tie in distance may resolve to either index in the tree: compare the distance there, the index elsewhere
        bd = np.where(want >= 0, np.sum((a.astype(np.float64) - b[np.maximum(want, 0)].astype(np.float64)) ** 2, 1), np.inf)
        assert np.array_equal(idx >= 0, want >= 0)
        assert np.array_equal(np.where(idx >= 0, d2.astype(np.float64), np.inf), bd)
        same = idx == want
        assert same.mean() > 0.98
        for i in np.flatnonzero(~same):                         # the twin's is the lowest index among the tied
            assert idx[i] < want[i] and np.sum((a[i].astype(np.float64) - b[idx[i]].astype(np.float64)) ** 2) == bd[i]
        k = ov.direction_kdtree(a, b, r)
        assert k["inliers"] == int((idx >= 0).sum()) and k["n_finite"] == len(a) - 1


def test_ties_resolve_to_the_lowest_index():
    a = np.array([[0, 0, 0]], np.float32)
    b = np.array([[2, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, -1, 0]], np.float32)
    d2, idx = ov.nearest(a, b, 1.5)
    assert idx[0] == 1 and d2[0] == 1.0
    d2, idx = ov.nearest(a, b[::-1].copy(), 1.5)
    assert idx[0] == 0


def test_the_radius_is_inclusive_to_the_f32_ulp():
    r = 0.3
    r2 = np.float32(r * r)
    x = np.float32(np.sqrt(np.float64(r2)))
    # find the f32 x whose rounded square is exactly r2, and the next whose square is above it
    while np.float32(x * x) > r2:
        x = np.nextafter(x, np.float32(0))
    while np.float32(np.nextafter(x, np.float32(1)) * np.nextafter(x, np.float32(1))) <= r2:
        x = np.nextafter(x, np.float32(1))
    assert np.float32(x * x) <= r2
    up = np.nextafter(x, np.float32(1))
    assert np.float32(up * up) > r2
    a = np.zeros((2, 3), np.float32)
    b = np.array([[x, 0, 0]], np.float32)
    assert ov.direction(a, b, r)["inliers"] == 2
    b[0, 0] = up
    assert ov.direction(a, b, r)["inliers"] == 0
    # a squared distance of exactly r2
    d = ov.direction(np.zeros((1, 3), np.float32), np.array([[3, 4, 0]], np.float32), 5.0, points=True)
    assert d["inliers"] == 1 and d["nn_d2"][0] == 25.0
    d = ov.direction(np.zeros((1, 3), np.float32), np.array([[3, 4, np.float32(2.0 ** -8)]], np.float32), 5.0)       # 25 + 2^-16 is above 25 in f32
    assert d["inliers"] == 0


def test_non_finite_points_follow_the_definition():
    a = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 0, 0]], np.float32)
    b = np.array([[np.nan, np.nan, np.nan], [0, 0, 0.25], [-np.inf, 0, 0]], np.float32)
    rec = ov.overlap(a, b, 2.0, points=True)
    ab, ba = rec["a_to_b"], rec["b_to_a"]
    assert (ab["n"], ab["n_finite"], ab["inliers"]) == (4, 2, 2) and list(ab["nn_idx"]) == [1, -1, -1, 1]
    assert np.isinf(ab["nn_d2"][[1, 2]]).all() and ab["nn_d2"][0] == np.float32(0.0625)
    assert (ba["n"], ba["n_finite"], ba["inliers"]) == (3, 1, 1) and list(ba["nn_idx"]) == [-1, 0, -1]
    none = ov.overlap(a, b[[0, 2]], 2.0)
    assert none["a_to_b"]["inliers"] == 0 and none["b_to_a"]["n_finite"] == 0 and ov.overlap_fraction(none["b_to_a"]) == 0.0
    empty = ov.overlap(np.zeros((0, 3), np.float32), a, 1.0)
    assert empty["a_to_b"] == dict(n=0, n_finite=0, inliers=0, sum_d2=0.0) and empty["b_to_a"]["inliers"] == 0


def test_a_cloud_against_itself():
    a, _ = _clouds(8, 500, 1)
    a[3] = np.nan
    rec = ov.overlap(a, a, 0.05)
    for d in rec.values():
        assert d["inliers"] == d["n_finite"] == 499 and d["sum_d2"] == 0.0
        assert ov.overlap_fraction(d) == 1.0 and ov.inlier_rmse(d) == 0.0


def test_helpers_and_bad_radii():
    d = dict(n=10, n_finite=8, inliers=4, sum_d2=1.0)
    assert ov.overlap_fraction(d) == 0.5 and ov.inlier_rmse(d) == 0.5
    assert ov.inlier_rmse(dict(n=3, n_finite=3, inliers=0, sum_d2=0.0)) == 0.0
    assert ov.radius2(0.3) == np.float32(0.3 * 0.3)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ov.nearest(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), r)
    assert math.isclose(ov.inlier_rmse(dict(n=1, n_finite=1, inliers=2, sum_d2=8.0)), 2.0)
