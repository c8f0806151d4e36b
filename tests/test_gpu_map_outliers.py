"""The map's outlier filter on the GPU (qn_kf_map_outliers / qn_kf_map_outlier_points / qn_kf_map_remove_outliers) against its specification, the numpy twin
qn_amd/mapoutliers.py, run on the map the store itself downloads.  Everything is an integer or follows from integers by the same f64 operations, so everything
is compared bit for bit: count, mean_q and the removed byte of every point, every field of the statistics, the filtered map, and a rerun.  The selection
kernel's block is 256 points (the sizes 1, k, k + 1, 255, 256, 257 and 513 are its launch seams) and its sorted list has 8, 16 or 32 registers (k = 1, 8, 9, 16,
17 and 32 are the seams of the three instantiations).  Hand-made points reach the map slot unchanged through the voxel grid's overflow guard: at leaf 1e-4 a
cloud that spans half a metre on every axis passes through as it is, duplicates and non-finite records included."""
import ctypes as C
import math
import subprocess
import numpy as np
import pytest
from qn_amd import mapoutliers as mo, mapnormals as mn, synth

pytestmark = pytest.mark.gpu
B = 256                                                              # MO_BLOCK of csrc/qn_mapoutliers.hip
F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
STAT_FIELDS = ("n", "n_finite", "dense", "sparse", "removed", "quant_exp", "sum_q", "sum_q2", "mean_q", "std_q", "thr_q")


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


@pytest.fixture(scope="module")
def scans(store):
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    return [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_the_twin(store, params, what):
    """map_outliers of the store's map against the twin on the downloaded map -> (the GPU result as the twin's dict, the twin's stats, the map)"""
    from qn_amd import engine
    pts = store.download_map(store._map_n)
    stats, cnt, mq, rm = store.map_outliers(engine.OutlierParams(*params))
    want = mo.classify(pts, params)
    w = want["stats"]
    print("%s: %d points, %d finite, %d dense, %d sparse, %d removed; mean %.6g std %.6g thr %.6g (2^-%d m)"
          % (what, stats["n"], stats["n_finite"], stats["dense"], stats["sparse"], stats["removed"], stats["mean_q"], stats["std_q"], stats["thr_q"], stats["quant_exp"]))
    assert len(cnt) == len(pts) and cnt.dtype == np.uint32 and mq.dtype == np.uint32 and rm.dtype == np.uint8
    assert np.array_equal(cnt, want["count"]), (what, int((cnt != want["count"]).sum()))
    assert np.array_equal(mq, want["mean_q"]), (what, int((mq != want["mean_q"]).sum()))
    assert np.array_equal(rm, want["removed"]), (what, int((rm != want["removed"]).sum()))
    for f in STAT_FIELDS:
        assert stats[f] == getattr(w, f), (what, f, stats[f], getattr(w, f))
    unit = math.ldexp(1.0, -w.quant_exp)
    assert (stats["mean"], stats["std"], stats["threshold"]) == (w.mean_q * unit, w.std_q * unit, w.thr_q * unit)
    # a rerun returns the same bytes
    again = store.map_outliers(engine.OutlierParams(*params))
    assert again[0] == stats and _same(again[1], cnt) and _same(again[2], mq) and _same(again[3], rm), what
    return dict(count=cnt, mean_q=mq, removed=rm, stats=stats), w, pts


def _map_of(store, clouds, poses, leaf):
    ids = [store.add(c) for c in clouds]
    return store.build_map(ids, poses, leaf)


def _as_it_is(store, pts):
    """the records themselves as the map (leaf 1e-4: the overflow guard passes them through)"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = _map_of(store, [pts], [np.eye(4)], 1e-4)
    got = store.download_map(n)
    assert n == len(pts) and _same(got[:, :3], pts[:, :3]), "the cloud did not pass through"
    return pts


def _cloud(rng, n, extent=(6.0, 6.0, 1.5)):
    """points of uneven density: a uniform box and three clumps in it"""
    a = rng.uniform(0.0, 1.0, (n, 3)) * extent
    for c in range(3):
        idx = rng.choice(n, n // 6, replace=False)
        a[idx] = rng.uniform(0.2, 0.8, 3) * extent + rng.normal(0.0, 0.15, (len(idx), 3))
    return a.astype(np.float32)


def test_ray_cast_map_with_injected_noise(store, scans):
    """four ray-cast keyframes at leaf 0.3 and a fifth keyframe of 50 stray points, each at least 2 r from every other map point: count 0 by construction, so
    every one of them must go"""
    r = 1.0
    g = np.stack(np.meshgrid(np.arange(10), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 2)
    noise = np.zeros((50, 3), np.float32)
    noise[:, :2] = g * 3.0 - [12.0, 6.0]; noise[:, 2] = 60.0 + 2.5 * (g[:, 0] % 2)             # a 3 m grid far above the scene
    nid = store.add(noise)
    n = store.build_map(scans + [nid], POSES + [np.eye(4)], 0.3)
    assert 3000 <= n <= 40000, n
    got, w, pts = equal_the_twin(store, (r, 2.0, 8), "ray-cast map with 50 stray points")
    stray = np.flatnonzero(pts[:, 2] > 50.0)
    assert len(stray) == 50
    d = np.sqrt(((pts[stray, None, :3].astype(np.float64) - pts[None, :, :3].astype(np.float64)) ** 2).sum(axis=2))
    d[np.arange(50), stray] = np.inf
    assert d.min() >= 2.0 * r
    assert (got["count"][stray] == 0).all() and (got["removed"][stray] == 1).all() and (got["mean_q"][stray] == mo.NO_MEAN).all()
    assert w.dense > 0 and 50 <= w.removed < n and w.std_q > 0
    equal_the_twin(store, (0.6, 1.0, 5), "ray-cast map, r = 0.6, k = 5")


@pytest.mark.parametrize("n", [1, 8, 9, B - 1, B, B + 1, 2 * B + 1])
def test_launch_seams(store, n):
    k = 8                                                            # the sizes 8 and 9 are k and k + 1
    rng = np.random.default_rng(100 + n)
    side = int(math.ceil(math.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    pts = np.zeros((n, 3), np.float32)
    pts[:, :2] = ij * 0.3 + rng.uniform(-0.05, 0.05, (n, 2)); pts[:, 2] = 0.02 * np.sin(ij[:, 0]) + rng.uniform(-0.01, 0.01, n)
    assert _map_of(store, [pts], [np.eye(4)], 0.1) == n              # at least 0.2 apart on an axis: every point is a voxel of its own
    got, w, _ = equal_the_twin(store, (1.0, 2.0, k), "map of %d points" % n)
    if n <= 9:                                                       # a 3 x 3 patch of spacing 0.3 +- 0.1 lies within 1 m of each of its points
        assert (got["count"] == n - 1).all() and w.dense == (n if n == 9 else 0) and w.sparse == n - w.dense
    else:
        assert w.dense == n


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32])
def test_list_seams(store, k):
    pts = _as_it_is(store, _cloud(np.random.default_rng(40 + k), 1500))
    got, w, _ = equal_the_twin(store, (0.5, 1.5, k), "k = %d" % k)
    assert w.dense > 100 and (w.sparse > 100 or k == 1), (w.dense, w.sparse)       # the counts straddle k
    assert int(got["count"].max()) > 32


def test_neighbours_across_cell_borders_on_every_axis(store):
    """radius 0.25 in a box of 3 x 3 x 2 m: cells of about the radius, more than ten a side on every axis, so most neighbourhoods reach into other cells in x, in
    y and in z; and radius 0.25 over integer multiples of 2^-3, where half of all partners sit exactly one cell edge away"""
    _as_it_is(store, _cloud(np.random.default_rng(3), 4000, (3.0, 3.0, 2.0)))
    _, w, _ = equal_the_twin(store, (0.25, 2.0, 6), "across cell borders")
    assert w.dense > 1000
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) * F(0.125)
    _as_it_is(store, g)
    got, w, pts = equal_the_twin(store, (0.25, 2.0, 6), "a cubic lattice of spacing 2^-3, r = 2^-2")
    inner = ((pts[:, :3] >= 0.25) & (pts[:, :3] <= [1.125, 1.125, 0.375])).all(axis=1)
    # by hand: offsets (a, b, c) h with a^2 + b^2 + c^2 <= 4 without the origin: 6 + 12 + 8 + 6 = 32, the six at 2 h exactly ON the radius
    assert inner.sum() == 8 * 8 * 2 and (got["count"][inner] == 32).all()
    assert (got["mean_q"][inner] == 2 ** 15).all()                     # k = 6: the six axis partners at h = 2^-3, e = 18


def test_a_neighbour_on_the_radius_and_one_just_beyond(store):
    """r = 0.5, r2 = 0.25: a partner at 0.5 has d2 == r2 and counts; one at 0.5 + 2^-24 (the next f32) has d2 = 0.25 + 2^-24 > r2 and does not"""
    up = np.nextafter(F(0.5), F(1))
    assert F(0.5) * F(0.5) == F(0.5 * 0.5) and up * up > F(0.25)
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [-up, 0, 0], [0, 0.5, 0], [0, -up, 0], [0, 0, -0.5], [0, 0, up], [0.25, 0, 0]], np.float32)
    _as_it_is(store, pts)
    got, _, _ = equal_the_twin(store, (0.5, 2.0, 2), "on the radius / just beyond")
    assert got["count"][0] == 4                                      # the three at exactly 0.5 and the one at 0.25
    assert got["mean_q"][0] == int(np.rint((0.25 + 0.5) / 2 * 2 ** 17))
    # the lattices of tests/test_gpu_map_normals.py: h = float32(0.3), 4 fl(h h) == float32(0.6 * 0.6), partners two steps away exactly ON the radius
    h = F(0.3)
    k = np.arange(-4, 5).astype(np.float32) * h
    x, y = np.meshgrid(k, k, indexing="ij")
    lat = np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, F(l) * h, np.float32)], axis=1) for l in (-8, -4, 0, 4, 8)]).astype(np.float32)
    assert F(4) * (h * h) == F(0.6 * 0.6)
    _as_it_is(store, lat)
    got, _, pts = equal_the_twin(store, (0.6, 2.0, 12), "lattice with partners on the radius")
    inner = (np.abs(pts[:, 0]) <= 0.61) & (np.abs(pts[:, 1]) <= 0.61)
    assert (got["count"][inner] == 12).all() and got["count"].max() == 12        # 13 offsets with a^2 + b^2 <= 4, the point itself not counted


def test_a_map_inside_one_cell(store):
    rng = np.random.default_rng(9)
    pts = (rng.uniform(0.0, 0.5, (60, 3)) + [100.0, -50.0, 2.0]).astype(np.float32)
    pts[:8] = [[100, -50, 2], [100.5, -50, 2], [100, -49.5, 2], [100, -50, 2.5], [100.5, -49.5, 2.5], [100.25, -50, 2], [100, -49.75, 2.25], [100.5, -50, 2.5]]
    _as_it_is(store, pts)
    got, w, _ = equal_the_twin(store, (1.0, 2.0, 8), "a map inside one cell")
    assert (got["count"] == 59).all() and w.dense == 60              # the box's diagonal is 0.87 m


def test_duplicates_of_the_query_and_ties_at_the_kth_distance(store):
    """six partners at exactly 0.5 on the axes and one at 0.25, then the origin twice more: with k = 3 the third smallest is one of six equal values for the
    first cloud, and for the second the query's duplicates are neighbours at distance 0"""
    pts = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32)
    _as_it_is(store, pts)
    got, _, _ = equal_the_twin(store, (0.6, 2.0, 3), "six tied at the third distance")
    assert got["count"][0] == 7 and got["mean_q"][0] == int(np.rint((0.25 + 0.5 + 0.5) / 3 * 2 ** 16))
    _as_it_is(store, np.concatenate([pts, pts[:1], pts[:1], pts[2:3]]))
    got, _, _ = equal_the_twin(store, (0.6, 2.0, 3), "duplicates of the query")
    assert got["count"][0] == 10 and got["mean_q"][0] == int(np.rint(0.25 / 3 * 2 ** 16))
    assert got["count"][8] == 10 and got["mean_q"][8] == got["mean_q"][0] and got["count"][2] == got["count"][10]


def test_passed_through_map_with_non_finite_records(store):
    rng = np.random.default_rng(5)
    a = np.zeros((1500, 3), np.float32); a[:, :2] = rng.uniform(-5, 5, (1500, 2)); a[:, 2] = 0.1 * np.sin(a[:, 0]) + rng.normal(0, 0.01, 1500)
    b = (rng.normal(0, 12, (1200, 3)) * 200.0).astype(np.float32)
    a[[5, 77, 901]] = [[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf]]
    b[10] = [np.nan, 1, 1]
    n = _map_of(store, [a, b], [np.eye(4), np.eye(4)], 1e-3)
    assert n == 2700 and "overflow" in store._l.qn_kf_last_error(store.h).decode()
    got, w, pts = equal_the_twin(store, (0.6, 2.0, 5), "passed-through map")
    bad = ~np.isfinite(pts[:, :3]).all(axis=1)
    assert bad.sum() == 4 and w.n_finite == 2696
    assert (got["count"][bad] == 0).all() and (got["mean_q"][bad] == mo.NO_MEAN).all() and (got["removed"][bad] == 0).all()      # never removed
    assert w.dense > 1000 and got["removed"][1500:][~bad[1500:]].all()                                                      # the wide-spread cloud is all strays
    ptr, m = store.map_remove_outliers()
    kept = store.download_map(m)
    assert m == n - w.removed and _same(kept, pts[got["removed"] == 0]) and (~np.isfinite(kept[:, :3]).all(axis=1)).sum() == 4


def test_std_mul_zero_and_large_and_all_equal_means(store):
    _as_it_is(store, _cloud(np.random.default_rng(21), 2000))
    at0, w0, _ = equal_the_twin(store, (0.5, 0.0, 8), "std_mul = 0")
    big, w1, _ = equal_the_twin(store, (0.5, 1e6, 8), "std_mul = 1e6")
    assert w0.thr_q == w0.mean_q and w0.removed > w0.sparse + w0.dense // 4          # everything above the mean goes
    assert w1.removed == w1.sparse == w0.sparse and _same(at0["mean_q"], big["mean_q"])
    # two planar lattices of spacing 2^-2, 3 m apart, r = 0.3, k = 4: every interior point has its four partners at exactly h, so every mean_q is h 2^17, the
    # variance is 0 and the threshold removes nothing - whatever std_mul is; the border goes by the radius rule
    k = np.arange(9).astype(np.float32) * F(0.25)
    x, y = np.meshgrid(k, k, indexing="ij")
    lat = np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, z, np.float32)], axis=1) for z in (0.0, 3.0)]).astype(np.float32)
    _as_it_is(store, lat)
    for std_mul in (0.0, 2.0):
        got, w, pts = equal_the_twin(store, (0.3, std_mul, 4), "all mean_q equal, std_mul = %g" % std_mul)
        inner = ((pts[:, :2] > 0.1) & (pts[:, :2] < 1.9)).all(axis=1)
        assert (got["mean_q"][inner] == 2 ** 15).all() and (w.dense, w.sparse, w.std_q, w.thr_q, w.removed) == (98, 64, 0.0, 32768.0, 64)
        assert np.array_equal(got["removed"], (~inner).astype(np.uint8))


def test_remove_serves_the_filtered_map_and_ends_what_was_computed_from_the_old_one(store, scans):
    from qn_amd import engine
    n = store.build_map(scans, POSES, 0.3)
    views = np.array([[p[0, 3], p[1, 3], p[2, 3]] for p in POSES])
    store.map_normals(engine.NormalParams(0.6, 5), views)
    got, w, pts = equal_the_twin(store, (1.0, 2.0, 8), "before the remove")
    assert 0 < w.removed < n
    nrm = np.zeros((n, 4), np.float32)
    assert store._l.qn_kf_download_map_normals(store.h, nrm.ctypes.data_as(C.c_void_p), None, None) == engine.QN_OK       # the classify did not touch the slot
    ptr, m = store.map_remove_outliers()
    want = mo.remove(pts, (1.0, 2.0, 8))
    assert m == n - w.removed == len(want) and ptr
    assert _same(store.download_map(m), want)                        # byte for byte, all 16 bytes of each kept record, in order
    # the slot's generation moved: what was computed from the old map is refused
    cnt = np.zeros(n, np.uint32)
    assert store._l.qn_kf_download_map_normals(store.h, nrm.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert store._l.qn_kf_map_outlier_points(store.h, cnt.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    p2 = C.c_void_p(); m2 = C.c_uint32()
    assert store._l.qn_kf_map_remove_outliers(store.h, C.byref(p2), C.byref(m2)) == engine.QN_ERR_NOT_READY
    assert _same(store.download_map(m), want)                        # the refused remove left the slot as it was
    # map_normals runs on the filtered map and equals the twin's there
    r = store.map_normals(engine.NormalParams(0.6, 5), views)
    s1, s2 = store.map_moments()
    t = mn.normals(want, (0.6, 5), views)
    assert len(r["count"]) == m and np.array_equal(r["count"], t["count"]) and np.array_equal(s1, t["s1"]) and np.array_equal(s2, t["s2"])
    assert np.array_equal(np.isnan(r["curvature"]), np.isnan(t["curvature"])) and np.array_equal(r["view_idx"], t["view_idx"])
    # until the next classify, which sees the filtered map
    again, w2, _ = equal_the_twin(store, (1.0, 2.0, 8), "after the remove")
    assert w2.n == m


def test_lifecycle_and_refusals(store, scans):
    from qn_amd import engine
    n = store.build_map(scans[:2], POSES[:2], 0.3)
    keep, _, _ = equal_the_twin(store, (1.0, 2.0, 8), "two keyframes")
    L = store._l
    st = engine.OutlierStats(); st.n = 12345
    bad = []
    for radius, std_mul, k in [(0.0, 2.0, 8), (-1.0, 2.0, 8), (float("nan"), 2.0, 8), (float("inf"), 2.0, 8), (1.0, -0.5, 8), (1.0, float("nan"), 8),
                               (1.0, float("inf"), 8), (1.0, 2.0, 0), (1.0, 2.0, 33), (1.0, 2.0, 0xffffffff)]:
        bad.append(engine.OutlierParams(radius, std_mul, k))
    p = engine.OutlierParams(); p.reserved = 1
    bad.append(p)
    for p in bad:
        assert L.qn_kf_map_outliers(store.h, C.byref(p), C.byref(st)) == engine.QN_ERR_INVALID_ARG, (p.radius, p.std_mul, p.k, p.reserved)
    assert L.qn_kf_map_outliers(store.h, None, C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_outliers(store.h, C.byref(engine.OutlierParams()), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_outlier_points(store.h, None, None, None) == engine.QN_ERR_INVALID_ARG
    ptr = C.c_void_p(); m = C.c_uint32()
    assert L.qn_kf_map_remove_outliers(store.h, None, C.byref(m)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_remove_outliers(store.h, C.byref(ptr), None) == engine.QN_ERR_INVALID_ARG
    assert st.n == 12345                                             # nothing was written
    # every refusal left the previous classification readable and unchanged; each output alone is served
    cnt = np.zeros(n, np.uint32); mq = np.zeros(n, np.uint32); rm = np.zeros(n, np.uint8)
    assert L.qn_kf_map_outlier_points(store.h, cnt.ctypes.data_as(C.c_void_p), None, None) == engine.QN_OK
    assert L.qn_kf_map_outlier_points(store.h, None, mq.ctypes.data_as(C.c_void_p), None) == engine.QN_OK
    assert L.qn_kf_map_outlier_points(store.h, None, None, rm.ctypes.data_as(C.c_void_p)) == engine.QN_OK
    assert _same(cnt, keep["count"]) and _same(mq, keep["mean_q"]) and _same(rm, keep["removed"])
    assert _same(store.download_map(n), store.download_map(n))
    # a rebuild replaces the slot: the classification is refused until the next classify, and so is the remove
    n2 = store.build_map(scans[:3], POSES[:3], 0.3)
    assert L.qn_kf_map_outlier_points(store.h, cnt.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_remove_outliers(store.h, C.byref(ptr), C.byref(m)) == engine.QN_ERR_NOT_READY
    assert store._map_n == n2 and len(store.download_map(n2)) == n2
    equal_the_twin(store, (1.0, 2.0, 8), "the map built afterwards")


def test_not_ready_without_a_map():
    from qn_amd import engine
    s = engine.KeyframeStore()
    try:
        st = engine.OutlierStats(); ptr = C.c_void_p(); m = C.c_uint32(); out = np.zeros(4, np.uint32)
        assert s._l.qn_kf_map_outliers(s.h, C.byref(engine.OutlierParams()), C.byref(st)) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_outlier_points(s.h, out.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_remove_outliers(s.h, C.byref(ptr), C.byref(m)) == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_outliers()
        assert ei.value.status == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_remove_outliers()
        assert ei.value.status == engine.QN_ERR_NOT_READY
    finally:
        s.close()


def _fnv(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def test_cpp_helper_gives_the_python_result(store, scans, tmp_path):
    from shim_build import build_shim
    from qn_amd import engine
    exe = build_shim("shim_map_outliers.cpp", tmp_path)
    ids, poses = scans[:2], POSES[:2]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    np.ascontiguousarray(np.array(poses, np.float64)).tofile(str(tmp_path / "poses.bin"))
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "1.0", "2.0", "8"], text=True)
    n = store.build_map(ids, poses, 0.3)
    stats, cnt, mq, rm = store.map_outliers(engine.OutlierParams(1.0, 2.0, 8))
    ho = _fnv(cnt[i].tobytes() + mq[i].tobytes() + rm[i].tobytes() for i in range(n))
    _, m = store.map_remove_outliers()
    kept = store.download_map(m)
    hm = _fnv(kept[i].tobytes() for i in range(m))
    assert txt.splitlines() == ["outliers %d %d %d %016x" % (n, stats["dense"], stats["removed"], ho), "filtered %d %016x" % (m, hm)], txt
