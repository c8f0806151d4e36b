"""The map's ground segmentation and occupancy grid on the GPU (qn_kf_map_ground / qn_kf_map_ground_points / qn_kf_map_ground_grid / qn_kf_map_keep_classes)
against their specification, the numpy twin qn_amd/mapground.py, run on the map the store itself downloads.  Everything after the quantisation is an integer
and the envelope is unique, so everything is compared bit for bit: the class and height_q of every point, ground_q and the occupancy of every column, the grid
info, every field of the statistics but `rounds`, and a rerun.  B is the point kernels' block and T the envelope's tile edge (MG_BLOCK, MG_TILE of
csrc/qn_mapground.hip): the point counts 1, B - 1, B, B + 1, 2 B + 1 and the grids 1 x 1 .. (2 T + 1)^2 are their launch and tile seams.  Hand-made points reach
the map slot unchanged through the voxel grid's overflow guard at leaf 1e-4."""
import ctypes as C
import math
import os
import re
import numpy as np
import pytest
from qn_amd import mapground as mg, mapoutliers as mo, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_mapground.hip")).read()
B = int(re.search(r"#define\s+MG_BLOCK\s+(\d+)", _SRC).group(1))
T = int(re.search(r"#define\s+MG_TILE\s+(\d+)", _SRC).group(1))
F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
DEFAULT = tuple(mg.GroundParams())


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
    """map_ground and map_ground_grid of the store's map against the twin on the downloaded map -> (the GPU results as the twin's dict, the map)"""
    from qn_amd import engine
    pts = store.download_map(store._map_n)
    stats, cls, hq = store.map_ground(engine.GroundParams(*params))
    info, gq, occ = store.map_ground_grid()
    want = mg.classify(pts, params)
    w = want["stats"]
    print("%s: %d points (%d finite), grid %d x %d, %d seeded, classes %s, occupied %d free %d unknown %d, rounds %d"
          % (what, stats["n"], stats["n_finite"], stats["width"], stats["height"], stats["seeded"],
             [stats[f] for f in ("n_none", "n_ground", "n_obstacle", "n_overhead", "n_below")], stats["occupied"], stats["free"], stats["unknown"], stats["rounds"]))
    assert len(cls) == len(pts) and cls.dtype == np.uint8 and hq.dtype == np.int32 and gq.dtype == np.int32 and occ.dtype == np.uint8
    for f in mg.GroundStats._fields:                                 # every field but rounds
        assert stats[f] == getattr(w, f), (what, f, stats[f], getattr(w, f))
    assert tuple(info[f] for f in mg.GridInfo._fields) == tuple(want["info"]), (what, info, want["info"])
    assert gq.shape == want["ground_q"].shape and np.array_equal(gq, want["ground_q"]), (what, int((gq != want["ground_q"]).sum()))
    assert np.array_equal(occ, want["occupancy"]), (what, int((occ != want["occupancy"]).sum()))
    assert np.array_equal(cls, want["classes"]), (what, int((cls != want["classes"]).sum()))
    assert np.array_equal(hq, want["height_q"]), (what, int((hq != want["height_q"]).sum()))
    assert 1 <= stats["rounds"] <= max(w.width, w.height) + 2 or w.width * w.height == 0
    # a rerun returns the same bytes
    again = store.map_ground(engine.GroundParams(*params)); grid2 = store.map_ground_grid()
    assert {k: v for k, v in again[0].items() if k != "rounds"} == {k: v for k, v in stats.items() if k != "rounds"}
    assert _same(again[1], cls) and _same(again[2], hq) and grid2[0] == info and _same(grid2[1], gq) and _same(grid2[2], occ), what
    return dict(classes=cls, height_q=hq, ground_q=gq, occupancy=occ, info=info, stats=stats), pts


def _slot(store, pts, leaf=1e-4, exact=True):
    """the records as the map (leaf 1e-4: the overflow guard passes a cloud that spans enough through as it is, duplicates and non-finite records included)"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = store.build_map([store.add(pts)], [np.eye(4)], leaf)
    if exact:
        got = store.download_map(n)
        fin = np.isfinite(pts[:, :3]).all(axis=1)                    # (the identity pose turns a record with one NaN into three)
        assert n == len(pts) and _same(got[fin, :3], pts[fin, :3]) and not np.isfinite(got[~fin, :3]).all(axis=1).any(), "the cloud did not pass through"
    return n


def _columns(rng, W, H, cell, z, jitter=0.4):
    """one point in every column of a W x H grid of edge `cell` whose corner is the origin: (H, W) heights z, x and y jittered inside the column"""
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    p = np.zeros((W * H, 3), np.float32)
    p[:, 0] = (ix.ravel() + 0.5 + rng.uniform(-jitter, jitter, W * H)) * cell
    p[:, 1] = (iy.ravel() + 0.5 + rng.uniform(-jitter, jitter, W * H)) * cell
    p[:, 2] = np.asarray(z, np.float64).reshape(-1)
    return p


@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 2 * B + 1])
def test_point_count_seams(store, n):
    rng = np.random.default_rng(100 + n)
    side = int(math.ceil(math.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    pts = np.zeros((n, 3), np.float32)
    pts[:, :2] = ij * 0.3 + rng.uniform(-0.05, 0.05, (n, 2)); pts[:, 2] = rng.choice([0.0, 0.1, 0.9, 3.5], n) + rng.uniform(-0.01, 0.01, n)
    assert _slot(store, pts, 0.1, exact=False) == n                  # at least 0.2 apart on an axis: every point is a voxel of its own
    got, _ = equal_the_twin(store, DEFAULT, "map of %d points" % n)
    assert got["stats"]["n_finite"] == n and got["stats"]["n_ground"] >= 1
    if n > 1:
        assert got["stats"]["n_obstacle"] >= 1 and got["stats"]["n_overhead"] >= 1


@pytest.mark.parametrize("W,H", [(1, 1), (1, T + 1), (T + 1, 1), (T, T), (T + 1, T + 1), (2 * T + 1, 2 * T + 1)])
def test_grid_seams(store, W, H):
    """a rough surface of one point a column (heights over 0 .. 3 m, slope limit 0.3 at cell 1: the envelope binds in most columns), and for the 1 x 1 grid three
    points in the one column"""
    rng = np.random.default_rng(W * 1000 + H)
    if W * H == 1:
        pts = np.array([[0.1, 0.1, 0.0], [0.9, 0.5, 0.5], [0.5, 0.9, 3.0]], np.float32)
    else:
        pts = _columns(rng, W, H, 1.0, rng.uniform(0.0, 3.0, (H, W)))
    _slot(store, pts)
    params = (1.0, 0.3, 0.2, 2.0, 1)
    got, _ = equal_the_twin(store, params, "grid %d x %d" % (W, H))
    assert (got["info"]["width"], got["info"]["height"]) == (W, H) and got["stats"]["seeded"] == W * H and got["stats"]["unknown"] == 0
    if W * H == 1:
        assert got["classes"].tolist() == [mg.GROUND, mg.OBSTACLE, mg.OVERHEAD] and got["occupancy"].tolist() == [[2]]
    else:
        assert got["stats"]["n_obstacle"] > 0 and got["stats"]["n_ground"] > 0


@pytest.mark.parametrize("corner", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_one_low_seed_in_a_corner_crosses_every_tile_seam(store, corner):
    """a (3 T + 1)^2 grid seeded at 50 m but for one column at 0 m in a corner: at slope 0.3 and cell 1 the far corner's envelope is step_d * 3 T = 41 m, so the
    low seed binds in every column and its value crosses every tile seam.  A launch reads one grid buffer and writes the other, so a value moves at most one tile
    a round: the far tile is reached in round 4 and rounds >= 5 is certain - the test asserts the issue's rounds >= 2 and prints the figure."""
    S = 3 * T + 1
    z = np.full((S, S), 50.0)
    y0, x0 = corner[1] * (S - 1), corner[0] * (S - 1)
    z[y0, x0] = 0.0
    _slot(store, _columns(np.random.default_rng(5), S, S, 1.0, z))
    got, _ = equal_the_twin(store, (1.0, 0.3, 0.2, 2.0, 1), "low seed in corner %s" % (corner,))
    e, step_s, step_d = got["stats"]["quant_exp"], got["stats"]["step_s"], got["stats"]["step_d"]
    assert (e, step_s, step_d) == (10, 307, 434)
    g = got["ground_q"]
    assert g[y0, x0] == 0 and g[S - 1 - y0, S - 1 - x0] == step_d * (S - 1) and g[y0, S - 1 - x0] == step_s * (S - 1) and g[S - 1 - y0, x0] == step_s * (S - 1)
    assert (g < 50 * 2 ** e).all() and got["stats"]["n_ground"] == 1 and got["stats"]["n_overhead"] == S * S - 1 - got["stats"]["n_obstacle"]
    print("rounds", got["stats"]["rounds"])
    assert got["stats"]["rounds"] >= 2


def test_no_seeded_column_and_step_one(store):
    rng = np.random.default_rng(8)
    W, H = T + 3, 5
    _slot(store, _columns(rng, W, H, 1.0, rng.uniform(0.0, 2.0, (H, W))))
    got, _ = equal_the_twin(store, (1.0, 0.3, 0.2, 2.0, 2), "min_points = 2, singleton columns")
    assert got["stats"]["seeded"] == 0 and got["stats"]["n_none"] == W * H and (got["ground_q"] == mg.INF).all() and (got["height_q"] == mg.NO_HEIGHT).all()
    assert (got["occupancy"] == 1).all()
    got, _ = equal_the_twin(store, (1.0, 1e-9, 0.0, 2.0, 1), "step_s = 1, ground_tol = 0")
    assert (got["stats"]["step_s"], got["stats"]["step_d"], got["stats"]["tol_q"]) == (1, 1, 0)


def test_non_finite_records_duplicates_and_below(store):
    """NaN / inf records interleaved, every finite record twice over in a third of the columns, min_points = 2: the doubled columns seed, and the single points
    below their envelope are BELOW"""
    rng = np.random.default_rng(9)
    W, H = 2 * T + 5, 7
    base = _columns(rng, W, H, 0.5, rng.uniform(0.0, 0.2, (H, W)))
    low = base[::3].copy()
    base[1::3, 2] -= 3.0                                             # singles far below the doubled columns' ground
    pts = np.concatenate([base, low])
    pts = pts[rng.permutation(len(pts))]
    pts[::17] = [np.nan, 0.0, 0.0]; pts[5] = [1.0, np.inf, 0.0]; pts[40] = [1.0, 1.0, -np.inf]
    _slot(store, pts)
    got, m = equal_the_twin(store, (0.5, 0.3, 0.2, 2.0, 2), "non-finite records, duplicates, min_points = 2")
    bad = ~np.isfinite(m[:, :3]).all(axis=1)
    assert bad.sum() >= 3 and (got["classes"][bad] == mg.NONE).all() and got["stats"]["n_below"] > 20 and got["stats"]["n_ground"] > 20
    assert 0 < got["stats"]["seeded"] < W * H


def test_cell_borders_and_negative_coordinates(store):
    k = np.arange(-9, 10).astype(np.float32) * F(0.5)
    x, y = np.meshgrid(k, k, indexing="ij")
    z = (0.05 * ((np.arange(x.size) * 7) % 11)).astype(np.float32)
    pts = np.stack([x.ravel(), y.ravel(), z], axis=1).astype(np.float32)
    pts = np.concatenate([pts, pts + F(1e-6), [[-4.5, -4.5, 4.0]]]).astype(np.float32)
    _slot(store, pts)
    got, _ = equal_the_twin(store, DEFAULT, "points on cell borders")
    assert (got["info"]["origin_x"], got["info"]["origin_y"], got["info"]["width"], got["info"]["height"]) == (-4.5, -4.5, 19, 19)
    assert got["occupancy"][0, 0] == 1 and got["classes"][-1] == mg.OVERHEAD


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 0b11101])
def test_keep_classes(store, mask):
    from qn_amd import engine
    rng = np.random.default_rng(12)
    W, H = T + 2, 9
    z = rng.choice([0.0, 0.05, 1.0, 4.0], (H, W), p=[0.5, 0.2, 0.2, 0.1])
    a = _columns(rng, W, H, 0.5, z)
    b = a[::4].copy(); b[:, 2] = 0.0                                 # a second point in a quarter of the columns
    a[2::4, 2] = np.where(rng.random(len(a[2::4])) < 0.5, -2.0, a[2::4, 2])      # singles below the ground: BELOW under min_points = 2
    pts = np.concatenate([a, b]); pts[3] = [np.nan, 1.0, 1.0]
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], axis=1)      # an intensity to carry along
    n = store.build_map([store.add(pts[:, :3], pts[:, 3])], [np.eye(4)], 1e-4)
    params = (0.5, 0.3, 0.2, 2.0, 2)
    views = np.zeros((1, 3))
    store.map_normals(engine.NormalParams(0.6, 3), views)
    store.map_outliers(engine.OutlierParams(1.0, 2.0, 4))
    got, m = equal_the_twin(store, params, "before keep_classes(%#x)" % mask)
    counts = [got["stats"][f] for f in ("n_none", "n_ground", "n_obstacle", "n_overhead", "n_below")]
    assert all(c > 0 for c in counts), counts
    want = mg.keep(m, got["classes"], mask)
    ptr, k = store.map_keep_classes(mask)
    assert k == len(want) == sum(c for i, c in enumerate(counts) if mask >> i & 1) and ptr
    assert _same(store.download_map(k), want)                        # byte for byte, all 16 bytes of each kept record, in order
    L = store._l
    out = np.zeros(n, np.uint32); nrm = np.zeros((n, 4), np.float32); p2 = C.c_void_p(); k2 = C.c_uint32()
    assert L.qn_kf_map_ground_points(store.h, out.ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_ground_grid(store.h, C.byref(engine.GroundGrid()), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_keep_classes(store.h, 1, C.byref(p2), C.byref(k2)) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_download_map_normals(store.h, nrm.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_outlier_points(store.h, out.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert _same(store.download_map(k), want)                        # the refused keep left the slot as it was
    if mask != 1:                                                    # (mask 1 keeps the non-finite record alone)
        st = store.map_outliers(engine.OutlierParams(1.0, 2.0, 4))   # the outlier filter serves the kept map
        assert st[0]["n"] == k and np.array_equal(st[1], mo.classify(want, (1.0, 2.0, 4))["count"])
    equal_the_twin(store, params, "after keep_classes(%#x)" % mask)


def test_a_mask_that_keeps_nothing_leaves_the_store_without_a_map(store):
    from qn_amd import engine
    assert _slot(store, _columns(np.random.default_rng(2), 6, 6, 0.5, np.zeros((6, 6))), exact=False) == 36      # (flat: no overflow, one voxel a point)
    got, _ = equal_the_twin(store, DEFAULT, "a flat floor")
    assert got["stats"]["n_ground"] == 36
    ptr, k = store.map_keep_classes(0b11100)
    assert k == 0 and not ptr
    st = engine.GroundStats()
    assert store._l.qn_kf_map_ground(store.h, C.byref(engine.GroundParams()), C.byref(st)) == engine.QN_ERR_NOT_READY


def test_refusals_leave_the_earlier_results_intact(store):
    from qn_amd import engine
    L = store._l
    # two points 10 km apart, one of them 4 10^6 m up: fine at cell 4000 (e = -2: 3 x 3 columns, zq = 10^6); too many columns at cell 0.5 and 1; at cell 1.25
    # (e = 9) the 8001^2 columns fit and only the height, 2^9 * 4 10^6 >= 2^30, refuses
    n = store.build_map([store.add(np.array([[0, 0, 0], [10000, 10000, 4e6], [5000, 100, 3]], np.float32))], [np.eye(4)], 1.0)
    assert n == 3
    keep, _ = equal_the_twin(store, (4000.0, 0.3, 0.2, 2.0, 1), "three far points, cell 4000")
    st = engine.GroundStats(); st.n = 12345

    def refused(p, status):
        assert L.qn_kf_map_ground(store.h, C.byref(p), C.byref(st)) == status, (p.cell, p.max_slope, p.ground_tol, p.clearance, p.min_points)
        assert st.n == 12345
        cls = np.zeros(n, np.uint8); hq = np.zeros(n, np.int32)
        assert L.qn_kf_map_ground_points(store.h, cls.ctypes.data_as(C.c_void_p), None) == engine.QN_OK
        assert L.qn_kf_map_ground_points(store.h, None, hq.ctypes.data_as(C.c_void_p)) == engine.QN_OK
        info, gq, occ = store.map_ground_grid()
        assert _same(cls, keep["classes"]) and _same(hq, keep["height_q"]) and info == keep["info"] and _same(gq, keep["ground_q"]) and _same(occ, keep["occupancy"])

    for cell in (0.5, 1.0, 1.25):
        refused(engine.GroundParams(cell), engine.QN_ERR_CAPACITY)
        with pytest.raises(mg.CapacityError):
            mg.classify(store.download_map(n), (cell, 0.3, 0.2, 2.0, 1))
    assert 8001 ** 2 <= mg.MAX_CELLS < 10001 ** 2 and mg.quant_exponent(1.25) == 9
    inf, nan = float("inf"), float("nan")
    bad = [(0.0, 0.3, 0.2, 2.0, 1), (-1.0, 0.3, 0.2, 2.0, 1), (nan, 0.3, 0.2, 2.0, 1), (inf, 0.3, 0.2, 2.0, 1), (0.5, 0.0, 0.2, 2.0, 1), (0.5, -0.3, 0.2, 2.0, 1),
           (0.5, nan, 0.2, 2.0, 1), (0.5, inf, 0.2, 2.0, 1), (0.5, 0.3, -0.1, 2.0, 1), (0.5, 0.3, nan, 2.0, 1), (0.5, 0.3, inf, 2.0, 1), (0.5, 0.3, 0.2, 0.2, 1),
           (0.5, 0.3, 0.2, 0.1, 1), (0.5, 0.3, 0.2, nan, 1), (0.5, 0.3, 0.2, inf, 1), (0.5, 0.3, 0.2, 2.0, 0), (0.5, 1e7, 0.2, 2.0, 1), (0.5, 0.3, 0.2, 1e6, 1),
           (0.5, 0.3, 6e5, 7e5, 1)]
    for b in bad:
        refused(engine.GroundParams(*b), engine.QN_ERR_INVALID_ARG)
        with pytest.raises(ValueError):
            mg.classify(np.zeros((1, 3), np.float32), b)
    p = engine.GroundParams(); p.reserved = 1
    refused(p, engine.QN_ERR_INVALID_ARG)
    assert L.qn_kf_map_ground(store.h, None, C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_ground(store.h, C.byref(engine.GroundParams()), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_ground_points(store.h, None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_ground_grid(store.h, None, None, None) == engine.QN_ERR_INVALID_ARG
    ptr = C.c_void_p(); m = C.c_uint32()
    for mask in (0, 32, 0x80000001):
        assert L.qn_kf_map_keep_classes(store.h, mask, C.byref(ptr), C.byref(m)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_keep_classes(store.h, 1, None, C.byref(m)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_keep_classes(store.h, 1, C.byref(ptr), None) == engine.QN_ERR_INVALID_ARG
    refused(engine.GroundParams(0.5), engine.QN_ERR_CAPACITY)                    # and everything is still there
    assert len(store.download_map(n)) == n


def test_not_ready_without_a_map():
    from qn_amd import engine
    s = engine.KeyframeStore()
    try:
        st = engine.GroundStats(); ptr = C.c_void_p(); m = C.c_uint32(); out = np.zeros(4, np.uint32)
        assert s._l.qn_kf_map_ground(s.h, C.byref(engine.GroundParams()), C.byref(st)) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_ground_points(s.h, out.ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_ground_grid(s.h, C.byref(engine.GroundGrid()), None, None) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_keep_classes(s.h, 2, C.byref(ptr), C.byref(m)) == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_ground()
        assert ei.value.status == engine.QN_ERR_NOT_READY
    finally:
        s.close()


def test_street_scene_map_and_the_chain_behind_the_static_map(store, scans):
    """the ray-cast street scene at leaf 0.3 through build_map; then build_map_static -> map_remove_outliers -> map_ground, each stage on what the one before
    left in the slot"""
    from qn_amd import engine
    n = store.build_map(scans, POSES, 0.3)
    assert 3000 <= n <= 40000, n
    got, _ = equal_the_twin(store, DEFAULT, "street scene, build_map")
    s = got["stats"]
    assert s["n_ground"] > n // 4 and s["n_obstacle"] > 100 and s["occupied"] > 20 and s["free"] > s["occupied"] and s["unknown"] > 0
    store.range_set_params(engine.RangeParams.for_sensor(SEN))
    store.range_describe(scans)
    store.static_classify(scans, POSES, radius=15.0, max_k=3)
    n1 = store.build_map_static(0.3)
    store.map_outliers(engine.OutlierParams(1.0, 2.0, 8))
    _, n2 = store.map_remove_outliers()
    assert 0 < n2 < n1 <= n
    got, _ = equal_the_twin(store, DEFAULT, "street scene, static map without its outliers")
    assert got["stats"]["n"] == n2 and got["stats"]["n_ground"] > n2 // 4
