"""The occupancy map's distance field on the GPU (qn_kf_map_distance / _grid / _slice / _query) against its specification, the numpy twin qn_amd/mapdistance.py,
run on the class bytes the store's own occupancy call produced.  Everything is an integer, so everything is compared for equality: every voxel's d2, every
field of the statistics, the returned info and parameters, the slices, the queries, and a rerun.  No tolerance appears anywhere.  The cases and what their
construction determines: tests/distance_cases.py."""
import numpy as np
import pytest
import distance_cases as dc
from qn_amd import mapdistance as md, mapoccupancy as mo, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_the_twin(store, params, what):
    """the distance field of the store's live occupancy result under `params` (an md.DistanceParams) against the twin's of the downloaded classes
    -> (the GPU's d2, its statistics, the occupancy info, the classes)"""
    from qn_amd import engine
    oinfo, _, _, cls = store.map_occupancy_grid()
    grid = mo.OccupancyGrid(*(oinfo[f] for f in mo.OccupancyGrid._fields))
    p = engine.DistanceParams(*params)
    stats = store.map_distance(p)
    info, used, d2 = store.map_distance_grid()
    want = md.transform(cls, params)
    print("%s: %d x %d x %d, mask %d, max_dist %d: sites %d reached %d far %d max_d2 %d sum_d2 %d"
          % (what, grid.width, grid.height, grid.depth, params[0], params[1], stats["sites"], stats["reached"], stats["far"], stats["max_d2"], stats["sum_d2"]))
    for f in md.DistanceStats._fields:
        assert stats[f] == getattr(want["stats"], f), (what, f, stats[f], getattr(want["stats"], f))
    assert info == oinfo and used == dict(site_mask=int(params[0]), max_dist=int(params[1])), (what, info, used)
    assert d2.dtype == np.uint16 and d2.shape == want["d2"].shape and np.array_equal(d2, want["d2"]), (what, int((d2 != want["d2"]).sum()))
    for lo, hi in dc.slice_ranges(grid.depth):
        assert _same(store.map_distance_slice(lo, hi), md.slice2d(want["d2"], lo, hi)), (what, lo, hi)
    xyz, first_outside = dc.query_points(grid)
    qd, qc = store.map_distance_query(xyz)
    wd, wc = md.query(want["d2"], cls, grid, xyz)
    assert _same(qd, wd) and _same(qc, wc), (what, int((qd != wd).sum()), int((qc != wc).sum()))
    assert (qd[first_outside:] == md.FAR).all() and (qc[first_outside:] == md.OUTSIDE).all() and (qc[:first_outside] <= 2).all(), what
    # a rerun returns the same bytes
    again = store.map_distance(p)
    assert again == stats and _same(store.map_distance_grid()[2], d2), what
    return d2, stats, oinfo, cls


def _run(store, c):
    kid = store.add(c.records)
    ostats = store.map_occupancy([kid], [dc.POSE], c.occ)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == c.sides, (c.name, ostats)
    d2, stats, _, _ = equal_the_twin(store, c.params, c.name)
    dc.holds(c, d2, stats)
    return d2


def test_not_ready_without_an_occupancy_result_or_a_field():
    from qn_amd import engine
    C = engine.C
    s = engine.KeyframeStore()
    try:
        L = engine.lib(); g = engine.OccupancyGrid(); p = engine.DistanceParams(); st = engine.DistanceStats()
        out = np.zeros(4, np.uint16); cls = np.zeros(4, np.uint8); xyz = np.zeros(3)
        pp = lambda a: a.ctypes.data_as(C.c_void_p)

        def getters_not_ready():
            assert L.qn_kf_map_distance_grid(s.h, C.byref(g), C.byref(p), None) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_distance_slice(s.h, 0, 0, pp(out)) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_distance_query(s.h, pp(xyz), 1, pp(out), pp(cls)) == engine.QN_ERR_NOT_READY
        # before any occupancy call
        assert L.qn_kf_map_distance(s.h, C.byref(p), C.byref(st)) == engine.QN_ERR_NOT_READY
        getters_not_ready()
        # with an occupancy result, before the first distance call
        kid = s.add(np.array([[3, 2, 1], [0, 0, 0]], F))
        s.map_occupancy([kid], [dc.POSE], dc.SITES)
        getters_not_ready()
        s.map_distance()
        assert s.map_distance_grid()[2].shape == (2, 3, 4)
        # a refused occupancy call leaves the field, a successful one ends it
        with pytest.raises(engine.EngineError):
            s.map_occupancy([kid + 7], [dc.POSE], dc.SITES)
        assert s.map_distance_grid()[2].shape == (2, 3, 4)
        s.map_occupancy([kid], [dc.POSE], dc.SITES)
        getters_not_ready()
        assert s.map_distance()["sites"] == 2
    finally:
        s.close()


@pytest.mark.parametrize("g", dc.NAMES)
def test_the_case_table(store, g):
    for c in dc.group(g):
        _run(store, c)


def test_the_empty_grid(store):
    """a keyframe whose records are all skipped: a 0 x 0 x 0 grid succeeds with zero statistics"""
    kid = store.add(np.array([[np.nan, 0, 0]], F))
    assert store.map_occupancy([kid], [dc.POSE], dc.SITES)["n_rays"] == 0
    assert store.map_distance() == dict(sites=0, reached=0, far=0, max_d2=0, sum_d2=0)
    info, used, d2 = store.map_distance_grid()
    assert d2.shape == (0, 0, 0) and used == dict(site_mask=4, max_dist=16) and info["width"] == 0
    assert store.map_distance_slice(0, 3).shape == (0, 0)
    qd, qc = store.map_distance_query(np.zeros((3, 3)))
    assert qd.tolist() == [md.FAR] * 3 and qc.tolist() == [md.OUTSIDE] * 3


def test_refusals_leave_the_previous_field_byte_identical(store):
    from qn_amd import engine
    C = engine.C
    c = dc.group("random")[0]
    before = _run(store, c)
    L = engine.lib(); st = engine.DistanceStats(); ok = engine.DistanceParams()
    pp = lambda a: a.ctypes.data_as(C.c_void_p)

    def intact():
        info, used, now = store.map_distance_grid()
        assert _same(now, before) and used == dict(site_mask=c.params.site_mask, max_dist=c.params.max_dist)

    for kw in (dict(site_mask=0), dict(site_mask=8), dict(site_mask=12), dict(site_mask=0x80000004), dict(max_dist=0), dict(max_dist=256), dict(max_dist=0xffffffff)):
        with pytest.raises(engine.EngineError) as ei:
            store.map_distance(engine.DistanceParams(**kw))
        assert ei.value.status == engine.QN_ERR_INVALID_ARG, kw
        intact()
    for k in (0, 1):
        r = engine.DistanceParams(); r.reserved[k] = 1
        assert L.qn_kf_map_distance(store.h, C.byref(r), C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance(store.h, None, C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance(store.h, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    g = engine.OccupancyGrid(); out = np.zeros(c.voxels, np.uint16); cls = np.zeros(4, np.uint8); xyz = np.zeros(3)
    assert L.qn_kf_map_distance_grid(store.h, None, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_grid(store.h, C.byref(g), None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_slice(store.h, 2, 1, pp(out)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_slice(store.h, 0, 1, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_query(store.h, pp(xyz), 0, pp(out), pp(cls)) == engine.QN_ERR_INVALID_ARG
    for args in ((None, 1, pp(out), pp(cls)), (pp(xyz), 1, None, pp(cls)), (pp(xyz), 1, pp(out), None)):
        assert L.qn_kf_map_distance_query(store.h, *args) == engine.QN_ERR_INVALID_ARG
    intact()
    # a refused occupancy call leaves it too
    with pytest.raises(engine.EngineError):
        store.map_occupancy([10 ** 6], [dc.POSE], c.occ)
    intact()


def test_street_scene(store):
    """the four ray-cast scans of the street scene of test_gpu_map_occupancy.py (344 x 334 x 14 voxels at the default 0.3 m), max_dist 16, both masks"""
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    ostats = store.map_occupancy(ids, POSES)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == (344, 334, 14)
    _, occ_stats, _, _ = equal_the_twin(store, md.DistanceParams(dc.OCC, 16), "street scene, occupied")
    _, unk_stats, _, _ = equal_the_twin(store, md.DistanceParams(dc.OCC | dc.UNK, 16), "street scene, occupied or unknown")
    assert occ_stats["sites"] == ostats["occupied"] > 5000 and unk_stats["sites"] == ostats["occupied"] + ostats["unknown"]
    assert occ_stats["far"] > 0 and unk_stats["reached"] < ostats["free"] + 1 and unk_stats["max_d2"] <= occ_stats["max_d2"] <= 256


def test_cpp_helper_gives_the_python_result(store, tmp_path):
    """tests/shim_map_distance.cpp (qn_map::mapDistance / distanceSlice / distanceAt against the stand-ins) on two scans of the street scene"""
    import os
    import subprocess
    from qn_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_shim("shim_map_distance.cpp", tmp_path)
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES[:2], [11, 12])]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, F).tobytes())
    np.ascontiguousarray(np.array(POSES[:2], np.float64)).tofile(str(tmp_path / "poses.bin"))
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "2", "6", "5", "12"], text=True)
    store.map_occupancy(ids, POSES[:2], engine.OccupancyParams(voxel=0.3))
    st = store.map_distance(engine.DistanceParams(5, 12))
    info = store.map_distance_grid()[0]

    def fnv(chunks):
        h = 1469598103934665603
        for b in chunks:
            for x in b:
                h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
        return h
    side = np.array([info["width"], info["height"], info["depth"]], np.float64)
    xyz = np.array([[info["origin"][k] + (float(i) - 0.5) / 62.0 * side[k] * info["voxel"] for k in range(3)] for i in range(64)], np.float64)
    d2, cls = store.map_distance_query(xyz)
    dist = md.metres(d2, info["voxel"])
    assert txt.splitlines() == ["distance %d %d %d %d %d" % (st["sites"], st["reached"], st["far"], st["max_d2"], st["sum_d2"]),
                                "slice %016x" % fnv([store.map_distance_slice(2, 6).tobytes()]),
                                "at %016x" % fnv(dist[i].tobytes() + cls[i].tobytes() for i in range(64))], txt
    assert cls[0] == cls[63] == md.OUTSIDE and (cls[1:63] <= 2).all() and st["sites"] > 1000
