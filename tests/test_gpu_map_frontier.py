"""The occupancy map's frontier regions on the GPU (qn_kf_map_frontiers / _frontier_grid / _frontier_regions / _frontier_list / _frontier_costs) against their
specification, the numpy twin qn_amd/mapfrontier.py, run on the class bytes the store's own occupancy call produced.  Everything is an integer, so everything
is compared for equality: every label, every row of the region table, every statistic the twin has, the list, the returned info and parameters, the costs
after map_distance and map_route, and a rerun.  No tolerance appears anywhere.  The cases and what their construction determines: tests/frontier_cases.py."""
import numpy as np
import pytest
import frontier_cases as fc
from test_map_route_twin import POSES, SEN
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, maproute as mr, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
F = np.float32
TWIN_STATS = mf.FrontierStats._fields


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_the_twin(store, params, what, route=None):
    """the frontier regions of the store's live occupancy result under `params` (an mf.FrontierParams) against the twin's of the downloaded classes; with
    route = (distance params, route params, goals) also the costs under the field of the store's own map_distance and map_route
    -> (labels, info, statistics)"""
    from qn_amd import engine
    oinfo, _, _, cls = store.map_occupancy_grid()
    p = mf.FrontierParams(*params)
    stats = store.map_frontiers(engine.FrontierParams(*p))
    ginfo, used, labels = store.map_frontier_grid()
    info = store.map_frontier_regions()
    want = mf.frontier(cls, p)
    print("%s: %d x %d x %d, %s: %s" % (what, oinfo["width"], oinfo["height"], oinfo["depth"], tuple(p), stats))
    for f in TWIN_STATS:
        assert stats[f] == getattr(want["stats"], f), (what, f, stats[f], getattr(want["stats"], f))
    assert stats["rounds"] >= 1
    assert ginfo == oinfo and used == p._asdict(), (what, ginfo, used)
    assert labels.dtype == np.int32 and labels.shape == want["labels"].shape and np.array_equal(labels, want["labels"]), (what, int((labels != want["labels"]).sum()))
    assert info.dtype == mf.INFO_DTYPE and len(info) == len(want["info"]), (what, len(info), len(want["info"]))
    for f in mf.INFO_DTYPE.names:
        assert np.array_equal(info[f], want["info"][f]), (what, f)
    assert info.tobytes() == want["info"].tobytes(), what
    ijk, lab = store.map_frontier_list()
    wi, wl = mf.voxel_list(want["labels"])
    assert _same(ijk, wi) and _same(lab, wl), what
    if route is not None:
        dist, rp, goals = route
        store.map_distance(dist)
        store.map_route(goals, engine.RouteParams(*rp))
        cost = store.map_route_grid()[2]
        k, at = store.map_frontier_costs()
        wk, wat = mf.costs(want["labels"], len(want["info"]), cost)
        assert _same(k, wk) and _same(at, wat), (what, k.tolist(), wk.tolist())
        assert _same(store.map_frontier_grid()[2], labels)           # neither the distance nor the route call touched the result
    # a rerun returns the same bytes
    again = store.map_frontiers(engine.FrontierParams(*p))
    assert {f: again[f] for f in TWIN_STATS} == {f: stats[f] for f in TWIN_STATS}, what
    assert _same(store.map_frontier_grid()[2], labels) and store.map_frontier_regions().tobytes() == info.tobytes(), what
    return labels, info, stats


def _prepare(store, c):
    kid = store.add(c.records)
    ostats = store.map_occupancy([kid], [fc.POSE], c.occ)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == c.sides, (c.name, ostats)
    assert np.array_equal(store.map_occupancy_grid()[3], c.layout), c.name


def _run(store, c):
    _prepare(store, c)
    labels, info, stats = equal_the_twin(store, c.params, c.name, route=(c.dist, c.route, c.goal))
    fc.holds(c, labels, info, stats)
    k, at = store.map_frontier_costs()
    fc.costs_hold(c, k, at)
    return labels


@pytest.mark.parametrize("g", fc.NAMES)
def test_the_case_table(store, g):
    for c in fc.group(g):
        _run(store, c)


def test_not_ready_and_the_results_lifetime():
    from qn_amd import engine
    C = engine.C
    s = engine.KeyframeStore()
    try:
        L = engine.lib(); g = engine.OccupancyGrid(); p = engine.FrontierParams(min_size=1); st = engine.FrontierStats(); cnt = C.c_uint32(77)
        out = np.zeros(64, np.uint32); ijk = np.zeros(3 * 64, np.int32); lab = np.zeros(64, np.int32); rows = np.zeros(8, mf.INFO_DTYPE)
        pp = lambda a: a.ctypes.data_as(C.c_void_p)

        def not_ready():
            assert L.qn_kf_map_frontier_grid(s.h, C.byref(g), C.byref(engine.FrontierParams()), None) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_frontier_regions(s.h, pp(rows), 8, C.byref(cnt)) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_frontier_list(s.h, pp(ijk), pp(lab), 64, C.byref(cnt)) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_frontier_costs(s.h, pp(out), pp(ijk)) == engine.QN_ERR_NOT_READY
        # before any occupancy call
        assert L.qn_kf_map_frontiers(s.h, C.byref(p), C.byref(st)) == engine.QN_ERR_NOT_READY
        not_ready()
        kid = s.add(np.array([[3, 2, 1], [3, 2, 1], [0, 0, 0], [1, 0, 0]], F))
        s.map_occupancy([kid], [fc.POSE], fc.TWO_HITS)
        not_ready()                                                  # an occupancy result, no frontier call yet
        # frontiers need neither the distance field nor the route field
        assert s.map_frontiers(p)["regions"] == 1
        before = s.map_frontier_grid()[2]
        assert before.shape == (2, 3, 4) and before[0, 0, 0] == 0 and before[0, 0, 1] == 0 and before[1, 2, 3] == mf.NONE
        # the costs need a live route field
        assert L.qn_kf_map_frontier_costs(s.h, pp(out), pp(ijk)) == engine.QN_ERR_NOT_READY
        s.map_distance(md.DistanceParams(1 << mo.OCCUPIED, 2))
        assert L.qn_kf_map_frontier_costs(s.h, pp(out), pp(ijk)) == engine.QN_ERR_NOT_READY
        s.map_route([[0.5, 0.5, 0.5]], engine.RouteParams(1 << mo.FREE, 0))
        k, at = s.map_frontier_costs()
        assert k.tolist() == [0] and at.tolist() == [[0, 0, 0]]
        assert _same(s.map_frontier_grid()[2], before)               # the distance and route calls did not touch it
        s.map_distance(md.DistanceParams(1 << mo.OCCUPIED, 2))      # a new distance field ends the route field, not the regions
        assert L.qn_kf_map_frontier_costs(s.h, pp(out), pp(ijk)) == engine.QN_ERR_NOT_READY
        assert _same(s.map_frontier_grid()[2], before)
        # a refused occupancy call leaves the result, a successful one ends it
        with pytest.raises(engine.EngineError):
            s.map_occupancy([kid + 7], [fc.POSE], fc.TWO_HITS)
        assert _same(s.map_frontier_grid()[2], before)
        s.map_occupancy([kid], [fc.POSE], fc.TWO_HITS)
        not_ready()
        assert s.map_frontiers(p)["regions"] == 1 and _same(s.map_frontier_grid()[2], before)
    finally:
        s.close()


def test_refusals_leave_the_previous_result_byte_identical(store):
    from qn_amd import engine
    C = engine.C
    c = fc.case("random/40x33x19-sparse")
    _prepare(store, c)
    before, rows, stats = equal_the_twin(store, c.params, c.name)
    L = engine.lib(); st = engine.FrontierStats(); ok = engine.FrontierParams(*c.params); cnt = C.c_uint32(0)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)

    def intact():
        info, used, now = store.map_frontier_grid()
        assert _same(now, before) and used == c.params._asdict() and store.map_frontier_regions().tobytes() == rows.tobytes()

    bad = [dict(free_mask=0), dict(free_mask=8), dict(free_mask=0x80000002), dict(unknown_mask=0), dict(unknown_mask=9), dict(unknown_mask=2), dict(free_mask=3),
           dict(free_mask=6, unknown_mask=5), dict(edge_unknown=2), dict(edge_unknown=0xffffffff), dict(min_size=0), dict(iz_lo=3, iz_hi=2), dict(iz_lo=0, iz_hi=-1)]
    for kw in bad:
        with pytest.raises(engine.EngineError) as ei:
            store.map_frontiers(engine.FrontierParams(**dict(c.params._asdict(), **kw)))
        assert ei.value.status == engine.QN_ERR_INVALID_ARG, kw
        intact()
    for k in (0, 1):
        r = engine.FrontierParams(*c.params); r.reserved[k] = 1
        assert L.qn_kf_map_frontiers(store.h, C.byref(r), C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontiers(store.h, None, C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontiers(store.h, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    g = engine.OccupancyGrid(); out = np.zeros(4096, np.uint32); ijk = np.zeros(3 * 4096, np.int32); lab = np.zeros(4096, np.int32)
    assert L.qn_kf_map_frontier_grid(store.h, None, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_grid(store.h, C.byref(g), None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_regions(store.h, pp(out), 4096, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_regions(store.h, None, 4096, C.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_list(store.h, pp(ijk), pp(lab), 4096, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_list(store.h, None, pp(lab), 4096, C.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_list(store.h, pp(ijk), None, 4096, C.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_costs(store.h, None, pp(ijk)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_costs(store.h, pp(out), None) == engine.QN_ERR_INVALID_ARG
    intact()
    # a capacity below the count: the count comes back, nothing else is written
    R, n = stats["regions"], stats["frontier"]
    assert R >= 2 and n > R
    guard = np.full(64 * R, 0xab, np.uint8)
    for cap in (0, R - 1):
        cnt.value = 0
        assert L.qn_kf_map_frontier_regions(store.h, pp(guard), cap, C.byref(cnt)) == engine.QN_ERR_CAPACITY and cnt.value == R and (guard == 0xab).all()
    cnt.value = 0
    assert L.qn_kf_map_frontier_regions(store.h, pp(guard), R, C.byref(cnt)) == engine.QN_OK and cnt.value == R and guard.tobytes() == rows.tobytes()
    gi = np.full(3 * n, -77, np.int32); gl = np.full(n, -77, np.int32)
    for cap in (0, n - 1):
        cnt.value = 0
        assert L.qn_kf_map_frontier_list(store.h, pp(gi), pp(gl), cap, C.byref(cnt)) == engine.QN_ERR_CAPACITY and cnt.value == n and (gi == -77).all() and (gl == -77).all()
    assert L.qn_kf_map_frontier_list(store.h, pp(gi), pp(gl), n, C.byref(cnt)) == engine.QN_OK and cnt.value == n and (gl != -77).all()
    intact()
    # a refused occupancy call leaves it too
    with pytest.raises(engine.EngineError):
        store.map_occupancy([10 ** 6], [fc.POSE], c.occ)
    intact()


def test_the_empty_grid(store):
    """a keyframe whose records are all skipped: a 0 x 0 x 0 grid succeeds with zero statistics"""
    import distance_cases as dc
    kid = store.add(np.array([[np.nan, 0, 0]], F))
    assert store.map_occupancy([kid], [fc.POSE], dc.SITES)["n_rays"] == 0
    st = store.map_frontiers()
    assert st == dict(dict.fromkeys(TWIN_STATS, 0), rounds=0)
    info, used, labels = store.map_frontier_grid()
    assert labels.size == 0 and used == mf.FrontierParams()._asdict() and info["width"] == 0
    assert len(store.map_frontier_regions()) == 0
    ijk, lab = store.map_frontier_list()
    assert len(ijk) == 0 and len(lab) == 0
    store.map_distance()
    store.map_route(np.zeros((1, 3)))
    k, at = store.map_frontier_costs()
    assert len(k) == 0 and at.shape == (0, 3)


def test_street_scene(store):
    """the four ray-cast scans of the street scene of test_gpu_map_route.py (344 x 334 x 14 voxels at 0.3 m): the default parameters and the planner's band,
    the costs under the 3-D and the planar route field to the position of POSES[0]"""
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    ostats = store.map_occupancy(ids, POSES)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == (344, 334, 14)
    goal = np.array([POSES[0][:3, 3]])
    dist = md.DistanceParams(1 << mo.OCCUPIED, 16)
    for params, rp in ((mf.FrontierParams(), mr.RouteParams()), (mf.FrontierParams(iz_lo=4, iz_hi=8, min_size=20), mr.RouteParams(1 << mo.FREE, 4, 6, 6, 1))):
        labels, info, stats = equal_the_twin(store, params, "street scene", route=(dist, rp, goal))
        assert stats["regions"] >= 1 and stats["frontier"] > 1000
        k, _ = store.map_frontier_costs()
        assert (k < mr.BLOCKED).any()                                # some region can be reached from the first pose


def test_cpp_helper_gives_the_python_result(store, tmp_path):
    """tests/shim_map_frontier.cpp (qn_map::mapFrontiers / frontierRegions / frontierCosts against the stand-ins) on two scans of the street scene"""
    import os
    import subprocess
    from qn_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_shim("shim_map_frontier.cpp", tmp_path)
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES[:2], [11, 12])]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, F).tobytes())
    np.ascontiguousarray(np.array(POSES[:2], np.float64)).tofile(str(tmp_path / "poses.bin"))
    goal = POSES[0][:3, 3]
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "12"] + [repr(float(v)) for v in goal], text=True)
    store.map_occupancy(ids, POSES[:2], engine.OccupancyParams(voxel=0.3))
    st = store.map_frontiers(engine.FrontierParams(min_size=12))
    rows = store.map_frontier_regions()
    store.map_distance(engine.DistanceParams(4, 16))
    store.map_route([goal], engine.RouteParams(2, 0))
    k, at = store.map_frontier_costs()

    def fnv(chunks):
        h = 1469598103934665603
        for b in chunks:
            for x in b:
                h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
        return h
    assert txt.splitlines() == ["frontiers " + " ".join(str(st[f]) for f in TWIN_STATS), "regions %d %016x" % (len(rows), fnv([rows.tobytes()])),
                                "costs %016x %016x" % (fnv([k.tobytes()]), fnv([at.tobytes()]))], txt
    assert st["regions"] >= 1 and st["frontier"] > 1000
