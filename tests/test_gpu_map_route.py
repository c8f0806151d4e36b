"""The occupancy map's route field on the GPU (qn_kf_map_route / _grid / _query / _path) against its specification, the numpy twin qn_amd/maproute.py, run on
the class bytes and the distance field the store's own calls produced.  Everything is an integer, so everything is compared for equality: every cell's cost,
every statistic the twin has, the returned info and parameters, the queries, the paths' lengths and voxels, and a rerun.  No tolerance appears anywhere.  The
cases and what their construction determines: tests/route_cases.py."""
import numpy as np
import pytest
import distance_cases as dc
import route_cases as rc
from test_map_route_twin import POSES, SEN, STREET, path_holds
from qn_amd import mapdistance as md, mapoccupancy as mo, maproute as mr, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
F = np.float32
TWIN_STATS = mr.RouteStats._fields


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_the_twin(store, goals, params, starts, what):
    """the route field of the store's live occupancy result and distance field under `params` (an mr.RouteParams) against the twin's of the downloaded classes
    and d2 -> (the GPU's cost, its statistics, the grid)"""
    from qn_amd import engine
    oinfo, _, _, cls = store.map_occupancy_grid()
    grid = mo.OccupancyGrid(*(oinfo[f] for f in mo.OccupancyGrid._fields))
    d2 = store.map_distance_grid()[2]
    p = mr.RouteParams(*params)
    stats = store.map_route(goals, engine.RouteParams(*p))
    info, used, cost = store.map_route_grid()
    want = mr.field(cls, d2, grid, goals, p)
    print("%s: %d x %d x %d, %s: %s" % (what, grid.width, grid.height, grid.depth, tuple(p), stats))
    for f in TWIN_STATS:
        assert stats[f] == getattr(want["stats"], f), (what, f, stats[f], getattr(want["stats"], f))
    assert info == oinfo and used == p._asdict(), (what, info, used)
    assert cost.dtype == np.uint32 and cost.shape == want["cost"].shape and np.array_equal(cost, want["cost"]), (what, int((cost != want["cost"]).sum()))
    assert 1 <= stats["rounds"] <= cost.size + 2 and stats["tile_visits"] <= stats["rounds"] * tiles_of(cost.shape), (what, stats)
    xyz, _ = dc.query_points(grid)
    q = store.map_route_query(xyz)
    assert _same(q, mr.query(want["cost"], grid, xyz, p)), what
    full = stats["max_cost"] // 3 + 1
    for max_len in (full, 3):                                        # whole paths, and every path longer than three voxels truncated
        lens, ijk = store.map_route_paths(starts, max_len)
        wl, wi = mr.paths(want["cost"], grid, starts, max_len, p)
        assert _same(lens, wl) and _same(ijk, wi), (what, max_len, lens.tolist(), wl.tolist())
        path_holds(cost, grid, p, np.asarray(starts, np.float64).reshape(-1, 3), lens, ijk, max_len, (what, max_len))
    # a rerun returns the same bytes
    again = store.map_route(goals, engine.RouteParams(*p))
    assert {f: again[f] for f in TWIN_STATS} == {f: stats[f] for f in TWIN_STATS} and _same(store.map_route_grid()[2], cost), what
    return cost, stats, grid


def tiles_of(shape):
    return int(np.prod([(n + rc.T - 1) // rc.T for n in shape]))


def _prepare(store, c):
    kid = store.add(c.records)
    ostats = store.map_occupancy([kid], [rc.POSE], c.occ)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == c.sides, (c.name, ostats)
    store.map_distance(c.dist)


_fields = {}


def _run(store, c):
    _prepare(store, c)
    cost, stats, _ = equal_the_twin(store, c.goals, c.params, c.starts(), c.name)
    _fields[c.name] = dict(cost=cost)
    rc.holds(c, cost, stats, other=lambda n: _fields[n] if n in _fields else rc.twin_field(n))
    if "min_rounds" in c.expect:
        assert stats["rounds"] >= c.expect["min_rounds"], (c.name, stats)
    if c.expect.get("dirty_rule"):
        assert stats["tile_visits"] < stats["rounds"] * tiles_of(cost.shape), (c.name, stats)      # a round loads only the tiles near the front
    return cost


@pytest.mark.parametrize("g", rc.NAMES)
def test_the_case_table(store, g):
    for c in rc.group(g):
        _run(store, c)


def test_not_ready_and_the_fields_lifetime():
    from qn_amd import engine
    C = engine.C
    s = engine.KeyframeStore()
    try:
        L = engine.lib(); g = engine.OccupancyGrid(); p = engine.RouteParams(2, 0); st = engine.RouteStats()
        out = np.zeros(64, np.uint32); ijk = np.zeros(64, np.int32); xyz = np.full(3, 0.5)
        pp = lambda a: a.ctypes.data_as(C.c_void_p)

        def not_ready():
            assert L.qn_kf_map_route_grid(s.h, C.byref(g), C.byref(engine.RouteParams()), None) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_route_query(s.h, pp(xyz), 1, pp(out)) == engine.QN_ERR_NOT_READY
            assert L.qn_kf_map_route_path(s.h, pp(xyz), 1, 4, pp(out), pp(ijk)) == engine.QN_ERR_NOT_READY
        # before any occupancy call, and with an occupancy result before the distance field
        assert L.qn_kf_map_route(s.h, pp(xyz), 1, C.byref(p), C.byref(st)) == engine.QN_ERR_NOT_READY
        not_ready()
        kid = s.add(np.array([[3, 2, 1], [3, 2, 1], [0, 0, 0]], F))
        s.map_occupancy([kid], [rc.POSE], rc.TWO_HITS)
        assert L.qn_kf_map_route(s.h, pp(xyz), 1, C.byref(p), C.byref(st)) == engine.QN_ERR_NOT_READY
        not_ready()
        s.map_distance(md.DistanceParams(rc.OCC, 2))
        not_ready()                                                  # a distance field, no route yet
        assert s.map_route([xyz], engine.RouteParams(3, 0))["reached"] == 23
        before = s.map_route_grid()[2]
        assert before.shape == (2, 3, 4) and before[0, 0, 0] == 0 and before[1, 2, 3] == mr.BLOCKED
        # a refused occupancy or distance call leaves the field, a successful one of either ends it
        with pytest.raises(engine.EngineError):
            s.map_occupancy([kid + 7], [rc.POSE], rc.TWO_HITS)
        with pytest.raises(engine.EngineError):
            s.map_distance(engine.DistanceParams(0, 2))
        assert _same(s.map_route_grid()[2], before)
        s.map_distance(md.DistanceParams(rc.OCC, 2))
        not_ready()
        assert s.map_route([xyz], engine.RouteParams(3, 0))["reached"] == 23 and _same(s.map_route_grid()[2], before)
        s.map_occupancy([kid], [rc.POSE], rc.TWO_HITS)
        not_ready()
        assert L.qn_kf_map_route(s.h, pp(xyz), 1, C.byref(p), C.byref(st)) == engine.QN_ERR_NOT_READY
        s.map_distance(md.DistanceParams(rc.OCC, 2))
        not_ready()
        assert s.map_route([xyz], engine.RouteParams(3, 0))["reached"] == 23
    finally:
        s.close()


def test_refusals_leave_the_previous_field_byte_identical(store):
    from qn_amd import engine
    C = engine.C
    c = rc.case("random/20x20x20-sparse-d2")
    before = _run(store, c)
    L = engine.lib(); st = engine.RouteStats(); ok = engine.RouteParams(*c.params)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    goals = np.ascontiguousarray(c.goals)

    def intact():
        info, used, now = store.map_route_grid()
        assert _same(now, before) and used == c.params._asdict()

    bad = [dict(pass_mask=0), dict(pass_mask=8), dict(pass_mask=12), dict(pass_mask=0x80000001), dict(planar=2), dict(planar=0xffffffff), dict(iz_lo=3, iz_hi=2),
           dict(iz_lo=0, iz_hi=-1), dict(min_d2=c.dist.max_dist ** 2 + 1), dict(min_d2=0xffffffff)]
    for kw in bad:
        with pytest.raises(engine.EngineError) as ei:
            store.map_route(goals, engine.RouteParams(**dict(c.params._asdict(), **kw)))
        assert ei.value.status == engine.QN_ERR_INVALID_ARG, kw
        intact()
    assert store.map_route(goals, engine.RouteParams(**dict(c.params._asdict(), min_d2=c.dist.max_dist ** 2)))["goals_used"] >= 0      # min_d2 = max_dist^2 is accepted
    _run(store, c)
    for k in (0, 1, 2):
        r = engine.RouteParams(*c.params); r.reserved[k] = 1
        assert L.qn_kf_map_route(store.h, pp(goals), len(goals), C.byref(r), C.byref(st)) == engine.QN_ERR_INVALID_ARG
    for args in ((None, 1, C.byref(ok), C.byref(st)), (pp(goals), 1, None, C.byref(st)), (pp(goals), 1, C.byref(ok), None), (pp(goals), 0, C.byref(ok), C.byref(st)),
                 (pp(goals), (1 << 20) + 1, C.byref(ok), C.byref(st))):
        assert L.qn_kf_map_route(store.h, *args) == engine.QN_ERR_INVALID_ARG
    g = engine.OccupancyGrid(); out = np.zeros(64, np.uint32); ijk = np.zeros(3 * 64, np.int32)
    assert L.qn_kf_map_route_grid(store.h, None, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_route_grid(store.h, C.byref(g), None, None) == engine.QN_ERR_INVALID_ARG
    for args in ((None, 1, pp(out)), (pp(goals), 1, None), (pp(goals), 0, pp(out)), (pp(goals), (1 << 20) + 1, pp(out))):
        assert L.qn_kf_map_route_query(store.h, *args) == engine.QN_ERR_INVALID_ARG
    for args in ((None, 1, 4, pp(out), pp(ijk)), (pp(goals), 1, 4, None, pp(ijk)), (pp(goals), 1, 4, pp(out), None), (pp(goals), 0, 4, pp(out), pp(ijk)),
                 (pp(goals), (1 << 20) + 1, 4, pp(out), pp(ijk)), (pp(goals), 1, 0, pp(out), pp(ijk))):
        assert L.qn_kf_map_route_path(store.h, *args) == engine.QN_ERR_INVALID_ARG
    intact()
    # a refused occupancy or distance call leaves it too
    with pytest.raises(engine.EngineError):
        store.map_occupancy([10 ** 6], [rc.POSE], c.occ)
    with pytest.raises(engine.EngineError):
        store.map_distance(engine.DistanceParams(4, 0))
    intact()


def test_the_empty_grid(store):
    """a keyframe whose records are all skipped: a 0 x 0 x 0 grid succeeds with zero statistics"""
    from qn_amd import engine
    kid = store.add(np.array([[np.nan, 0, 0]], F))
    assert store.map_occupancy([kid], [rc.POSE], dc.SITES)["n_rays"] == 0
    store.map_distance()
    for planar in (0, 1):
        st = store.map_route(np.zeros((2, 3)), engine.RouteParams(planar=planar))
        assert st == dict(passable=0, blocked=0, reached=0, unreached=0, goals_used=0, goals_blocked=2, max_cost=0, sum_cost=0, rounds=0, tile_visits=0)
        info, used, cost = store.map_route_grid()
        assert cost.size == 0 and used == mr.RouteParams(planar=planar)._asdict() and info["width"] == 0
        assert store.map_route_query(np.zeros((3, 3))).tolist() == [mr.BLOCKED] * 3
        lens, ijk = store.map_route_paths(np.zeros((2, 3)), 4)
        assert lens.tolist() == [0, 0] and not ijk.any()


def test_street_scene(store):
    """the four ray-cast scans of the street scene of test_gpu_map_distance.py (344 x 334 x 14 voxels at 0.3 m), distance (OCC, 16), pass FREE, goal = the
    position of POSES[0]: 3-D at min_d2 4 and 0, planar over the band (6, 6) at min_d2 4, with the numbers the twin's field and dijkstra agree on"""
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    ostats = store.map_occupancy(ids, POSES)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == (344, 334, 14)
    store.map_distance(md.DistanceParams(dc.OCC, 16))
    at = np.array([P[:3, 3] for P in POSES])
    for params, passable, reached, max_cost, at_poses in STREET:
        cost, stats, grid = equal_the_twin(store, at[:1], params, at, "street scene")
        assert (stats["passable"], stats["reached"], stats["max_cost"], stats["goals_used"]) == (passable, reached, max_cost, 1), stats
        assert store.map_route_query(at).tolist() == list(at_poses)
        assert stats["tile_visits"] < stats["rounds"] * tiles_of(cost.shape)


def test_cpp_helper_gives_the_python_result(store, tmp_path):
    """tests/shim_map_route.cpp (qn_map::mapRoute / routeCostAt / routePath against the stand-ins) on two scans of the street scene"""
    import os
    import subprocess
    from qn_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_shim("shim_map_route.cpp", tmp_path)
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES[:2], [11, 12])]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, F).tobytes())
    np.ascontiguousarray(np.array(POSES[:2], np.float64)).tofile(str(tmp_path / "poses.bin"))
    goal, start = POSES[0][:3, 3], POSES[1][:3, 3]
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "0", "0"] + [repr(float(v)) for v in list(goal) + list(start)], text=True)
    store.map_occupancy(ids, POSES[:2], engine.OccupancyParams(voxel=0.3))
    store.map_distance(engine.DistanceParams(4, 16))
    st = store.map_route([goal], engine.RouteParams(2, 0))
    info = store.map_route_grid()[0]

    def fnv(chunks):
        h = 1469598103934665603
        for b in chunks:
            for x in b:
                h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
        return h
    side = np.array([info["width"], info["height"], info["depth"]], np.float64)
    xyz = np.array([[info["origin"][k] + (float(i) - 0.5) / 62.0 * side[k] * info["voxel"] for k in range(3)] for i in range(64)], np.float64)
    q = store.map_route_query(xyz)
    lens, ijk = store.map_route_paths([start], int(store.map_route_query([start])[0]) // 3 + 1)
    n = int(lens[0])
    assert txt.splitlines() == ["route %d %d %d %d %d %d %d %d" % tuple(st[f] for f in TWIN_STATS),
                                "at %016x" % fnv([mr.metres(q, info["voxel"]).tobytes()]),
                                "path %d %016x" % (n, fnv([ijk[0, :n].tobytes()]))], txt
    assert n > 10 and q[0] == q[63] == mr.BLOCKED and st["reached"] > 1000
