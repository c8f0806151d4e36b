"""The occupancy map's view gain on the GPU (qn_kf_map_view_gain / qn_kf_map_view_grid) against its specification, the numpy twin qn_amd/mapview.py, run on the
class bytes the store's own occupancy call produced.  Everything behind the viewpoint's quantisation is an integer, so everything is compared for equality:
every row, every statistic the twin has, the whole cover volume, the returned grid and parameters, and a rerun.  No tolerance appears anywhere.  The cases and
what their construction determines: tests/view_cases.py.  The knobs QN_VIEW_PASS and QN_VIEW_NO_PEEK are read by the library per call, so the tests set them in
this process's environment around a call and need no child process."""
import contextlib
import os
import numpy as np
import pytest
import view_cases as vc
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, mapview as mv, synth

pytestmark = pytest.mark.gpu
F = np.float32
TWIN_STATS = mv.ViewStats._fields
KNOBS = ({}, {"QN_VIEW_PASS": "1"}, {"QN_VIEW_PASS": "2"}, {"QN_VIEW_NO_PEEK": "1"}, {"QN_VIEW_PASS": "3", "QN_VIEW_NO_PEEK": "1"})


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


@contextlib.contextmanager
def knobs(env):
    old = {k: os.environ.get(k) for k in ("QN_VIEW_PASS", "QN_VIEW_NO_PEEK")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_the_twin(store, viewpoints, offsets, params, what, want=None, env=KNOBS):
    """the view gain of the store's live occupancy result against the twin's of the downloaded classes (want: the twin's result where the caller has it), under
    every set of knobs of env, the first also rerun -> (info, cover, statistics)"""
    from qn_amd import engine
    oinfo, _, _, cls = store.map_occupancy_grid()
    p = mv.ViewParams(*params)
    if want is None:
        want = mv.gain(cls, mo.OccupancyGrid(**oinfo), viewpoints, offsets, p)
    first = None
    for e in env:
        for rerun in range(2 if first is None else 1):
            with knobs(e):
                info, stats = store.map_view_gain(viewpoints, offsets, engine.ViewParams(*p))
            ginfo, used, cover = store.map_view_grid()
            if first is None:
                print("%s: %d x %d x %d, %s: %s" % (what, oinfo["width"], oinfo["height"], oinfo["depth"], tuple(p), stats))
            for f in TWIN_STATS:
                assert stats[f] == getattr(want["stats"], f), (what, e, f, stats[f], getattr(want["stats"], f))
            assert stats["passes"] >= 1 and ginfo == oinfo and used == p._asdict(), (what, e, ginfo, used)
            assert info.dtype == mv.VIEW_DTYPE and len(info) == len(want["info"]), what
            for f in mv.VIEW_DTYPE.names:
                assert np.array_equal(info[f], want["info"][f]), (what, e, f, info[f].tolist(), want["info"][f].tolist())
            assert info.tobytes() == want["info"].tobytes(), (what, e)
            assert _same(cover, want["cover"]), (what, e, int((cover != want["cover"]).sum()))
            first = first or (info, cover, stats)
    if any("QN_VIEW_PASS" in e for e in env) and len(want["info"]) > 1:
        with knobs({"QN_VIEW_PASS": "1"}):
            assert store.map_view_gain(viewpoints, offsets, engine.ViewParams(*p))[1]["passes"] == len(want["info"]), what      # the knob is read per call
    return first


def _prepare(store, c):
    kid = store.add(c.records)
    ostats = store.map_occupancy([kid], [vc.POSE], c.occ)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == c.sides, (c.name, ostats)
    assert np.array_equal(store.map_occupancy_grid()[3], c.layout), c.name


@pytest.mark.parametrize("g", vc.NAMES)
def test_the_case_table(store, g):
    for c in vc.group(g):
        _prepare(store, c)
        info, cover, stats = equal_the_twin(store, c.viewpoints, c.offsets, c.params, c.name, want=vc.twin(c.name))
        vc.holds(c, info, cover, stats)


def test_not_ready_and_the_results_lifetime():
    from qn_amd import engine
    C = engine.C
    s = engine.KeyframeStore()
    try:
        L = engine.lib(); g = engine.OccupancyGrid(); p = engine.ViewParams(); st = engine.ViewStats()
        xyz = np.array([[0.5, 0.5, 0.5]]); off = np.array([[3 * 1024, 0, 0]], np.int32); rows = np.zeros(1, mv.VIEW_DTYPE)
        pp = lambda a: a.ctypes.data_as(C.c_void_p)
        gain = lambda: L.qn_kf_map_view_gain(s.h, pp(xyz), 1, pp(off), 1, C.byref(p), pp(rows), C.byref(st))
        not_ready = lambda: L.qn_kf_map_view_grid(s.h, C.byref(g), C.byref(engine.ViewParams()), None) == engine.QN_ERR_NOT_READY
        # before any occupancy call
        assert gain() == engine.QN_ERR_NOT_READY and not_ready()
        kid = s.add(np.array([[3, 2, 1], [3, 2, 1], [0, 0, 0]], F))      # 4 x 3 x 2: voxel (0, 0, 0) FREE, the far corner OCCUPIED, the rest UNKNOWN
        s.map_occupancy([kid], [vc.POSE], vc.TWO_HITS)
        assert not_ready()                                               # an occupancy result, no view call yet
        info, stats = s.map_view_gain(xyz, off)
        assert info["gain"].tolist() == [3] and info["reached"].tolist() == [1] and stats["total_gain"] == 3
        before = s.map_view_grid()[2]
        assert before.shape == (2, 3, 4) and before[0, 0].tolist() == [0, 1, 1, 1] and before.sum() == 3
        # the distance, route and frontier calls do not touch it
        s.map_distance(md.DistanceParams(1 << mo.OCCUPIED, 2))
        s.map_route([[0.5, 0.5, 0.5]], engine.RouteParams(1 << mo.FREE, 0))
        s.map_frontiers(engine.FrontierParams(min_size=1))
        assert _same(s.map_view_grid()[2], before)
        # a refused occupancy call leaves the result, a successful one ends it
        with pytest.raises(engine.EngineError):
            s.map_occupancy([kid + 7], [vc.POSE], vc.TWO_HITS)
        assert _same(s.map_view_grid()[2], before)
        s.map_occupancy([kid], [vc.POSE], vc.TWO_HITS)
        assert not_ready()
        assert s.map_view_gain(xyz, off)[0]["gain"].tolist() == [3] and _same(s.map_view_grid()[2], before)
    finally:
        s.close()


def test_refusals_leave_the_previous_result_byte_identical(store):
    from qn_amd import engine
    C = engine.C
    c = vc.case("random/14x12x6-band-through")
    _prepare(store, c)
    rows, before, stats = equal_the_twin(store, c.viewpoints, c.offsets, c.params, c.name, env=({},))
    L = engine.lib(); st = engine.ViewStats(); ok = engine.ViewParams(*c.params)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    xyz, off = c.viewpoints, c.offsets
    Q, R = len(xyz), len(off)
    out = np.zeros(Q, mv.VIEW_DTYPE)

    def intact():
        info, used, now = store.map_view_grid()
        assert _same(now, before) and used == c.params._asdict()

    bad = [dict(gain_mask=0), dict(gain_mask=8), dict(gain_mask=0x80000001), dict(stop_mask=8), dict(stop_mask=0x80000004), dict(stop_mask=1), dict(gain_mask=5),
           dict(gain_mask=6, stop_mask=2), dict(iz_lo=3, iz_hi=2), dict(iz_lo=0, iz_hi=-1)]
    for kw in bad:
        with pytest.raises(engine.EngineError) as ei:
            store.map_view_gain(xyz, off, engine.ViewParams(**dict(c.params._asdict(), **kw)))
        assert ei.value.status == engine.QN_ERR_INVALID_ARG, kw
        intact()
    for k in (0, 1, 2):
        r = engine.ViewParams(*c.params); r.reserved[k] = 1
        assert L.qn_kf_map_view_gain(store.h, pp(xyz), Q, pp(off), R, C.byref(r), pp(out), C.byref(st)) == engine.QN_ERR_INVALID_ARG
    call = lambda x, q, o, r, p, i, s_: L.qn_kf_map_view_gain(store.h, x, q, o, r, p, i, s_)
    args = [pp(xyz), Q, pp(off), R, C.byref(ok), pp(out), C.byref(st)]
    for k in (0, 2, 4, 5, 6):                                            # a null pointer
        a = list(args); a[k] = None
        assert call(*a) == engine.QN_ERR_INVALID_ARG, k
    for k, v in ((1, 0), (1, (1 << 16) + 1), (3, 0), (3, (1 << 20) + 1)):      # Q or R outside its range (refused before anything is read)
        a = list(args); a[k] = v
        assert call(*a) == engine.QN_ERR_INVALID_ARG, (k, v)
    for v in (mv.MAX_OFFSET + 1, -mv.MAX_OFFSET - 1, -(1 << 31)):        # an offset beyond the limit, in the last row
        o2 = off.copy(); o2[-1, 1] = v
        assert call(pp(xyz), Q, pp(o2), R, C.byref(ok), pp(out), C.byref(st)) == engine.QN_ERR_INVALID_ARG, v
    g = engine.OccupancyGrid()
    assert L.qn_kf_map_view_grid(store.h, None, C.byref(ok), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_view_grid(store.h, C.byref(g), None, None) == engine.QN_ERR_INVALID_ARG
    assert not out.view(np.uint8).any()                                  # nothing was written
    intact()
    with pytest.raises(engine.EngineError):                              # a refused occupancy call leaves it too
        store.map_occupancy([10 ** 6], [vc.POSE], c.occ)
    intact()
    o2 = off.copy(); o2[0] = [mv.MAX_OFFSET, -mv.MAX_OFFSET, 0]          # the limit itself is allowed
    equal_the_twin(store, xyz, o2, c.params, c.name + " with an offset at the limit", env=({},))


def test_the_empty_grid(store):
    """a keyframe whose records are all skipped: on a 0 x 0 x 0 grid every viewpoint is OUTSIDE and the call succeeds"""
    import distance_cases as dc
    kid = store.add(np.array([[np.nan, 0, 0]], F))
    assert store.map_occupancy([kid], [vc.POSE], dc.SITES)["n_rays"] == 0
    info, st = store.map_view_gain([[0.5, 0.5, 0.5], [np.nan, 0, 0]], [[1024, 0, 0]])
    assert st == dict(viewpoints=2, outside=2, rays=1, covered=0, max_cover=0, passes=0, total_gain=0, steps=0)
    want = np.zeros(2, mv.VIEW_DTYPE); want["status"] = mv.OUTSIDE
    assert info.tobytes() == want.tobytes()
    ginfo, used, cover = store.map_view_grid()
    assert cover.size == 0 and used == mv.ViewParams()._asdict() and ginfo["width"] == 0


def test_street_scene(store):
    """the four ray-cast scans of the street scene of test_map_route_twin (344 x 334 x 14 voxels at 0.3 m): 8 viewpoints at the centres of the frontier regions'
    cheapest voxels (map_frontier_costs) and a 16-beam, 300-step sensor of 20 m"""
    from test_map_route_twin import POSES, SEN
    from qn_amd import engine
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    ostats = store.map_occupancy(ids, POSES)
    assert (ostats["width"], ostats["height"], ostats["depth"]) == (344, 334, 14)
    store.map_frontiers(engine.FrontierParams(min_size=4))                # 13 regions (the default min_size leaves 7)
    store.map_distance(md.DistanceParams(1 << mo.OCCUPIED, 16))
    store.map_route(np.array([POSES[0][:3, 3]]), engine.RouteParams())
    cost, at = store.map_frontier_costs()
    order = np.argsort(cost, kind="stable")[:8]
    assert len(order) == 8 and cost[order[0]] < 0xfffffffe
    oinfo = store.map_occupancy_grid()[0]
    vps = mo.centres(at[order], mo.OccupancyGrid(**oinfo))
    off = mv.sensor_offsets(0.3, 20.0, 16, 300, -15, 15)
    info, cover, stats = equal_the_twin(store, vps, off, mv.ViewParams(), "street scene", env=({}, {"QN_VIEW_PASS": "3"}, {"QN_VIEW_NO_PEEK": "1"}))
    assert stats["outside"] == 0 and stats["total_gain"] > 1000 and stats["max_cover"] >= 2 and (info["gain"] > 0).any()
