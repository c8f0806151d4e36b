"""qn_kf_map_occupancy_update on the GPU against a second store's qn_kf_map_occupancy of the same list and against the twin (mapoccupancy.update), on the
sequences of tests/occupancy_update_cases.py.  After every step every getter returns the same bytes on both stores and the twin's, and update_out equals the
twin's counters: that is what shows the work was incremental and not a silent rebuild.  Equality everywhere; no tolerance."""
import os
import sys
import numpy as np
import pytest
from qn_amd import mapoccupancy as mo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_update_cases as uc

pytestmark = pytest.mark.gpu
NO_FOLD = ["seams", "duplicates", "shrink-regrow"]


class World:
    """two stores with the same keyframes: `live` is updated in place, `fresh` rebuilds every list from nothing"""

    def __init__(self, engine):
        self.engine = engine
        self.live, self.fresh = engine.KeyframeStore(), engine.KeyframeStore()
        self.ids = {s: [s.add(c) for c in uc.KEYFRAMES] for s in (self.live, self.fresh)}

    def args(self, store, st):
        return [self.ids[store][k] for k in st["keys"]], st["poses"], self.engine.OccupancyParams(*st["params"])


@pytest.fixture(scope="module")
def world():
    from qn_amd import engine
    w = World(engine)
    yield w
    w.live.close(); w.fresh.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fetch(store):
    """everything the getters serve: the grid, the four lists, the slices"""
    info, hits, misses, cls = store.map_occupancy_grid()
    out = dict(info=info, hits=hits, misses=misses, classes=cls)
    for mask in uc.MASKS:
        out["list", mask] = store.map_occupancy_list(mask)
    for lo, hi in uc.slice_ranges(info["depth"]):
        out["slice", lo, hi] = store.map_occupancy_slice(lo, hi)
    return out


def same_results(a, b, what):
    assert a["info"] == b["info"], (what, a["info"], b["info"])
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "info":
            continue
        x, y = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        assert all(_same(p, q) for p, q in zip(x, y)), (what, k)


def of_twin(result):
    g = result["grid"]
    out = dict(info=dict(zip(mo.OccupancyGrid._fields, g)), hits=result["hits"], misses=result["misses"], classes=result["classes"])
    for mask in uc.MASKS:
        out["list", mask] = mo.voxel_list(result, mask)
    for lo, hi in uc.slice_ranges(g.depth):
        out["slice", lo, hi] = mo.slice2d(result["classes"], lo, hi)
    return out


def run_sequence(world, name):
    """-> the live store's results after every step.  A full call of the first list comes first: it drops whatever ledger the store had, so the first update
    starts from nothing like the twin's"""
    steps = uc.SEQUENCES[name]
    world.live.map_occupancy(*world.args(world.live, steps[0]))
    out = []
    for k, (st, (want, wupd, _)) in enumerate(zip(steps, uc.twin(name))):
        stats, upd = world.live.map_occupancy_update(*world.args(world.live, st))
        full = world.fresh.map_occupancy(*world.args(world.fresh, st))
        print("%s[%d]: kept %d added %d removed %d rebuilt %d regridded %d walked %d dirty %s..%s, grid %d x %d x %d"
              % (name, k, upd["entries_kept"], upd["entries_added"], upd["entries_removed"], upd["rebuilt"], upd["regridded"], upd["records_walked"], upd["dirty_lo"],
                 upd["dirty_hi"], stats["width"], stats["height"], stats["depth"]))
        assert stats == full, (name, k, stats, full)
        assert stats == want["stats"]._asdict(), (name, k, stats, want["stats"])
        assert upd == wupd._asdict(), (name, k, upd, wupd)
        uc.check_expect(name, k, upd)
        got = fetch(world.live)
        same_results(got, fetch(world.fresh), (name, k, "against a rebuild"))
        same_results(got, of_twin(want), (name, k, "against the twin"))
        out.append(got)
    return out


@pytest.mark.parametrize("name", uc.NAMES)
def test_every_step_equals_a_rebuild_and_the_twin(world, name, monkeypatch):
    monkeypatch.delenv("QN_OCC_NO_FOLD", raising=False)
    run_sequence(world, name)


@pytest.mark.parametrize("name", NO_FOLD)
def test_no_fold_gives_the_folded_bytes(world, name, monkeypatch):
    """k_oc_carve<false> and k_oc_uncarve<false>: every lane adds and subtracts its own miss at v_0.  The library reads QN_OCC_NO_FOLD at every call."""
    monkeypatch.delenv("QN_OCC_NO_FOLD", raising=False)
    folded = run_sequence(world, name)
    monkeypatch.setenv("QN_OCC_NO_FOLD", "1")
    plain = run_sequence(world, name)
    monkeypatch.delenv("QN_OCC_NO_FOLD", raising=False)
    for k, (a, b) in enumerate(zip(folded, plain)):
        same_results(a, b, (name, k, "no fold"))


@pytest.mark.parametrize("name", ["correct", "shrink-regrow"])
def test_a_rerun_of_a_sequence_returns_the_same_bytes(world, name):
    first = run_sequence(world, name)
    for k, (a, b) in enumerate(zip(first, run_sequence(world, name))):
        same_results(a, b, (name, k, "rerun"))


def test_after_a_full_call_the_update_starts_from_nothing(world):
    steps = uc.SEQUENCES["grow"]
    world.live.map_occupancy(*world.args(world.live, steps[0]))
    stats, upd = world.live.map_occupancy_update(*world.args(world.live, steps[2]))
    assert upd["rebuilt"] == 1 and upd["entries_added"] == 3 and upd["entries_kept"] == 0 and upd["entries_removed"] == 0 and upd["regridded"] == 0
    assert stats == world.fresh.map_occupancy(*world.args(world.fresh, steps[2]))
    same_results(fetch(world.live), fetch(world.fresh), "after a full call")
    _, upd = world.live.map_occupancy_update(*world.args(world.live, steps[3]))
    assert upd["rebuilt"] == 0 and upd["entries_kept"] == 3 and upd["entries_added"] == 1


def test_refusals_leave_the_result_the_ledger_and_the_fields(world):
    engine, store = world.engine, world.live
    st = uc.SEQUENCES["grow"][1]
    ids, poses, p = world.args(store, st)
    store.map_occupancy(ids, poses, p)
    store.map_occupancy_update(ids, poses, p)
    before = fetch(store)
    store.map_distance()
    dist = store.map_distance_grid()[2]
    L = engine.lib(); C = engine.C
    pp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(status, ids_, poses_, p_=p):
        with pytest.raises(engine.EngineError) as ei:
            store.map_occupancy_update(ids_, poses_, p_)
        assert ei.value.status == status, (ei.value.status, status)
        same_results(fetch(store), before, "after a refusal")
        assert _same(store.map_distance_grid()[2], dist)

    third = world.ids[store][2]
    refused(engine.QN_ERR_CAPACITY, ids + [third], poses + [uc.pose((400000.0, 0, 0))])                  # 400 000 / 0.3 >= 2^20 voxels
    refused(engine.QN_ERR_CAPACITY, ids + [third], poses + [uc.pose((9900.0, 0, 0))])                    # 33 000 voxels a side
    refused(engine.QN_ERR_INVALID_ARG, ids + [len(uc.KEYFRAMES) + 1000], poses + [np.eye(4)])
    refused(engine.QN_ERR_INVALID_ARG, [-1], [np.eye(4)])
    bad = np.eye(4); bad[1, 2] = np.inf
    refused(engine.QN_ERR_INVALID_ARG, ids, [poses[0], bad])
    refused(engine.QN_ERR_INVALID_ARG, ids, poses, engine.OccupancyParams(voxel=0.0))
    a = np.array(ids, np.int32); P = np.ascontiguousarray(np.array(poses, np.float64)); s_ = engine.OccupancyStats(); u_ = engine.OccupancyUpdate()
    for args in ((None, pp(P), 2, C.byref(p), C.byref(s_), C.byref(u_)), (pp(a), None, 2, C.byref(p), C.byref(s_), C.byref(u_)),
                 (pp(a), pp(P), 0, C.byref(p), C.byref(s_), C.byref(u_)), (pp(a), pp(P), 2, None, C.byref(s_), C.byref(u_)),
                 (pp(a), pp(P), 2, C.byref(p), None, C.byref(u_)), (pp(a), pp(P), 2, C.byref(p), C.byref(s_), None)):
        assert L.qn_kf_map_occupancy_update(store.h, *args) == engine.QN_ERR_INVALID_ARG
    same_results(fetch(store), before, "after the null pointers")
    assert _same(store.map_distance_grid()[2], dist)
    _, upd = store.map_occupancy_update(ids + [third], poses + [uc.POSES[2]], p)                         # the ledger survived: every old entry is kept
    assert upd["rebuilt"] == 0 and upd["entries_kept"] == 2 and upd["entries_added"] == 1 and upd["entries_removed"] == 0


def test_an_update_ends_the_fields_and_serves_the_next_ones(world):
    engine, live, fresh = world.engine, world.live, world.fresh
    steps = uc.SEQUENCES["correct"]
    live.map_occupancy(*world.args(live, steps[0]))
    live.map_occupancy_update(*world.args(live, steps[0]))
    g = live.map_occupancy_grid()[0]
    centre = (np.array(g["minc"]) + np.array([g["width"], g["height"], g["depth"]]) / 2.0) * g["voxel"]
    offsets = np.array([[5 << 10, 0, 0], [0, 5 << 10, 0], [0, 0, 5 << 10], [-(5 << 10), 300, 0]], np.int32)
    live.map_distance(); live.map_route([centre]); live.map_frontiers(); live.map_view_gain([centre], offsets)
    for getter in (live.map_distance_grid, live.map_route_grid, live.map_frontier_grid, live.map_view_grid):
        getter()
    live.map_occupancy_update(*world.args(live, steps[1]))
    for getter in (live.map_distance_grid, live.map_route_grid, live.map_frontier_grid, live.map_view_grid):
        with pytest.raises(engine.EngineError) as ei:
            getter()
        assert ei.value.status == engine.QN_ERR_NOT_READY, getter.__name__
    fresh.map_occupancy(*world.args(fresh, steps[1]))
    assert live.map_distance() == fresh.map_distance() and _same(live.map_distance_grid()[2], fresh.map_distance_grid()[2])
    a, b = live.map_frontiers(), fresh.map_frontiers()
    assert {k: v for k, v in a.items() if k != "rounds"} == {k: v for k, v in b.items() if k != "rounds"}
    assert _same(live.map_frontier_grid()[2], fresh.map_frontier_grid()[2]) and a["regions"] > 0
