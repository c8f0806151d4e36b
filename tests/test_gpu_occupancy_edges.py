"""The occupancy kernels (k_oc_extent, k_oc_carve<true> and <false>, k_oc_classify, k_dg_list_flag / _pick and k_dg_slice of qn_dense_grid.cuh, with k_slot_fold, k_scan_rows and
sv_each_chunk behind them) on the edge cases of tests/occupancy_edge_cases.py: every byte against the numpy twin qn_amd/mapoccupancy.py - hits, misses,
classes, all 13 statistics, the grid info, the lists under all seven masks, the slices, a rerun - with no tolerance, and then against what the generators
state by construction (tests/test_occupancy_edges_cpu.py holds the twin to the same statements and to a scalar restatement, and shows which mistake each
knife-edge case tells apart, without a GPU).

What the cases reach that the scenes, the Gaussian directions and the five hand rays of test_gpu_map_occupancy.py do not:
  walk          all 27 sign patterns, edge and corner ties, origins on corners and faces heading down, zero-length axes, B == A, both sides of zero
  fold          a non-ray first lane, lane 63 the only carving lane, a wave of skipped records, n == shell beside n == shell + 1, a lone long ray; and
                k_oc_carve<false> (QN_OCC_NO_FOLD) on the same inputs: the same bytes
  gates         d2 equal to a bound and one ulp off it, where a contracted x x + y y + z z decides otherwise; half-to-even at k + 0.5 fixed-point units and a
                transform that lands on 1023.5; shell at 0, n and 0xFFFFFFFF; hits * hit_weight == misses, hits == min_hits - 1, a product that needs 64 bits
  limits        coordinates next to +-2^20 voxels, a side of exactly 2^15, the refusals (one bad record among 1 025) and the result they leave readable
  seams         SV_CHUNK + 3 entries (a second launch of the extent and the carve; k_slot_fold over 32 771 tiles), 255 / 256 / 257 cells and columns
Everything runs on ONE store; the twin of a case is computed once (occupancy_edge_cases.twin) and shared by the folded and the unfolded run."""
import os
import sys
import numpy as np
import pytest
from qn_amd import mapoccupancy as mo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_edge_cases as oc

pytestmark = pytest.mark.gpu
NO_FOLD = ["octants", "fold-lanes", "shell", "many-entries"]


class World:
    def __init__(self, engine):
        self.engine = engine
        self.store = engine.KeyframeStore()
        self.kids = {}                                               # id(record array) -> keyframe id: a keyframe is added once

    def ids_of(self, clouds):
        out = []
        for c in clouds:
            if id(c) not in self.kids:
                self.kids[id(c)] = (self.store.add(c), c)            # (the array is kept: its id stays its own)
            out.append(self.kids[id(c)][0])
        return out

    def fetch(self):
        info, hits, misses, cls = self.store.map_occupancy_grid()
        return dict(info=info, hits=hits, misses=misses, classes=cls)


@pytest.fixture(scope="module")
def world():
    from qn_amd import engine
    w = World(engine)
    yield w
    w.store.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_case(world, case):
    """the case on the engine against the twin, byte for byte, and against its `expect` -> the engine's results (with the statistics)"""
    store = world.store
    ids = world.ids_of(case.clouds)
    p = world.engine.OccupancyParams(*case.params)
    stats = store.map_occupancy(ids, case.poses, p)
    got = world.fetch()
    want = oc.twin(case.name)
    w, g = want["stats"], want["grid"]
    print("%s: %d records, %d rays (%d non-finite, %d near, %d far), grid %d x %d x %d, %d misses, occupied %d free %d unknown %d"
          % (case.name, stats["n_records"], stats["n_rays"], stats["n_nonfinite"], stats["n_near"], stats["n_far"], stats["width"], stats["height"], stats["depth"],
             stats["total_misses"], stats["occupied"], stats["free"], stats["unknown"]))
    assert len(mo.OccupancyStats._fields) == 13
    for f in mo.OccupancyStats._fields:
        assert stats[f] == getattr(w, f), (case.name, f, stats[f], getattr(w, f))
    assert tuple(got["info"][f] for f in mo.OccupancyGrid._fields) == tuple(g), (case.name, got["info"], g)
    for k in ("hits", "misses", "classes"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case.name, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (case.name, k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:5].tolist())
    for mask in oc.MASKS:
        a = store.map_occupancy_list(mask); b = mo.voxel_list(want, mask)
        assert all(_same(x, y) for x, y in zip(a, b)), (case.name, mask, len(a[0]), len(b[0]))
    for lo, hi in oc.slice_ranges(g.depth):
        assert _same(store.map_occupancy_slice(lo, hi), mo.slice2d(want["classes"], lo, hi)), (case.name, lo, hi)
    again = store.map_occupancy(ids, case.poses, p); got2 = world.fetch()                                 # a rerun returns the same bytes
    assert again == stats and got2["info"] == got["info"] and all(_same(got2[k], got[k]) for k in ("hits", "misses", "classes")), case.name
    oc.holds(case, got["hits"], got["misses"], got["classes"], stats, got["info"]["minc"])               # the engine's output against the construction, directly
    got["stats"] = stats
    return got


@pytest.mark.parametrize("name", oc.NAMES)
def test_every_case_equals_the_twin_and_its_construction(world, name):
    for case in oc.group(name):
        got = run_case(world, case)
        if "path" in case.meta:                                      # the hand walks: the whole volume, written out
            minc = got["info"]["minc"]
            visited = {tuple(int(v) for v in (np.array(i[::-1]) + minc)) for i in np.argwhere(got["misses"] > 0)}
            assert visited == set(case.meta["path"][:-1]) and got["stats"]["total_misses"] == len(case.meta["path"]) - 1
    if name == "many-entries":
        assert got["stats"]["n_records"] == case.meta["records"] and len(case.ids) == oc.SV_CHUNK + 3
        minc = got["info"]["minc"]
        assert all(got["hits"][z - minc[2], y - minc[1], x - minc[0]] == 1 for x, y, z in case.meta["last"])        # the second launch's three entries


@pytest.mark.parametrize("name", NO_FOLD)
def test_no_fold_gives_the_folded_bytes(world, name, monkeypatch):
    """k_oc_carve<false>: every lane adds its own miss to v_0.  The library reads QN_OCC_NO_FOLD at every call."""
    for case in oc.group(name):
        monkeypatch.delenv("QN_OCC_NO_FOLD", raising=False)
        folded = run_case(world, case)
        monkeypatch.setenv("QN_OCC_NO_FOLD", "1")
        plain = run_case(world, case)
        assert plain["stats"] == folded["stats"] and plain["info"] == folded["info"], case.name
        assert all(_same(plain[k], folded[k]) for k in ("hits", "misses", "classes")), case.name
    monkeypatch.delenv("QN_OCC_NO_FOLD", raising=False)


def test_refusals_leave_the_previous_result_readable(world):
    engine, store = world.engine, world.store
    before = run_case(world, oc.get("cell-seams/16x16x3"))
    listed = store.map_occupancy_list(7)
    for ref in oc.refusals():
        with pytest.raises(mo.CapacityError) as ti:
            mo.classify(ref.clouds, ref.poses, ref.params)
        assert ref.message in str(ti.value), (ref.name, str(ti.value))
        ids = world.ids_of(ref.clouds)
        with pytest.raises(engine.EngineError) as ei:
            store.map_occupancy(ids, ref.poses, engine.OccupancyParams(*ref.params))
        assert ei.value.status == engine.QN_ERR_CAPACITY, (ref.name, ei.value.status)
        assert ref.message in str(ei.value), (ref.name, str(ei.value))
        now = world.fetch()
        assert now["info"] == before["info"] and all(_same(now[k], before[k]) for k in ("hits", "misses", "classes")), ref.name
        assert all(_same(x, y) for x, y in zip(store.map_occupancy_list(7), listed)), ref.name
        assert _same(store.map_occupancy_slice(0, 2), mo.slice2d(before["classes"], 0, 2)), ref.name
    # the entry whose last record is refused is accepted without it
    ref = [r for r in oc.refusals() if r.name.startswith("one-record")][0]
    stats = store.map_occupancy([store.add(ref.clouds[0][:-1])], ref.poses, engine.OccupancyParams(*ref.params))
    assert stats["n_rays"] == 4 * oc.OC_BLOCK and stats["width"] == 2
