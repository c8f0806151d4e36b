"""The keyframe store's map getters at the degenerate sizes a shared getter gets wrong first: a result of no rows behind a buffer padded to one element, the
reshape of nothing, a planar field beside a volume.  One keyframe of 64 points on a 6 m line straight up from the sensor, identity pose, voxel 1 m: the volume
is one column of D layers (W = H = 1) without an unknown voxel, so the list of the unknown class is empty, and a min_size above the grid rejects every frontier
voxel, so there is no region.  Only shapes, dtypes and the documented fill values are asserted; what the fields hold is the other GPU tests' business.

Two calls the library refuses rather than answers with nothing are pinned as refusals: map_occupancy_list(mask=0) (qn_kf_map_occupancy_list refuses an empty
class mask, so the empty list is asked for with the class the volume lacks) and map_crop([], 1.0) (qn_kf_map_crop refuses zero centres)."""
import numpy as np
import pytest
from qn_amd import mapfrontier as mf, mapview as mv

pytestmark = pytest.mark.gpu
GRID_KEYS = ["origin", "voxel", "width", "height", "depth", "minc"]


def _is(a, shape, dtype):
    return isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.dtype(dtype)


def test_getters_at_empty_results_and_one_column_grids():
    from qn_amd import engine
    pts = np.zeros((64, 3), np.float32)
    pts[:, 2] = np.linspace(1.0, 7.0, 64)
    store = engine.KeyframeStore()
    try:
        kid = store.add(pts)
        stats = store.map_occupancy([kid], [np.eye(4)], engine.OccupancyParams(voxel=1.0, max_range=10))
        W, H, D = stats["width"], stats["height"], stats["depth"]
        assert (W, H) == (1, 1) and D > 1 and stats["unknown"] == 0 and stats["free"] > 0 and stats["occupied"] > 0, stats
        ginfo, hits, misses, cls = store.map_occupancy_grid()
        assert list(ginfo) == GRID_KEYS and (ginfo["width"], ginfo["height"], ginfo["depth"]) == (W, H, D), ginfo
        assert _is(hits, (D, H, W), np.uint32) and _is(misses, (D, H, W), np.uint32) and _is(cls, (D, H, W), np.uint8)

        # ---- a list of no voxels: the second call is skipped, the padded buffers are cut to nothing
        ijk, h, m = store.map_occupancy_list(1 << engine.QN_OCC_UNKNOWN)
        assert _is(ijk, (0, 3), np.int32) and _is(h, (0,), np.uint32) and _is(m, (0,), np.uint32)
        with pytest.raises(engine.EngineError) as e:
            store.map_occupancy_list(mask=0)
        assert e.value.status == engine.QN_ERR_INVALID_ARG

        # ---- a band above the grid
        occ = store.map_occupancy_slice(D + 5, D + 9)
        assert _is(occ, (H, W), np.uint8) and (occ == 0).all()
        store.map_distance()
        dinfo, dparams, d2 = store.map_distance_grid()
        assert list(dinfo) == GRID_KEYS and dinfo == ginfo and list(dparams) == ["site_mask", "max_dist"] and _is(d2, (D, H, W), np.uint16)
        far = store.map_distance_slice(D + 5, D + 9)
        assert _is(far, (H, W), np.uint16) and (far == engine.QN_DIST_FAR).all()

        # ---- the route field: one layer in planar mode, the volume otherwise
        for planar, depth in ((1, 1), (0, D)):
            store.map_route([[0.0, 0.0, 0.5]], engine.RouteParams(planar=planar))
            rinfo, rparams, cost = store.map_route_grid()
            assert list(rinfo) == GRID_KEYS and rinfo == ginfo and rparams["planar"] == planar, (rinfo, rparams)
            assert _is(cost, (depth, H, W), np.uint32), (planar, cost.shape, cost.dtype)

        # ---- frontiers without a region
        fstats = store.map_frontiers(engine.FrontierParams(min_size=W * H * D + 1))
        assert fstats["regions"] == 0, fstats
        finfo, fparams, lab = store.map_frontier_grid()
        assert list(finfo) == GRID_KEYS and finfo == ginfo and fparams["min_size"] == W * H * D + 1 and _is(lab, (D, H, W), np.int32)
        regions = store.map_frontier_regions()
        assert _is(regions, (0,), mf.INFO_DTYPE)
        cost, at = store.map_frontier_costs()
        assert _is(cost, (0,), np.uint32) and _is(at, (0, 3), np.int32)
        fijk, flab = store.map_frontier_list()
        assert fijk.dtype == np.int32 and fijk.shape == (len(flab), 3) and flab.dtype == np.int32 and len(flab) == fstats["frontier"]
        assert (flab == engine.QN_FRONTIER_REJECTED).all()

        # ---- one viewpoint, one ray
        vinfo, vstats = store.map_view_gain([[0.0, 0.0, 0.5]], [[0, 0, 3 * 1024]])
        assert _is(vinfo, (1,), mv.VIEW_DTYPE) and vstats["viewpoints"] == 1, vstats
        cinfo, cparams, cover = store.map_view_grid()
        assert list(cinfo) == GRID_KEYS and cinfo == ginfo and list(cparams) == ["gain_mask", "stop_mask", "max_through", "iz_lo", "iz_hi"]
        assert _is(cover, (D, H, W), np.uint32)

        # ---- no centres: the library's refusal, not an empty list
        with pytest.raises(engine.EngineError) as e:
            store.map_crop([], 1.0)
        assert e.value.status == engine.QN_ERR_INVALID_ARG
    finally:
        store.close()
