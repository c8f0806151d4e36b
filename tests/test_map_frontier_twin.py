"""The numpy twin of the occupancy map's frontier regions (qn_amd/mapfrontier.py) against the definition: its propagated frontier() equals its brute() - a
literal flood fill per component - byte for byte on the case table of tests/frontier_cases.py, and both meet what the construction of each case determines.
Then costs() against a literal loop, the voxel list, the refusals of check_params, the flood fill without scipy, and the street scene of
tests/test_map_route_twin.py.  Integers throughout: no tolerance.  No GPU."""
import sys
import numpy as np
import pytest
import frontier_cases as fc
from test_map_route_twin import POSES, SEN
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, maproute as mr, synth

# the street scene under the default parameters: what frontier() and brute() agree on (regions, frontier voxels, the largest region); the scene of
# test_map_route_twin.py gives regions as it stands, so its parameters are unchanged
STREET_MIN_REGIONS = 1


def same(a, b):
    return a["labels"].tobytes() == b["labels"].tobytes() and a["info"].tobytes() == b["info"].tobytes() and a["stats"] == b["stats"]


@pytest.mark.parametrize("g", fc.NAMES)
def test_frontier_is_the_definition_on_the_table(g):
    for c in fc.group(g):
        cls, _ = fc.inputs(c.name)
        got = fc.twin(c.name)
        fc.holds(c, got["labels"], got["info"], got["stats"]._asdict())
        want = mf.brute(cls, c.params)
        fc.holds(c, want["labels"], want["info"], want["stats"]._asdict())
        assert same(got, want), (c.name, int((got["labels"] != want["labels"]).sum()), got["stats"], want["stats"])


def test_brute_without_scipy_is_the_same_flood_fill(monkeypatch):
    names = ("knife/corner-touch", "min-size/5", "late/u", "random/40x33x19-sparse")
    with_scipy = {n: mf.brute(fc.inputs(n)[0], fc.case(n).params) for n in names}
    monkeypatch.setitem(sys.modules, "scipy", None)                  # the import fails: the plain stack runs
    for n in names:
        assert same(mf.brute(fc.inputs(n)[0], fc.case(n).params), with_scipy[n]), n


def literal_costs(labels, R, cost):
    D, H, W = labels.shape
    best = [(mr.UNREACHED, (0, 0, 0))] * R
    for z in range(D):
        for y in range(H):
            for x in range(W):
                k = int(labels[z, y, x])
                if k < 0:
                    continue
                c = int(cost[z if cost.shape[0] == D else 0, y, x])
                if c < mr.BLOCKED and c < best[k][0]:                 # ascending linear index: the first voxel at the smallest cost stays
                    best[k] = (c, (x, y, z))
    return best


@pytest.mark.parametrize("g", fc.NAMES)
def test_costs_are_the_literal_loop(g):
    for c in fc.group(g):
        cls, grid = fc.inputs(c.name)
        got = fc.twin(c.name)
        d2 = md.transform(cls, c.dist)["d2"]
        cost = mr.field(cls, d2, grid, c.goal, c.route)["cost"]
        R = len(got["info"])
        k, ijk = mf.costs(got["labels"], R, cost)
        assert k.dtype == np.uint32 and ijk.dtype == np.int32 and k.shape == (R,) and ijk.shape == (R, 3), c.name
        assert [(int(a), tuple(int(v) for v in b)) for a, b in zip(k, ijk)] == literal_costs(got["labels"], R, cost), c.name
        fc.costs_hold(c, k, ijk)


def test_costs_refuse_a_field_of_another_shape():
    lab = np.full((2, 3, 4), mf.NONE, np.int32)
    with pytest.raises(ValueError):
        mf.costs(lab, 0, np.zeros((2, 3, 5), np.uint32))
    k, ijk = mf.costs(lab, 0, np.zeros((1, 3, 4), np.uint32))
    assert k.shape == (0,) and ijk.shape == (0, 3)


def test_voxel_list_is_ascending_and_complete():
    for name in ("min-size/5", "costs/planar", "random/40x33x19-sparse"):
        lab = fc.twin(name)["labels"]
        ijk, l = mf.voxel_list(lab)
        D, H, W = lab.shape
        lin = (ijk[:, 2].astype(np.int64) * H + ijk[:, 1]) * W + ijk[:, 0]
        assert ijk.dtype == np.int32 and l.dtype == np.int32 and (np.diff(lin) > 0).all() and np.array_equal(lin, np.flatnonzero(lab.ravel() != mf.NONE))
        assert np.array_equal(l, lab.ravel()[lin])


def test_check_params_refusals_and_defaults():
    assert mf.FrontierParams() == (1 << mo.FREE, 1 << mo.UNKNOWN, 1, 8, 0, 0x7fffffff) and (mf.REJECTED, mf.NONE) == (-1, -2) and mf.INFO_DTYPE.itemsize == 64
    bad = ((0, 1, 1, 8, 0, 1), (8, 1, 1, 8, 0, 1), (2, 0, 1, 8, 0, 1), (2, 9, 1, 8, 0, 1), (2, 2, 1, 8, 0, 1), (3, 1, 1, 8, 0, 1), (6, 5, 1, 8, 0, 1), (2.5, 1, 1, 8, 0, 1),
           (2, 1, 2, 8, 0, 1), (2, 1, -1, 8, 0, 1), (2, 1, 0.5, 8, 0, 1), (2, 1, 1, 0, 0, 1), (2, 1, 1, 2 ** 32, 0, 1), (2, 1, 1, 1.5, 0, 1), (2, 1, 1, 8, 2, 1),
           (2, 1, 1, 8, 0, 2 ** 31), (2, 1, 1, 8, -2 ** 31 - 1, 0), (2, 1, 1, 8, 0.5, 1))
    for p in bad:
        with pytest.raises(ValueError):
            mf.check_params(mf.FrontierParams(*p))
        for f in (mf.frontier, mf.brute, mf.mark):
            with pytest.raises(ValueError):
                f(np.zeros((1, 1, 1), np.uint8), p)
    for ok in ((1, 2, 0, 1, 0, 0), (6, 1, 1, 2 ** 32 - 1, -2 ** 31, 2 ** 31 - 1), (2, 5, 1, 8, 3, 3), (4, 3, 0, 1, -5, -5)):
        mf.check_params(mf.FrontierParams(*ok))
    with pytest.raises(ValueError):
        mf.frontier(np.zeros((2, 2), np.uint8))


def test_the_empty_grid():
    for f in (mf.frontier, mf.brute):
        r = f(np.zeros((0, 0, 0), np.uint8))
        assert r["labels"].shape == (0, 0, 0) and r["labels"].dtype == np.int32 and len(r["info"]) == 0 and r["stats"] == (0,) * 9
    k, ijk = mf.costs(np.zeros((0, 0, 0), np.int32), 0, np.zeros((0, 0, 0), np.uint32))
    assert len(k) == 0 and ijk.shape == (0, 3)


def test_centroid_in_metres():
    info = np.zeros(2, mf.INFO_DTYPE)
    info["size"] = [4, 1]; info["sum"] = [[6, 2, 0], [3, 4, 5]]
    c = mf.centroid(info)
    assert c.tolist() == [[1.5, 0.5, 0.0], [3.0, 4.0, 5.0]]
    grid = mo.OccupancyGrid((-0.6, 0.3, 0.9), 0.3, 4, 5, 6, (-2, 1, 3))
    assert np.allclose(mo.centres(c, grid), [[(-2 + 2.0) * 0.3, (1 + 1.0) * 0.3, (3 + 0.5) * 0.3], [(-2 + 3.5) * 0.3, (1 + 4.5) * 0.3, (3 + 5.5) * 0.3]], atol=1e-12)


@pytest.fixture(scope="module")
def street():
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    scans = [synth.lidar_scan(prims, SEN, T, sd) for T, sd in zip(POSES, [11, 12, 13, 14])]
    occ = mo.classify(scans, POSES)
    assert occ["classes"].shape == (14, 334, 344)
    return occ["classes"], occ["grid"]


def test_street_scene(street):
    """the four scans of the street scene under the default parameters: at least one region, frontier() = brute(); and with the planner's band"""
    cls, grid = street
    for params in (mf.FrontierParams(), mf.FrontierParams(iz_lo=4, iz_hi=8, min_size=20)):
        got = mf.frontier(cls, params)
        want = mf.brute(cls, params)
        print(params, got["stats"])
        assert same(got, want), (got["stats"], want["stats"])
        s = got["stats"]
        assert s.regions >= STREET_MIN_REGIONS and s.frontier > 1000 and s.largest == int(got["info"]["size"].max())
        assert np.isfinite(mo.centres(mf.centroid(got["info"]), grid)).all()
