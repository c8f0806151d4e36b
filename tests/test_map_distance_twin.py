"""The numpy twin of the occupancy map's distance field (qn_amd/mapdistance.py) against the definition: its windowed separable transform() equals its brute()
- every voxel against every site - byte for byte on the case table of tests/distance_cases.py, and both meet what the construction of each case determines.
Then the statistics identities, slice2d and query against direct indexing, query's outside, non-finite and 2^20 points, the refusals of check_params, inflate
and metres; with scipy, its exact Euclidean transform too.  No GPU."""
import numpy as np
import pytest
import distance_cases as dc
from qn_amd import mapdistance as md, mapoccupancy as mo


def _stats(r):
    return r["stats"]._asdict()


@pytest.mark.parametrize("g", dc.NAMES)
def test_transform_is_the_definition_on_the_table(g):
    for c in dc.group(g):
        occ = dc.occupancy(c.name)
        cls = occ["classes"]
        assert cls.shape == c.sides[::-1], (c.name, cls.shape)
        got = md.transform(cls, c.params)
        dc.holds(c, got["d2"], _stats(got))
        assert c.voxels <= dc.SLICE_CAP or "full" in c.expect      # (brute() is voxels x sites: the large case of fold-seams, nearly all sites, states its whole field)
        if c.voxels <= dc.SLICE_CAP:
            want = md.brute(cls, c.params)
            assert got["d2"].tobytes() == want["d2"].tobytes() and got["stats"] == want["stats"], (c.name, int((got["d2"] != want["d2"]).sum()))
        assert got["stats"] == md.stats_of(got["d2"], c.params.max_dist)


@pytest.mark.parametrize("g", ["knife-edge", "wide-window", "fan", "random", "lines-z"])
def test_slices_and_queries_are_direct_indexing(g):
    for c in dc.group(g)[-4:]:
        occ = dc.occupancy(c.name)
        cls, grid = occ["classes"], occ["grid"]
        d2 = md.transform(cls, c.params)["d2"]
        D = grid.depth
        for lo, hi in dc.slice_ranges(D):
            s = md.slice2d(d2, lo, hi)
            a, b = max(lo, 0), min(hi, D - 1)
            want = np.full(d2.shape[1:], md.FAR, np.uint16)
            for z in range(a, b + 1):
                want = np.minimum(want, d2[z])
            assert s.dtype == np.uint16 and np.array_equal(s, want), (c.name, lo, hi)
        xyz, first_outside = dc.query_points(grid)
        qd, qc = md.query(d2, cls, grid, xyz)
        assert qd.dtype == np.uint16 and qc.dtype == np.uint8 and len(qd) == len(qc) == len(xyz)
        assert (qd[first_outside:] == md.FAR).all() and (qc[first_outside:] == md.OUTSIDE).all(), c.name
        inside = np.floor(xyz[:first_outside] / grid.voxel).astype(np.int64) - np.asarray(grid.minc)      # (voxel 1: exact)
        assert np.array_equal(qd[:first_outside], d2[inside[:, 2], inside[:, 1], inside[:, 0]]), c.name
        assert np.array_equal(qc[:first_outside], cls[inside[:, 2], inside[:, 1], inside[:, 0]]), c.name


def test_slice_refuses_a_reversed_band():
    with pytest.raises(ValueError):
        md.slice2d(np.zeros((2, 2, 2), np.uint16), 1, 0)


def test_query_quantises_like_the_occupancy_map():
    """voxel 0.3 and a grid that starts at voxel -1: -0.3 * (1 / 0.3) * 1024 rounds to -1024, so -0.3 is in voxel -1, grid index 0; 0.0 is in index 1"""
    grid = mo.OccupancyGrid((-0.3, -0.3, -0.3), 0.3, 3, 2, 2, (-1, -1, -1))
    cls = np.arange(12, dtype=np.uint8).reshape(2, 2, 3) % 3
    d2 = (np.arange(12, dtype=np.uint16) * 7).reshape(2, 2, 3)
    xyz = np.array([[-0.3, -0.3, -0.3], [0.0, 0.0, 0.0], [0.45, 0.1, -0.01], [0.6, 0.0, 0.0], [-0.31, 0.0, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, np.nan],
                    [0.3 * 2.0 ** 20, 0.0, 0.0], [-np.inf, 0.0, 0.0]])
    qd, qc = md.query(d2, cls, grid, xyz)
    assert qd.tolist() == [0, 7 * (6 + 3 + 1), 7 * (0 + 3 + 2), md.FAR, md.FAR, md.FAR, md.FAR, md.FAR, md.FAR]
    assert qc.tolist() == [0, 10 % 3, 5 % 3] + [md.OUTSIDE] * 6
    qd, qc = md.query(d2[:0], cls[:0], mo.OccupancyGrid((0.0, 0.0, 0.0), 0.3, 0, 0, 0, (0, 0, 0)), xyz[:2])
    assert qd.tolist() == [md.FAR] * 2 and qc.tolist() == [md.OUTSIDE] * 2


def test_check_params_refusals_and_defaults():
    assert md.DistanceParams() == (1 << mo.OCCUPIED, 16) and md.FAR == 0xffff and md.OUTSIDE == 0xff and md.MAX_RADIUS == 255
    for bad in ((0, 16), (8, 16), (9, 16), (1.5, 16), (4, 0), (4, 256), (4, 2.5), (-1, 3)):
        with pytest.raises(ValueError):
            md.check_params(md.DistanceParams(*bad))
        with pytest.raises(ValueError):
            md.transform(np.zeros((1, 1, 1), np.uint8), bad)
    for ok in ((1, 1), (7, 255), (4, 16), (5, 64)):
        md.check_params(md.DistanceParams(*ok))
    with pytest.raises(ValueError):
        md.transform(np.zeros((2, 2), np.uint8))


def test_the_empty_grid():
    r = md.transform(np.zeros((0, 0, 0), np.uint8))
    assert r["d2"].shape == (0, 0, 0) and r["d2"].dtype == np.uint16 and r["stats"] == (0, 0, 0, 0, 0)
    assert md.slice2d(r["d2"], 0, 3).shape == (0, 0)


def test_inflate_and_metres():
    occ = np.array([[0, 1, 2, 1], [1, 1, 0, 0]], np.uint8)
    d2 = np.array([[9, 4, 0, 1], [md.FAR, 5, 10, 3]], np.uint16)
    assert md.inflate(occ, d2, 4).tolist() == [[0, 2, 2, 2], [1, 1, 0, 2]]
    assert md.inflate(occ, d2, 0).tolist() == [[0, 1, 2, 1], [1, 1, 0, 0]]
    assert md.inflate(occ, d2, 10 ** 9).tolist() == [[2, 2, 2, 2], [1, 2, 2, 2]]                  # FAR is never inflated
    assert md.inflate(occ, d2, 4).dtype == np.uint8
    with pytest.raises(ValueError):
        md.inflate(occ, d2[:1], 4)
    m = md.metres(d2, 0.5)
    assert m.dtype == np.float64 and m[0].tolist() == [1.5, 1.0, 0.0, 0.5] and np.isinf(m[1, 0]) and m[1, 1] == np.sqrt(5.0) * 0.5


def test_scipy_agrees_where_it_applies():
    """rint(edt^2), capped, equals transform on the cases that have both a site and a voxel that is none (scipy's transform needs a background)"""
    ndi = pytest.importorskip("scipy.ndimage")
    seen = 0
    for c in dc.all_cases():
        cls = dc.occupancy(c.name)["classes"]
        site = md.sites_of(cls, c.params.site_mask)
        if not site.any() or site.all():
            continue
        e2 = np.rint(ndi.distance_transform_edt(~site) ** 2).astype(np.int64)
        want = np.where(e2 > c.params.max_dist ** 2, md.FAR, e2).astype(np.uint16)
        assert np.array_equal(md.transform(cls, c.params)["d2"], want), c.name
        seen += 1
    assert seen > 100
