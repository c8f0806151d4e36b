"""The seams of the 3 x 3 x 3 cell walk (csrc/qn_cell_walk.cuh) that the map's normals, the map's outlier filter and the two-way overlap share, on one
hand-made table all three run against, bit for bit against their numpy twins.

The walk reads a query's candidates as nine x-runs (the points in the cells x-1 .. x+1 of one (y, z)), four candidates a trip, its loads clamped to the last
finite record.  The table, for a radius r: on each of three y rows and two z layers, each r apart and so in adjacent cells, seven cluster places 3 r apart along
x (two or more empty cells between neighbours, so an x-run holds one cluster and nothing else) with 0, 1, 3, 4, 5, 8 and 9 points: x-runs that are empty,
shorter than a trip, exactly one and two trips, and one past each.  The order of the sizes along x turns with the variant, so that the run with the highest
cell key - the last finite records of the sorted order, where the clamp binds - has 9, 8 and 5 points; three non-finite records sit in the middle of the
cloud and are sorted behind it.  Singletons 4 r apart, at least four cells away from every cluster, pad the cloud to 255, 256 and 257 points: a launch of one
block that is one short, one that is full, and two blocks.

test_the_table_has_its_seams needs no GPU: it derives the runs from the twin's neighbour counts at r / 4 (a cluster is 0.1 r wide: the count of a point is
its cluster's size) and from the index's documented cell arithmetic (csrc/qn_kf_internal.h, the edge as csrc/qn_cloud.hip derives it)."""
import math
import numpy as np
import pytest
from qn_amd import mapnormals as mn, mapoutliers as mo, overlap as ov

R = 0.5
SIZES = (0, 1, 3, 4, 5, 8, 9)
TOTALS = (255, 256, 257)
F = np.float32
SHIFT = np.array([R / 2, 0.0, 0.0], F)                                           # the overlap case: the table against itself moved along x


def _table(variant):
    """-> the cloud (TOTALS[variant], 3) f32, and per point its cluster's size (0: a pad or a non-finite record)"""
    rng = np.random.default_rng(40 + variant)
    sizes = SIZES[len(SIZES) - variant:] + SIZES[:len(SIZES) - variant]          # the last place along x holds 9, 8, 5 points
    pts, size = [], []
    for k in range(2):
        for j in range(3):
            for i, s in enumerate(sizes):
                c = np.array([4.5 + 3 * i, 0.5 + j, 0.5 + k]) * R                # the middle of a cell; the origin (a pad) is the box's corner
                pts += list(c + rng.uniform(-0.05, 0.05, (s, 3)) * R); size += [s] * s
    n_pad = TOTALS[variant] - len(pts) - 3
    pads = [(0.0, 0.0, 0.0)] + [(4.0 * R * u, (8.0 + 4.0 * v) * R, 0.0) for v in range(9) for u in range(9)]
    pts += pads[:n_pad]; size += [0] * n_pad
    order = rng.permutation(len(pts))                                            # clusters and pads interleaved in the cloud's own order
    pts = np.array(pts)[order]; size = np.array(size)[order]
    bad = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf]])
    m = len(pts) // 2
    return np.concatenate([pts[:m], bad, pts[m:]]).astype(F), np.concatenate([size[:m], [0, 0, 0], size[m:]])


def _cells(pts, r):
    """the f32 cell coordinates the index gives the finite points of a cloud at radius r"""
    fin = pts[np.isfinite(pts).all(axis=1)]
    edge = (r + math.ldexp(float(np.abs(fin).max()), -21)) * (1.0 + 1e-5)
    inv = F(1.0) / F(edge)
    return (np.floor(fin * inv) - np.floor(fin.min(axis=0) * inv)).astype(np.int64), fin


@pytest.fixture(scope="module", params=range(3), ids=["n%d" % n for n in TOTALS])
def table(request):
    pts, size = _table(request.param)
    return request.param, pts, size


def test_the_table_has_its_seams(table):
    variant, pts, size = table
    fin_mask = np.isfinite(pts).all(axis=1)
    assert len(pts) == TOTALS[variant] and int((~fin_mask).sum()) == 3 and not fin_mask[(len(pts) - 3) // 2:][:3].any()
    # the twin's neighbour counts at r / 4: every point of a cluster counts exactly its cluster, every pad only itself
    count, _, _ = mn.moments(pts, R / 4)
    assert np.array_equal(count[fin_mask], np.maximum(size, 1)[fin_mask])
    # the runs: a cluster lies in one cell, alone in the five cells x-2 .. x+2 of its (y, z); the six (y, z) of the clusters are 3 x 2 adjacent cells
    cell, fin = _cells(pts, R)
    sz = size[fin_mask]
    runs = {}
    for c, s in zip(map(tuple, cell), sz):
        if s:
            runs.setdefault(c, []).append(s)
    assert all(len(v) == v[0] for v in runs.values()), "a cluster in more than one cell, or two in one"
    for c in runs:
        near = (cell[:, 1] == c[1]) & (cell[:, 2] == c[2]) & (np.abs(cell[:, 0] - c[0]) <= 2)
        assert int(near.sum()) == len(runs[c]), c
    rows = sorted({(c[2], c[1]) for c in runs})
    assert rows == [(z, y) for z in (0, 1) for y in (0, 1, 2)]
    for z, y in rows:
        xs = sorted(c[0] for c in runs if (c[2], c[1]) == (z, y))
        assert [len(runs[(x, y, z)]) for x in xs] == [s for s in SIZES[len(SIZES) - variant:] + SIZES[:len(SIZES) - variant] if s], (z, y)
        assert np.diff(xs).min() >= 3                                            # (the place with 0 points leaves a gap of 6: empty runs between populated ones)
    # the highest cell key of the cloud is the last cluster of the top row: the sorted order's finite part ends with that run
    div = cell.max(axis=0) + 1
    key = cell[:, 0] + div[0] * (cell[:, 1] + div[1] * cell[:, 2])
    assert int((key == key.max()).sum()) == (9, 8, 5)[variant] and sz[key == key.max()].min() == (9, 8, 5)[variant]
    # every pad is at least three cells from every other point on some axis: alone in its 27 cells
    for c in cell[sz == 0]:
        assert int((np.abs(cell - c).max(axis=1) <= 2).sum()) == 1
    # the overlap case's f64 sums are exact (257 f32 terms within 2^20 of each other), so they are compared bit for bit as well
    shifted = pts + SHIFT
    for a, b in ((pts, shifted), (shifted, pts)):
        d2 = ov.nearest(a, b, R)[0]
        d2 = d2[np.isfinite(d2)]
        assert len(d2) > 100 and d2.min() > 0 and d2.max() / d2.min() < 2.0 ** 20
        assert ov.record(a, ov.nearest(a, b, R)[0])["sum_d2"] == math.fsum(float(v) for v in d2)


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


@pytest.fixture(scope="module")
def as_map(store, table):
    """the table as the store's map slot (leaf 1e-4: the voxel grid's overflow guard passes the records through, the finite ones as they are, the others
    still non-finite and in their places) -> the map as the store downloads it, which is what the twins are given"""
    _, pts, _ = table
    n = store.build_map([store.add(pts)], [np.eye(4)], 1e-4)
    got = store.download_map(n)
    fin = np.isfinite(pts).all(axis=1)
    assert n == len(pts) and got[fin, :3].tobytes() == pts[fin].tobytes() and not np.isfinite(got[~fin, :3]).all(axis=1).any(), "the cloud did not pass through"
    return got


@pytest.mark.gpu
def test_map_normals_on_the_table(store, as_map):
    from qn_amd import engine
    views = np.array([[0.0, 0.0, 5.0], [8.0, 1.0, 5.0]])
    got = store.map_normals(engine.NormalParams(R, 3), views)
    s1, s2 = store.map_moments()
    want = mn.normals(as_map, (R, 3), views)
    assert int(want["count"].max()) >= 9
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
    assert np.array_equal(got["view_idx"], want["view_idx"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 9])
def test_map_outliers_on_the_table(store, as_map, k):
    from qn_amd import engine
    stats, cnt, mq, rm = store.map_outliers(engine.OutlierParams(R, 1.0, k))
    want = mo.classify(as_map, (R, 1.0, k))
    assert stats["dense"] == want["stats"].dense > 0 and stats["sparse"] == want["stats"].sparse > 0
    assert np.array_equal(cnt, want["count"]) and np.array_equal(mq, want["mean_q"]) and np.array_equal(rm, want["removed"])


@pytest.mark.gpu
def test_overlap_on_the_table(store, table):
    import torch
    _, pts, _ = table
    shifted = pts + SHIFT
    dev = [torch.from_numpy(np.concatenate([c, np.ones((len(c), 1), F)], axis=1)).cuda() for c in (pts, shifted)]
    rec, = store.overlap_batch([(dev[0].data_ptr(), len(pts), dev[1].data_ptr(), len(shifted))], R)
    assert rec["status"] == 0
    for d, key, a, b in ((0, "a_to_b", pts, shifted), (1, "b_to_a", shifted, pts)):
        want = ov.direction(a, b, R, points=True)
        d2, idx = store.overlap_points(0, d)
        assert np.array_equal(d2.view(np.uint32), want["nn_d2"].view(np.uint32)) and np.array_equal(idx, want["nn_idx"]), key
        assert (rec[key]["n"], rec[key]["n_finite"], rec[key]["inliers"]) == (want["n"], want["n_finite"], want["inliers"]) and want["inliers"] > 100, key
        assert rec[key]["sum_d2"] == want["sum_d2"], key
