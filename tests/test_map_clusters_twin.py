"""The specification of the map's clusters, qn_amd/mapclusters.py, on its own: against scipy (cKDTree.query_pairs in f64 plus csgraph.connected_components) on
seeded random clouds for which no pair lies within a relative 1e-5 of the tolerance, so the f32 and the f64 distances agree on every pair; and on hand-made
clouds whose answers are worked out by hand.  The clouds and their hand-made answers (the case_* / check_* functions) are what tests/test_gpu_map_clusters.py
runs on the GPU as well.  No GPU needed."""
import math
import numpy as np
import pytest
from qn_amd import mapclusters as mc

F = np.float32
UP = np.nextafter(F(0.5), F(1))


# ---- hand-made clouds: case_*() -> (points (n, 3) f32, params), check_*(result) asserts the answers worked out by hand on a classify() result
def case_line(n=3000, tol=0.5, opened=None, seed=11):
    """n points at 0.9 tol spacing along a snake on a lattice (rows of 60 points in x, five steps in y between them, z rising by 0.6 m over the line so the
    cloud spans every axis): lattice neighbours that are not consecutive on the line are at least sqrt 2 steps apart, beyond the tolerance, so the graph is the
    path itself.  The map order is shuffled with index 0 in the middle of the line.  opened = k: everything behind position k moves along the line so that
    the link k - k + 1 is the next f32 beyond the tolerance.  -> (points, params, position of every map index on the line)"""
    h = 0.9 * tol
    pos = np.zeros((n, 3))
    x = y = 0; d = 1
    for k in range(n):
        pos[k] = (x * h, y * h, 0.6 * k / n)
        r = k % 64
        if r < 59:
            x += d
        else:
            y += 1
            if r == 63:
                d = -d
    pts = pos.astype(np.float32)
    if opened is not None:
        k = opened
        assert k % 64 < 58                                           # inside a row
        step = np.sign(pts[k + 1, 0] - pts[k, 0])
        gap = np.nextafter(F(tol), F(np.inf))
        pts[k + 1:, 0] += (pts[k, 0] + F(step) * gap) - pts[k + 1, 0]
        dd = pts[k + 1] - pts[k]
        assert (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2] > F(tol * tol)
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)                                       # order[i] = the line position of map index i
    j = int(np.flatnonzero(order == n // 2)[0])
    order[[0, j]] = order[[j, 0]]
    return pts[order], (tol, 1, 0xffffffff, 0), order


def check_line(r, order, opened=None):
    n = len(order)
    s = r["stats"]
    assert order[0] == n // 2
    if opened is None:
        assert (s.components, s.clusters, s.largest, s.edges, s.members) == (1, 1, n, n - 1, n)
        assert (r["root"] == 0).all() and (r["size"] == n).all() and (r["label"] == 0).all()
        return
    first = order <= opened
    r0, r1 = int(np.flatnonzero(first)[0]), int(np.flatnonzero(~first)[0])
    assert (s.components, s.clusters, s.edges, s.largest) == (2, 2, n - 2, max(opened + 1, n - opened - 1))
    assert (r["root"][first] == r0).all() and (r["root"][~first] == r1).all()
    assert (r["size"][first] == opened + 1).all() and (r["size"][~first] == n - opened - 1).all()
    assert (r["label"][first] == (0 if r0 < r1 else 1)).all() and (r["label"][~first] == (1 if r0 < r1 else 0)).all()


def case_knife_edge():
    """tolerance 0.5, r2 = 0.25: a partner at exactly 0.5 joins, one at the next f32 does not"""
    assert F(0.5) * F(0.5) == F(0.5 * 0.5) and UP * UP > F(0.25)
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [-UP, 0, 0], [0, 0.5, 0], [0, -UP, 0], [0, 0, -0.5], [0, 0, UP], [0.25, 0, 0]], np.float32)
    return pts, (0.5, 1, 0xffffffff, 0)


def check_knife_edge(r):
    # by hand: 0 joins 1, 3, 5 (exactly on the radius) and 7; 1 joins 7; 2, 4 and 6 are one f32 beyond 0 and further from everything else
    s = r["stats"]
    assert (s.components, s.clusters, s.edges, s.largest, s.too_small, s.too_large) == (4, 4, 5, 5, 0, 0)
    assert list(r["root"]) == [0, 0, 2, 0, 4, 0, 6, 0] and list(r["size"]) == [5, 5, 1, 5, 1, 5, 1, 5] and list(r["label"]) == [0, 0, 1, 0, 2, 0, 3, 0]
    assert list(r["clusters"]["root"]) == [0, 2, 4, 6] and list(r["clusters"]["size"]) == [5, 1, 1, 1]


def case_lattice_on_the_radius():
    """the lattice of tests/test_gpu_map_outliers.py: h = float32(0.3), 4 fl(h h) == float32(0.6 * 0.6), partners two steps away exactly ON the radius; five
    9 x 9 layers four steps apart"""
    h = F(0.3)
    assert F(4) * (h * h) == F(0.6 * 0.6)
    k = np.arange(-4, 5).astype(np.float32) * h
    x, y = np.meshgrid(k, k, indexing="ij")
    lat = np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, F(l) * h, np.float32)], axis=1) for l in (-8, -4, 0, 4, 8)]).astype(np.float32)
    return lat, (0.6, 81, 81, 0)


def check_lattice_on_the_radius(r):
    # by hand, per layer: offsets (1, 0) 2 x 72, (1, 1) 2 x 64, (2, 0) 2 x 63 = 398 joined pairs, the 126 at two steps exactly on the radius
    s = r["stats"]
    assert (s.components, s.clusters, s.edges, s.largest) == (5, 5, 5 * 398, 81)
    assert np.array_equal(r["root"], np.repeat(np.arange(5) * 81, 81)) and np.array_equal(r["label"], np.repeat(np.arange(5), 81))


def case_duplicates():
    """twelve copies of one point, three of another, and four corners that make the cloud span every axis"""
    pts = np.array([[1, 1, 1]] * 5 + [[3, 0, 0]] + [[1, 1, 1]] * 7 + [[0, 0, 0], [4, 4, 2]] + [[2, 3, 1]] * 3 + [[4, 0, 2]], np.float32)
    return pts, (0.25, 3, 12, 0)


def check_duplicates(r):
    s = r["stats"]
    assert (s.components, s.clusters, s.too_small, s.too_large, s.edges, s.largest) == (6, 2, 4, 0, 66 + 3, 12)
    assert list(r["label"]) == [0] * 5 + [-1] + [0] * 7 + [-1, -1] + [1] * 3 + [-1]
    assert list(r["root"]) == [0] * 5 + [5] + [0] * 7 + [13, 14] + [15] * 3 + [18]
    c = r["clusters"]
    assert list(c["size"]) == [12, 3] and np.array_equal(c["lo"], c["hi"]) and np.array_equal(c["lo"], np.array([[1, 1, 1], [2, 3, 1]], np.float32))
    assert np.array_equal(c["sum_q"], np.array([[12 << 12] * 3, [6 << 12, 9 << 12, 3 << 12]]))      # e = 12: 0.25 * 2^12 = 2^10


def case_size_seams(min_size=4, max_size=7):
    """isolated clumps of min_size - 1, min_size, max_size and max_size + 1 points (0.1 m apart on a line, the clumps 3 m apart), their points dealt out in turn
    so that every clump is spread over the map order"""
    sizes = [min_size - 1, min_size, max_size, max_size + 1]
    rows = []
    for j in range(max(sizes)):
        for c, m in enumerate(sizes):
            if j < m:
                rows.append((3.0 * c, 0.1 * j, 0.7 * c, c))
    a = np.array(rows)
    return a[:, :3].astype(np.float32), (0.15, min_size, max_size, 0), a[:, 3].astype(int), sizes


def check_size_seams(r, clump, sizes):
    s = r["stats"]
    assert (s.components, s.clusters, s.too_small, s.too_large, s.largest) == (4, 2, 1, 1, sizes[3])
    assert (s.clustered_points, s.rejected_points, s.edges) == (sizes[1] + sizes[2], sizes[0] + sizes[3], sum(sizes) - 4)
    assert np.array_equal(r["label"], np.array([-1, 0, 1, -1])[clump]) and np.array_equal(r["size"], np.array(sizes)[clump])
    assert np.array_equal(r["root"], clump)                             # the first four records are the clumps' first points


def case_numbering(pairs=700, seed=5):
    """isolated pairs on a 2 m grid, the partner 0.2 m beside: the first points of all pairs in a shuffled order, then the second points in another one, so map
    order and spatial order disagree and the roots are the indices 0 .. pairs - 1"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(28), np.arange(25), indexing="ij"), axis=-1).reshape(-1, 2)[:pairs]
    base = np.concatenate([g * 2.0, (g[:, :1] % 3) * 0.5], axis=1)
    a, b = rng.permutation(pairs), rng.permutation(pairs)
    pts = np.concatenate([base[a], base[b] + [0.2, 0.0, 0.0]]).astype(np.float32)
    inv = np.empty(pairs, np.int64); inv[a] = np.arange(pairs)
    return pts, (0.3, 2, 2, 0), np.concatenate([np.arange(pairs), inv[b]])


def check_numbering(r, pair):
    m = len(pair) // 2
    s = r["stats"]
    assert (s.components, s.clusters, s.edges, s.largest, s.rejected_points) == (m, m, m, 2, 0)
    assert np.array_equal(r["root"], pair) and np.array_equal(r["label"], pair) and (r["size"] == 2).all()      # the cluster's number is its root's rank: the root
    assert np.array_equal(r["clusters"]["root"], np.arange(m))


def case_blob(seed=3):
    """one dense blob of 32 x 32 x 20 = 20480 points: a lattice of spacing 0.2 m, every point moved by at most 0.03 m on every axis, in a shuffled order - axis
    neighbours are at most sqrt(0.26^2 + 2 0.06^2) = 0.274 m apart, within the tolerance 0.3, so the blob is one component by construction"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(20), indexing="ij"), axis=-1).reshape(-1, 3)
    a = g * 0.2 + rng.uniform(-0.03, 0.03, g.shape) - [3.0, 1.0, 0.5]
    return a[rng.permutation(len(a))].astype(np.float32), (0.3, 10, 0xffffffff, 0)


def check_blob(r, pts):
    n = len(pts)
    s = r["stats"]
    assert (s.components, s.clusters, s.largest, s.clustered_points, s.quant_exp) == (1, 1, n, n, 11)
    c = r["clusters"]
    assert len(c) == 1 and c["root"][0] == 0 and c["size"][0] == n
    assert np.array_equal(c["lo"][0], pts.min(axis=0)) and np.array_equal(c["hi"][0], pts.max(axis=0))
    assert np.array_equal(c["sum_q"][0], np.rint(pts.astype(np.float64) * 2048.0).astype(np.int64).sum(axis=0))


def case_signed_zeros():
    """three clusters at a box face: the first has x in {+0, -0, 0.1, 0.2} - its low face is -0; the second x in {-0.1, -0, +0} - its high face is +0; the
    third y in {-0, +0, 0.1} and z in {+0, +0, -0}.  (Wherever a coordinate is -0 the other two of the record are > 0 or +0: such a record survives a
    transform whose zero entries are all -0, which is how the GPU test brings it into the map slot.)"""
    pts = np.array([[0.0, 0, 0], [-0.0, 0.1, 0], [0.1, 0.1, 0], [0.2, 0, 0.1],
                    [-0.1, 3, 1], [-0.0, 3, 1], [0.0, 3.1, 1], [3, -0.0, 0.0], [3.1, 0.0, 0.0], [3, 0.1, -0.0]], np.float32)
    return pts, (0.2, 3, 0xffffffff, 0)


def check_signed_zeros(r):
    c = r["clusters"]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert list(r["label"]) == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert bits(c["lo"][0])[0] == 0x80000000 and bits(c["hi"][0])[0] == bits(F(0.2))          # -0 is the low face
    assert bits(c["hi"][1])[0] == 0x00000000 and bits(c["lo"][1])[0] == bits(F(-0.1))         # +0 is the high face
    assert bits(c["lo"][2])[1] == 0x80000000 and bits(c["hi"][2])[1] == bits(F(0.1)) and bits(c["lo"][2])[2] == 0x80000000 and bits(c["hi"][2])[2] == 0
    q = lambda v: int(np.rint(np.float64(F(v)) * 4096))
    assert list(c["sum_q"][0]) == [q(0.1) + q(0.2), 2 * q(0.1), q(0.1)]


def case_non_finite(seed=5):
    rng = np.random.default_rng(seed)
    a = np.zeros((1500, 3), np.float32); a[:, :2] = rng.uniform(-5, 5, (1500, 2)); a[:, 2] = 0.1 * np.sin(a[:, 0]) + rng.normal(0, 0.01, 1500)
    a[[5, 77, 901, 1499]] = [[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf], [np.nan, np.nan, np.nan]]
    return a, (0.3, 5, 0xffffffff, 0)


def check_non_finite(r, pts):
    bad = ~np.isfinite(pts[:, :3]).all(axis=1)
    s = r["stats"]
    assert bad.sum() == 4 and (s.n, s.n_finite, s.members) == (1500, 1496, 1496)
    assert (r["label"][bad] == mc.NONE).all() and (r["root"][bad] == mc.NO_ROOT).all() and (r["size"][bad] == 0).all()
    assert (r["label"][~bad] != mc.NONE).all() and s.clusters >= 1 and s.too_small >= 1


# ---- the twin against scipy
def _scipy_components(a, tol):
    from scipy.spatial import cKDTree
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(a)
    tree = cKDTree(a.astype(np.float64))
    pr = tree.query_pairs(tol, output_type="ndarray")
    wide = tree.query_pairs(tol * (1 + 1e-5), output_type="ndarray"); narrow = tree.query_pairs(tol * (1 - 1e-5), output_type="ndarray")
    k, lab = connected_components(coo_matrix((np.ones(len(pr)), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    low = np.full(k, n); np.minimum.at(low, lab, np.arange(n))
    return len(pr), len(wide) - len(narrow), low[lab], np.bincount(lab, minlength=k)[lab]


@pytest.mark.parametrize("seed,n,extent,tol", [(0, 10000, (20.0, 20.0, 4.0), 0.4), (2, 10000, (20.0, 20.0, 4.0), 0.4), (1, 6000, (8.0, 8.0, 3.0), 0.25),
                                                (3, 4000, (30.0, 3.0, 3.0), 0.5), (4, 777, (3.0, 3.0, 3.0), 0.3)])
def test_the_twin_against_scipy(seed, n, extent, tol):
    rng = np.random.default_rng(seed)
    a = (rng.uniform(0.0, 1.0, (n, 3)) * extent - [1.0, 2.0, 0.5]).astype(np.float32)
    a[rng.choice(n, n // 10, replace=False)] += F(50.0)              # a second, sparser part far away: negative and positive cells
    edges, near, root, size = _scipy_components(a, tol)
    assert near == 0, "a pair within 1e-5 of the tolerance: pick another seed"
    p = (tol, 3, 40, 0)
    r = mc.classify(a, p)
    s = r["stats"]
    assert s.edges == edges and np.array_equal(r["root"], root) and np.array_equal(r["size"], size)
    roots = np.flatnonzero(root == np.arange(n))
    kept = roots[(size[roots] >= 3) & (size[roots] <= 40)]
    want = np.full(n, mc.REJECTED); want[np.isin(root, kept)] = np.searchsorted(kept, root[np.isin(root, kept)])
    assert np.array_equal(r["label"], want) and r["label"].dtype == np.int32 and r["root"].dtype == np.uint32 and r["size"].dtype == np.uint32
    assert (s.n, s.n_finite, s.members, s.components, s.clusters) == (n, n, n, len(roots), len(kept))
    assert (s.too_small, s.too_large, s.largest) == (int((size[roots] < 3).sum()), int((size[roots] > 40).sum()), int(size.max()))
    assert (s.clustered_points, s.rejected_points) == (int((want >= 0).sum()), int((want < 0).sum())) and s.components > 100 and s.clusters > 10
    c = r["clusters"]
    e = mc.quant_exponent(tol)
    assert s.quant_exp == e and tol * 2.0 ** e <= 1024 < tol * 2.0 ** (e + 1)
    for j in (0, len(kept) // 2, len(kept) - 1):
        m = a[r["label"] == j]
        assert c["root"][j] == kept[j] and c["size"][j] == len(m) and np.array_equal(c["lo"][j], m.min(axis=0)) and np.array_equal(c["hi"][j], m.max(axis=0))
        assert np.array_equal(c["sum_q"][j], np.rint(m.astype(np.float64) * 2.0 ** e).astype(np.int64).sum(axis=0))
        assert np.allclose(r["centroid"][j], m.astype(np.float64).mean(axis=0), atol=2.0 ** -e)


def test_the_class_mask_selects_the_members():
    pts = case_line(600)[0]
    cls = (np.arange(600) % 5).astype(np.uint8)
    r = mc.classify(pts, (0.5, 1, 0xffffffff, 0b01100), cls)
    mem = (cls == 2) | (cls == 3)
    assert r["stats"].members == mem.sum() and (r["label"][~mem] == mc.NONE).all() and (r["root"][~mem] == mc.NO_ROOT).all() and (r["label"][mem] >= 0).all()
    sub = mc.classify(pts[mem], (0.5, 1, 0xffffffff, 0))
    idx = np.flatnonzero(mem)
    assert np.array_equal(r["root"][mem], idx[sub["root"]]) and np.array_equal(r["size"][mem], sub["size"]) and np.array_equal(r["label"][mem], sub["label"])
    assert np.array_equal(r["clusters"]["root"], idx[sub["clusters"]["root"]])
    for f in ("size", "lo", "hi", "sum_q"):
        assert np.array_equal(r["clusters"][f], sub["clusters"][f]), f
    with pytest.raises(ValueError):
        mc.classify(pts, (0.5, 1, 0xffffffff, 4))                    # a mask without classes


def test_hand_made_cases():
    pts, p, order = case_line()
    check_line(mc.classify(pts, p), order)
    pts, p, order = case_line(opened=1310)
    check_line(mc.classify(pts, p), order, 1310)
    pts, p = case_knife_edge(); check_knife_edge(mc.classify(pts, p))
    pts, p = case_lattice_on_the_radius(); check_lattice_on_the_radius(mc.classify(pts, p))
    pts, p = case_duplicates(); check_duplicates(mc.classify(pts, p))
    pts, p, clump, sizes = case_size_seams(); check_size_seams(mc.classify(pts, p), clump, sizes)
    pts, p, pair = case_numbering(); check_numbering(mc.classify(pts, p), pair)
    pts, p = case_blob(); check_blob(mc.classify(pts, p), pts)
    pts, p = case_non_finite(); check_non_finite(mc.classify(pts, p), pts)


def test_the_box_order_of_signed_zeros():
    pts, p = case_signed_zeros()
    check_signed_zeros(mc.classify(pts, p))
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    o = mc.ordered(x)
    assert (np.diff(o.astype(np.int64)) > 0).all() and np.array_equal(mc.unordered(o).view(np.uint32), x.view(np.uint32))


def test_drop_rejected_keeps_the_order_and_every_byte():
    pts, p, clump, sizes = case_size_seams()
    rec = np.concatenate([pts, np.arange(len(pts), dtype=np.float32)[:, None] + 0.5], axis=1)
    rec[3, 3] = np.nan                                               # an intensity is carried along whatever it is
    kept = mc.drop_rejected(rec, p)
    keep = np.isin(clump, (1, 2))
    assert kept.dtype == rec.dtype and kept.tobytes() == np.ascontiguousarray(rec[keep]).tobytes()
    a, p = case_non_finite()
    r = mc.classify(a, p)
    kept = mc.drop_rejected(a, p)
    assert kept.tobytes() == np.ascontiguousarray(a[r["label"] != mc.REJECTED]).tobytes() and (~np.isfinite(kept).all(axis=1)).sum() == 4      # non-members stay


def test_parameters_are_checked():
    pts, _ = case_knife_edge()
    for bad in [(0.0, 1, 2, 0), (-1.0, 1, 2, 0), (float("nan"), 1, 2, 0), (float("inf"), 1, 2, 0), (0.5, 0, 2, 0), (0.5, 3, 2, 0), (0.5, 1, 2, 32), (0.5, 1, 2 ** 32, 0),
                (0.5, 1.5, 2, 0)]:
        with pytest.raises(ValueError):
            mc.classify(pts, bad)
    with pytest.raises(mc.CapacityError):
        mc.classify(np.array([[2.0 ** 20, 0, 0], [0, 0, 0]], np.float32), (0.5, 1, 2, 0))       # e = 11: 2^20 * 2^11 = 2^31
    assert mc.classify(np.array([[np.nextafter(F(2.0 ** 20), F(0)), 0, 0]], np.float32), (0.5, 1, 2, 0))["stats"].clusters == 1
    assert [mc.quant_exponent(t) for t in (0.5, 0.3, 1.0, 1.5, 1024.0, 2.0 ** -140)] == [11, 11, 10, 9, 0, 127]
    assert math.ldexp(0.5, 11) == 1024
