"""The specification of the map normals, qn_amd/mapnormals.py, against brute force and against geometry whose answer is known by hand.  No GPU.
The lattices have the spacing h = float32(0.3) and indices in [-4, 4]: every coordinate k h and every difference of up to two steps is exact in f32, and
4 fl(h h) == float32(0.6 * 0.6) bit for bit, so the partners two steps away sit exactly ON the radius and only an inclusive <= counts them."""
import math
import numpy as np
import pytest
from qn_amd import mapnormals as mn, overlap

H = np.float32(0.3)
TOL = 2.0 ** -22


def lattice(lo, hi, z=0.0):
    k = np.arange(lo, hi + 1).astype(np.float32) * H
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, np.float32(z))], axis=1).astype(np.float32)


def test_the_lattice_sits_on_the_knife_edge():
    assert np.float32(4) * (H * H) == overlap.radius2(0.6)
    k = np.arange(-4, 5).astype(np.float32) * H
    assert all(float(k[i + 2] - k[i]) == float(np.float32(2) * H) for i in range(7))


def test_plane_lattice_counts_the_partners_on_the_radius():
    pts = lattice(-4, 4)
    r = mn.normals(pts, (0.6, 5), viewpoints=[[0.0, 0.0, 5.0]])
    idx = np.arange(-4, 5)
    ii, jj = np.meshgrid(idx, idx, indexing="ij")
    ii = ii.ravel(); jj = jj.ravel()
    # by hand: the lattice offsets (a, b) with a^2 + b^2 <= 4 that stay inside the 9 x 9 lattice - 13 for an interior point, four of them ON the radius
    offs = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if a * a + b * b <= 4]
    assert len(offs) == 13
    want = np.array([sum(1 for a, b in offs if abs(i + a) <= 4 and abs(j + b) <= 4) for i, j in zip(ii, jj)])
    assert np.array_equal(r["count"], want)
    inner = (np.abs(ii) <= 2) & (np.abs(jj) <= 2)
    assert (r["count"][inner] == 13).all() and (r["s1"][inner] == 0).all()
    assert np.array_equal(r["normals"], np.tile(np.float32([0, 0, 1]), (81, 1)))          # a corner has 6 neighbours: every point is valid
    assert (r["curvature"] == 0).all()
    assert (r["s2"][:, [2, 4, 5]] == 0).all()                                              # nothing leaves the plane
    # the exclusive comparison would lose the four partners on the radius
    assert (overlap.sqdist3_block(pts[40:41], pts)[0] < overlap.radius2(0.6)).sum() == 9


def test_inclined_plane_has_its_known_normal():
    rng = np.random.default_rng(1)
    nrm = np.array([1.0, 2.0, 2.0]) / 3.0
    u = np.array([2.0, -1.0, 0.0]) / math.sqrt(5.0); v = np.cross(nrm, u)
    ab = rng.uniform(-1.5, 1.5, (600, 2))
    pts = (ab[:, :1] * u + ab[:, 1:] * v + np.array([3.0, -2.0, 1.0])).astype(np.float32)
    r = mn.normals(pts, (0.6, 5), viewpoints=[np.array([3.0, -2.0, 1.0]) + 10.0 * nrm])
    ok = np.isfinite(r["curvature"])
    assert ok.sum() >= 590
    # the points are on the plane to f32 rounding of coordinates of size 4 (2^-22 each): the normal to about 2^-22 / 0.3
    assert np.abs(r["normals"][ok] - nrm.astype(np.float32)).max() < 1e-5
    assert r["curvature"][ok].max() < 1e-10
    back = mn.normals(pts, (0.6, 5), viewpoints=[np.array([3.0, -2.0, 1.0]) - 10.0 * nrm])
    assert np.array_equal(back["normals"][ok], -r["normals"][ok])


def test_sphere_patch_curvature_grows_with_the_radius():
    rng = np.random.default_rng(2)
    d = rng.normal(size=(6000, 3)); d[:, 2] = np.abs(d[:, 2]) + 1.5
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([[[0.0, 0.0, 2.0]], 2.0 * d]).astype(np.float32)                     # point 0: the pole of a sphere of radius 2
    curv = []
    for rad in (0.3, 0.6, 0.9):
        r = mn.normals(pts, (rad, 5), viewpoints=[[0.0, 0.0, 10.0]])
        assert r["count"][0] >= 20 and abs(float(r["normals"][0, 2])) > 0.99
        curv.append(float(r["curvature"][0]))
    assert 0.0 < curv[0] < curv[1] < curv[2]


def test_collinear_points_are_nan_or_fall_to_the_gap_rule():
    t = np.linspace(-2.0, 2.0, 41)
    pts = (t[:, None] * np.array([1.0, 2.0, -0.5])[None, :] / 2.29).astype(np.float32)
    r = mn.normals(pts, (0.6, 5))
    valid = np.isfinite(r["curvature"])
    assert (r["count"] >= 5).all()
    assert (r["gap"][valid] < 1e-3).all()                                                    # no normal here is one to compare
    same = np.tile(np.float32([[1, 2, 3]]), (7, 1))
    r = mn.normals(same, (0.6, 5))
    assert (r["count"] == 7).all() and np.isnan(r["normals"]).all() and np.isnan(r["curvature"]).all()      # the trace is 0


def test_min_neighbors_cut():
    pts = lattice(-4, 4)
    r = mn.normals(pts, (0.6, 7))
    assert np.array_equal(np.isnan(r["curvature"]), r["count"] < 7) and (r["count"] < 7).sum() == 4          # the four corners have 6
    assert np.array_equal(np.isnan(r["normals"]).all(axis=1), r["count"] < 7)
    with pytest.raises(ValueError):
        mn.normals(pts, (0.6, 2))


def test_orientation_by_viewpoint_and_without():
    pts = lattice(-4, 4)
    up = mn.normals(pts, (0.6, 5), viewpoints=[[0, 0, 1.0], [0, 0, -1.0]])
    # x = y = 0 is equally far from both viewpoints: the lowest index wins, whichever side it is on
    centre = 40
    assert up["view_idx"][centre] == 0 and (up["view_idx"] == 0).all()
    assert (up["normals"][:, 2] == 1).all()
    down = mn.normals(pts, (0.6, 5), viewpoints=[[0, 0, -1.0], [0, 0, 1.0]])
    assert (down["view_idx"] == 0).all() and (down["normals"][:, 2] == -1).all()
    two = mn.normals(pts, (0.6, 5), viewpoints=[[-5.0, 0, 1.0], [5.0, 0, 1.0]])
    assert np.array_equal(two["view_idx"], np.where(pts[:, 0] <= 0, 0, 1))                   # ties on x = 0 to the lowest index
    none = mn.normals(pts, (0.6, 5))
    assert (none["view_idx"] == -1).all() and (none["normals"][:, 2] == 1).all()             # the largest component is made positive
    # the largest-magnitude rule on a plane whose normal is (-3, 1, 2) / sqrt(14) up to sign: x leads and comes out positive
    rng = np.random.default_rng(3)
    nrm = np.array([-3.0, 1.0, 2.0]) / math.sqrt(14.0)
    u = np.array([1.0, 3.0, 0.0]) / math.sqrt(10.0); v = np.cross(nrm, u)
    ab = rng.uniform(-1.0, 1.0, (300, 2))
    q = mn.normals((ab[:, :1] * u + ab[:, 1:] * v).astype(np.float32), (0.6, 5))
    ok = np.isfinite(q["curvature"])
    lead = np.argmax(np.abs(q["normals"][ok]), axis=1)
    assert ok.sum() > 250 and (lead == 0).all() and (q["normals"][ok][:, 0] > 0).all()
    nan = pts.copy(); nan[3, 1] = np.nan; nan[5, 0] = np.inf
    r = mn.normals(nan, (0.6, 5), viewpoints=[[0, 0, 1.0]])
    assert r["view_idx"][3] == -1 and r["view_idx"][5] == -1 and r["count"][3] == 0 and np.isnan(r["normals"][[3, 5]]).all()
    assert (np.delete(r["view_idx"], [3, 5]) == 0).all()


def test_quantisation_exponent_and_range():
    assert mn.quant_exponent(0.6) == 20 and mn.quant_exponent(1.0) == 20 and mn.quant_exponent(2.0 ** -3) == 23
    for rad in (0.6, 1.0, 2.0 ** -3, 0.3, 7.7):
        e = mn.quant_exponent(rad)
        assert rad * 2.0 ** e <= 2.0 ** 20 < rad * 2.0 ** (e + 1)
    rng = np.random.default_rng(4)
    for rad in (0.6, 1.0, 2.0 ** -3):
        pts = (rng.uniform(-1, 1, (400, 3)) * 2.5 * rad + 50.0).astype(np.float32)
        # pairs on and just inside the radius along an axis: the largest offsets there are
        pts[1] = pts[0] + np.float32([rad, 0, 0]); pts[2] = pts[0] - np.float32([0, rad, 0])
        scale = np.float32(2.0 ** mn.quant_exponent(rad))
        d = pts[None, :, :] - pts[:, None, :]
        nb = overlap.sqdist3_block(pts, pts) <= overlap.radius2(rad)
        di = np.rint(d * scale)[nb]
        assert nb.sum() > 400 and np.abs(di).max() <= 2 ** 20 + 1
        assert np.abs(di).max() >= 2 ** 19                                                    # (the range is used, not a tenth of it)


def test_moments_and_normals_equal_a_point_by_point_loop():
    rng = np.random.default_rng(5)
    pts = (rng.normal(size=(70, 3)) * np.array([1.0, 1.0, 0.05]) + np.array([20.0, -7.0, 3.0])).astype(np.float32)
    pts[11] = [np.nan, 0, 0]; pts[12] = [0, -np.inf, 0]
    rad, r2 = 0.8, overlap.radius2(0.8)
    scale = np.float32(2.0 ** mn.quant_exponent(rad))
    view = np.array([[20.0, -7.0, 30.0], [0.0, 0.0, -30.0]])
    got = mn.normals(pts, (rad, 5), viewpoints=view, block=16)
    for i in range(70):
        k = 0; s1 = [0] * 3; s2 = [0] * 6; nbrs = []
        if np.isfinite(pts[i]).all():
            for j in range(70):
                if not np.isfinite(pts[j]).all():
                    continue
                d = pts[i] - pts[j]
                if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= r2:
                    di = [int(np.rint((pts[j][a] - pts[i][a]) * scale)) for a in range(3)]
                    k += 1; nbrs.append(j)
                    for a in range(3):
                        s1[a] += di[a]
                    q = 0
                    for a in range(3):
                        for b in range(a, 3):
                            s2[q] += di[a] * di[b]; q += 1
        assert int(got["count"][i]) == k and got["s1"][i].tolist() == s1 and got["s2"][i].tolist() == s2, i
        if k >= 5:
            P = pts[nbrs].astype(np.float64)
            w, U = np.linalg.eigh(np.cov(P.T, bias=True))
            assert abs(abs(float(U[:, 0] @ got["normals"][i].astype(np.float64))) - 1.0) < 1e-6 / max(got["gap"][i], 1e-3), i
            assert abs(w[0] / w.sum() - float(got["curvature"][i])) < 1e-5
            d = view[got["view_idx"][i]] - pts[i].astype(np.float64)
            assert got["view_idx"][i] == int(np.argmin(((view - pts[i].astype(np.float64)) ** 2).sum(axis=1)))
            assert float(got["normals"][i].astype(np.float64) @ d) > 0
            assert abs(float(np.linalg.norm(got["normals"][i].astype(np.float64))) - 1.0) < TOL
        else:
            assert np.isnan(got["normals"][i]).all() and np.isnan(got["curvature"][i])


def test_argument_refusals():
    pts = lattice(-2, 2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mn.normals(pts, (bad, 5))
        with pytest.raises(ValueError):
            mn.quant_exponent(bad)
    for bad in (0, 2, 2.5, -3):
        with pytest.raises(ValueError):
            mn.normals(pts, (0.6, bad))
    for bad in ([[0, 0, np.nan]], [[np.inf, 0, 0]]):
        with pytest.raises(ValueError):
            mn.normals(pts, (0.6, 5), viewpoints=bad)
    with pytest.raises(ValueError):
        mn.normals(np.zeros((4, 2), np.float32), (0.6, 5))
    empty = mn.normals(np.zeros((0, 3), np.float32), (0.6, 5), viewpoints=[[0, 0, 1.0]])
    assert empty["normals"].shape == (0, 3) and empty["count"].shape == (0,)
