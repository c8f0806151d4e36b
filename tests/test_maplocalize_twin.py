"""The specification of the map crop, qn_amd/maplocalize.py, on its own: hand-made points whose answers are worked out by hand.  The clouds and their answers
(the case_* functions) are what tests/test_gpu_map_crop.py runs on the GPU as well.  No GPU needed."""
import numpy as np
import pytest
from qn_amd import maplocalize as ml

F = np.float32
H = F(0.5)
UP = np.nextafter(H, F(1))                                           # the next f32 above 0.5: its square rounds above 0.25
NAN, INF = F(np.nan), F(np.inf)


def case_knife():
    """centre 0, R = 0.5 (r2 = 0.25 exactly) -> (points (n, 4) f32 with the index as intensity, centre, R, members of the sphere, members of the cylinder)"""
    pts = np.array([
        (H, 0, 0),                   # 0  d2 == r2: in
        (UP, 0, 0),                  # 1  the next f32 above: out
        (0, 0, -H),                  # 2  d2 == r2 along z: in, both shapes
        (0, 0, -UP),                 # 3  out of the sphere; the cylinder leaves dz dz out: in
        (0.0, -0.0, 0.0),            # 4  +-0: d2 = 0, in
        (-0.0, 0.0, -0.0),           # 5
        (NAN, 0, 0), (0, NAN, 0),    # 6 7
        (0, 0, NAN),                 # 8  a NaN z: out of the cylinder as well
        (INF, 0, 0), (0, -INF, 0),   # 9 10
        (0, 0, INF), (0, 0, -INF),   # 11 12  out of the cylinder as well
        (0.25, 0.25, 7.0),           # 13 seven metres up: the cylinder only
        (-H, 0, 0),                  # 14 in
        (0, UP, 0),                  # 15 out
        (0.25, 0.25, 0.25),          # 16 d2 = 0.1875: in
    ], dtype=F)
    xyzi = np.concatenate([pts, np.arange(len(pts), dtype=F)[:, None]], axis=1)
    return xyzi, (0.0, 0.0, 0.0), 0.5, [0, 2, 4, 5, 14, 16], [0, 2, 3, 4, 5, 13, 14, 16]


def case_rounded_centre():
    """the f64 centre 1 + 2^-30 rounds to the f32 1.0: 0.5 is then exactly R away (in f64 it would be 2^-30 beyond).  0.5 - 2^-25 is in as well: its f32
    difference from 1.0, 0.5 + 2^-25, is a tie that rounds to the even 0.5; 0.5 - 2^-24 gives the representable 0.5 + 2^-24 and is out
    -> (points, centre, R, members)"""
    pts = np.array([(H, 0, 0), (H - F(2.0 ** -25), 0, 0), (H - F(2.0 ** -24), 0, 0), (1.5, 0, 0), (np.nextafter(F(1.5), F(2)), 0, 0), (1.0, 0.75, 0.6)], dtype=F)
    xyzi = np.concatenate([pts, np.full((len(pts), 1), 3.5, F)], axis=1)
    return xyzi, (1.0 + 2.0 ** -30, 0.0, 0.0), 0.5, [0, 1, 3]


def test_the_knife_edge_the_signed_zeros_and_the_non_finite_records():
    xyzi, c, R, sphere, cyl = case_knife()
    assert F(UP * UP) > F(0.25) and F(H * H) == F(R * R)
    got = ml.crop_indices(xyzi, c, R)
    assert got.dtype == np.uint32 and got.tolist() == sphere
    assert ml.crop_indices(xyzi, c, R, ml.SPHERE).tolist() == sphere
    assert ml.crop_indices(xyzi, c, R, ml.CYLINDER).tolist() == cyl            # keeps what the sphere drops (3, 13), never a NaN or infinite z (8, 11, 12)
    assert ml.crop_indices(xyzi, (-0.0, 0.0, -0.0), R).tolist() == sphere      # a centre of the other zeros


def test_a_radius_whose_square_underflows_keeps_only_the_centre_itself():
    xyzi, c, _, _, _ = case_knife()
    assert ml.crop_indices(xyzi, c, 1e-30).tolist() == [4, 5] and ml.crop_indices(xyzi, c, 1e-30, ml.CYLINDER).tolist() == [2, 3, 4, 5]


def test_the_centre_is_rounded_to_f32_once():
    xyzi, c, R, members = case_rounded_centre()
    assert ml.centre_f32(c).tolist() == [1.0, 0.0, 0.0] and c[0] != 1.0
    assert ml.crop_indices(xyzi, c, R).tolist() == members
    assert ml.crop_indices(xyzi, (1.0, 0.0, 0.0), R).tolist() == members


def test_crop_carries_whole_records_in_ascending_map_order():
    rng = np.random.default_rng(5)
    xyzi = rng.uniform(-3, 3, (2000, 4)).astype(F)
    rec, idx = ml.crop(xyzi, (0.5, -0.25, 0.125), 2.0)
    assert rec.dtype == F and rec.shape == (len(idx), 4) and idx.dtype == np.uint32 and 0 < len(idx) < len(xyzi)
    assert (np.diff(idx.astype(np.int64)) > 0).all() and rec.tobytes() == xyzi[idx].tobytes()
    d = np.linalg.norm(xyzi[:, :3].astype(np.float64) - np.array([0.5, -0.25, 0.125]), axis=1)
    far = np.abs(d - 2.0) > 1e-5                                     # away from the edge f32 and f64 agree
    inside = np.zeros(len(xyzi), bool); inside[idx] = True
    assert np.array_equal(inside[far], (d <= 2.0)[far])
    cyl = ml.crop_indices(xyzi, (0.5, -0.25, 0.125), 2.0, ml.CYLINDER)
    assert set(idx.tolist()) < set(cyl.tolist())


def test_an_empty_crop_and_an_empty_map():
    xyzi, _, R, _, _ = case_knife()
    rec, idx = ml.crop(xyzi, (100.0, 0.0, 0.0), R)
    assert rec.shape == (0, 4) and idx.shape == (0,) and idx.dtype == np.uint32
    rec, idx = ml.crop(np.zeros((0, 4), F), (0.0, 0.0, 0.0), R)
    assert rec.shape == (0, 4) and idx.shape == (0,)


def test_refusals():
    xyzi, c, R, _, _ = case_knife()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ml.crop_indices(xyzi, c, bad)
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, 1e300)):
        with pytest.raises(ValueError):
            ml.crop_indices(xyzi, bad, R)
    with pytest.raises(ValueError):
        ml.crop_indices(xyzi, c, R, 2)


def test_guess_f32_is_one_rounding_for_centre_and_seed():
    P = np.eye(4); P[:3, 3] = (1.0 + 2.0 ** -30, -2.0, 0.1); P[0, 0] = 0.1
    g = ml.guess_f32(P)
    assert g.dtype == F and g[0, 3] == F(1.0) and g[2, 3] == F(0.1) and g[0, 0] == F(0.1) and float(g[0, 0]) != 0.1
    for bad in (np.full((4, 4), np.nan), np.vstack([np.eye(4)[:3], [0, 0, 0, 2.0]]), np.vstack([np.eye(4)[:3], [1e-9, 0, 0, 1.0]])):
        with pytest.raises(ValueError):
            ml.guess_f32(bad)
    assert ml.LocalizeParams() == (35.0, 0.3, 1.5, ml.SPHERE)


def test_transform_final_is_the_f32_chain():
    T = np.eye(4, dtype=F); T[0, 3] = F(0.1); T[1, 0] = F(0.3)
    p = np.array([[1.0, 2.0, 3.0]], F)
    out = ml.transform_final(p, T)
    assert out.dtype == F and out[0, 0] == F(1.0) * F(1.0) + (F(0.0) * F(2.0) + (F(0.0) * F(3.0) + F(0.1)))
    assert out[0, 1] == F(0.3) * F(1.0) + (F(1.0) * F(2.0) + (F(0.0) * F(3.0) + F(0.0)))
