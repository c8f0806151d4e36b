"""Scan Context twin (qn_amd/scancontext.py), the specification of csrc/qn_sc.hip: bins, edges and dropped points on hand-built clouds, exact
zero distance for a scan against itself and against itself turned by whole sectors (and the pinned yaw sign), the empty-column rules, the
query's admissibility / prefilter / order, the C-ABI declarations and the C++ helper compiling against the stand-ins.  No GPU needed."""
import math
import os
import numpy as np
import pytest
from qn_amd import scancontext as sc
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = sc.Params()                                    # 20 rings of 4 m, 60 sectors of 6 degrees, 80 m, lidar height 2


def _at(ring, sector, z, p=P):
    """a point at the centre of bin (ring, sector)"""
    r = (ring + 0.5) * p.max_radius / p.n_rings
    a = 2 * math.pi * (sector + 0.5) / p.n_sectors
    return [r * math.cos(a), r * math.sin(a), z]


def _rot(xyz, k, p=P):
    th = 2 * math.pi * k / p.n_sectors
    R = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
    return (np.asarray(xyz, np.float64) @ R.T).astype(np.float32)


def test_points_at_bin_centres_give_exactly_those_values():
    pts = np.array([_at(0, 0, 1.5), _at(3, 7, -0.25), _at(3, 7, 0.5), _at(19, 59, 10.0), _at(10, 30, -2.0), _at(10, 31, -3.0)], np.float32)
    d, rk, cn = sc.descriptor(pts, P)
    want = np.zeros((20, 60), np.float32)
    want[0, 0] = np.float32(1.5 + 2.0); want[3, 7] = np.float32(np.float64(np.float32(0.5)) + 2.0); want[19, 59] = 12.0
    want[10, 30] = 0.0; want[10, 31] = -1.0                          # a bin whose maximum is 0 or negative keeps it (only empty bins are 0)
    assert np.array_equal(d.view(np.uint32), want.view(np.uint32))
    acc = np.zeros(20)
    for j in range(60):
        acc = acc + want[:, j].astype(np.float64)
    assert np.array_equal(rk, acc / 60.0)
    assert cn[0] == 3.5 and cn[7] == np.float64(want[3, 7]) and cn[59] == 12.0 and cn[31] == 1.0 and cn[1] == 0.0


def test_points_on_edges_land_in_the_upper_bin():
    ring, sector, keep = sc.bins(np.array([[4.0, 0.0, 0.0], [0.0, 8.0, 0.0], [-12.0, 0.0, 0.0], [0.0, -16.0, 0.0], [79.0, 0.0, 0.0],
                                           [3.9999998, 0.0, 0.0]], np.float32), P)
    assert keep.all()
    assert list(ring) == [1, 2, 3, 4, 19, 0]                         # r = 4 i exactly: ring i
    assert list(sector) == [0, 15, 30, 45, 0, 0]                     # azimuth 0, 90, 180, 270 degrees: sectors 0, 15, 30, 45
    _, sector, _ = sc.bins(np.array([[1.0, -1e-30, 0.0], [1.0, 1e-30, 0.0]], np.float32), P)
    assert list(sector) == [59, 0]                                   # just below 2 pi / at 0+


def test_dropped_points():
    nan, inf = float("nan"), float("inf")
    pts = np.array([[nan, 1, 1], [1, inf, 1], [1, 1, -inf], [0, 0, 5], [-0.0, 0.0, 5], [80, 0, 1], [0, -80, 1], [60, 60, 1], [1e30, 0, 1]], np.float32)
    _, _, keep = sc.bins(pts, P)
    assert not keep.any()
    d, rk, cn = sc.descriptor(pts, P)
    assert not d.any() and not rk.any() and not cn.any()
    d, _, _ = sc.descriptor(np.concatenate([pts, [[79.99, 0, 1]]]).astype(np.float32), P)
    assert d[19, 0] == 3.0 and np.count_nonzero(d) == 1


def _cloud(seed, n=4000):
    rng = np.random.default_rng(seed)
    return np.array([_at(r, s, z) for r, s, z in zip(rng.integers(0, 20, n), rng.integers(0, 60, n), rng.uniform(-1.5, 8, n))], np.float32)


def test_self_distance_is_exactly_zero():
    for seed in range(3):
        a = sc.descriptor(np.random.default_rng(seed).uniform(-60, 60, (3000, 3)).astype(np.float32), P)
        assert sc.distance(a, a) == (0.0, 0)


@pytest.mark.parametrize("k", [1, 7, 30, 59])
def test_turned_by_whole_sectors_is_exactly_zero_at_the_pinned_shift(k):
    pts = _cloud(k)
    q = sc.descriptor(pts, P)
    c = sc.descriptor(_rot(pts, k), P)
    assert np.array_equal(np.roll(q[0], k, axis=1), c[0])            # the candidate's column j + k is the query's column j
    assert sc.distance(q, c) == (0.0, k)
    # the cloud turned by +k sectors is what a sensor turned by -k sectors sees: the candidate's heading minus the query's
    assert sc.yaw_of_shift(k, 60) == pytest.approx(((-2 * math.pi * k / 60) + math.pi) % (2 * math.pi) - math.pi)
    assert sc.distance(c, q) == (0.0, (60 - k) % 60)


def test_empty_column_rules():
    empty = sc.descriptor(np.zeros((0, 3), np.float32), P)
    a = sc.descriptor(_cloud(4), P)
    assert sc.distance(empty, a) == (1.0, 0) and sc.distance(a, empty) == (1.0, 0) and sc.distance(empty, empty) == (1.0, 0)
    # columns 0 and 1 in the query, only column 0 (equal to the query's) in the candidate: the empty column does not count
    q = sc.descriptor(np.array([_at(2, 0, 1.0), _at(5, 1, 3.0)], np.float32), P)
    c = sc.descriptor(np.array([_at(2, 0, 1.0)], np.float32), P)
    assert sc.distance(q, c) == (0.0, 0)
    # a column full of zero-valued bins is empty too (its norm is 0): z = -lidar_height everywhere
    z = sc.descriptor(np.array([_at(2, 0, -2.0), _at(3, 0, -2.0)], np.float32), P)
    assert sc.distance(z, a) == (1.0, 0)


def test_query_admissibility_prefilter_and_order():
    clouds = [_cloud(10 + i % 4) for i in range(9)]                   # keyframes 0..8, repeats: ties between different ids
    descs = {i: sc.descriptor(c, P) for i, c in enumerate(clouds)}
    stamps = np.arange(9) * 10.0
    res = sc.query(descs, 8, stamps, 30.0, 10)
    assert [r[0] for r in res if r[1] == 0.0] == [0, 4]                # 8 repeats 0 and 4 (seed 10): both at 0, the lower id first
    assert {r[0] for r in res} == {0, 1, 2, 3, 4}                      # 80 - 50 = 30 is not > 30: keyframe 5 is excluded
    assert all((a[1], a[0]) < (b[1], b[0]) for a, b in zip(res, res[1:]))
    assert sc.query(descs, 8, stamps, 30.0, 2) == res[:2]
    pre = sc.query(descs, 8, stamps, 30.0, 10, prefilter=2)
    assert [r[0] for r in pre] == [0, 4]
    rkd = sorted((sc.ringkey_distance(descs[8][1], descs[c][1]), c) for c in range(5))
    assert [c for _, c in rkd[:2]] == [0, 4]
    del descs[0]
    assert [r[0] for r in sc.query(descs, 8, stamps, 30.0, 1)] == [4]  # undescribed keyframes are not candidates


def test_capi_declares_the_scan_context_surface():
    import test_capi_symbols
    syms = test_capi_symbols.declared_symbols()
    for s in ["qn_kf_sc_set_params", "qn_kf_sc_get_params", "qn_kf_sc_describe", "qn_kf_sc_get", "qn_kf_sc_query"]:
        assert s in syms


def test_engine_params_mirror_the_twin():
    from qn_amd import engine
    e, t = engine.ScParams(), sc.Params()
    assert (e.n_rings, e.n_sectors, e.max_radius, e.lidar_height, e.ringkey_prefilter) == (t.n_rings, t.n_sectors, t.max_radius, t.lidar_height, t.ringkey_prefilter)


def test_scan_context_helper_compiles_against_the_standins(tmp_path):
    out = build_shim("shim_scan_context.cpp", tmp_path)
    assert os.path.exists(out)
