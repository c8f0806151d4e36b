"""The map normals on the GPU (qn_kf_map_normals / qn_kf_download_map_normals / qn_kf_map_moments) against their specification, the numpy twin
qn_amd/mapnormals.py, run on the map the store itself downloads.  Bit for bit: count, s1, s2 and view_idx of every point, NaN where the twin has NaN, and a
rerun.  Normals and curvature: within 2^-22 per component wherever the answer is well conditioned - the twin's relative eigen-gap (l1 - l0) / l2 >= 1e-3 and
|n . (v - p)| >= 1e-6 |v - p| (without viewpoints the same margin between the normal's two largest components: the sign rule's own coin toss) - which is two
f32 roundings of values <= 1 (2^-25 each) on top of two backward-stable f64 solves (angle error about 2^-53 / gap <= 1e-12), about 2^-24, times four.
Elsewhere that comparison asks only for unit length within 2^-22 (and the curvature, which no gap touches).  The ill-conditioned share is printed and may not
pass 10 % of the valid points.  Every valid point, ill conditioned or not, is held to its own covariance instead: the normal's Rayleigh quotient exceeds the
smallest eigenvalue by at most 2^-44 of the trace, so no normal goes unchecked.  The kernel's block is 256 points: the sizes 1, 2, 255, 256, 257 and 513 are
its launch seams."""
import ctypes as C
import math
import subprocess
import numpy as np
import pytest
from qn_amd import mapnormals as mn, staticmap as sm, synth
import eig3_checks as chk

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -22
RAYLEIGH = 2.0 ** -44                                                # of trace(C): the bound on a normal's Rayleigh excess (equal_the_twin)
B = 256                                                              # MN_BLOCK of csrc/qn_mapnormals.hip
H = np.float32(0.3)
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2)]


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


@pytest.fixture(scope="module")
def scans(store):
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    return [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13])]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def equal_the_twin(store, params, views, what, max_share=0.10):
    """map_normals of the store's map against the twin on the downloaded map -> the GPU result"""
    from qn_amd import engine
    pts = store.download_map(store._map_n)
    got = store.map_normals(engine.NormalParams(*params), views)
    s1, s2 = store.map_moments()
    want = mn.normals(pts, params, views)
    n = len(pts)
    assert len(got["count"]) == n and got["normals"].shape == (n, 3) and got["normals"].dtype == np.float32
    assert np.array_equal(got["count"], want["count"]), (what, int((got["count"] != want["count"]).sum()))
    assert np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"]), what
    assert np.array_equal(got["view_idx"], want["view_idx"]), what
    valid = np.isfinite(want["curvature"])
    assert np.array_equal(np.isnan(got["curvature"]), ~valid) and np.array_equal(np.isnan(got["normals"]).all(axis=1), ~valid), what
    good = valid & (want["gap"] >= 1e-3) & (want["view_cos"] >= 1e-6)
    share = float((valid & ~good).sum()) / max(int(valid.sum()), 1)
    dn = np.abs(got["normals"][good].astype(np.float64) - want["normals"][good].astype(np.float64))
    dc = np.abs(got["curvature"][valid].astype(np.float64) - want["curvature"][valid].astype(np.float64))
    unit = np.abs(np.linalg.norm(got["normals"][valid].astype(np.float64), axis=1) - 1.0)
    print("%s: %d points, %d valid, %d compared, ill-conditioned share %.4f; max |dn| %.3g, |dcurv| %.3g, | |n| - 1 | %.3g (2^-22 = %.3g)"
          % (what, n, valid.sum(), good.sum(), share, dn.max() if dn.size else 0.0, dc.max() if dc.size else 0.0, unit.max() if unit.size else 0.0, TOL))
    assert share <= max_share, (what, share)
    assert not dn.size or dn.max() <= TOL, (what, dn.max())
    assert not dc.size or dc.max() <= TOL, (what, dc.max())
    assert not unit.size or unit.max() <= TOL, (what, unit.max())
    # every valid point, the ill-conditioned ones included: the normal's Rayleigh quotient on the point's own covariance lies within 2^-44 trace of the smallest
    # eigenvalue.  A backward-stable solve puts the f64 normal's quotient within K eps ||C|| of l0 whatever the gap (K <= 128: tests/eig3_checks.py); rounding
    # the normal to f32 adds at most l2 |e|^2 with |e| <= sqrt(3) 2^-25, about 2^-48.4 trace; 2^-44 is 16 times that.  So a collinear neighbourhood's normal
    # is perpendicular to the line, and a nearly degenerate plane's lies in the right eigenspace - where the comparison above asks for unit length only.
    C, tr = mn.covariance(want["count"], want["s1"], want["s2"])                     # (the kernel's C is the same bits)
    excess = chk.rayleigh_excess(C[valid], tr[valid], got["normals"][valid]) if valid.any() else np.zeros(0)
    print("%s: largest Rayleigh excess (n'Cn / n'n - l0) / trace over all %d valid points: 2^%.1f (bound 2^-44)"
          % (what, valid.sum(), math.log2(max(float(excess.max()), 2.0 ** -99)) if excess.size else -99.0))
    assert not excess.size or excess.max() <= RAYLEIGH, (what, excess.max())
    # a rerun returns the same bytes
    again = store.map_normals(engine.NormalParams(*params), views)
    a1, a2 = store.map_moments()
    for k in ("normals", "curvature", "count", "view_idx"):
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (what, k)
    assert np.array_equal(s1, a1) and np.array_equal(s2, a2), what
    return got, want, pts


def _map_of(store, clouds, poses, leaf):
    ids = [store.add(c) for c in clouds]
    return store.build_map(ids, poses, leaf)


def _views(poses, dx=0.0):
    return np.array([[p[0, 3] + dx, p[1, 3], p[2, 3]] for p in poses])


def test_ray_cast_map(store, scans):
    n = store.build_map(scans, POSES, 0.3)
    assert 2000 <= n <= 20000, n
    got, want, pts = equal_the_twin(store, (0.6, 5), _views(POSES), "ray-cast map")
    valid = np.isfinite(got["curvature"])
    assert valid.sum() >= 0.5 * n
    d = _views(POSES)[got["view_idx"][valid]] - pts[valid, :3]
    assert ((got["normals"][valid].astype(np.float64) * d).sum(axis=1) > -1e-6 * np.linalg.norm(d, axis=1)).all()          # every normal faces its viewpoint
    # the flat ground of the scene, seen from above: where the neighbourhood spreads in both horizontal directions the normal is the vertical.  A low
    # curvature alone does not say so - five points of one scan ring are nearly collinear, and a ring arc plus one point at a wall's foot is a perfectly
    # planar, tilted neighbourhood - so the bound comes from the covariance C itself: for n = c ez + s h (h horizontal, unit) and C positive semi-definite,
    # sqrt(n'Cn) >= s sqrt(h'Ch) - c sqrt(Czz), and n'Cn = l0 <= Czz, hence s <= 2 sqrt(Czz / mu) with mu the smaller eigenvalue of C's horizontal 2 x 2
    # block.  Below 0.3 that is |nz| >= sqrt(1 - 0.09) > 0.95.
    k = want["count"].astype(np.float64); s1 = want["s1"].astype(np.float64); s2 = want["s2"].astype(np.float64)
    with np.errstate(all="ignore"):
        m = s1 / k[:, None]
        cxx, cxy, cyy, czz = s2[:, 0] / k - m[:, 0] ** 2, s2[:, 1] / k - m[:, 0] * m[:, 1], s2[:, 3] / k - m[:, 1] ** 2, s2[:, 5] / k - m[:, 2] ** 2
        mu = 0.5 * (cxx + cyy) - np.sqrt(0.25 * (cxx - cyy) ** 2 + cxy ** 2)
        ground = valid & (np.abs(pts[:, 2]) < 0.05) & (mu > 0) & (2.0 * np.sqrt(np.maximum(czz, 0.0) / mu) < 0.3)
    assert ground.sum() > 1000 and (np.abs(got["normals"][ground][:, 2]) > 0.95).all()


def test_offset_map_76_km_out(store, scans):
    far = [p.copy() for p in POSES]
    for p in far:
        p[0, 3] += 76000.0
    n = store.build_map(scans, far, 0.3)
    assert n >= 2000
    equal_the_twin(store, (0.6, 5), _views(far), "ray-cast map at 76 km")


def test_no_viewpoints(store, scans):
    store.build_map(scans, POSES, 0.3)
    got, _, _ = equal_the_twin(store, (0.6, 5), None, "ray-cast map, V = 0")
    valid = np.isfinite(got["curvature"])
    assert (got["view_idx"] == -1).all()
    lead = np.argmax(np.abs(got["normals"][valid]), axis=1)
    assert (got["normals"][valid][np.arange(valid.sum()), lead] > 0).all()
    equal_the_twin(store, (1.0, 12), np.zeros((0, 3)), "ray-cast map, V = 0, r = 1, 12 neighbours")


def _lattice(levels):
    """9 x 9 lattices of spacing h = float32(0.3), indices -4 .. 4, at the heights levels[] h.  k h is exact in f32 for |k| <= 4 and for 6 and 8, and so is every
    difference of up to two steps, and 4 fl(h h) == float32(0.6 * 0.6): a partner two steps away - along an axis, or straight above in a layer 2 h = float32(0.6)
    higher - is exactly ON the radius.  Layers 4 h apart do not see each other."""
    k = np.arange(-4, 5).astype(np.float32) * H
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, np.float32(l) * H, np.float32)], axis=1) for l in levels]).astype(np.float32)


@pytest.mark.parametrize("name", ["plane", "two_layers"])
def test_lattices_on_the_knife_edge(store, name):
    pts = _lattice([-8, -4, 0, 4, 8]) if name == "plane" else _lattice([-8, -6, -2, 0, 4, 6])          # five single layers / three pairs exactly r apart
    assert np.float32(4) * (H * H) == np.float32(0.6 * 0.6) and len(pts) > B
    n = _map_of(store, [pts], [np.eye(4)], 1e-4)                     # the overflow guard trips at this leaf: the map is the records themselves
    assert n == len(pts) and np.array_equal(store.download_map(n)[:, :3], pts)
    got, want, _ = equal_the_twin(store, (0.6, 5), [[0.3, -0.2, 9.0]], "lattice " + name)
    inner = (np.abs(pts[:, 0]) <= 0.61) & (np.abs(pts[:, 1]) <= 0.61)                                   # indices -2 .. 2: all partners inside the lattice
    assert inner.sum() == 25 * len(pts) // 81
    # by hand: 13 offsets (a, b) with a^2 + b^2 <= 4, four of them on the radius; with the second layer one more, straight above or below, on the radius too
    assert (got["count"][inner] == (13 if name == "plane" else 14)).all() and got["count"].max() == (13 if name == "plane" else 14)
    if name == "plane":
        assert np.array_equal(got["normals"], np.tile(np.float32([0, 0, 1]), (n, 1))) and (got["curvature"] == 0).all()
    else:
        assert (got["normals"][inner][:, 2] == 1).all()


@pytest.mark.parametrize("n", [1, 2, B - 1, B, B + 1, 2 * B + 1])
def test_launch_seams(store, n):
    rng = np.random.default_rng(100 + n)
    side = int(math.ceil(math.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    pts = np.zeros((n, 3), np.float32)
    pts[:, :2] = ij * 0.3 + rng.uniform(-0.05, 0.05, (n, 2)); pts[:, 2] = 0.02 * np.sin(ij[:, 0]) + rng.uniform(-0.01, 0.01, n)
    got_n = _map_of(store, [pts], [np.eye(4)], 0.1)                  # at least 0.2 apart on an axis: every point is a voxel of its own
    assert got_n == n
    got, _, _ = equal_the_twin(store, (0.6, 3), [[1.0, 1.0, 6.0], [-4.0, 2.0, 5.0]], "map of %d points" % n)
    assert np.isfinite(got["curvature"]).sum() == (0 if n < 3 else n)


def test_passed_through_map_with_non_finite_records(store):
    rng = np.random.default_rng(5)
    a = np.zeros((1500, 3), np.float32); a[:, :2] = rng.uniform(-5, 5, (1500, 2)); a[:, 2] = 0.1 * np.sin(a[:, 0]) + rng.normal(0, 0.01, 1500)
    b = (rng.normal(0, 12, (1200, 3)) * 200.0).astype(np.float32)
    a[[5, 77, 901]] = [[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf]]
    b[10] = [np.nan, 1, 1]
    n = _map_of(store, [a, b], [np.eye(4), np.eye(4)], 1e-3)
    assert n == 2700 and "overflow" in store._l.qn_kf_last_error(store.h).decode()
    got, _, pts = equal_the_twin(store, (0.6, 5), [[0.0, 0.0, 8.0], [3.0, 3.0, 8.0]], "passed-through map")
    bad = ~np.isfinite(pts[:, :3]).all(axis=1)
    assert bad.sum() == 4
    assert (got["count"][bad] == 0).all() and np.isnan(got["normals"][bad]).all() and np.isnan(got["curvature"][bad]).all() and (got["view_idx"][bad] == -1).all()
    assert (got["view_idx"][~bad] >= 0).all() and np.isfinite(got["curvature"][:1500]).sum() > 1000


def test_collinear_points(store):
    t = np.linspace(-3.0, 3.0, 61)
    pts = (t[:, None] * np.array([1.0, 2.0, -0.5])[None, :] / 2.29 + np.array([4.0, 1.0, 2.0])).astype(np.float32)
    assert _map_of(store, [pts], [np.eye(4)], 0.02) == 61
    equal_the_twin(store, (0.6, 5), [[0.0, 0.0, 9.0]], "collinear points", max_share=1.0)


def test_static_map_and_stale_results(store, scans):
    from qn_amd import engine
    store.range_set_params(engine.RangeParams.for_sensor(SEN))
    store.range_describe(scans)
    store.static_classify(scans, POSES, witnesses=sm.window_witnesses(scans, 2))
    n = store.build_map_static(0.3)
    assert n >= 2000
    equal_the_twin(store, (0.6, 5), _views(POSES), "static map")
    keep = store.map_normals(engine.NormalParams(0.6, 5), _views(POSES))
    # every refusal leaves the results as they were
    v = _views(POSES)
    for p, views, nv in [(engine.NormalParams(0.0, 5), v, 3), (engine.NormalParams(float("nan"), 5), v, 3), (engine.NormalParams(float("inf"), 5), v, 3),
                         (engine.NormalParams(-0.6, 5), v, 3), (engine.NormalParams(0.6, 2), v, 3), (None, v, 3), (engine.NormalParams(0.6, 5), None, 3),
                         (engine.NormalParams(0.6, 5), np.array([[0.0, np.nan, 0.0]] * 3), 3), ("reserved", v, 3)]:
        if p == "reserved":
            p = engine.NormalParams(0.6, 5); p.reserved = 1
        ptr = C.c_void_p(); cnt = C.c_uint32()
        rc = store._l.qn_kf_map_normals(store.h, C.byref(p) if p is not None else None, views.ctypes.data_as(C.c_void_p) if views is not None else None,
                                        C.c_uint32(nv), C.byref(ptr), C.byref(cnt))
        assert rc == engine.QN_ERR_INVALID_ARG
    assert store._l.qn_kf_map_normals(store.h, C.byref(engine.NormalParams()), None, C.c_uint32(0), None, C.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert store._l.qn_kf_download_map_normals(store.h, None, None, None) == engine.QN_ERR_INVALID_ARG
    assert store._l.qn_kf_map_moments(store.h, None, None) == engine.QN_ERR_INVALID_ARG
    out = np.zeros((n, 4), np.float32)
    assert store._l.qn_kf_download_map_normals(store.h, out.ctypes.data_as(C.c_void_p), None, None) == engine.QN_OK
    assert np.array_equal(_bits(out[:, :3]), _bits(keep["normals"])) and np.array_equal(_bits(out[:, 3]), _bits(keep["curvature"]))
    # a later map build replaces the slot: the downloads are refused until the normals are computed again
    m = store.build_map(scans[:2], POSES[:2], 0.3)
    assert m > 0
    assert store._l.qn_kf_download_map_normals(store.h, out.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    s1 = np.zeros((n, 3), np.int64)
    assert store._l.qn_kf_map_moments(store.h, s1.ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
    equal_the_twin(store, (0.6, 5), _views(POSES[:2]), "the map built afterwards")


def test_not_ready_without_a_map():
    from qn_amd import engine
    s = engine.KeyframeStore()
    try:
        ptr = C.c_void_p(); cnt = C.c_uint32()
        assert s._l.qn_kf_map_normals(s.h, C.byref(engine.NormalParams()), None, C.c_uint32(0), C.byref(ptr), C.byref(cnt)) == engine.QN_ERR_NOT_READY
        out = np.zeros((4, 4), np.float32)
        assert s._l.qn_kf_download_map_normals(s.h, out.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_normals()
        assert ei.value.status == engine.QN_ERR_NOT_READY
    finally:
        s.close()


def _fnv(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def test_cpp_helper_gives_the_python_result(store, scans, tmp_path):
    from shim_build import build_shim
    exe = build_shim("shim_map_normals.cpp", tmp_path)
    ids, poses = scans[:2], POSES[:2]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    np.ascontiguousarray(np.array(poses, np.float64)).tofile(str(tmp_path / "poses.bin"))
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "0.6", "5"], text=True)
    from qn_amd import engine
    n = store.build_map(ids, poses, 0.3)
    m = store.download_map(n)
    r = store.map_normals(engine.NormalParams(0.6, 5), _views(poses))
    hm = _fnv(m[i].tobytes() for i in range(n))
    hn = _fnv(r["normals"][i].tobytes() + r["curvature"][i].tobytes() + r["count"][i].tobytes() + r["view_idx"][i].tobytes() for i in range(n))
    assert txt.splitlines() == ["map %d %016x" % (n, hm), "normals %d %d %016x" % (n, int(np.isfinite(r["curvature"]).sum()), hn)], txt
