"""Spinning-LiDAR scans (qn_sim_lidar_to_store, qn_kf_add_device, qn_kf_download_keyframe): the C-ABI surface, and the numpy twin
synth.lidar_scan - the specification the ray-casting kernel matches bit for bit - against the geometry it models.  No GPU needed."""
import ctypes
import hashlib
import numpy as np
from qn_amd import synth

SIM_SYMBOLS = ["qn_sim_lidar_to_store", "qn_kf_add_device", "qn_kf_download_keyframe"]


def test_header_declares_and_library_exports_the_sim_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in SIM_SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in SIM_SYMBOLS)


def test_prim_dtype_is_the_c_struct():
    assert synth.PRIM_DTYPE.itemsize == 56 and synth.PRIM_DTYPE.fields["p"][1] == 8


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_primitives_draw_no_rng_and_pairs_stay_byte_identical():
    # digests of the parent commit's make_pair: Scene.primitives() must not move any RNG stream
    assert _digest(*synth.make_pair(0, 2000)) == "641e5a92f5886ee5829ded717f99da971e04cf4c478b36cbbbbc914e067e6113"
    assert _digest(*synth.make_pair(5, 2000, mode="quatro")) == "280e8494c12eef29f11027ca81c1b7e3aa8cfaf51277ee958ab0c6f34a090465"
    rng = np.random.Generator(np.random.PCG64(3))
    scene = synth.Scene(rng)
    state = rng.bit_generator.state
    p = scene.primitives()
    assert rng.bit_generator.state == state
    assert len(p) == 1 + len(scene.walls) + len(scene.poles) + len(scene.boxes) == 81
    assert list(np.bincount(p["kind"])) == [1, 10, 40, 30]


def _prims(rows):
    return np.array([(k, tuple(v) + (0.0,) * (6 - len(v))) for k, v in rows], dtype=synth.PRIM_DTYPE)


GROUND = (synth.PRIM_GROUND, (-200.0, -200.0, 200.0, 200.0))


def test_ground_only_ranges_follow_the_beam_elevation():
    h = 1.73
    sen = synth.SpinningLidar(n_beams=16, n_cols=90, sigma=0.0, max_range=200.0)
    pts = synth.lidar_scan(_prims([GROUND]), sen, synth.sensor_pose(3.0, -2.0, 0.7, z=h), 11)
    el = sen.elevations()
    down = np.flatnonzero(el < 0)
    want_r = h / np.sin(-el)
    expect = [b for b in down if sen.min_range <= want_r[b] <= sen.max_range]
    assert len(pts) == len(expect) * sen.n_cols
    r = np.linalg.norm(pts[:, :3].astype(np.float64), axis=1)
    beam = np.repeat(expect, sen.n_cols)                          # (beam, col) order
    # range from the f32 record: 1e-9 relative on the f64 range is below f32 resolution, so compare the f64 hit with the formula
    # through the record's own rounding (|x - fl32(x)| <= 2^-24 |x|) and the elevation through z / r
    assert np.all(np.abs(r - want_r[beam]) <= 1.2e-7 * want_r[beam])
    assert np.all(np.abs(pts[:, 2] / r - np.sin(el[beam])) <= 3e-7)
    assert np.all(np.abs(pts[:, 2] + 0.0) <= h)


def test_ground_only_range_is_exact_in_f64():
    # the f64 range the kernel rounds: with sigma = 0 the stored point is fl32(t u) with t = -h / dz; reproduce t exactly
    h = 1.73
    sen = synth.SpinningLidar(n_beams=8, n_cols=4, sigma=0.0, max_range=200.0)
    pts = synth.lidar_scan(_prims([GROUND]), sen, synth.sensor_pose(0.0, 0.0, 0.0, z=h), 1)
    ce, se, ca, sa = sen.tables()
    down = [b for b in range(sen.n_beams) if se[b] < 0 and sen.min_range <= h / -se[b] <= sen.max_range]
    t = np.repeat([(0.0 - h) / se[b] for b in down], sen.n_cols)
    assert np.all(np.abs(t - np.repeat([h / np.sin(-sen.elevations()[b]) for b in down], sen.n_cols)) <= 1e-9 * t)
    ux = np.repeat(ce[down], sen.n_cols) * np.tile(ca, len(down))
    assert np.array_equal(pts[:, 0], (t * ux).astype(np.float32))


def test_front_wall_shadows_the_rear_wall():
    # wall A: plane x = 10, y in [-2, 2]; wall B: plane x = 20, y in [-10, 10]; both 5 m high; sensor at the origin looking along +x
    prims = _prims([GROUND, (synth.PRIM_WALL, (10.0, -2.0, 0.0, 4.0, 5.0)), (synth.PRIM_WALL, (20.0, -10.0, 0.0, 20.0, 5.0))])
    sen = synth.SpinningLidar(n_beams=32, n_cols=720, sigma=0.0)
    pts = synth.lidar_scan(prims, sen, synth.sensor_pose(0.0, 0.0, 0.0), 5).astype(np.float64)
    above = pts[pts[:, 2] > -1.7]                                  # not ground
    on_b = above[np.abs(above[:, 0] - 20.0) < 1e-3]
    on_a = above[np.abs(above[:, 0] - 10.0) < 1e-3]
    assert len(on_a) > 50 and len(on_b) > 50
    # the shadow of A on B: |y| < 4 (the cone y / x = +-0.2 at x = 20), minus the rays that pass above A (z / x > 3.27 / 10)
    shadow = (np.abs(on_b[:, 1]) < 4.0 - 1e-6) & ((on_b[:, 2] + 1.73) / 20.0 < (5.0 - 1.73) / 10.0)
    assert not shadow.any()
    assert (np.abs(on_b[:, 1]) > 4.0).sum() > 20


def test_every_range_is_inside_the_gate():
    rng = np.random.Generator(np.random.PCG64(9))
    scene = synth.Scene(rng)
    sen = synth.SpinningLidar(n_beams=32, n_cols=360, min_range=3.0, max_range=40.0, sigma=0.05)
    pts = synth.lidar_scan(scene.primitives(), sen, synth.sensor_pose(1.0, 2.0, 0.3), 77)
    r = np.linalg.norm(pts[:, :3].astype(np.float64), axis=1)
    assert len(pts) > 1000
    assert r.min() >= 3.0 * (1 - 1e-6) and r.max() <= 40.0 * (1 + 1e-6)


def test_density_falls_with_range():
    sen = synth.SpinningLidar(sigma=0.0)
    pts = synth.lidar_scan(_prims([GROUND]), sen, synth.sensor_pose(0.0, 0.0, 0.0), 3)
    d = np.linalg.norm(pts[:, :2].astype(np.float64), axis=1)

    def per_m2(a, b):
        return ((d >= a) & (d < b)).sum() / (np.pi * (b * b - a * a))
    assert per_m2(5, 10) >= 10 * per_m2(40, 60) > 0


def test_twin_is_deterministic_and_seeded():
    rng = np.random.Generator(np.random.PCG64(4))
    prims = synth.Scene(rng).primitives()
    sen = synth.SpinningLidar(n_beams=16, n_cols=240, sigma=0.02)
    P = synth.sensor_pose(-3.0, 4.0, 1.1)
    a, b, c = (synth.lidar_scan(prims, sen, P, s) for s in (1, 1, 2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(a) != len(c) or not np.array_equal(a, c)
    z = synth.SpinningLidar(n_beams=16, n_cols=240, sigma=0.0)
    assert np.array_equal(synth.lidar_scan(prims, z, P, 1), synth.lidar_scan(prims, z, P, 2))


def test_make_lidar_pair_is_reproducible():
    s1, t1, T1 = synth.make_lidar_pair(0, sensor=synth.SpinningLidar(n_beams=16, n_cols=360))
    s2, t2, T2 = synth.make_lidar_pair(0, sensor=synth.SpinningLidar(n_beams=16, n_cols=360))
    assert _digest(s1, t1, T1) == _digest(s2, t2, T2)
    assert s1.dtype == np.float32 and s1.shape[1] == 3 and len(s1) > 1000 and len(t1) > 1000
