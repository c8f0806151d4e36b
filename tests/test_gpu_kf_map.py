"""The corrected global map on the GPU (qn_kf_build_map, fast_lio_sam_qn.cpp:302-316, 398-411, 435-448): bit for bit against the
numpy restatement of pcl::VoxelGrid with intensity (tests/test_kf_map_api.py) and, for xyz, against the oracle's assemble_submap."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

from test_kf_map_api import voxel_grid_xyzi, transform_xyzi, build_map_program, MAP_BIN

pytestmark = pytest.mark.gpu


def _pose(rng, scale=20.0):
    a, b, c = rng.uniform(-np.pi, np.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    T = np.eye(4); T[:3, :3] = Rz @ Ry @ Rx; T[:3, 3] = rng.uniform(-scale, scale, 3) * [1, 1, 0.1]
    return T


def _keyframes(rng, count, n):
    xyz = [np.c_[rng.uniform(-15, 15, (n, 2)), rng.uniform(-1.5, 4, n)].astype(np.float32) for _ in range(count)]
    inten = [rng.uniform(0, 255, n).astype(np.float32) for _ in range(count)]
    return xyz, inten


def _check(store, xyz, inten, with_i, poses, ids, leaf, oracle=None):
    """build the map of `ids` and compare it with the restatement; -> the downloaded map"""
    n = store.build_map(ids, [poses[i] for i in ids], leaf)
    got = store.download_map(n)
    cat = np.concatenate([transform_xyzi(np.c_[xyz[i], inten[i] if with_i[i] else np.zeros(len(xyz[i]), np.float32)], poses[i]) for i in ids])
    want, of = voxel_grid_xyzi(cat, leaf)
    assert not of
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if oracle is not None:
        fin = cat[np.isfinite(cat[:, :3]).all(1), :3]
        ref = oracle.voxel_grid(fin, leaf) if len(fin) < len(cat) else oracle.assemble_submap(xyz, poses, ids, leaf)
        assert np.array_equal(got[:, :3].view(np.uint32), ref.view(np.uint32))
    return got


@pytest.fixture
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _fill(store, xyz, inten, with_i):
    return [store.add(x, i) if w else store.add(x) for x, i, w in zip(xyz, inten, with_i)]


def test_one_keyframe(store, oracle):
    rng = np.random.default_rng(1)
    xyz, inten = _keyframes(rng, 1, 30000)
    _fill(store, xyz, inten, [True])
    _check(store, xyz, inten, [True], [_pose(rng)], [0], 0.3, oracle)


def test_two_hundred_keyframes_any_order_and_repeats(store, oracle):
    rng = np.random.default_rng(2)
    xyz, inten = _keyframes(rng, 200, 3000)
    _fill(store, xyz, inten, [True] * 200)
    poses = [_pose(rng) for _ in range(200)]
    _check(store, xyz, inten, [True] * 200, poses, list(range(200)), 0.3, oracle)
    _check(store, xyz, inten, [True] * 200, poses, list(range(199, -1, -1)), 0.3, oracle)
    _check(store, xyz, inten, [True] * 200, poses, [5, 17, 5, 3, 17, 5], 0.5, oracle)


def test_mixed_intensity_and_xyz_only_keyframes(store, oracle):
    rng = np.random.default_rng(3)
    xyz, inten = _keyframes(rng, 12, 8000)
    with_i = [k % 3 != 0 for k in range(12)]
    _fill(store, xyz, inten, with_i)
    got = _check(store, xyz, inten, with_i, [_pose(rng, 5.0) for _ in range(12)], list(range(12)), 0.3, oracle)
    assert (got[:, 3] == 0).any() and (got[:, 3] > 0).any()


def test_non_finite_xyz_dropped_and_nan_intensity_poisons_its_leaf(store, oracle):
    rng = np.random.default_rng(4)
    xyz, inten = _keyframes(rng, 3, 10000)
    xyz[0][[5, 77, 901]] = [[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf]]
    xyz[2][4000, 2] = np.nan
    inten[1][123] = np.nan
    _fill(store, xyz, inten, [True] * 3)
    poses = [_pose(rng, 5.0) for _ in range(3)]
    got = _check(store, xyz, inten, [True] * 3, poses, [0, 1, 2], 0.3, oracle)
    assert np.isfinite(got[:, :3]).all() and np.isnan(got[:, 3]).sum() == 1


def test_overflow_guard_passes_the_concatenation_through(store):
    from qn_amd import engine
    rng = np.random.default_rng(5)
    xyz, inten = _keyframes(rng, 2, 5000)
    xyz[1] = xyz[1] * 200.0
    xyz[1][10] = [np.nan, 1, 1]
    _fill(store, xyz, inten, [True, False])
    poses = [np.eye(4), _pose(rng)]
    n = store.build_map([0, 1], poses, 1e-3)
    got = store.download_map(n)
    cat = np.concatenate([transform_xyzi(np.c_[xyz[0], inten[0]], poses[0]), transform_xyzi(np.c_[xyz[1], np.zeros(5000, np.float32)], poses[1])])
    assert n == 10000 and np.array_equal(got.view(np.uint32), cat.view(np.uint32))
    assert "overflow" in store._l.qn_kf_last_error(store.h).decode()
    n2 = store.build_map([0], [poses[0]], 0.3)                        # a normal build clears the warning
    assert n2 < 5000 and store._l.qn_kf_last_error(store.h).decode() == ""


def test_status_codes(store):
    from qn_amd import engine
    rng = np.random.default_rng(6)
    xyz, inten = _keyframes(rng, 1, 100)
    store.add(xyz[0], inten[0]); store.add(np.zeros((0, 3), np.float32))
    with pytest.raises(engine.EngineError) as e:
        store.build_map([], np.zeros((0, 16)), 0.3)
    assert e.value.status == engine.QN_ERR_EMPTY_CLOUD
    with pytest.raises(engine.EngineError) as e:
        store.build_map([1], [np.eye(4)], 0.3)
    assert e.value.status == engine.QN_ERR_EMPTY_CLOUD
    with pytest.raises(engine.EngineError) as e:
        store.build_map([0, 7], [np.eye(4)] * 2, 0.3)
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    a = np.ascontiguousarray(np.c_[xyz[0], inten[0]], np.float32); kid = C.c_int32()
    l = store._l
    for stride, off in ((16, 8), (16, 14), (16, 16), (18, 12), (32, 30)):
        assert l.qn_kf_add_xyzi(store.h, a.ctypes.data_as(C.c_void_p), C.c_uint32(25), C.c_uint32(stride), C.c_uint32(off), C.byref(kid)) == engine.QN_ERR_INVALID_ARG
        assert l.qn_kf_download_map(store.h, a.ctypes.data_as(C.c_void_p), C.c_uint32(stride), C.c_uint32(off)) == engine.QN_ERR_INVALID_ARG
    n = store.build_map([0], [np.eye(4)], 0.3)
    assert n > 0


def test_map_and_assemble_slots_are_isolated(store):
    rng = np.random.default_rng(7)
    xyz, inten = _keyframes(rng, 10, 6000)
    _fill(store, xyz, inten, [True] * 10)
    poses = [_pose(rng, 5.0) for _ in range(10)]
    _, n0 = store.assemble([0, 1], poses[:2], 0.3, 0)
    _, n1 = store.assemble([2, 3, 4], poses[2:5], 0.3, 1)
    a0, a1 = store.download(0, n0), store.download(1, n1)
    nm = store.build_map(list(range(10)), poses, 0.3)
    m = store.download_map(nm)
    assert np.array_equal(store.download(0, n0).view(np.uint32), a0.view(np.uint32)) and np.array_equal(store.download(1, n1).view(np.uint32), a1.view(np.uint32))
    store.assemble([5, 6, 7, 8], poses[5:9], 0.2, 0)
    store.assemble([9], poses[9:], 0.4, 1)
    assert np.array_equal(store.download_map(nm).view(np.uint32), m.view(np.uint32))


def test_strided_download_writes_only_xyz_and_intensity(store):
    rng = np.random.default_rng(8)
    xyz, inten = _keyframes(rng, 2, 5000)
    _fill(store, xyz, inten, [True, True])
    n = store.build_map([0, 1], [_pose(rng, 3.0), _pose(rng, 3.0)], 0.3)
    want = store.download_map(n)
    buf = np.full(32 * n, 0xA5, np.uint8)
    assert store._l.qn_kf_download_map(store.h, buf.ctypes.data_as(C.c_void_p), C.c_uint32(32), C.c_uint32(16)) == 0
    rec = buf.reshape(n, 32)
    assert np.array_equal(rec[:, :12].copy().view(np.float32).view(np.uint32), want[:, :3].view(np.uint32))
    assert np.array_equal(rec[:, 16:20].copy().view(np.float32)[:, 0].view(np.uint32), want[:, 3].view(np.uint32))
    assert (rec[:, 12:16] == 0xA5).all() and (rec[:, 20:] == 0xA5).all()


def test_map_scale_thirty_million_points(store):
    """500 keyframes x 60k points along a 400 m path, leaf 0.3 (save_voxel_resolution): the restatement bit for bit, two builds identical."""
    rng = np.random.default_rng(9)
    nkf, npts = 500, 60000
    xyz = [np.c_[rng.uniform(-30, 30, (npts, 2)), rng.uniform(-1.5, 3.5, npts)].astype(np.float32) for _ in range(nkf)]
    inten = [rng.uniform(0, 255, npts).astype(np.float32) for _ in range(nkf)]
    poses = []
    for k in range(nkf):
        a = 0.3 * np.sin(k / 60.0); T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; T[:3, 3] = [0.8 * k, 15.0 * np.sin(k / 50.0), 0.002 * k]
        poses.append(T)
    for x, i in zip(xyz, inten):
        store.add(x, i)
    ids = list(range(nkf))
    n = store.build_map(ids, poses, 0.3)
    got = store.download_map(n)
    n2 = store.build_map(ids, poses, 0.3)
    assert n2 == n and np.array_equal(store.download_map(n2).view(np.uint32), got.view(np.uint32))
    cat = np.concatenate([transform_xyzi(np.c_[xyz[k], inten[k]], poses[k]) for k in ids])
    del xyz
    want, of = voxel_grid_xyzi(cat, 0.3)
    assert not of and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_cpp_helper_gives_the_python_map(store, tmp_path):
    if not os.path.exists(MAP_BIN):
        build_map_program()
    rng = np.random.default_rng(10)
    xyz, inten = _keyframes(rng, 20, 4000)
    poses = [_pose(rng, 8.0) for _ in range(20)]
    with open(tmp_path / "kf.bin", "wb") as f:
        for x, i in zip(xyz, inten):
            f.write(np.uint32(len(x)).tobytes()); f.write(np.ascontiguousarray(np.c_[x, i], np.float32).tobytes())
    np.ascontiguousarray(poses, np.float64).tofile(tmp_path / "poses.bin")
    out = subprocess.check_output([MAP_BIN, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", str(tmp_path / "map.bin")], timeout=120).decode()
    cpp = np.fromfile(tmp_path / "map.bin", np.float32).reshape(-1, 4)
    _fill(store, xyz, inten, [True] * 20)
    n = store.build_map(list(range(20)), poses, 0.3)
    assert int(out.split()[0]) == n and np.array_equal(cpp.view(np.uint32), store.download_map(n).view(np.uint32))


def test_replay_writes_the_corrected_map(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import replay
    out = replay.run(n_kf=16, seed=7, verbose=False, save_dir=str(tmp_path), save_map_leaf=0.3)
    lines = open(tmp_path / "map.pcd").read().splitlines()
    assert "FIELDS x y z intensity" in lines and lines[10] == "DATA ascii"
    n = int(lines[9].split()[1])
    pts = np.array([[float(v) for v in l.split()] for l in lines[11:]], np.float32)
    assert n > 1000 and pts.shape == (n, 4) and (pts[:, 3] == 0).all()
    scans = replay.make_stream(16, 7)[0]
    cat = np.concatenate([transform_xyzi(s, T) for s, T in zip(scans, out["poses"])])
    want, _ = voxel_grid_xyzi(cat, 0.3)
    assert np.array_equal(pts, want)
