"""The 3-D occupancy map on the GPU (qn_kf_map_occupancy / _grid / _list / _slice) against its specification, the numpy twin qn_amd/mapoccupancy.py, run on the
records the store itself holds.  Both ray ends are quantised once and everything behind that is an integer, so everything is compared for equality: the hits,
misses and class of every voxel, every field of the statistics, the grid info, the lists, the slices, and a rerun.  No tolerance appears anywhere.  B is the
block of the record kernels (OC_BLOCK = MO_BLOCK): the record counts 1, 63, 64, 65, 255, 256, 257 and 1 025 per entry are their wave and launch seams."""
import numpy as np
import pytest
from qn_amd import mapoccupancy as mo, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
UNIT = (1.0, 0.0, 100.0, 1, 1, 2)                                    # voxel 1: the hand cases' coordinates are voxel coordinates


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _fetch(store):
    info, hits, misses, cls = store.map_occupancy_grid()
    return dict(info=info, hits=hits, misses=misses, classes=cls)


def equal_the_twin(store, clouds, poses, params, what, ids=None):
    """clouds[e]: the records of entry e, added to the store here unless ids names resident keyframes -> (the GPU results, the twin's)"""
    from qn_amd import engine
    if ids is None:
        ids = [store.add(np.ascontiguousarray(c, F).reshape(-1, 3)) for c in clouds]
    poses = np.asarray(poses, np.float64).reshape(len(ids), 4, 4)
    p = engine.OccupancyParams(*params)
    stats = store.map_occupancy(ids, poses, p)
    got = _fetch(store)
    want = mo.classify(clouds, poses, params)
    w = want["stats"]; g = want["grid"]
    print("%s: %d records, %d rays (%d non-finite, %d near, %d far), grid %d x %d x %d, %d misses, occupied %d free %d unknown %d"
          % (what, stats["n_records"], stats["n_rays"], stats["n_nonfinite"], stats["n_near"], stats["n_far"], stats["width"], stats["height"], stats["depth"],
             stats["total_misses"], stats["occupied"], stats["free"], stats["unknown"]))
    for f in mo.OccupancyStats._fields:
        assert stats[f] == getattr(w, f), (what, f, stats[f], getattr(w, f))
    assert tuple(got["info"][f] for f in mo.OccupancyGrid._fields) == tuple(g), (what, got["info"], g)
    for k in ("hits", "misses", "classes"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    for mask in (1 << mo.OCCUPIED, 1 << mo.FREE, (1 << mo.OCCUPIED) | (1 << mo.FREE), 7):
        a = store.map_occupancy_list(mask); b = mo.voxel_list(want, mask)
        assert all(_same(x, y) for x, y in zip(a, b)), (what, mask, len(a[0]), len(b[0]))
    D = g.depth
    for lo, hi in ((0, max(D - 1, 0)), (-5, 0), (D // 2, D // 2), (D - 1, D + 7), (D, D + 1), (-3, -1)):
        assert _same(store.map_occupancy_slice(lo, hi), mo.slice2d(want["classes"], lo, hi)), (what, lo, hi)
    # a rerun returns the same bytes
    again = store.map_occupancy(ids, poses, p); got2 = _fetch(store)
    assert again == stats and got2["info"] == got["info"] and all(_same(got2[k], got[k]) for k in ("hits", "misses", "classes")), what
    return got, want


def _pose(o, yaw=0.0, pitch=0.0):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = o
    return T


def _one_ray(store, o, w, shell, what):
    params = UNIT[:3] + (shell,) + UNIT[4:]
    return equal_the_twin(store, [np.array([np.subtract(w, o)], F)], [_pose(o)], params, what)[0]


def test_not_ready_before_the_first_call():
    from qn_amd import engine
    s = engine.KeyframeStore()
    try:
        L = engine.lib(); g = engine.OccupancyGrid(); n = engine.C.c_uint32(); out = np.zeros(4, np.uint8)
        assert L.qn_kf_map_occupancy_grid(s.h, engine.C.byref(g), None, None, None) == engine.QN_ERR_NOT_READY
        assert L.qn_kf_map_occupancy_list(s.h, 4, engine.C.byref(n), None, None, None) == engine.QN_ERR_NOT_READY
        assert L.qn_kf_map_occupancy_slice(s.h, 0, 0, out.ctypes.data_as(engine.C.c_void_p)) == engine.QN_ERR_NOT_READY
    finally:
        s.close()


@pytest.mark.parametrize("shell,misses", [(0, [1, 1, 1, 1, 1, 0]), (1, [1, 1, 1, 1, 0, 0]), (5, [0] * 6), (6, [0] * 6)])
def test_one_ray_along_x(store, shell, misses):
    got = _one_ray(store, (0.5, 0.5, 0.5), (5.5, 0.5, 0.5), shell, "+x, shell %d" % shell)
    assert got["hits"].ravel().tolist() == [0, 0, 0, 0, 0, 1] and got["misses"].ravel().tolist() == misses
    assert got["info"]["minc"] == (0, 0, 0) and got["classes"].ravel().tolist() == [1 if m else 0 for m in misses[:5]] + [2]
    # the same ray along -x from an origin exactly on a face: it leaves voxel 5 at once
    got = _one_ray(store, (5.0, 0.5, 0.5), (0.5, 0.5, 0.5), shell, "-x from a face, shell %d" % shell)
    assert got["hits"].ravel().tolist() == [1, 0, 0, 0, 0, 0] and got["misses"].ravel().tolist() == misses[::-1]


def test_diagonal_through_corners_and_a_ray_inside_one_voxel(store):
    got = _one_ray(store, (0.0, 0.0, 0.0), (3.0, 3.0, 3.0), 0, "diagonal")
    path = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2)]        # x before y before z at every corner
    want = np.zeros((4, 4, 4), np.uint32)
    for x, y, z in path:
        want[z, y, x] = 1
    assert np.array_equal(got["misses"], want) and got["hits"][3, 3, 3] == 1 and got["hits"].sum() == 1
    got = _one_ray(store, (0.25, 0.25, 0.25), (0.75, 0.5, 0.25), 0, "inside one voxel")
    assert got["hits"].tolist() == [[[1]]] and got["misses"].tolist() == [[[0]]] and got["classes"].tolist() == [[[2]]]


def _entry(rng, n, reach):
    """n records around the sensor, some of them skipped: a NaN, a near one, a far one"""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * rng.uniform(0.6, reach, (n, 1))).astype(F)
    if n >= 8:
        p[n // 2, 1] = np.nan; p[n // 3] = [0.1, 0.0, 0.1]; p[n // 4] = [200.0, 1.0, 0.0]; p[n // 5, 2] = np.inf
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_records_per_entry_at_the_launch_seams(store, n):
    rng = np.random.default_rng(500 + n)
    for entries in (1, 2, 5):
        clouds = [_entry(rng, n, 9.0) for _ in range(entries)]
        poses = [_pose(rng.uniform(-4, 4, 3), rng.uniform(-3, 3), rng.uniform(-0.4, 0.4)) for _ in range(entries)]
        got, _ = equal_the_twin(store, clouds, poses, mo.OccupancyParams(), "%d entries of %d records" % (entries, n))
        assert got["hits"].sum() >= entries * (n - 4 if n >= 8 else n)


@pytest.mark.parametrize("voxel", [0.3, 0.25, 1.0])
def test_repeated_empty_and_skipped_entries(store, voxel):
    """five entries: two of one keyframe under two poses, an empty keyframe, one whose records are all skipped, and an ordinary one"""
    rng = np.random.default_rng(int(voxel * 100))
    a, b = _entry(rng, 300, 12.0), _entry(rng, 129, 7.0)
    skipped = np.array([[np.nan, 0, 0], [0.1, 0.1, 0.1], [90.0, 0, 0], [0, np.inf, 0], [0.2, 0, 0]], F)
    ka, kb, ke, ks = store.add(a), store.add(b), store.add(np.zeros((0, 3), F)), store.add(skipped)
    poses = [_pose((0.3, -1.2, 0.5), 0.4), _pose((2.0, 1.0, 0.7), -2.0, 0.2), _pose((1, 1, 1)), _pose((-3.0, 0.5, 0.2), 1.0), _pose((0.15, 0.3, -0.6), 3.0, -0.3)]
    params = mo.OccupancyParams(voxel=voxel)
    got, want = equal_the_twin(store, [a, a, np.zeros((0, 3), F), skipped, b], poses, params, "voxel %g" % voxel, ids=[ka, ka, ke, ks, kb])
    s = want["stats"]
    assert s.n_records == 2 * 300 + 5 + 129 and s.n_nonfinite == 2 * 2 + 2 + 2 and s.n_near == 2 + 2 + 1 and s.n_far == 2 + 1 + 1 and s.n_rays == 2 * 296 + 125
    # an entry of skipped records alone: no ray, an empty grid
    got, _ = equal_the_twin(store, [skipped], [poses[3]], params, "skipped alone", ids=[ks])
    assert got["hits"].shape == (0, 0, 0) and got["info"]["minc"] == (0, 0, 0) and len(store.map_occupancy_list(7)[0]) == 0


def test_a_long_ray_beside_one_voxel_rays_in_one_wave(store):
    """record 0 walks more than 600 voxels while the 64 records behind it, which share its first wave and the next, end one voxel from the origin"""
    rng = np.random.default_rng(9)
    short = np.zeros((64, 3), F); short[:, 0] = 0.32 + rng.uniform(0, 0.05, 64); short[:, 1:] = rng.uniform(-0.02, 0.02, (64, 2))
    cloud = np.concatenate([np.array([[170.0, 31.0, 7.0]], F), short])
    params = (0.3, 0.1, 400.0, 1, 1, 2)
    got, want = equal_the_twin(store, [cloud], [_pose((0.05, 0.1, 0.1))], params, "long ray")
    A, B, _ = mo.rays([cloud], [_pose((0.05, 0.1, 0.1))], params)
    steps = np.abs((B >> mo.S) - (A >> mo.S)).sum(axis=1)
    assert steps[0] > 600 and (steps[1:] == 1).all() and got["misses"].sum() == steps[0] - 1


def test_contention_on_one_end_voxel(store):
    cloud = np.tile(np.array([[3.1, 2.2, 1.3]], F), (4096, 1))
    got, _ = equal_the_twin(store, [cloud], [_pose((0.1, 0.1, 0.1))], mo.OccupancyParams(), "4 096 rays into one voxel")
    assert got["hits"].max() == 4096 and got["hits"].sum() == 4096 and got["misses"].max() == 4096


def test_refusals_leave_the_previous_result_readable(store):
    from qn_amd import engine
    rng = np.random.default_rng(3)
    cloud = _entry(rng, 200, 8.0)
    kid = store.add(cloud)
    before, _ = equal_the_twin(store, [cloud], [_pose((1, 2, 3), 0.5)], mo.OccupancyParams(), "before the refusals", ids=[kid])

    def refused(status, ids, poses, p):
        with pytest.raises(engine.EngineError) as ei:
            store.map_occupancy(ids, poses, p)
        assert ei.value.status == status, (ei.value.status, status)
        now = _fetch(store)
        assert now["info"] == before["info"] and all(_same(now[k], before[k]) for k in ("hits", "misses", "classes"))

    ok = engine.OccupancyParams()
    refused(engine.QN_ERR_CAPACITY, [kid], [_pose((400000.0, 0, 0))], ok)                        # 400 000 / 0.3 >= 2^20 voxels
    with pytest.raises(mo.CapacityError):
        mo.classify([cloud], [_pose((400000.0, 0, 0))])
    refused(engine.QN_ERR_CAPACITY, [kid], [_pose((1, 2, 3))], engine.OccupancyParams(voxel=0.005))   # 16 m across at 5 mm: 3 200^3 voxels
    with pytest.raises(mo.CapacityError):
        mo.classify([cloud], [_pose((1, 2, 3))], mo.OccupancyParams(voxel=0.005))
    refused(engine.QN_ERR_CAPACITY, [kid, kid], [_pose((0, 0, 0)), _pose((9000.0, 0, 0))], engine.OccupancyParams(voxel=0.25))      # 36 000 voxels a side
    bad_pose = _pose((0, 0, 0)); bad_pose[1, 2] = np.nan
    refused(engine.QN_ERR_INVALID_ARG, [kid], [bad_pose], ok)
    refused(engine.QN_ERR_INVALID_ARG, [kid + 1000], [_pose((0, 0, 0))], ok)
    refused(engine.QN_ERR_INVALID_ARG, [-1], [_pose((0, 0, 0))], ok)
    for kw in (dict(voxel=0.0), dict(voxel=float("nan")), dict(min_range=-1.0), dict(max_range=0.5), dict(max_range=float("inf")), dict(min_hits=0), dict(hit_weight=0)):
        refused(engine.QN_ERR_INVALID_ARG, [kid], [_pose((0, 0, 0))], engine.OccupancyParams(**kw))
    r = engine.OccupancyParams(); r.reserved[1] = 1
    refused(engine.QN_ERR_INVALID_ARG, [kid], [_pose((0, 0, 0))], r)
    L = engine.lib(); st = engine.OccupancyStats(); ids = np.array([kid], np.int32); P = np.eye(4).reshape(-1)
    pp = lambda a: a.ctypes.data_as(engine.C.c_void_p)
    assert L.qn_kf_map_occupancy(store.h, pp(ids), pp(P), 0, engine.C.byref(ok), engine.C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy(store.h, pp(ids), pp(P), 1, None, engine.C.byref(st)) == engine.QN_ERR_INVALID_ARG
    n = engine.C.c_uint32()
    for mask in (0, 8, 9):
        assert L.qn_kf_map_occupancy_list(store.h, mask, engine.C.byref(n), None, None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy_slice(store.h, 2, 1, pp(np.zeros(4, np.uint8))) == engine.QN_ERR_INVALID_ARG
    now = _fetch(store)
    assert all(_same(now[k], before[k]) for k in ("hits", "misses", "classes"))


def test_a_map_build_does_not_end_the_result(store):
    rng = np.random.default_rng(4)
    cloud = _entry(rng, 100, 6.0)
    kid = store.add(cloud)
    before, _ = equal_the_twin(store, [cloud], [_pose((0, 0, 1))], mo.OccupancyParams(), "before a map build", ids=[kid])
    store.build_map([kid], [np.eye(4)], 0.2)
    now = _fetch(store)
    assert now["info"] == before["info"] and all(_same(now[k], before[k]) for k in ("hits", "misses", "classes"))


def test_street_scene(store):
    """the four ray-cast scans of the street scene (16 x 300 rays each), default parameters, in full against the twin (equal_the_twin runs it twice)"""
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    clouds = [store.keyframe(i)[:, :3] for i in ids]
    got, want = equal_the_twin(store, clouds, POSES, mo.OccupancyParams(), "street scene", ids=ids)
    s = want["stats"]
    assert s.n_rays > 15000 and s.occupied > 5000 and s.free > 100000 and s.unknown > s.free


def test_cpp_helper_gives_the_python_result(store, tmp_path):
    """tests/shim_map_occupancy.cpp (qn_map::mapOccupancy / occupiedVoxels / occupancySlice against the stand-ins) on two scans of the street scene"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_shim("shim_map_occupancy.cpp", tmp_path)
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES[:2], [11, 12])]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, F).tobytes())
    np.ascontiguousarray(np.array(POSES[:2], np.float64)).tofile(str(tmp_path / "poses.bin"))
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "2", "6"], text=True)
    from qn_amd import engine
    st = store.map_occupancy(ids, POSES[:2], engine.OccupancyParams(voxel=0.3))
    info = store.map_occupancy_grid()[0]
    ijk, hits, misses = store.map_occupancy_list(1 << mo.OCCUPIED)
    xyz = mo.centres(ijk, mo.OccupancyGrid(*(info[f] for f in mo.OccupancyGrid._fields))).astype(F)

    def fnv(chunks):
        h = 1469598103934665603
        for b in chunks:
            for x in b:
                h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
        return h
    hv = fnv(xyz[i].tobytes() + F(hits[i]).tobytes() + misses[i].tobytes() for i in range(len(ijk)))
    hs = fnv([store.map_occupancy_slice(2, 6).tobytes()])
    assert txt.splitlines() == ["occupancy %d %d %d %d %d %d %d %d" % (st["n_rays"], st["total_misses"], st["width"], st["height"], st["depth"], st["occupied"], st["free"],
                                                                    st["unknown"]),
                                "voxels %d %016x" % (len(ijk), hv), "slice %016x" % hs], txt
    assert len(ijk) == st["occupied"] > 1000
