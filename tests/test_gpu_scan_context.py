"""Scan Context loop candidates on the GPU (qn_kf_sc_*): descriptors, ring keys and column norms of resident keyframes equal the numpy twin
qn_amd/scancontext.py bit for bit (ray-cast and uniform keyframes, an adversarial and an empty one, other shapes); query results (ids, D, shifts,
order) equal the twin's, exhaustive and prefiltered, ties included; admissibility at the tdiff boundary; argument checks leave the store
unchanged; a scale case; retrieval of revisits on the street scene that the radius search cannot reach; the C++ helper."""
import ctypes as C
import math
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import scancontext as sc, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _store():
    from qn_amd import engine
    return engine.KeyframeStore()


def _u(a, dt):
    return np.ascontiguousarray(a).view(dt)


def _twin(store, kid, p):
    return sc.descriptor(store.keyframe(kid)[:, :3], p)


def _check_descriptors(store, ids, p):
    for kid in ids:
        d, rk, cn = store.sc_descriptor(kid)
        wd, wrk, wcn = _twin(store, kid, p)
        assert np.array_equal(_u(d, np.uint32), _u(wd, np.uint32)), "descriptor of keyframe %d differs from the twin" % kid
        assert np.array_equal(_u(rk, np.uint64), _u(wrk, np.uint64)), "ring key of keyframe %d differs" % kid
        assert np.array_equal(_u(cn, np.uint64), _u(wcn, np.uint64)), "column norms of keyframe %d differ" % kid


def _adversarial():
    nan, inf = float("nan"), float("inf")
    rows = [[nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, 0, 1], [0, -inf, 1], [1, 1, inf], [0, 0, 3], [-0.0, 0.0, 3],
            [80, 0, 1], [0, 80, 2], [-57, -57, 1], [1e30, 1e30, 1], [3e38, 0, 1],
            [4, 0, 1], [0, 8, 2], [-12, 0, 3], [0, -16, 4], [20, 0, 5], [79.99, 0, -1], [1, -1e-30, 1], [1, 1e-30, 7],
            [5, 5, 3.4e38], [6, 6, -3.4e38], [7, 7, -2.0], [7.01, 7, -2.5], [1e-40, 1e-40, 0.5], [-1e-44, 1e-45, 0.25]]
    return np.array(rows, np.float32)


def test_descriptors_are_bit_identical_to_the_twin():
    store = _store(); p = sc.Params()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    prims = synth.Scene(np.random.Generator(np.random.PCG64(3))).primitives()
    cast = list(store.add_lidar_scans(prims, sen, [synth.sensor_pose(3.0 * i, -2.0, 0.7 * i) for i in range(4)], [11, 12, 13, 14]))
    rng = np.random.default_rng(5)
    uni = [store.add(rng.uniform(-90, 90, (n, 3)).astype(np.float32)) for n in (1, 100, 20000, 100000)]
    adv = store.add(_adversarial())
    empty = store.add(np.zeros((0, 3), np.float32))
    ids = cast + uni + [adv, empty]
    store.sc_describe(ids)
    _check_descriptors(store, ids, p)
    d, rk, cn = store.sc_descriptor(empty)
    assert not d.any() and not rk.any() and not cn.any()
    store.sc_describe(ids + ids[::-1])                                 # again, repeats: idempotent
    _check_descriptors(store, ids, p)
    store.close()


@pytest.mark.parametrize("shape", [(7, 13, 25.0, -1.5), (64, 128, 120.0, 0.0), (1, 1, 80.0, 2.0), (3, 360, 10.0, 1.0), (40, 2, 50.0, 2.0)])
def test_other_shapes_are_bit_identical_to_the_twin(shape):
    nr, ns, R, h = shape
    store = _store()
    p = sc.Params(n_rings=nr, n_sectors=ns, max_radius=R, lidar_height=h)
    store.sc_set_params(n_rings=nr, n_sectors=ns, max_radius=R, lidar_height=h)
    rng = np.random.default_rng(nr * 1000 + ns)
    ids = [store.add(rng.uniform(-1.2 * R, 1.2 * R, (n, 3)).astype(np.float32)) for n in (5000, 300)] + [store.add(_adversarial())]
    store.sc_describe(ids)
    _check_descriptors(store, ids, p)
    descs = {k: _twin(store, k, p) for k in ids}
    got = store.sc_query([ids[0]], np.array([10.0, 0.0, 0.0]), -1.0, 5)[0]
    want = sc.query(descs, ids[0], [10.0, 0.0, 0.0], -1.0, 5)
    assert [(int(a), float(b), int(c)) for a, b, c in zip(*got)] == want
    store.close()


def _same(got, want):
    ids, D, sh = got
    assert len(ids) == len(want), (ids, want)
    assert list(ids) == [w[0] for w in want] and list(sh) == [w[2] for w in want], (list(zip(ids, D, sh)), want)
    assert np.array_equal(_u(np.asarray(D, np.float64), np.uint64), _u(np.array([w[1] for w in want], np.float64), np.uint64)), (D, want)


def _query_store(seed=21, n_kf=40):
    """keyframes of a few places (ray-cast) with repeats: the same scan under several ids, so ties must go to the lower id"""
    store = _store()
    sen = synth.SpinningLidar(n_beams=16, n_cols=360)
    prims = synth.Scene(np.random.Generator(np.random.PCG64(seed))).primitives()
    rng = np.random.default_rng(seed)
    poses = [synth.sensor_pose(*rng.uniform(-30, 30, 2), rng.uniform(-math.pi, math.pi)) for _ in range(n_kf // 2)]
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 7))
    dup = [store.add(store.keyframe(ids[k % 5])[:, :3]) for k in range(n_kf - len(ids))]
    return store, ids + dup


@pytest.mark.parametrize("prefilter", [0, 3, 12, 1024])
def test_query_is_bit_identical_to_the_twin(prefilter):
    store, ids = _query_store()
    p = sc.Params(ringkey_prefilter=prefilter)
    store.sc_set_params(ringkey_prefilter=prefilter)
    store.sc_describe(ids)
    descs = {k: _twin(store, k, p) for k in ids}
    stamps = np.arange(len(ids)) * 2.0
    queries = [len(ids) - 1, len(ids) - 2, 30, 25, 7, 0]
    for k in (1, 4, 50):
        res = store.sc_query(queries, stamps, 3.0, k)
        for q, got in zip(queries, res):
            _same(got, sc.query(descs, q, stamps, 3.0, k, prefilter=prefilter))
    store.close()


def test_ties_go_to_the_lower_id():
    store, ids = _query_store()
    store.sc_describe(ids)
    stamps = np.arange(len(ids)) * 2.0
    ids_q, D, _ = store.sc_query([39], stamps, 3.0, 40)[0]
    # keyframe 39 repeats keyframe 4 (as does 24, 29, 34): they are all at distance 0, in id order
    zero = [int(i) for i, d in zip(ids_q, D) if d == 0.0]
    assert zero == [4, 24, 29, 34], list(zip(ids_q, D))
    store.close()


def test_admissibility_follows_stamps_exactly():
    store, ids = _query_store(n_kf=12)
    store.sc_describe(ids)
    stamps = np.array([0.0, 0.1, 0.2, 0.3, 1.0, 2.5, 2.5, 3.0, 3.5, 4.0, 4.9, 5.0])
    for tdiff in (0.0, 2.5, 4.0, 4.9, 5.0, -1.0, float("inf"), -float("inf")):
        got = set(store.sc_query([11], stamps, tdiff, 20)[0][0].tolist())
        want = {c for c in range(12) if c != 11 and stamps[11] - stamps[c] > tdiff}
        assert got == want, (tdiff, got, want)
    assert 4 not in set(store.sc_query([11], stamps, 4.0, 20)[0][0].tolist())     # 5.0 - 1.0 == 4.0: excluded
    # undescribed keyframes are not candidates; an undescribed query is not ready
    s2 = _store()
    a = [s2.add(store.keyframe(k)[:, :3]) for k in range(4)]
    s2.sc_describe([a[0], a[3]])
    assert s2.sc_query([3], [0, 1, 2, 9.0], 0.5, 5)[0][0].tolist() == [0]
    from qn_amd import engine
    with pytest.raises(engine.EngineError) as ei:
        s2.sc_query([2], [0, 1, 2, 9.0], 0.5, 5)
    assert ei.value.status == engine.QN_ERR_NOT_READY
    store.close(); s2.close()


def test_argument_checks_leave_the_store_unchanged():
    from qn_amd import engine
    store, ids = _query_store(n_kf=10)
    l, h = store._l, store.h
    ids_a = np.array(ids, np.int32)
    stamps = np.arange(10) * 3.0
    out_i = np.zeros(40, np.int32); out_d = np.zeros(40); out_s = np.zeros(40, np.int32); out_n = np.zeros(4, np.uint32)

    def query(q, st, tdiff, k, n_st=None):
        q = np.ascontiguousarray(q, np.int32)
        return l.qn_kf_sc_query(h, q.ctypes.data_as(C.c_void_p), C.c_uint32(len(q)), st.ctypes.data_as(C.c_void_p), C.c_uint32(len(st) if n_st is None else n_st),
                                C.c_double(tdiff), C.c_uint32(k), out_i.ctypes.data_as(C.c_void_p), out_d.ctypes.data_as(C.c_void_p),
                                out_s.ctypes.data_as(C.c_void_p), out_n.ctypes.data_as(C.c_void_p))
    assert query([9], stamps, 1.0, 3) == engine.QN_ERR_NOT_READY                        # nothing described yet
    bad = np.array([3, 10], np.int32)
    assert l.qn_kf_sc_describe(h, bad.ctypes.data_as(C.c_void_p), C.c_uint32(2)) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_sc_get(h, C.c_int32(3), None, None, None) == engine.QN_ERR_NOT_READY  # the good id of the refused list was not described
    assert l.qn_kf_sc_describe(h, ids_a.ctypes.data_as(C.c_void_p), C.c_uint32(0)) == engine.QN_ERR_INVALID_ARG
    store.sc_describe(ids)
    before = [store.sc_descriptor(k) for k in ids]
    want = store.sc_query([9, 8], stamps, 1.0, 3)
    for args in [([10], stamps, 1.0, 3), ([-1], stamps, 1.0, 3), ([9], stamps, float("nan"), 3), ([9], stamps, 1.0, 0), ([9], stamps, 1.0, 1025),
                 ([9], stamps[:9], 1.0, 3), ([], stamps, 1.0, 3)]:
        assert query(*args) == engine.QN_ERR_INVALID_ARG, args
    for bad_p in [dict(n_rings=0), dict(n_rings=65), dict(n_sectors=0), dict(n_sectors=361), dict(n_rings=64, n_sectors=360), dict(max_radius=0.0),
                  dict(max_radius=float("nan")), dict(max_radius=float("inf")), dict(lidar_height=float("nan")), dict(lidar_height=1e5), dict(ringkey_prefilter=1025)]:
        with pytest.raises(engine.EngineError) as ei:
            store.sc_set_params(**bad_p)
        assert ei.value.status == engine.QN_ERR_INVALID_ARG, bad_p
    p = store.sc_params()
    assert (p.n_rings, p.n_sectors, p.max_radius, p.lidar_height, p.ringkey_prefilter) == (20, 60, 80.0, 2.0, 0)
    for k, b in zip(ids, before):
        a = store.sc_descriptor(k)
        assert all(np.array_equal(_u(x, np.uint8), _u(y, np.uint8)) for x, y in zip(a, b))
    again = store.sc_query([9, 8], stamps, 1.0, 3)
    assert all(np.array_equal(x, y) for g, w in zip(again, want) for x, y in zip(g, w))
    # the prefilter alone keeps the descriptors; a shape change discards them
    store.sc_set_params(ringkey_prefilter=4)
    assert np.array_equal(store.sc_descriptor(9)[0], before[9][0])
    store.sc_set_params(n_rings=10, ringkey_prefilter=4)
    with pytest.raises(engine.EngineError) as ei:
        store.sc_descriptor(9)
    assert ei.value.status == engine.QN_ERR_NOT_READY
    assert query([9], stamps, 1.0, 3) == engine.QN_ERR_NOT_READY
    store.sc_describe([9, 2])
    assert store.sc_descriptor(9)[0].shape == (10, 60)
    assert store.sc_query([9], stamps, 1.0, 5)[0][0].tolist() == [2]
    store.close()


def test_scale_many_keyframes_and_queries_in_one_call():
    store = _store()
    rng = np.random.default_rng(77)
    N = 3000
    centres = rng.uniform(-40, 40, (N, 2))
    ids = [store.add(np.c_[rng.uniform(-30, 30, (60, 2)) + centres[k] * 0.2, rng.uniform(-2, 6, 60)].astype(np.float32)) for k in range(N)]
    store.sc_describe(ids)
    stamps = np.arange(N) * 1.0
    queries = list(range(N - 1, N - 1 - 1500, -1))
    for prefilter in (0, 16):
        store.sc_set_params(ringkey_prefilter=prefilter)
        res = store.sc_query(queries, stamps, 10.0, 5)
        assert len(res) == len(queries) and all(len(r[0]) == 5 for r in res)
        p = sc.Params(ringkey_prefilter=prefilter)
        spot = [0, 777, 1499]
        need = set(ids)
        descs = {k: sc.descriptor(store.keyframe(k)[:, :3], p) for k in need}
        for s in spot:
            _same(res[s], sc.query(descs, queries[s], stamps, 10.0, 5, prefilter=prefilter))
    store.close()


def _street():
    """places seen first under one heading and revisited 0.4 m away under another, among distractor keyframes elsewhere"""
    rng = np.random.Generator(np.random.PCG64(4242))
    scene = synth.Scene(rng, 120.0)
    spots = []
    while len(spots) < 10:
        x, y = rng.uniform(-35, 35, 2)
        if synth._free_spot(scene, x, y, 2.0) and all(math.hypot(x - a, y - b) > 12 for a, b in spots):
            spots.append((x, y))
    places, distract = spots[:4], spots[4:]
    poses = [synth.sensor_pose(x, y, rng.uniform(-math.pi, math.pi)) for x, y in places + distract]
    poses += [synth.sensor_pose(x + 0.3, y - 0.25, rng.uniform(-math.pi, math.pi)) for x, y in places]
    return scene.primitives(), poses


def test_revisits_are_found_where_the_radius_search_finds_nothing():
    from qn_amd import engine
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = _store()
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100))
    store.sc_describe(ids)
    stamps = np.arange(len(ids)) * 10.0
    # corrected poses after drift: each revisit is placed 200 m further off, beyond loop_detection_radius of every older keyframe
    pos = np.array([P[:3, 3] for P in poses]); pos[10:, 0] += 200.0 * np.arange(1, 5)
    revisits = list(range(10, 14))
    res = store.sc_query(revisits, stamps, 5.0, 3)
    for q, (cid, D, sh) in zip(revisits, res):
        place = q - 10
        assert len(engine.loop_candidates(pos, stamps[:q + 1], q, 12.0, 5.0)) == 0
        assert int(cid[0]) == place, (q, cid, D)
        assert D[0] < 0.3 and D[1] > 0.4, D
        hq = math.atan2(poses[q][1, 0], poses[q][0, 0]); hc = math.atan2(poses[place][1, 0], poses[place][0, 0])
        err = (sc.yaw_of_shift(int(sh[0]), 60) - (hc - hq) + math.pi) % (2 * math.pi) - math.pi
        assert abs(err) <= 2 * math.pi / 60, (q, sh[0], hc - hq)
    store.close()


def test_cpp_helper_returns_the_python_candidates(tmp_path):
    exe = build_shim("shim_scan_context.cpp", tmp_path)
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    clouds = [synth.lidar_scan(prims, sen, P, 100 + k)[:, :3] for k, P in enumerate(poses)]
    stamps = np.arange(len(clouds)) * 10.0
    with open(tmp_path / "kf.bin", "wb") as f:
        for c in clouds:
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    stamps.tofile(tmp_path / "st.bin")
    store = _store()
    ids = [store.add(c) for c in clouds]
    store.sc_describe(ids)
    for q in (10, 13):
        out = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "st.bin"), str(q), "5.0", "4", "0.5"], text=True).split("\n")
        got = [tuple(l.split()) for l in out if l.strip()]
        cid, D, sh = store.sc_query([q], stamps, 5.0, 4)[0]
        want = [(int(i), float(d), sc.yaw_of_shift(int(s), 60)) for i, d, s in zip(cid, D, sh) if d < 0.5]
        assert len(want) >= 1 and [int(g[0]) for g in got] == [w[0] for w in want]
        assert all(float(g[1]) == w[1] and abs(float(g[2]) - w[2]) < 1e-12 for g, w in zip(got, want)), (got, want)
    store.close()
