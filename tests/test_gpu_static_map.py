"""The static map on the GPU (qn_kf_static_classify / qn_kf_static_points / qn_kf_build_map_static) against its specification, the numpy twin
qn_amd/staticmap.py, on the ray-cast stream of tests/test_static_map_twin.py: 12 scans of a 32 x 900 spinning LiDAR, a 4 x 2 x 1.5 m box that is somewhere
else in every scan.  Bit for bit: seen_through, agree and removed of every record of every entry; the map, byte for byte and in order, against build_map on
a second store filled with the twin's kept records; a rerun; and every refusal leaves the previous classify and the map slot as they were."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import freespace as fs, staticmap as sm, synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 12
SEN = synth.SpinningLidar(n_beams=32, n_cols=900)
WIDE = synth.SpinningLidar(n_beams=16, n_cols=4608)                 # more than 4096 columns: the column table is read from global memory


def _stream(store, sensor, n):
    """scan s of the twin test's stream, ray-cast on the GPU (the box is a primitive of scan s only: one call per scan) -> ids, poses"""
    static = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    poses = [synth.sensor_pose(-8.0 + 1.5 * s, 0.3 * np.sin(0.5 * s), 0.05 * s) for s in range(n)]
    ids = []
    for s in range(n):
        box = np.array([(synth.PRIM_BOX, (-20.0 + 3.5 * s, 6.0, 4.0, 2.0, 1.5, 0.0))], dtype=synth.PRIM_DTYPE)
        ids.append(int(store.add_lidar_scans(np.concatenate([static, box]), sensor, [poses[s]], [100 + s])[0]))
    return ids, poses


def _extra_clouds():
    rng = np.random.default_rng(5)
    a = rng.normal(0, 12, (5000, 3)).astype(np.float32); a[:, 2] = np.abs(a[:, 2]) * 0.1 - 1.5
    a[7] = [np.nan, 1, 1]; a[8] = [3, np.inf, 0]; a[9] = [1, 2, -np.inf]; a[10] = [0, 0, 0]
    return a, np.zeros((0, 3), np.float32)


@pytest.fixture(scope="module")
def world():
    from qn_amd import engine
    store = engine.KeyframeStore()
    ids, poses = _stream(store, SEN, S)
    odd, empty = _extra_clouds()
    ODD = store.add(odd); EMPTY = store.add(empty)
    clouds = {i: store.keyframe(i) for i in ids + [ODD, EMPTY]}
    params = engine.RangeParams.for_sensor(SEN)
    store.range_set_params(params)
    store.range_describe(ids + [ODD, EMPTY])
    yield dict(store=store, ids=ids, poses=poses, clouds=clouds, params=params, ODD=ODD, EMPTY=EMPTY, has_i={**{i: True for i in ids}, ODD: False, EMPTY: False})
    store.close()


def _twin(world, ids, poses, wit, p, rule=None):
    return sm.classify(world["clouds"], ids, poses, wit[0], wit[1], p, rule)


def _equal_the_twin(store, got, want, what):
    for e, w in enumerate(want):
        st, ag, rm = store.static_points(e)
        assert st.dtype == np.uint8 and len(st) == len(w["removed"]), (what, e)
        assert np.array_equal(st, w["seen_through"]), (what, e, int((st != w["seen_through"]).sum()))
        assert np.array_equal(ag, w["agree"]), (what, e, int((ag != w["agree"]).sum()))
        assert np.array_equal(rm, w["removed"].astype(np.uint8)), (what, e)
        assert int(got["removed"][e]) == int(w["removed"].sum()), (what, e)
    print(what, "removed per entry", got["removed"].tolist())


def _lists(world):
    """name -> (ids, poses, witnesses or None for the helper's)"""
    ids, poses, ODD, EMPTY = world["ids"], world["poses"], world["ODD"], world["EMPTY"]
    rep_ids = [ids[3], ids[4], ids[5], ids[4], ODD, EMPTY, ids[6], ids[3]]                       # ids repeat; an entry without records; one with non-finite records
    rep_poses = [poses[3], poses[4], poses[5], poses[4], synth.sensor_pose(-1.0, 0.5, 0.1), poses[2], poses[6], synth.sensor_pose(-3.4, 0.2, 0.16)]
    return dict(window2=(ids, poses, sm.window_witnesses(ids, 2)), helper=(ids, poses, None), repeated=(rep_ids, rep_poses, sm.window_witnesses(rep_ids, 3)),
                repeated_helper=(rep_ids, rep_poses, None))


@pytest.mark.parametrize("window", [(1, 1), (0, 0)])
@pytest.mark.parametrize("name", ["window2", "helper", "repeated", "repeated_helper"])
def test_votes_equal_the_twin(world, name, window):
    from qn_amd import engine
    store = world["store"]
    ids, poses, wit = _lists(world)[name]
    p = engine.RangeParams.for_sensor(SEN, window_rows=window[0], window_cols=window[1])
    store.range_set_params(p)                                       # (the images do not depend on the window)
    try:
        got = store.static_classify(ids, poses, witnesses=wit, radius=4.0, max_k=3)
        if wit is None:
            off, w = sm.witnesses(ids, poses, 4.0, 3)
            assert np.array_equal(got["wit_off"], off) and np.array_equal(got["wit"], w) and len(w) > len(ids)
        want = _twin(world, ids, poses, (got["wit_off"], got["wit"]), p.twin())
        _equal_the_twin(store, got, want, "%s %s" % (name, window))
        assert got["status"] == [engine.QN_ERR_EMPTY_CLOUD if i == world["EMPTY"] else 0 for i in ids]
        assert sum(int(r["removed"].sum()) for r in want) > 500    # (the comparison is not of empty sets)
        if name.startswith("repeated"):
            odd = ids.index(world["ODD"])
            assert not store.static_points(odd)[2][7:10].any()     # the non-finite records stay
    finally:
        store.range_set_params(world["params"])


@pytest.mark.parametrize("rule", [(1, 0), (3, 2), (2, 0xFFFFFFFF)])
def test_another_rule(world, rule):
    from qn_amd import engine
    store, ids, poses = world["store"], world["ids"][2:9], world["poses"][2:9]
    wit = sm.window_witnesses(ids, 3)
    got = store.static_classify(ids, poses, witnesses=wit, params=engine.StaticParams(*rule))
    _equal_the_twin(store, got, _twin(world, ids, poses, wit, world["params"].twin(), sm.StaticParams(*rule)), str(rule))


def test_more_than_4096_columns_on_a_store_of_their_own():
    from qn_amd import engine
    store = engine.KeyframeStore()
    try:
        ids, poses = _stream(store, WIDE, 4)
        w = dict(clouds={i: store.keyframe(i) for i in ids})
        p = engine.RangeParams.for_sensor(WIDE)
        assert p.n_cols == 4608
        store.range_set_params(p)
        store.range_describe(ids)
        wit = sm.window_witnesses(ids, 3)
        got = store.static_classify(ids, poses, witnesses=wit)
        want = _twin(w, ids, poses, wit, p.twin())
        _equal_the_twin(store, got, want, "16x4608")
        assert sum(int(r["removed"].sum()) for r in want) > 100
    finally:
        store.close()


def _second_store_map(engine, world, ids, poses, kept, leaf):
    """build_map on a store filled with the kept records of every entry (one keyframe per entry)"""
    other = engine.KeyframeStore()
    try:
        k2 = [other.add(c[:, :3], c[:, 3]) if world["has_i"][i] else other.add(c[:, :3]) for i, c in zip(ids, kept)]
        n = other.build_map(k2, poses, leaf)
        return other.download_map(n)
    finally:
        other.close()


def _in_corridor(m):
    """map points where the box passed (x -22 .. 20.5 at y 6 +- 1), above the ground"""
    return int(((m[:, 0] > -22.0) & (m[:, 0] < 20.5) & (np.abs(m[:, 1] - 6.0) < 1.0) & (m[:, 2] > 0.3) & (m[:, 2] < 1.6)).sum())


@pytest.mark.parametrize("name", ["window2", "repeated"])
def test_the_map_equals_build_map_of_the_kept_records(world, name):
    from qn_amd import engine
    store = world["store"]
    ids, poses, wit = _lists(world)[name]
    store.static_classify(ids, poses, witnesses=wit)
    want = _twin(world, ids, poses, wit, world["params"].twin())
    kept = sm.static_clouds(world["clouds"], ids, want)
    for leaf in (0.3, 1.0):
        n = store.build_map_static(leaf)
        got = store.download_map(n)
        ref = _second_store_map(engine, world, ids, poses, kept, leaf)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (name, leaf, got.shape, ref.shape)
        plain = store.download_map(store.build_map(ids, poses, leaf))
        print(name, "leaf", leaf, "plain map", len(plain), "static map", n, "in the corridor", _in_corridor(plain), _in_corridor(got), "the twin leaves", _in_corridor(ref))
        assert len(plain) > n
        if name == "window2":
            assert _in_corridor(plain) > 0 and _in_corridor(got) <= _in_corridor(ref)
        assert store.build_map_static(leaf) == n and store.download_map(n).tobytes() == got.tobytes()      # after a plain map, again


def test_a_rerun_is_bitwise_identical(world):
    store = world["store"]
    ids, poses, wit = _lists(world)["repeated"]
    runs = []
    for _ in range(2):
        got = store.static_classify(ids, poses, witnesses=wit)
        pts = [store.static_points(e) for e in range(len(ids))]
        m = store.download_map(store.build_map_static(0.4))
        runs.append((got["removed"].tobytes(), [tuple(a.tobytes() for a in p) for p in pts], m.tobytes()))
    assert runs[0] == runs[1]


def test_refused_calls_change_nothing(world):
    from qn_amd import engine
    store, ids, poses = world["store"], world["ids"], world["poses"]
    wit = sm.window_witnesses(ids, 2)
    store.static_classify(ids, poses, witnesses=wit)
    n_map = store.build_map_static(0.5)
    before_pts = [store.static_points(e) for e in range(S)]
    before_map = store.download_map(n_map)
    sizes = list(store._static_n)
    late = store.add(world["clouds"][ids[0]][:, :3])                # a keyframe without images
    two, P2 = [ids[0], ids[1]], [poses[0], poses[1]]
    w2 = (np.array([0, 1, 2], np.uint32), np.array([1, 0], np.uint32))
    nanP = poses[0].copy(); nanP[1, 3] = np.nan
    infP = poses[1].copy(); infP[0, 0] = np.inf
    bad = engine.QN_ERR_INVALID_ARG
    cases = [(([], np.zeros((0, 4, 4)), (np.zeros(1, np.uint32), np.zeros(0, np.uint32))), {}, bad),                    # count == 0
             (([ids[0], -1], P2, w2), {}, bad), (([ids[0], late + 1], P2, w2), {}, bad),                                # a bad id
             ((two, [nanP, poses[1]], w2), {}, bad), ((two, [poses[0], infP], w2), {}, bad),                            # a non-finite pose
             (([ids[0], late], P2, w2), {}, bad),                                                                       # a witness without images
             ((two, P2, (np.array([0, 1, 2], np.uint32), np.array([1, 2], np.uint32))), {}, bad),                       # a witness position >= count
             ((two, P2, (np.array([0, 1, 2], np.uint32), np.array([0, 0], np.uint32))), {}, bad),                       # the entry itself
             (([ids[0], ids[1], ids[0]], P2 + [poses[2]], (np.array([0, 1, 2, 3], np.uint32), np.array([1, 0, 0], np.uint32))), {}, bad),      # the entry's own id
             ((two, P2, (np.array([0, 2, 1], np.uint32), np.array([1, 0], np.uint32))), {}, bad),                       # a non-monotone wit_off
             ((two, P2, w2), dict(params=engine.StaticParams(0, 1)), bad),                                              # a bad parameter
             ((two, P2, (np.array([0, 256, 256], np.uint32), np.full(256, 1, np.uint32))), {}, engine.QN_ERR_CAPACITY)]  # more than 255 witnesses
    for args, kw, code in cases:
        with pytest.raises(engine.EngineError) as e:
            store.static_classify(args[0], args[1], witnesses=args[2], **kw)
        assert e.value.status == code, (args[0], code)
    l = engine.lib()
    one = np.zeros(4, np.uint8)
    assert l.qn_kf_static_points(store.h, C.c_uint32(S), one.ctypes.data_as(C.c_void_p), None, None) == bad
    assert l.qn_kf_static_points(store.h, C.c_uint32(0), None, None, None) == bad
    for leaf in (0.0, -1.0, float("nan")):
        with pytest.raises(engine.EngineError) as e:
            store.build_map_static(leaf)
        assert e.value.status == bad
    store._static_n = sizes                                         # (the wrapper's own bookkeeping of the refused calls)
    for e in range(S):
        assert all(np.array_equal(x, y) for x, y in zip(before_pts[e], store.static_points(e)))
    store._map_n = n_map
    assert store.download_map(n_map).tobytes() == before_map.tobytes()
    only_rm = np.zeros(sizes[3], np.uint8)                          # any output may be NULL, not all
    assert l.qn_kf_static_points(store.h, C.c_uint32(3), None, None, only_rm.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(only_rm, before_pts[3][2])
    assert store.build_map_static(0.5) == n_map and store.download_map(n_map).tobytes() == before_map.tobytes()


def test_not_ready_before_a_classify(world):
    from qn_amd import engine
    store = engine.KeyframeStore()
    try:
        a = store.add(world["clouds"][world["ids"][0]][:, :3]); b = store.add(world["clouds"][world["ids"][1]][:, :3])
        store._static_n = [10, 10]
        with pytest.raises(engine.EngineError) as e:
            store.static_points(0)
        assert e.value.status == engine.QN_ERR_NOT_READY
        n = store.build_map([a, b], world["poses"][:2], 0.5)
        m = store.download_map(n)
        with pytest.raises(engine.EngineError) as e:
            store.build_map_static(0.5)
        assert e.value.status == engine.QN_ERR_NOT_READY
        assert store._map_n == n and store.download_map(n).tobytes() == m.tobytes()       # the map slot is as it was
        with pytest.raises(engine.EngineError) as e:                                       # no images yet: refused, and still nothing to read
            store.static_classify([a, b], world["poses"][:2], witnesses=sm.window_witnesses([a, b], 1))
        assert e.value.status == engine.QN_ERR_INVALID_ARG
        with pytest.raises(engine.EngineError) as e:
            store.build_map_static(0.5)
        assert e.value.status == engine.QN_ERR_NOT_READY
        # without any witness nothing needs an image: nothing is removed and the static map is the plain map
        got = store.static_classify([a, b], world["poses"][:2], witnesses=(np.zeros(3, np.uint32), np.zeros(0, np.uint32)))
        assert got["removed"].tolist() == [0, 0] and not store.static_points(1)[0].any()
        assert store.build_map_static(0.5) == n and store.download_map(n).tobytes() == m.tobytes()
    finally:
        store.close()


def test_cpp_helper_gives_the_python_result(world, tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_static_map.cpp", tmp_path)
    ids, poses = world["ids"][:6], world["poses"][:6]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = world["clouds"][i]
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    np.ascontiguousarray(poses, np.float64).tofile(tmp_path / "poses.bin")
    with open(tmp_path / "rp.bin", "wb") as f:
        f.write(bytes(world["params"]))
    out = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), str(tmp_path / "rp.bin"), "3.5", "4", "0.3"], text=True).splitlines()
    store = world["store"]
    got = store.static_classify(ids, poses, radius=3.5, max_k=4)
    m = store.download_map(store.build_map_static(0.3))
    h = 1469598103934665603
    for b in m.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert out[0].split() == ["witnesses"] + [str(int(w)) for w in got["wit"]]
    assert [l.split() for l in out[1:1 + len(ids)]] == [["removed", str(e), str(int(got["removed"][e])), "0"] for e in range(len(ids))]
    assert out[1 + len(ids)].split() == ["map", str(len(m)), str(h)]
    assert int(got["removed"].sum()) > 500


def test_the_three_kernels_have_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_static_vote", "k_static_scan", "k_static_compact"):
        rows = [l for l in out.splitlines() if re.search(r"\b%s\b" % k, l)]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows
