"""Many queries in one drift-free verification (qn_kf_verify_loop_pairs / KeyframeStore.verify_loop_pairs, the coarse-to-fine qn_kf_verify_loop_pairs_c2f)
and the debug clouds of a verified pair (qn_kf_verify_cloud), on the street scene of tests/test_gpu_sc_verify.py: every pair's record equals the
single-query call for that pair bit for bit (pairs shuffled, candidates shared between queries), the batch slot holds each distinct query and candidate
window once, byte-identical to the single-query call's segment, street revisits verified in one call land on inv(P_place) P_revisit, refused arguments
change nothing, an empty window sits beside valid pairs, SRC / DST / COARSE / FINAL equal their one-pair restatements, the C++ helpers, and the replay's
catch-up timer.

Tolerance: 0.05 m / 0.2 degrees, as tests/test_gpu_sc_verify.py and tests/test_gpu_kf_quatro.py (the same pairs, calibrated there on the CPU oracle).
Catch-up replay: spinning sensor, n_kf 66, seed 7, yaw_bias 0.02, loop_every 4 - chosen on the oracle backend, where the latest-only timer closes no loop
(the centre crossing at keyframe 33 falls between two ticks) and catch-up closes (33, 0), ATE 22.2 -> 7.9 m."""
import ctypes as C
import math
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import scancontext as sc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_sc_verify as scv                                                   # noqa: E402  (the street scene and its drifted poses)
from shim_build import build_shim

TOL_T, TOL_R = 0.05, math.radians(0.2)
LEAF, RANGE, MAX_CORR, CAP, GCAP = 0.3, 5, 18.0, 60000, 200000
QUERIES = [8, 9, 10, 11, 12, 13]


def _records(ptr, n):
    from qn_amd import engine
    out = np.zeros((n, 4), np.float32)
    if n:
        l = engine.lib(); l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; l.hipMemcpy.restype = C.c_int
        assert l.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), 16 * n, 2) == 0
    return out


def _ctx(engine, quatro=False, cap=CAP):
    ctx = engine.Context(cap)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    if quatro:
        engine.Quatro(ctx)
    return ctx


@pytest.fixture(scope="module")
def street():
    from qn_amd import engine
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100)]
    store.sc_describe(ids)
    ctx = _ctx(engine, quatro=True)
    assert store.quatro_describe(ctx, ids, LEAF) == [0] * len(ids)
    stamps = np.arange(len(ids)) * 10.0
    # 2-4 Scan Context candidates per query, flat and shuffled
    pairs = []
    for q, (cid, _, sh) in zip(QUERIES, store.sc_query(QUERIES, stamps, 5.0, 4)):
        k = 2 + q % 3
        pairs += [(q, int(c), sc.yaw_of_shift(int(s), 60)) for c, s in list(zip(cid, sh))[:k]]
    rng = np.random.default_rng(5)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    gctx = _ctx(engine, cap=GCAP)                                                  # (the candidate windows are larger than one scan)
    yield dict(store=store, ctx=ctx, gctx=gctx, poses=poses, drift=scv._drifted(poses), stamps=stamps, pairs=pairs, prims=prims, sen=sen)
    gctx.close(); ctx.close(); store.close()


def _grec(o):
    r = o["record"]
    return (o["status"], o["valid"], r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def _crec(o):
    return (o["status"], o["valid"], o["iterations"], o["converged"], o["score"], o["T"].tobytes(), o["T_quatro"].tobytes(), o["T_gicp"].tobytes())


def _segments(store):
    return [store.download_batch(s, n) for s, n in enumerate(store._batch_n)]


def test_pairs_equal_single_query_calls_gicp(street):
    st = street; store, ctx, pairs = st["store"], st["gctx"], st["pairs"]
    qs, cs, ys = zip(*pairs)
    shared = [c for c in set(cs) if len({q for q, c2 in zip(qs, cs) if c2 == c}) > 1]
    assert len(pairs) >= 12 and shared, pairs
    out = store.verify_loop_pairs(ctx, qs, cs, ys, st["drift"], RANGE, LEAF)
    assert any(o["valid"] for o in out)
    for (q, c, y), o in zip(pairs, out):
        w, = store.verify_loop_candidates(ctx, q, [c], [y], st["drift"], RANGE, LEAF)
        assert _grec(o) == _grec(w), (q, c)


def test_segments_are_the_distinct_queries_then_candidates(street):
    st = street; store, ctx, pairs = st["store"], st["gctx"], st["pairs"]
    qs, cs, ys = zip(*pairs)
    store.verify_loop_pairs(ctx, qs, cs, ys, st["drift"], RANGE, LEAF)
    uq, uc = list(dict.fromkeys(qs)), list(dict.fromkeys(cs))
    segs = _segments(store)
    assert len(segs) == len(uq) + len(uc)
    for s, kf in enumerate(uq + uc):
        q, c, y = next(p for p in pairs if (p[0] if s < len(uq) else p[1]) == kf)
        store.verify_loop_candidates(ctx, q, [c], [y], st["drift"], RANGE, LEAF)
        want = store.download_batch(0 if s < len(uq) else 1, store._batch_n[0 if s < len(uq) else 1])
        assert len(want) > 0 and np.array_equal(segs[s].view(np.uint32), want.view(np.uint32)), (s, kf)


def test_pairs_equal_single_query_calls_c2f(street):
    st = street; store, ctx, pairs = st["store"], st["ctx"], st["pairs"]
    qs, cs, _ = zip(*pairs)
    out = store.verify_loop_pairs_c2f(ctx, qs, cs)
    for (q, c, _), o in zip(pairs, out):
        w, = store.verify_loop_candidates_c2f(ctx, q, [c])
        assert _crec(o) == _crec(w), (q, c)


def test_street_revisits_in_one_call(street):
    st = street; store, ctx = st["store"], st["ctx"]
    qs = [10, 11, 12, 13]
    best = store.sc_query(qs, st["stamps"], 5.0, 1)
    cs = [int(b[0][0]) for b in best]; ys = [sc.yaw_of_shift(int(b[2][0]), 60) for b in best]
    assert cs == [q - 10 for q in qs]
    for name, out in (("gicp", store.verify_loop_pairs(st["gctx"], qs, cs, ys, st["drift"], RANGE, LEAF)), ("c2f", store.verify_loop_pairs_c2f(ctx, qs, cs))):
        for q, c, r in zip(qs, cs, out):
            assert r["status"] == 0 and r["valid"], (name, q, r)
            et, er = synth.pose_error(r["T"], np.linalg.inv(st["poses"][c]) @ st["poses"][q])
            assert et <= TOL_T and er <= TOL_R, (name, q, et, math.degrees(er))


def test_refused_arguments_change_nothing(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["gctx"]
    store.verify_loop_pairs(ctx, [10, 11], [0, 1], [0.5, -0.5], st["drift"], RANGE, LEAF)
    n_before = list(store._batch_n); segs = _segments(store)
    pairs_before = ctx.debug_get("batch_pairs")
    nan_pose = [P.copy() for P in st["drift"]]; nan_pose[3][1, 1] = float("nan")
    base = dict(query=[10, 11], cand=[0, 1], yaw=[0.0, 0.0], poses=st["drift"], leaf=LEAF)
    bad = [dict(query=[-1, 11]), dict(cand=[0, 99]), dict(cand=[10, 1]), dict(query=[10, 10], cand=[0, 0]), dict(query=[], cand=[], yaw=[]),
           dict(poses=st["drift"][:11]), dict(poses=nan_pose), dict(yaw=[float("nan"), 0.0]), dict(yaw=[0.0, float("inf")]), dict(leaf=0.0), dict(leaf=-0.3)]
    for b in bad:
        a = dict(base); a.update(b)
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_pairs(ctx, a["query"], a["cand"], a["yaw"], a["poses"], RANGE, a["leaf"])
        assert e.value.status == engine.QN_ERR_INVALID_ARG, b
        assert ctx.debug_get("batch_pairs") == pairs_before, b
        for s, n in enumerate(n_before):
            n_now = C.c_uint32()
            assert store._l.qn_kf_batch_count(store.h, C.c_uint32(s), C.byref(n_now)) == 0 and n_now.value == n, b
            assert np.array_equal(store.download_batch(s, n).view(np.uint32), segs[s].view(np.uint32)), b
    cctx = st["ctx"]
    other = engine.Context(4 * CAP)                                               # another grid capacity: the descriptions do not fit it
    for b in [dict(query=[-1], cand=[0]), dict(query=[10], cand=[10]), dict(query=[10, 10], cand=[0, 0]), dict(query=[], cand=[]), dict(query=[10], cand=[99])]:
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_pairs_c2f(cctx, b["query"], b["cand"])
        assert e.value.status == engine.QN_ERR_INVALID_ARG, b
    with pytest.raises(engine.EngineError) as e:
        store.verify_loop_pairs_c2f(other, [10], [0])
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    other.close()
    assert ctx.debug_get("batch_pairs") == pairs_before
    # the verify record of the GICP call above is still there
    assert np.array_equal(store.verify_cloud(0, engine.QN_VERIFY_SRC).view(np.uint32), segs[0].view(np.uint32))


def test_an_empty_window_sits_beside_valid_pairs():
    from qn_amd import engine
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100))
    empty = store.add(np.zeros((0, 3), np.float32)); store.add(synth.lidar_scan(prims, sen, poses[5], 7)[:, :3])
    P = scv._drifted(poses) + [np.eye(4), np.eye(4)]
    ctx = _ctx(engine, cap=GCAP)
    store.sc_describe(ids)
    best = store.sc_query([10, 11], np.arange(16) * 10.0, 5.0, 1)
    ys = [sc.yaw_of_shift(int(b[2][0]), 60) for b in best]
    out = store.verify_loop_pairs(ctx, [10, 11, 10], [0, 1, empty], ys + [0.0], P, 0, LEAF)
    assert out[2]["status"] == engine.QN_ERR_EMPTY_CLOUD and not out[2]["valid"]
    for q, r in zip((10, 11), out[:2]):
        assert r["status"] == 0 and r["valid"], r
        et, er = synth.pose_error(r["T"], np.linalg.inv(poses[q - 10]) @ poses[q])
        assert et <= TOL_T and er <= TOL_R, (q, et, er)
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(2, engine.QN_VERIFY_FINAL)
    assert e.value.status == engine.QN_ERR_NOT_READY
    ctx.close(); store.close()


def test_verify_cloud_gicp(street):
    from qn_amd import engine
    st = street; store, ctx, pairs = st["store"], st["gctx"], st["pairs"]
    qs, cs, ys = zip(*pairs)
    out = store.verify_loop_pairs(ctx, qs, cs, ys, st["drift"], RANGE, LEAF)
    segs = _segments(store)
    uq, uc = list(dict.fromkeys(qs)), list(dict.fromkeys(cs))
    for j in (0, 3, len(pairs) - 1):
        q, c, y = pairs[j]
        src, dst = store.verify_cloud(j, engine.QN_VERIFY_SRC), store.verify_cloud(j, engine.QN_VERIFY_DST)
        assert np.array_equal(src.view(np.uint32), segs[uq.index(q)].view(np.uint32))
        assert np.array_equal(dst.view(np.uint32), segs[len(uq) + uc.index(c)].view(np.uint32))
        final = store.verify_cloud(j, engine.QN_VERIFY_FINAL)
        sp, sn, dp, dn = C.c_void_p(), C.c_uint32(), C.c_void_p(), C.c_uint32()
        assert store._l.qn_kf_verify_cloud(store.h, C.c_uint32(j), C.c_int(0), C.byref(sp), C.byref(sn)) == 0
        assert store._l.qn_kf_verify_cloud(store.h, C.c_uint32(j), C.c_int(1), C.byref(dp), C.byref(dn)) == 0
        fresh = _ctx(engine, cap=GCAP); l = fresh._l
        assert l.qn_gicp_set_source_device(fresh.h, sp, sn, C.c_uint32(16)) == 0 and l.qn_gicp_set_target_device(fresh.h, dp, dn, C.c_uint32(16)) == 0
        assert l.qn_gicp_compute_covariances(fresh.h, C.c_int(0)) == 0 and l.qn_gicp_compute_covariances(fresh.h, C.c_int(1)) == 0
        g = np.ascontiguousarray(sc.seed_from_yaw(y), dtype=np.float32); res = engine.GicpResult()
        assert l.qn_gicp_align(fresh.h, g.ctypes.data_as(C.c_void_p), C.byref(res)) == 0
        assert np.array_equal(np.array(res.T, np.float32), np.array(out[j]["record"].T, np.float32)), j
        want = np.zeros((sn.value, 4), np.float32)
        assert l.qn_gicp_transformed_source(fresh.h, want.ctypes.data_as(C.c_void_p), C.c_uint32(16)) == 0
        assert np.array_equal(final.view(np.uint32), want[:, :3].view(np.uint32)), j
        fresh.close()
    for bad, code in (((0, engine.QN_VERIFY_COARSE), engine.QN_ERR_NOT_READY), ((len(pairs), engine.QN_VERIFY_SRC), engine.QN_ERR_INVALID_ARG),
                      ((0, 4), engine.QN_ERR_INVALID_ARG), ((0, -1), engine.QN_ERR_INVALID_ARG)):
        with pytest.raises(engine.EngineError) as e:
            store.verify_cloud(*bad)
        assert e.value.status == code, bad
    store.assemble_batch([[0]], [[np.eye(4)]], LEAF)                              # the batch slot is rebuilt: the GICP record goes
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(0, engine.QN_VERIFY_SRC)
    assert e.value.status == engine.QN_ERR_NOT_READY


def test_verify_cloud_c2f(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    qs, cs = [10, 12, 11], [0, 2, 1]
    out = store.verify_loop_pairs_c2f(ctx, qs, cs)
    for j, (q, c) in enumerate(zip(qs, cs)):
        assert out[j]["valid"], out[j]
        sp, sn = store.quatro_cloud(q); dp, dn = store.quatro_cloud(c)
        src = _records(sp, sn)[:, :3].copy()
        assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_SRC).view(np.uint32), src.view(np.uint32))
        assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_DST).view(np.uint32), _records(dp, dn)[:, :3].view(np.uint32))
        T = out[j]["T_quatro"]; x, y, z = (src[:, i].astype(np.float64) for i in range(3))
        coarse = np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32) for r in range(3)], 1)
        assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_COARSE).view(np.uint32), coarse.view(np.uint32)), j
        fresh = _ctx(engine)
        r = engine.coarse_to_fine_alignment_device(fresh, sp, sn, dp, dn, 16, quatro=engine.Quatro(fresh), max_corr_dist=MAX_CORR)
        assert np.array_equal(r["T"], out[j]["T"]), j
        want = np.zeros((sn, 4), np.float32)
        assert fresh._l.qn_gicp_transformed_source(fresh.h, want.ctypes.data_as(C.c_void_p), C.c_uint32(16)) == 0
        assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_FINAL).view(np.uint32), want[:, :3].view(np.uint32)), j
        fresh.close()
    store.quatro_describe(ctx, [12], LEAF)                                         # describing a keyframe of the call again: its record goes
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(0, engine.QN_VERIFY_COARSE)
    assert e.value.status == engine.QN_ERR_NOT_READY


def test_a_single_query_call_leaves_no_record_of_its_own(street):
    """verify_loop_candidates ends a live GICP record (its assembly rebuilds the batch slot that record names) and no other; verify_loop_candidates_c2f
    touches no record.  Either call's records are the pairs form's for the same pairs."""
    from qn_amd import engine
    st = street; store, ctx, gctx = st["store"], st["ctx"], st["gctx"]
    q = st["pairs"][0][0]
    cs, ys = zip(*[(c, y) for q2, c, y in st["pairs"] if q2 == q])
    qs = [q] * len(cs)
    assert len(cs) >= 2

    def src_bytes():
        a = store.verify_cloud(0, engine.QN_VERIFY_SRC)
        assert len(a) > 0
        return a.tobytes()
    gwant = [_grec(o) for o in store.verify_loop_pairs(gctx, qs, cs, ys, st["drift"], RANGE, LEAF)]
    assert [_grec(o) for o in store.verify_loop_candidates(gctx, q, cs, ys, st["drift"], RANGE, LEAF)] == gwant
    with pytest.raises(engine.EngineError) as e:                                   # a GICP record: gone with the batch slot
        store.verify_cloud(0, engine.QN_VERIFY_SRC)
    assert e.value.status == engine.QN_ERR_NOT_READY
    cwant = [_crec(o) for o in store.verify_loop_pairs_c2f(ctx, qs, cs)]
    before = src_bytes()
    assert [_grec(o) for o in store.verify_loop_candidates(gctx, q, cs, ys, st["drift"], RANGE, LEAF)] == gwant
    assert src_bytes() == before                                                   # a coarse-to-fine record names described clouds: it stays
    store.verify_loop_pairs(gctx, qs, cs, ys, st["drift"], RANGE, LEAF)
    before = src_bytes()
    assert [_crec(o) for o in store.verify_loop_candidates_c2f(ctx, q, cs)] == cwant
    assert src_bytes() == before                                                   # the coarse-to-fine call assembles nothing: the GICP record stays


def test_cpp_helpers_return_the_python_records(tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_loop_pairs.cpp", tmp_path)
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    clouds = [synth.lidar_scan(prims, sen, P, 100 + k)[:, :3] for k, P in enumerate(poses)]
    stamps = np.arange(len(clouds)) * 10.0
    drift = scv._drifted(poses)
    with open(tmp_path / "kf.bin", "wb") as f:
        for c in clouds:
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    stamps.tofile(tmp_path / "st.bin")
    np.ascontiguousarray(np.array(drift, np.float64).reshape(-1, 16)).tofile(tmp_path / "poses.bin")
    store = engine.KeyframeStore()
    ids = [store.add(c) for c in clouds]
    store.sc_describe(ids)
    ctx = engine.Context(200000)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    qs = [10, 11, 12, 13]
    keep = [(q, int(i), sc.yaw_of_shift(int(s), 60)) for q, (cid, D, sh) in zip(qs, store.sc_query(qs, stamps, 5.0, 3)) for i, d, s in zip(cid, D, sh) if d < 0.5]
    assert len(keep) >= 4
    for c2f in (0, 1):
        got = [l.split() for l in subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "st.bin"), str(tmp_path / "poses.bin"), "5.0", "3", "0.5",
                                                           str(RANGE), str(LEAF), str(MAX_CORR), str(c2f)] + [str(q) for q in qs], text=True).split("\n") if l.strip()]
        assert [(int(g[0]), int(g[1])) for g in got] == [(q, c) for q, c, _ in keep]
        if c2f:
            store.quatro_describe(ctx, ids, LEAF)
            want = store.verify_loop_pairs_c2f(ctx, [k[0] for k in keep], [k[1] for k in keep])
        else:
            want = store.verify_loop_pairs(ctx, [k[0] for k in keep], [k[1] for k in keep], [k[2] for k in keep], drift, RANGE, LEAF)
        assert any(w["valid"] for w in want)
        for g, w in zip(got, want):
            assert (int(g[2]) == 1) == w["valid"] and int(g[3]) == w["status"] and float(g[4]) == w["score"], (g, w)
            assert np.array_equal(np.array([float(x) for x in g[5:21]]), w["T"].reshape(-1)), (g, w)
    ctx.close(); store.close()


def test_catch_up_replay_closes_the_skipped_revisit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    kw = dict(verbose=False, n_kf=66, seed=7, sensor="spinning", detector="scancontext", verify="relative", yaw_bias=0.02, loop_every=4)
    late = replay.run(catch_up=False, **kw)
    up = replay.run(catch_up=True, **kw)
    assert up["loops"] >= late["loops"] + 1, (late["loop_list"], up["loop_list"])
    assert up["ate_corrected"] <= late["ate_corrected"], (up["ate_corrected"], late["ate_corrected"])
    for (k, c, _), T in zip(up["loop_list"], up["loop_T"]):
        et, er = synth.pose_error(T, np.linalg.inv(up["gt"][c]) @ up["gt"][k])
        assert et <= TOL_T and er <= TOL_R, (k, c, et, er)
    orc = replay.run(catch_up=True, backend="oracle", **kw)
    assert [(k, c) for k, c, _ in up["loop_list"]] == [(k, c) for k, c, _ in orc["loop_list"]] and up["attempts"] == orc["attempts"]
