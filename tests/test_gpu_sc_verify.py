"""Drift-free verification of Scan Context loop candidates (qn_kf_verify_loop_candidates / KeyframeStore.verify_loop_candidates): on the street
scene with the revisits' corrected poses 200 m off, the query scan in its sensor frame against the candidate's window in the candidate's sensor
frame, seeded with the Scan Context heading, recovers inv(P_place) P_revisit where the reference-style world-frame pair cannot; the assembled
clouds equal assemble_batch of the twins' relative poses and the records equal gicp_align_batch with the twins' seeds, bit for bit; argument
checks leave the store and context unchanged; an empty candidate submap sits beside valid ones; the C++ helper; the replay's --verify relative.

Tolerance: 0.05 m / 0.2 degrees against the ground truth.  Calibrated on the CPU oracle (the same clouds and guesses from the twins): the four
seeded street revisits land within 0.0036 m / 0.016 degrees, the replay's loop within 0.0095 m / 0.03 degrees; unseeded or world-frame pairs miss
by metres and tens of degrees."""
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
TOL_T, TOL_R = 0.05, math.radians(0.2)
LEAF, RANGE, MAX_CORR = 0.3, 5, 18.0


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


def _drifted(poses):
    """corrected poses after drift: each revisit is placed 200 m further off"""
    d = [P.copy() for P in poses]
    for j, q in enumerate(range(10, 14)):
        d[q][0, 3] += 200.0 * (j + 1)
    return d


def _ctx(engine, cap=200000):
    ctx = engine.Context(cap)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    return ctx


def _heading(P):
    return math.atan2(P[1, 0], P[0, 0])


@pytest.fixture(scope="module")
def street():
    from qn_amd import engine
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100))
    store.sc_describe(ids)
    ctx = _ctx(engine)
    yield dict(store=store, ctx=ctx, poses=poses, drift=_drifted(poses), stamps=np.arange(len(ids)) * 10.0, prims=prims, sen=sen)
    ctx.close(); store.close()


def _best(st, q, k=1):
    cid, D, sh = st["store"].sc_query([q], st["stamps"], 5.0, k)[0]
    return [int(c) for c in cid], [sc.yaw_of_shift(int(s), 60) for s in sh], D


def test_revisits_are_verified_drift_free(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    worst = (None, -1.0)
    for q in range(10, 14):
        place = q - 10
        (c,), (yaw,), _ = _best(st, q)
        assert c == place
        truth = np.linalg.inv(st["poses"][place]) @ st["poses"][q]
        r, = store.verify_loop_candidates(ctx, q, [c], [yaw], st["drift"], RANGE, LEAF)
        assert r["status"] == 0 and r["valid"], (q, r)
        et, er = synth.pose_error(r["T"], truth)
        assert et <= TOL_T and er <= TOL_R, (q, et, math.degrees(er))
        # the reference-style pair (world frame of the drifted poses, identity seed) misses the same truth by the drift
        pairs, sts = store.loop_submap_pairs(st["drift"], q, [c], RANGE, LEAF, enable_quatro=False)
        res, val, _ = engine.gicp_align_batch(ctx, pairs)
        Tw = np.array(res[0].T, dtype=np.float32).reshape(4, 4).astype(np.float64)
        et, er = synth.pose_error(np.linalg.inv(st["drift"][place]) @ Tw @ st["drift"][q], truth)
        assert et > TOL_T or er > TOL_R, (q, et, er)
        dh = abs((_heading(st["poses"][place]) - _heading(st["poses"][q]) + math.pi) % (2 * math.pi) - math.pi)
        if dh > worst[1]:
            worst = (q, dh)
    # the largest heading difference (revisit 12: 167 degrees): from yaw 0 the relative pair misses, seeded it hits (above)
    q, dh = worst
    assert dh > math.radians(120), math.degrees(dh)
    r0, = store.verify_loop_candidates(ctx, q, [q - 10], None, st["drift"], RANGE, LEAF)
    et, er = synth.pose_error(r0["T"], np.linalg.inv(st["poses"][q - 10]) @ st["poses"][q])
    assert et > TOL_T or er > TOL_R, (et, er)


def _rec(r, v, s):
    return (s, v, r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.H).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def test_clouds_and_records_equal_the_twins_bit_for_bit(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    q = 12
    cand, yaw, _ = _best(st, q, 3)
    assert len(cand) == 3
    out = store.verify_loop_candidates(ctx, q, cand, yaw, st["drift"], RANGE, LEAF)
    segs = [store.download_batch(s, store._batch_n[s]) for s in range(len(cand) + 1)]
    assert all(len(s) > 0 for s in segs)
    # the twins: the query alone with the identity, each window with inv(P_c) P_i
    lists = [[q]] + [engine.loop_submap_ids(q, c, RANGE, False, False, len(st["drift"]))[1] for c in cand]
    rel = [[np.eye(4)]] + [[sc.relative_pose(st["drift"][c], st["drift"][i]) for i in l] for c, l in zip(cand, lists[1:])]
    got = store.assemble_batch(lists, rel, LEAF)
    for s, (ptr, n, status) in enumerate(got):
        assert status == 0 and n == len(segs[s])
        assert np.array_equal(store.download_batch(s, n).view(np.uint32), segs[s].view(np.uint32)), "segment %d differs from the twin's assembly" % s
    pairs = [(got[0][0], got[0][1], p, n, 16, 1) for p, n, _ in got[1:]]
    res, val, sts = engine.gicp_align_batch(ctx, pairs, guesses=[sc.seed_from_yaw(y) for y in yaw])
    for j, o in enumerate(out):
        assert _rec(o["record"], int(o["valid"]), o["status"]) == _rec(res[j], val[j], sts[j]), "candidate %d differs" % j
        assert np.array_equal(o["T"], np.array(res[j].T, dtype=np.float32).reshape(4, 4).astype(np.float64))


def test_refused_arguments_leave_store_and_context_unchanged(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    q = 10
    store.verify_loop_candidates(ctx, q, [0, 1], [0.5, -0.5], st["drift"], RANGE, LEAF)
    n_before = list(store._batch_n)
    segs = [store.download_batch(s, n) for s, n in enumerate(n_before)]
    pairs_before = ctx.debug_get("batch_pairs")
    nan_pose = [P.copy() for P in st["drift"]]; nan_pose[3][1, 1] = float("nan")
    bad = [dict(candidates=[-1]), dict(candidates=[99]), dict(candidates=[0, 0]), dict(candidates=[q]), dict(candidates=[]),
           dict(poses=st["drift"][:q]), dict(candidates=[13], query=4, poses=st["drift"][:13]), dict(poses=nan_pose),
           dict(yaw=[float("nan")]), dict(yaw=[float("inf")]), dict(leaf=0.0), dict(leaf=-0.3), dict(query=-1), dict(query=99)]
    for b in bad:
        a = dict(query=q, candidates=[0], yaw=[0.0], poses=st["drift"], leaf=LEAF); a.update(b)
        if a["yaw"] is not None and len(a["yaw"]) != len(a["candidates"]):
            a["yaw"] = [0.0] * len(a["candidates"])
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_candidates(ctx, a["query"], a["candidates"], a["yaw"], a["poses"], RANGE, a["leaf"])
        assert e.value.status == engine.QN_ERR_INVALID_ARG, b
        assert ctx.debug_get("batch_pairs") == pairs_before, b
        for s, n in enumerate(n_before):
            n_now = C.c_uint32()
            assert store._l.qn_kf_batch_count(store.h, C.c_uint32(s), C.byref(n_now)) == 0 and n_now.value == n, b
            assert np.array_equal(store.download_batch(s, n).view(np.uint32), segs[s].view(np.uint32)), b


def test_an_empty_candidate_submap_sits_beside_valid_ones():
    from qn_amd import engine
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100))
    empty = store.add(np.zeros((0, 3), np.float32)); last = store.add(synth.lidar_scan(prims, sen, poses[5], 7)[:, :3])
    assert (empty, last) == (14, 15)
    P = _drifted(poses) + [np.eye(4), np.eye(4)]
    ctx = _ctx(engine)
    store.sc_describe(ids)
    cid, _, sh = store.sc_query([10], np.arange(16) * 10.0, 5.0, 1)[0]
    assert int(cid[0]) == 0
    yaw = sc.yaw_of_shift(int(sh[0]), 60)
    out = store.verify_loop_candidates(ctx, 10, [empty, 0], [0.0, yaw], P, 0, LEAF)
    assert out[0]["status"] == engine.QN_ERR_EMPTY_CLOUD and not out[0]["valid"]
    assert out[1]["status"] == 0 and out[1]["valid"]
    et, er = synth.pose_error(out[1]["T"], np.linalg.inv(poses[0]) @ poses[10])
    assert et <= TOL_T and er <= TOL_R, (et, er)
    assert store._batch_n[1] == 0 and store._batch_n[2] > 0
    ctx.close(); store.close()


def test_cpp_helper_returns_the_python_records(tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_sc_verify.cpp", tmp_path)
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    clouds = [synth.lidar_scan(prims, sen, P, 100 + k)[:, :3] for k, P in enumerate(poses)]
    stamps = np.arange(len(clouds)) * 10.0
    drift = _drifted(poses)
    with open(tmp_path / "kf.bin", "wb") as f:
        for c in clouds:
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    stamps.tofile(tmp_path / "st.bin")
    np.ascontiguousarray(np.array(drift, np.float64).reshape(-1, 16)).tofile(tmp_path / "poses.bin")
    store = engine.KeyframeStore()
    ids = [store.add(c) for c in clouds]
    store.sc_describe(ids)
    ctx = _ctx(engine)
    for q in (10, 12):
        out = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "st.bin"), str(tmp_path / "poses.bin"), str(q), "5.0", "4", "0.5",
                                       str(RANGE), str(LEAF), str(MAX_CORR)], text=True).split("\n")
        got = [l.split() for l in out if l.strip()]
        cid, D, sh = store.sc_query([q], stamps, 5.0, 4)[0]
        keep = [(int(i), sc.yaw_of_shift(int(s), 60)) for i, d, s in zip(cid, D, sh) if d < 0.5]
        assert len(keep) >= 1 and [int(g[0]) for g in got] == [c for c, _ in keep]
        want = store.verify_loop_candidates(ctx, q, [c for c, _ in keep], [y for _, y in keep], drift, RANGE, LEAF)
        assert any(w["valid"] for w in want)
        for g, w in zip(got, want):
            assert (int(g[1]) == 1) == w["valid"] and int(g[2]) == w["status"] and float(g[3]) == w["score"], (g, w)
            assert np.array_equal(np.array([float(x) for x in g[4:20]], np.float32), w["T"].astype(np.float32).reshape(-1)), (g, w)
    ctx.close(); store.close()


def test_replay_verifies_scan_context_loops_drift_free():
    """yaw_bias 0.02 (chosen on the oracle backend): the reference-style verification accepts no Scan Context candidate, the relative one closes the loop"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    ref = replay.run(verbose=False, sensor="spinning", detector="scancontext", yaw_bias=0.02)
    assert ref["loops"] == 0, ref["loop_list"]
    a = replay.run(verbose=False, sensor="spinning", detector="scancontext", verify="relative", yaw_bias=0.02)
    assert a["loops"] >= 1 and a["ate_corrected"] < a["ate_odometry"], (a["loop_list"], a["ate_corrected"], a["ate_odometry"])
    for (k, c, _), T in zip(a["loop_list"], a["loop_T"]):
        et, er = synth.pose_error(T, np.linalg.inv(a["gt"][c]) @ a["gt"][k])
        assert et <= TOL_T and er <= TOL_R, (k, c, et, er)
    b = replay.run(verbose=False, sensor="spinning", detector="scancontext", verify="relative", yaw_bias=0.02, backend="oracle")
    assert [(k, c) for k, c, _ in a["loop_list"]] == [(k, c) for k, c, _ in b["loop_list"]] and a["attempts"] == b["attempts"]
    for (_, _, sa), (_, _, sb) in zip(a["loop_list"], b["loop_list"]):
        assert abs(sa - sb) <= 1e-5 * max(sb, 1e-9)
    d = max(np.linalg.norm(p[:3, 3] - q[:3, 3]) for p, q in zip(a["poses"], b["poses"]))
    assert d < 1e-3, d
    with pytest.raises(ValueError):
        replay.run(verbose=False, detector="radius", verify="relative")
