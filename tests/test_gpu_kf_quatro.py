"""Resident Quatro descriptors per keyframe (qn_kf_quatro_describe) and the drift-free coarse-to-fine check that borrows them
(qn_kf_verify_loop_candidates_c2f): described clouds equal qn_kf_assemble with the identity in all 16 bytes, rows equal qn_fpfh bit for bit and
the oracle's FPFH within the Quatro tests' tolerance, one call for S keyframes equals S calls, records equal qn_coarse_to_fine_align_batch on the
described device clouds bit for bit (sharing on and off, and a rerun), valid pairs agree with oracle.coarse_to_fine_alignment, street revisits with
large heading differences are recovered, refused arguments change nothing, an empty keyframe sits beside valid ones, the C++ helper, the replay.

Revisit tolerance: 0.05 m / 0.2 degrees against inv(P_place) P_revisit, as tests/test_gpu_sc_verify.py.  Calibrated on the CPU oracle
(oracle.coarse_to_fine_alignment of oracle.voxel_grid of the sensor-frame scans, leaf 0.3): the four street revisits, 89-167 degrees apart,
land within 0.0125 m / 0.026 degrees."""
import ctypes as C
import math
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import synth
from shim_build import build_shim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
TOL_T, TOL_R = 0.05, math.radians(0.2)
LEAF, MAX_CORR, CAP = 0.3, 18.0, 60000
EYE = np.eye(4)


def _records(ptr, n):
    """the n float4 records at a device pointer, all 16 bytes"""
    from qn_amd import engine
    out = np.zeros((n, 4), np.float32)
    if n:
        l = engine.lib(); l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; l.hipMemcpy.restype = C.c_int
        assert l.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), 16 * n, 2) == 0
    return out


def _ctx(engine, batch_lanes=None):
    ctx = engine.Context(CAP)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    if batch_lanes:
        ctx.debug_set("batch_lanes", batch_lanes)
    return ctx


def _street():
    import test_gpu_sc_verify
    return test_gpu_sc_verify._street()


@pytest.fixture(scope="module")
def street():
    from qn_amd import engine
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100)]
    uni = [store.add(synth.make_pair(900 + i, 5000, extent=40.0, mode="quatro")[0]) for i in range(2)]
    ctx = _ctx(engine)
    st = store.quatro_describe(ctx, ids + uni, LEAF)
    assert st == [0] * len(st)
    yield dict(store=store, ctx=ctx, poses=poses, ids=ids, uni=uni, prims=prims, sen=sen)
    ctx.close(); store.close()


def test_described_clouds_equal_assemble_with_the_identity(street):
    store = street["store"]
    for k in street["ids"][:6] + street["uni"]:
        p, n = store.quatro_cloud(k)
        ap, an = store.assemble([k], [EYE], LEAF, 0)
        assert n == an and n > 0
        assert np.array_equal(_records(p, n).view(np.uint32), _records(ap, an).view(np.uint32)), k


def test_described_rows_equal_qn_fpfh_and_the_oracle(street):
    from qn_amd import engine
    from oracle import oracle
    store = street["store"]
    ctx = engine.Context(CAP); engine.Quatro(ctx)
    for k in street["ids"][:3] + street["uni"]:
        p, n = store.quatro_cloud(k)
        cloud = _records(p, n)[:, :3].copy()
        rows = store.quatro_features(k)
        want = engine.fpfh(ctx, cloud)
        assert rows.shape == (n, 33) and np.array_equal(rows.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), k
        _, _, ofp = oracle.quatro_fpfh(cloud, 0.9, 1.5)
        assert np.array_equal(np.isnan(rows), np.isnan(ofp))
        good = ~np.isnan(ofp[:, 0])
        assert (np.abs(rows[good] - ofp[good]).max(1) > 1e-3).mean() < 5e-3
    ctx.close()


def test_one_call_equals_one_by_one(street):
    from qn_amd import engine
    store = street["store"]
    ks = street["ids"][:5] + street["uni"][:1]
    want = {k: (_records(*store.quatro_cloud(k)), store.quatro_features(k)) for k in ks}
    ctx = _ctx(engine)
    for k in ks:                                          # describing again replaces the entry
        assert store.quatro_describe(ctx, [k], LEAF) == [0]
        r, f = _records(*store.quatro_cloud(k)), store.quatro_features(k)
        assert np.array_equal(r.view(np.uint32), want[k][0].view(np.uint32)) and np.array_equal(f.view(np.uint32), want[k][1].view(np.uint32)), k
    assert store.quatro_describe(ctx, ks, LEAF) == [0] * len(ks)
    for k in ks:
        assert np.array_equal(_records(*store.quatro_cloud(k)).view(np.uint32), want[k][0].view(np.uint32))
        assert np.array_equal(store.quatro_features(k).view(np.uint32), want[k][1].view(np.uint32))
    ctx.close()


def _rec(o):
    return (o["status"], o["valid"], o["iterations"], o["converged"], o["score"], o["T"].tobytes(), o["T_quatro"].tobytes(), o["T_gicp"].tobytes())


@pytest.mark.parametrize("share", [1, 0])
def test_records_equal_the_batch_on_the_described_clouds(street, share):
    from qn_amd import engine
    store, ids = street["store"], street["ids"]
    ctx = _ctx(engine, batch_lanes=4); ctx.debug_set("batch_share_source", share)
    q, cand = ids[12], [ids[2], ids[0], ids[5], ids[3], ids[8], street["uni"][0]]      # more candidates than lanes: two runs
    out = store.verify_loop_candidates_c2f(ctx, q, cand)
    qp, qn = store.quatro_cloud(q)
    pairs = [(qp, qn) + store.quatro_cloud(c) + (16, 1) for c in cand]
    want = engine.coarse_to_fine_align_batch([ctx], pairs)
    assert [_rec(o) for o in out] == [_rec(w) for w in want]
    again = store.verify_loop_candidates_c2f(ctx, q, cand)
    assert [_rec(o) for o in again] == [_rec(o) for o in out]
    assert out[0]["valid"] and out[0]["status"] == 0
    ctx.close()


def test_valid_pairs_agree_with_the_oracle(street):
    from oracle import oracle
    store, ctx, ids = street["store"], street["ctx"], street["ids"]
    for q, cand in ((10, [0, 4]), (13, [3, 1])):
        out = store.verify_loop_candidates_c2f(ctx, ids[q], [ids[c] for c in cand])
        src = _records(*store.quatro_cloud(ids[q]))[:, :3].copy()
        for c, o in zip(cand, out):
            dst = _records(*store.quatro_cloud(ids[c]))[:, :3].copy()
            w = oracle.coarse_to_fine_alignment(src, dst, max_corr_dist=MAX_CORR)
            assert o["valid"] == w["valid"], (q, c)
            if w["valid"]:
                dt, dr = synth.pose_error(o["T"], w["T"])
                assert dt <= 1e-4 and dr <= 1e-4, (q, c, dt, dr)


def test_street_revisits_are_recovered(street):
    store, ctx, ids, poses = street["store"], street["ctx"], street["ids"], street["poses"]
    worst = 0.0
    for q in range(10, 14):
        place = q - 10
        r, = store.verify_loop_candidates_c2f(ctx, ids[q], [ids[place]])
        assert r["status"] == 0 and r["valid"], (q, r)
        et, er = synth.pose_error(r["T"], np.linalg.inv(poses[place]) @ poses[q])
        assert et <= TOL_T and er <= TOL_R, (q, et, math.degrees(er))
        hq, hp = math.atan2(poses[q][1, 0], poses[q][0, 0]), math.atan2(poses[place][1, 0], poses[place][0, 0])
        worst = max(worst, abs((hp - hq + math.pi) % (2 * math.pi) - math.pi))
    assert worst > math.radians(120), math.degrees(worst)


def test_refused_arguments_leave_store_and_context_unchanged(street):
    from qn_amd import engine
    store, ids = street["store"], street["ids"]
    ctx = _ctx(engine)
    fresh = store.add(synth.lidar_scan(street["prims"], street["sen"], street["poses"][7], 3)[:, :3])      # never described
    before = {k: (_records(*store.quatro_cloud(k)), store.quatro_features(k)) for k in ids[:3]}
    pairs_before = ctx.debug_get("batch_pairs")
    bad = [(ids[0], [fresh]), (fresh, [ids[0]]), (ids[0], [ids[1], ids[1]]), (ids[0], [ids[0]]), (ids[0], []), (ids[0], [-1]), (ids[0], [10 ** 6]), (-1, [ids[1]])]
    for q, cand in bad:
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_candidates_c2f(ctx, q, cand)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, (q, cand)
    other = _ctx(engine); engine.Quatro(other, fpfh_normal_radius=1.0, fpfh_radius=1.6)      # the entries were described with 0.9 / 1.5
    with pytest.raises(engine.EngineError) as e:
        store.verify_loop_candidates_c2f(other, ids[0], [ids[1]])
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    for args in (([-1], LEAF), ([10 ** 6], LEAF), ([ids[0]], 0.0), ([ids[0]], -0.3), ([], LEAF)):
        with pytest.raises(engine.EngineError) as e:
            store.quatro_describe(ctx, *args)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, args
    with pytest.raises(engine.EngineError) as e:
        store.quatro_cloud(fresh)
    assert e.value.status == engine.QN_ERR_NOT_READY
    assert ctx.debug_get("batch_pairs") == pairs_before and other.debug_get("batch_pairs") == 0
    for k, (r, f) in before.items():
        assert np.array_equal(_records(*store.quatro_cloud(k)).view(np.uint32), r.view(np.uint32))
        assert np.array_equal(store.quatro_features(k).view(np.uint32), f.view(np.uint32))
    ctx.close(); other.close()


def test_an_empty_keyframe_sits_beside_valid_ones(street):
    from qn_amd import engine
    store, ids, poses = street["store"], street["ids"], street["poses"]
    ctx = _ctx(engine)
    empty = store.add(np.zeros((0, 3), np.float32))
    nonfinite = store.add(np.full((10, 3), np.nan, np.float32))
    st = store.quatro_describe(ctx, [empty, ids[0], nonfinite], LEAF)
    assert st == [engine.QN_ERR_EMPTY_CLOUD, 0, engine.QN_ERR_EMPTY_CLOUD]
    assert store.quatro_cloud(empty) == (None, 0) and store.quatro_features(empty).shape == (0, 33)
    out = store.verify_loop_candidates_c2f(ctx, ids[10], [empty, ids[0], nonfinite])
    assert [o["status"] for o in out] == [engine.QN_ERR_EMPTY_CLOUD, 0, engine.QN_ERR_EMPTY_CLOUD]
    assert [o["valid"] for o in out] == [False, True, False]
    et, er = synth.pose_error(out[1]["T"], np.linalg.inv(poses[0]) @ poses[10])
    assert et <= TOL_T and er <= TOL_R, (et, er)
    e2 = store.verify_loop_candidates_c2f(ctx, empty, [ids[0]])
    assert e2[0]["status"] == engine.QN_ERR_EMPTY_CLOUD and not e2[0]["valid"]
    ctx.close()


def test_cpp_helper_returns_the_python_records(tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_kf_quatro.cpp", tmp_path)
    prims, poses = _street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    clouds = [synth.lidar_scan(prims, sen, P, 100 + k)[:, :3] for k, P in enumerate(poses)]
    stamps = np.arange(len(clouds)) * 10.0
    with open(tmp_path / "kf.bin", "wb") as f:
        for c in clouds:
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    stamps.tofile(tmp_path / "st.bin")
    store = engine.KeyframeStore()
    ids = [store.add(c) for c in clouds]
    store.sc_describe(ids)
    ctx = _ctx(engine)
    for q in (10, 12):
        out = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "st.bin"), str(q), "5.0", "4", "0.5", str(LEAF), str(MAX_CORR), str(CAP)],
                                      text=True).split("\n")
        got = [l.split() for l in out if l.strip()]
        cid, D, _ = store.sc_query([q], stamps, 5.0, 4)[0]
        keep = [int(i) for i, d in zip(cid, D) if d < 0.5]
        assert len(keep) >= 1 and [int(g[0]) for g in got] == keep
        store.quatro_describe(ctx, keep + [q], LEAF)
        want = store.verify_loop_candidates_c2f(ctx, q, keep)
        assert any(w["valid"] for w in want)
        for g, w in zip(got, want):
            assert (int(g[1]) == 1) == w["valid"] and int(g[2]) == w["status"] and float(g[3]) == w["score"], (g, w)
            assert np.array_equal(np.array([float(x) for x in g[4:20]]), w["T"].reshape(-1)), (g, w)
    ctx.close(); store.close()


def test_replay_verifies_scan_context_loops_coarse_to_fine():
    """--verify relative --quatro: yaw_bias 0.02, chosen on the oracle backend, where the reference-style check closes no loop (tests/test_gpu_sc_verify.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    a = replay.run(verbose=False, sensor="spinning", detector="scancontext", verify="relative", use_quatro=True, yaw_bias=0.02)
    assert a["loops"] >= 1 and a["ate_corrected"] < a["ate_odometry"], (a["loop_list"], a["ate_corrected"], a["ate_odometry"])
    for (k, c, _), T in zip(a["loop_list"], a["loop_T"]):
        et, er = synth.pose_error(T, np.linalg.inv(a["gt"][c]) @ a["gt"][k])
        assert et <= TOL_T and er <= TOL_R, (k, c, et, er)
    b = replay.run(verbose=False, sensor="spinning", detector="scancontext", verify="relative", use_quatro=True, yaw_bias=0.02, backend="oracle")
    assert [(k, c) for k, c, _ in a["loop_list"]] == [(k, c) for k, c, _ in b["loop_list"]] and a["attempts"] == b["attempts"]
    for (_, _, sa), (_, _, sb) in zip(a["loop_list"], b["loop_list"]):
        assert abs(sa - sb) <= 1e-5 * max(sb, 1e-9)
    d = max(np.linalg.norm(p[:3, 3] - q[:3, 3]) for p, q in zip(a["poses"], b["poses"]))
    assert d < 1e-3, d
