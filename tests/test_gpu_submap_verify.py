"""Resident local submaps (qn_kf_submap_describe / KeyframeStore.submap_describe) and the drift-free submap-to-submap verification that borrows them
(qn_kf_verify_loop_pairs_submap, qn_kf_verify_loop_pairs_submap_c2f), on the ray-cast street scene of tests/test_gpu_sc_verify.py (four places, six
distractors, four revisits) with every pose perturbed by ~1 cm / 0.1 degrees.

What is pinned bit for bit: an entry's cloud to qn_kf_assemble_batch of its window with scancontext.relative_pose (and, where the window rules agree, to the
candidate segment of qn_kf_verify_loop_pairs), its rows to qn_fpfh of that cloud, every record to qn_gicp_align_batch_guess / qn_coarse_to_fine_align_batch on
the entry clouds.  Against the CPU oracle: 1e-4 m / 1e-4 rad, the valid flag and the iteration count, on the oracle's own assembly of the same windows.

The oracle pairs were chosen on the CPU oracle alone (SUBMAP_RANGE 2, leaf 0.3, max_corr_dist 18, score_thr 1.5; window 12 = keyframes 10..13, window 13 =
11..13, window 2 = 0..4, window 3 = 1..5, window 5 = 3..7, window 7 = 5..9):
  GICP, seeded with the true heading difference rounded to a Scan Context sector:  (12, 2) converged, score 0.0468;  (13, 3) converged, score 0.0407;
        (10, 5) score 30.1;  (12, 7) score 6.60  - accepted far below, rejected far above the threshold 1.5;
  coarse to fine:  (13, 3) valid, score 0.0407;  (10, 5) score 15.7;  (12, 7) score 4.67;  (12, 2) GICP not converged after 32 iterations, score 10.9.
(11, 3) scores 1.70 on both paths - too near the threshold to ask the flag of it, so it is not among the oracle pairs.)

Invariance (the drift-free property as a test): describing with G P_i for a rigid G, or with poses changed outside every described window, gives identical
verify records.  G is a 90 degree yaw and an integer translation, exact in f32; the relative poses still differ in the last bits of their f64 entries (the
sums run over permuted rows), far below half an f32 ulp of any point for all but a ~1e-8 share of coordinates, so the clouds come out identical."""
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
import test_gpu_sc_verify as scv                                                   # noqa: E402  (the street scene)
from shim_build import build_shim

LEAF, RANGE, MAX_CORR, CAP, THR = 0.3, 2, 18.0, 60000, 1.5
N = 14                                                                             # keyframes of the street scene
GICP_PAIRS = [(12, 2, True), (13, 3, True), (10, 5, False), (12, 7, False)]        # (query, candidate, the oracle's valid flag)
C2F_PAIRS = [(13, 3, True), (10, 5, False), (12, 7, False), (12, 2, False)]


def _records(ptr, n):
    from qn_amd import engine
    out = np.zeros((n, 4), np.float32)
    if n:
        l = engine.lib(); l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; l.hipMemcpy.restype = C.c_int
        assert l.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), 16 * n, 2) == 0
    return out


def _ctx(engine, cap=CAP, lanes=None):
    ctx = engine.Context(cap)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    if lanes:
        ctx.debug_set("batch_lanes", lanes)
    return ctx


def _perturbed(poses):
    rng = np.random.default_rng(77)
    out = []
    for P in poses:
        a = rng.normal(0, math.radians(0.1)); T = np.eye(4)
        T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]; T[:3, 3] = rng.normal(0, 0.01, 3)
        out.append(P @ T)
    return out


def _yaw(poses, q, c):
    """the true heading of q minus that of c, rounded to a Scan Context sector (what sc_query's shift gives when it finds the place)"""
    h = lambda P: math.atan2(P[1, 0], P[0, 0])
    return sc.yaw_of_shift(int(round((h(poses[q]) - h(poses[c])) / (2 * math.pi / 60))) % 60, 60)


def _window(engine, c, poses, r=RANGE):
    ids = engine.local_submap_ids(c, r, len(poses))
    return ids, [sc.relative_pose(poses[c], poses[i]) for i in ids]


@pytest.fixture(scope="module")
def street():
    from qn_amd import engine
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100)]
    assert ids == list(range(N))
    empty = store.add(np.zeros((0, 3), np.float32))                                # keyframe 14: no point (its r = 0 window is an empty entry)
    pp = _perturbed(poses)
    ctx = _ctx(engine, lanes=4)
    assert store.submap_describe(ctx, ids, pp, RANGE, LEAF) == [0] * N              # (14 poses: the windows stop at keyframe 13)
    assert store.submap_describe(ctx, [empty], pp + [np.eye(4)], 0, LEAF) == [engine.QN_ERR_EMPTY_CLOUD]
    yield dict(store=store, ctx=ctx, poses=poses, pp=pp, ids=ids, empty=empty, prims=prims, sen=sen)
    ctx.close(); store.close()


def _entry(store, k):
    p, n = store.submap_cloud(k)
    return p, n, _records(p, n)


def _grec(r, v, s):
    return (int(s), bool(v), r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def _gout(o):
    return _grec(o["record"], o["valid"], o["status"])


def _crec(o):
    return (o["status"], o["valid"], o["iterations"], o["converged"], o["score"], o["T"].tobytes(), o["T_quatro"].tobytes(), o["T_gicp"].tobytes())


# ------------------------------------------------------------------ 1. the entries
def test_entry_clouds_equal_assemble_batch_of_their_windows(street):
    from qn_amd import engine
    st = street; store, pp = st["store"], st["pp"]
    lists, rels = zip(*[_window(engine, c, pp) for c in range(N)])
    assert lists[0] == [0, 1, 2] and lists[1] == [0, 1, 2, 3] and lists[12] == [10, 11, 12, 13] and lists[13] == [11, 12, 13]     # clipped at both ends
    got = store.assemble_batch(lists, rels, LEAF)
    for c, (ap, an, ast) in enumerate(got):
        p, n, rec = _entry(store, c)
        assert ast == 0 and n == an and n > 0, c
        assert np.array_equal(rec.view(np.uint32), _records(ap, an).view(np.uint32)), c
    assert store.submap_cloud(st["empty"]) == (None, 0)


def test_entry_clouds_equal_the_candidate_segments_of_verify_loop_pairs(street):
    from qn_amd import engine
    st = street; store, ctx, pp = st["store"], st["ctx"], st["pp"]
    cs = [c for c in range(N) if c + RANGE < N - 1]                                # where `i < n` and `i < n - 1` give the same window
    assert cs == list(range(11))
    store.verify_loop_pairs(ctx, [13] * len(cs), cs, None, pp, RANGE, LEAF)
    for j, c in enumerate(cs):
        assert engine.local_submap_ids(c, RANGE, N) == engine.loop_submap_ids(13, c, RANGE, False, False, N)[1]
        dst = store.verify_cloud(j, engine.QN_VERIFY_DST)
        assert np.array_equal(dst.view(np.uint32), _entry(store, c)[2][:, :3].copy().view(np.uint32)), c


def _rows_equal_qn_fpfh(engine, store, ctx, ks):
    for k in ks:
        p, n, rec = _entry(store, k)
        rows = store.submap_features(k)
        want = engine.fpfh(ctx, rec[:, :3].copy())
        assert rows.shape == (n, 33) and np.array_equal(rows.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), k
        assert not np.isnan(rows).all()


def test_entry_rows_equal_qn_fpfh(street):
    from qn_amd import engine
    fresh = _ctx(engine)
    _rows_equal_qn_fpfh(engine, street["store"], fresh, [0, 1, 5, 12, 13])
    fresh.close()
    assert street["store"].submap_features(street["empty"]).shape == (0, 33)


def test_describe_in_chunks_gives_the_same_entries():
    """a context of 200000 points has 3.2 M grid cells: 25.6 MB of tables per window, so 42 windows pass the 1 GiB budget and are taken in two chunks"""
    from qn_amd import engine
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100)]
    pp = _perturbed(poses)
    big = engine.Context(200000); engine.Quatro(big)
    assert store.submap_describe(big, ids, pp, RANGE, LEAF) == [0] * N
    want = {k: (_entry(store, k)[2], store.submap_features(k)) for k in ids}
    per_window = 2 * 4 * (16 * 200000 + 1)
    assert 42 * per_window > (1 << 30) > 14 * per_window
    assert store.submap_describe(big, ids * 3, pp, RANGE, LEAF) == [0] * (3 * N)
    for k in ids:
        assert np.array_equal(_entry(store, k)[2].view(np.uint32), want[k][0].view(np.uint32)), k
        assert np.array_equal(store.submap_features(k).view(np.uint32), want[k][1].view(np.uint32)), k
    _rows_equal_qn_fpfh(engine, store, big, [0, 6, 13])
    big.close(); store.close()


# ------------------------------------------------------------------ 2. the records
def _scrambled_pairs(street):
    """every oracle pair, more pairs that repeat queries and candidates, one pair with an empty side; scrambled; more pairs than the context has lanes (4)"""
    pairs = [(q, c) for q, c, _ in GICP_PAIRS] + [(13, 2), (10, 0), (11, 1), (11, 3), (10, 2), (0, 10), (street["empty"], 3), (12, 3)]
    rng = np.random.default_rng(9)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert len(pairs) > 4 and len({q for q, _ in pairs}) < len(pairs) and len({c for _, c in pairs}) < len(pairs)
    yaws = [0.0 if street["empty"] in (q, c) else _yaw(street["poses"], q, c) for q, c in pairs]
    return pairs, yaws


def test_gicp_records_equal_the_batch_on_the_entry_clouds(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    pairs, yaws = _scrambled_pairs(st)
    out = store.verify_loop_pairs_submap(ctx, [p[0] for p in pairs], [p[1] for p in pairs], yaws, THR)
    live = [j for j, (q, c) in enumerate(pairs) if st["empty"] not in (q, c)]
    descs = []
    for j in live:
        (sp, sn), (dp, dn) = store.submap_cloud(pairs[j][0]), store.submap_cloud(pairs[j][1])
        descs.append((sp, sn, dp, dn, 16, 1))
    res, val, sta = engine.gicp_align_batch(ctx, descs, score_thr=THR, guesses=[sc.seed_from_yaw(yaws[j]) for j in live])
    for k, j in enumerate(live):
        print("gicp", pairs[j], out[j]["valid"], out[j]["score"], out[j]["iterations"])
        assert _gout(out[j]) == _grec(res[k], val[k], sta[k]), pairs[j]
    j, = [j for j in range(len(pairs)) if j not in live]
    assert out[j]["status"] == engine.QN_ERR_EMPTY_CLOUD and not out[j]["valid"] and out[j]["score"] == sys.float_info.max
    assert np.array_equal(out[j]["T"], np.eye(4))
    assert any(o["valid"] for o in out) and any(not o["valid"] and o["status"] == 0 for o in out)
    # SRC / DST of the record are the entries; FINAL = SRC through the pair's f32 T as k_transform_cloud applies it
    j = pairs.index((12, 2))
    src = _entry(store, 12)[2][:, :3].copy()
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_SRC).view(np.uint32), src.view(np.uint32))
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_DST).view(np.uint32), _entry(store, 2)[2][:, :3].copy().view(np.uint32))
    T = np.array(out[j]["record"].T, np.float32).reshape(4, 4); x, y, z = src[:, 0], src[:, 1], src[:, 2]
    final = np.stack([T[r, 0] * x + (T[r, 1] * y + (T[r, 2] * z + T[r, 3])) for r in range(3)], 1).astype(np.float32)
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_FINAL).view(np.uint32), final.view(np.uint32))
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(j, engine.QN_VERIFY_COARSE)
    assert e.value.status == engine.QN_ERR_NOT_READY


def test_c2f_records_equal_the_batch_on_the_entry_clouds(street):
    from qn_amd import engine
    st = street; store, ctx = st["store"], st["ctx"]
    pairs, _ = _scrambled_pairs(st)
    pairs += [(q, c) for q, c, _ in C2F_PAIRS if (q, c) not in pairs]
    out = store.verify_loop_pairs_submap_c2f(ctx, [p[0] for p in pairs], [p[1] for p in pairs], THR)
    descs = []
    for q, c in pairs:
        (sp, sn), (dp, dn) = store.submap_cloud(q), store.submap_cloud(c)
        descs.append((sp or 0, sn, dp or 0, dn, 16, 1))
    want = engine.coarse_to_fine_align_batch([ctx], descs, score_thr=THR)
    for p, o, w in zip(pairs, out, want):
        print("c2f", p, o["status"], o["valid"], o["score"], o["iterations"])
        assert _crec(o) == _crec(w), p
    j, = [j for j, (q, c) in enumerate(pairs) if st["empty"] in (q, c)]
    assert out[j]["status"] == engine.QN_ERR_EMPTY_CLOUD and not out[j]["valid"]
    assert any(o["valid"] for o in out) and any(not o["valid"] and o["status"] == 0 for o in out)
    j = pairs.index((13, 3))
    src = _entry(store, 13)[2][:, :3].copy()
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_SRC).view(np.uint32), src.view(np.uint32))
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_DST).view(np.uint32), _entry(store, 3)[2][:, :3].copy().view(np.uint32))
    T = out[j]["T_quatro"]; x, y, z = (src[:, i].astype(np.float64) for i in range(3))
    coarse = np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32) for r in range(3)], 1)
    assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_COARSE).view(np.uint32), coarse.view(np.uint32))
    assert len(store.verify_cloud(j, engine.QN_VERIFY_FINAL)) == len(src)


# ------------------------------------------------------------------ 3. against the CPU oracle
def _oracle_clouds(street):
    from qn_amd import engine
    from oracle import oracle as orc
    scans = [synth.lidar_scan(street["prims"], street["sen"], P, 100 + k)[:, :3] for k, P in enumerate(street["poses"])]
    def local(x):
        ids, rel = _window(engine, x, street["pp"])
        return orc.assemble_submap(scans, dict(zip(ids, rel)), ids, LEAF)
    return local


def test_gicp_against_the_oracle(street):
    from oracle import oracle as orc
    st = street; store, ctx = st["store"], st["ctx"]
    local = _oracle_clouds(st)
    yaws = [_yaw(st["poses"], q, c) for q, c, _ in GICP_PAIRS]
    out = store.verify_loop_pairs_submap(ctx, [p[0] for p in GICP_PAIRS], [p[1] for p in GICP_PAIRS], yaws, THR)
    for (q, c, flag), y, o in zip(GICP_PAIRS, yaws, out):
        g = orc.GicpOracle(k=15, max_iter=32, max_corr_dist=MAX_CORR, trans_eps=0.01)
        g.set_source(local(q)); g.compute_covariances(0); g.set_target(local(c)); g.compute_covariances(1)
        r = g.align(sc.seed_from_yaw(y).astype(np.float64))
        valid = bool(r["converged"] and r["fitness"] < THR)
        et, er = synth.pose_error(o["T"], r["Tf"].astype(np.float64))
        print("oracle gicp", (q, c), valid, r["fitness"], r["iterations"], "engine", o["valid"], o["score"], o["iterations"], et, er)
        assert valid == flag, (q, c, r["fitness"])
        assert o["status"] == 0 and o["valid"] == valid and o["iterations"] == r["iterations"], (q, c)
        assert et <= 1e-4 and er <= 1e-4, (q, c, et, er)
        if valid:
            gt, gr = synth.pose_error(o["T"], np.linalg.inv(st["poses"][c]) @ st["poses"][q])
            assert gt <= 0.05 and gr <= math.radians(0.2), (q, c, gt, gr)


def test_c2f_against_the_oracle(street):
    from oracle import oracle as orc
    st = street; store, ctx = st["store"], st["ctx"]
    local = _oracle_clouds(st)
    out = store.verify_loop_pairs_submap_c2f(ctx, [p[0] for p in C2F_PAIRS], [p[1] for p in C2F_PAIRS], THR)
    for (q, c, flag), o in zip(C2F_PAIRS, out):
        w = orc.coarse_to_fine_alignment(local(q), local(c), max_corr_dist=MAX_CORR, score_thr=THR)
        et, er = synth.pose_error(o["T"], w["T"])
        print("oracle c2f", (q, c), w["valid"], w["score"], w.get("iterations"), "engine", o["valid"], o["score"], o["iterations"], et, er)
        assert w["valid"] == flag and w["quatro"]["valid"], (q, c, w["score"])
        assert o["status"] == 0 and o["valid"] == w["valid"] and o["iterations"] == w["iterations"], (q, c)
        assert et <= 1e-4 and er <= 1e-4, (q, c, et, er)


# ------------------------------------------------------------------ 4. invariance
def test_records_do_not_depend_on_the_frame_or_on_poses_outside_the_windows(street):
    from qn_amd import engine
    st = street; pp = st["pp"]
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(st["prims"], st["sen"], st["poses"], np.arange(N) + 100)]
    ctx = _ctx(engine, lanes=4)
    qs, cs = [12, 13, 10, 12], [2, 3, 5, 7]
    yaws = [_yaw(st["poses"], q, c) for q, c in zip(qs, cs)]
    used = sorted(set(qs + cs))

    def records(poses, which, n_pairs=len(qs)):
        q, c, y = qs[:n_pairs], cs[:n_pairs], yaws[:n_pairs]
        assert store.submap_describe(ctx, which, poses, RANGE, LEAF) == [0] * len(which)
        return ([_gout(o) for o in store.verify_loop_pairs_submap(ctx, q, c, y, THR)], [_crec(o) for o in store.verify_loop_pairs_submap_c2f(ctx, q, c, THR)],
                [_entry(store, k)[2].tobytes() for k in sorted(set(q + c))])
    base = records(pp, ids)
    G = np.array([[0.0, -1.0, 0.0, 731.0], [1.0, 0.0, 0.0, -2048.0], [0.0, 0.0, 1.0, 16.0], [0.0, 0.0, 0.0, 1.0]])
    assert np.array_equal(G, G.astype(np.float32))
    moved = records([G @ P for P in pp], ids)
    assert moved[2] == base[2] and moved[0] == base[0] and moved[1] == base[1]
    # corrected poses that leave the windows alone: only the entries of (12, 2) and (13, 3) are described, every pose outside their windows is moved
    base2 = records(pp, ids, 2)
    assert base2[0] == base[0][:2] and base2[1] == base[1][:2]                      # (a pair's record does not depend on the pairs beside it)
    inside = {i for k in qs[:2] + cs[:2] for i in engine.local_submap_ids(k, RANGE, N)}
    outside = [i for i in range(N) if i not in inside]
    assert outside == [6, 7, 8, 9]
    drift = [P.copy() for P in pp]
    for i in outside:
        drift[i] = G @ drift[i]
    store.submap_release()
    far = records(drift, qs[:2] + cs[:2], 2)
    assert far == base2
    ctx.close(); store.close()


# ------------------------------------------------------------------ 5. lifetime and refused arguments
def test_refused_arguments_change_nothing(street):
    from qn_amd import engine
    st = street; store, ctx, pp = st["store"], st["ctx"], st["pp"]
    out = store.verify_loop_pairs_submap(ctx, [12, 13], [2, 3], [_yaw(st["poses"], 12, 2), _yaw(st["poses"], 13, 3)], THR)
    before = {k: (_entry(store, k)[0], _entry(store, k)[2].tobytes()) for k in range(N)}
    src0 = store.verify_cloud(0, engine.QN_VERIFY_SRC).tobytes()
    pairs_before = ctx.debug_get("batch_pairs")
    nan = [P.copy() for P in pp]; nan[6][0, 3] = float("nan")
    base = dict(ids=[1, 2], poses=pp, leaf=LEAF)
    for b in (dict(ids=[]), dict(ids=[-1]), dict(ids=[99]), dict(ids=[13], poses=pp[:13]), dict(poses=nan), dict(leaf=0.0), dict(leaf=-1.0),
              dict(ids=[st["empty"]], poses=pp + [np.eye(4)] * 3)):          # (17 poses but 15 keyframes: a window member that is no keyframe)
        a = dict(base); a.update(b)
        with pytest.raises(engine.EngineError) as e:
            store.submap_describe(ctx, a["ids"], a["poses"], RANGE, a["leaf"])
        assert e.value.status == engine.QN_ERR_INVALID_ARG, b
    other = engine.KeyframeStore()
    for b in (dict(query=[-1], cand=[2]), dict(query=[12], cand=[12]), dict(query=[12, 12], cand=[2, 2]), dict(query=[], cand=[]), dict(query=[12], cand=[99])):
        for call in (lambda: store.verify_loop_pairs_submap(ctx, b["query"], b["cand"], None, THR), lambda: store.verify_loop_pairs_submap_c2f(ctx, b["query"], b["cand"], THR)):
            with pytest.raises(engine.EngineError) as e:
                call()
            assert e.value.status == engine.QN_ERR_INVALID_ARG, b
    for y in ([float("nan")], [float("inf")]):
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_pairs_submap(ctx, [12], [2], y, THR)
        assert e.value.status == engine.QN_ERR_INVALID_ARG
    with pytest.raises(engine.EngineError) as e:
        store.submap_release([99])
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    # entries of another grid capacity or other radii, or without rows: refused by the coarse-to-fine form only
    bigger = _ctx(engine, cap=4 * CAP)
    radii = _ctx(engine); engine.Quatro(radii, fpfh_normal_radius=1.0, fpfh_radius=1.6)
    for c2 in (bigger, radii):
        with pytest.raises(engine.EngineError) as e:
            store.verify_loop_pairs_submap_c2f(c2, [12], [2], THR)
        assert e.value.status == engine.QN_ERR_INVALID_ARG
    bigger.close(); radii.close(); other.close()
    assert ctx.debug_get("batch_pairs") == pairs_before
    for k in range(N):
        assert (_entry(store, k)[0], _entry(store, k)[2].tobytes()) == before[k], k
    assert store.verify_cloud(0, engine.QN_VERIFY_SRC).tobytes() == src0
    assert _gout(store.verify_loop_pairs_submap(ctx, [12, 13], [2, 3], [_yaw(st["poses"], 12, 2), _yaw(st["poses"], 13, 3)], THR)[0]) == _gout(out[0])


def test_entries_without_rows_and_over_capacity():
    from qn_amd import engine
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(N) + 100)]
    pp = _perturbed(poses)
    ctx = _ctx(engine)
    assert store.submap_describe(ctx, [12, 2], pp, RANGE, LEAF, with_features=False) == [0, 0]
    with pytest.raises(engine.EngineError) as e:
        store.submap_features(12)
    assert e.value.status == engine.QN_ERR_NOT_READY
    with pytest.raises(engine.EngineError) as e:
        store.verify_loop_pairs_submap_c2f(ctx, [12], [2], THR)
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    r, = store.verify_loop_pairs_submap(ctx, [12], [2], [_yaw(poses, 12, 2)], THR)          # the GICP form needs no rows
    assert r["status"] == 0 and r["valid"]
    with pytest.raises(engine.EngineError) as e:
        store.submap_cloud(5)
    assert e.value.status == engine.QN_ERR_NOT_READY
    # a context that takes fewer points than a window holds: no entry for it (an earlier one goes), the single scan beside it is described
    n12 = store.submap_cloud(12)[1]
    n_scan = store.assemble([3], [np.eye(4)], LEAF, 0)[1]
    assert n_scan < n12
    small = engine.Context(n12 - 1); engine.Quatro(small)
    assert store.submap_describe(small, [12], pp, RANGE, LEAF) == [engine.QN_ERR_CAPACITY]
    with pytest.raises(engine.EngineError) as e:
        store.submap_cloud(12)
    assert e.value.status == engine.QN_ERR_NOT_READY
    assert store.submap_cloud(2)[1] > 0
    small.close(); ctx.close(); store.close()


def test_redescribe_and_release_drop_the_record_and_spare_the_scan_entries(street):
    from qn_amd import engine
    st = street; store, ctx, pp = st["store"], st["ctx"], st["pp"]
    assert store.quatro_describe(ctx, [12, 2, 13, 3], LEAF) == [0] * 4
    scan = {k: (store.quatro_cloud(k), store.quatro_features(k).tobytes()) for k in (12, 2, 13, 3)}
    s2s = store.verify_loop_pairs_c2f(ctx, [12], [2], THR)
    store.verify_loop_pairs_submap_c2f(ctx, [12, 13], [2, 3], THR)
    assert len(store.verify_cloud(1, engine.QN_VERIFY_COARSE)) == store.submap_cloud(13)[1]
    store.submap_describe(ctx, [5], pp, RANGE, LEAF)                               # an entry the record does not name: it stays
    assert len(store.verify_cloud(0, engine.QN_VERIFY_SRC)) == store.submap_cloud(12)[1]
    store.quatro_describe(ctx, [12], LEAF)                                         # the scan entry of an involved keyframe: the submap record stays
    assert len(store.verify_cloud(0, engine.QN_VERIFY_SRC)) == store.submap_cloud(12)[1]
    store.submap_describe(ctx, [3], pp, RANGE, LEAF)                               # an involved entry described again: the record goes
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(0, engine.QN_VERIFY_SRC)
    assert e.value.status == engine.QN_ERR_NOT_READY
    store.verify_loop_pairs_submap(ctx, [12, 13], [2, 3], None, THR)
    store.submap_release([7])                                                      # not involved
    assert len(store.verify_cloud(1, engine.QN_VERIFY_DST)) == store.submap_cloud(3)[1]
    store.submap_release([13])
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(1, engine.QN_VERIFY_DST)
    assert e.value.status == engine.QN_ERR_NOT_READY
    for k in (13, 7):
        with pytest.raises(engine.EngineError) as e:
            store.submap_cloud(k)
        assert e.value.status == engine.QN_ERR_NOT_READY
    with pytest.raises(engine.EngineError) as e:
        store.verify_loop_pairs_submap(ctx, [13], [3], None, THR)
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    store.verify_loop_pairs_submap(ctx, [12], [2], None, THR)
    store.submap_release()                                                         # all
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(0, engine.QN_VERIFY_SRC)
    assert e.value.status == engine.QN_ERR_NOT_READY
    # the scan-to-scan entries of the same keyframes lived through all of it
    for k in (2, 13, 3):
        assert (store.quatro_cloud(k), store.quatro_features(k).tobytes()) == scan[k], k
    assert _crec(store.verify_loop_pairs_c2f(ctx, [12], [2], THR)[0]) == _crec(s2s[0])
    # and back, for the tests that follow in this module; a store destroyed with live entries is the fixture's teardown
    assert store.submap_describe(ctx, st["ids"], pp, RANGE, LEAF) == [0] * N
    assert store.submap_describe(ctx, [st["empty"]], pp + [np.eye(4)], 0, LEAF) == [engine.QN_ERR_EMPTY_CLOUD]


# ------------------------------------------------------------------ 6. the layers above
def test_cpp_helpers_return_the_python_records(tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_submap_verify.cpp", tmp_path)
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    clouds = [synth.lidar_scan(prims, sen, P, 100 + k)[:, :3] for k, P in enumerate(poses)]
    stamps = np.arange(len(clouds)) * 10.0
    pp = _perturbed(poses)
    with open(tmp_path / "kf.bin", "wb") as f:
        for c in clouds:
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    stamps.tofile(tmp_path / "st.bin")
    np.ascontiguousarray(np.array(pp, np.float64).reshape(-1, 16)).tofile(tmp_path / "poses.bin")
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
        assert store.submap_describe(ctx, ids, pp, RANGE, LEAF, with_features=bool(c2f)) == [0] * len(ids)
        if c2f:
            want = store.verify_loop_pairs_submap_c2f(ctx, [k[0] for k in keep], [k[1] for k in keep])
        else:
            want = store.verify_loop_pairs_submap(ctx, [k[0] for k in keep], [k[1] for k in keep], [k[2] for k in keep])
        assert any(w["valid"] for w in want)
        for g, w in zip(got, want):
            assert (int(g[2]) == 1) == w["valid"] and int(g[3]) == w["status"] and float(g[4]) == w["score"], (g, w)
            assert np.array_equal(np.array([float(x) for x in g[5:21]]), w["T"].reshape(-1)), (g, w)
    ctx.close(); store.close()


@pytest.mark.parametrize("quatro", [False, True])
def test_replay_with_submap_matching_matches_the_oracle_backend(quatro):
    """spinning sensor, 66 keyframes, seed 7, yaw_bias 0.02 (the stream of tests/test_gpu_loop_pairs.py's catch-up replay), submap_range 2: chosen on the oracle
    backend, which closes (33, 0) with score 0.789 on both paths, ATE 22.2 -> 10.7 m.  Tolerance 1e-3 m on the corrected poses, as tests/test_replay.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    kw = dict(verbose=False, n_kf=66, seed=7, sensor="spinning", detector="scancontext", verify="relative", yaw_bias=0.02, submap_matching=True, submap_range=2,
              use_quatro=quatro)
    gpu = replay.run(**kw)
    orc = replay.run(backend="oracle", **kw)
    assert [(k, c) for k, c, _ in orc["loop_list"]] == [(33, 0)]
    assert [(k, c) for k, c, _ in gpu["loop_list"]] == [(k, c) for k, c, _ in orc["loop_list"]] and gpu["attempts"] == orc["attempts"]
    for (_, _, sa), (_, _, sb) in zip(gpu["loop_list"], orc["loop_list"]):
        assert abs(sa - sb) <= 1e-5 * max(sb, 1e-9)
    assert gpu["ate_corrected"] < 0.6 * gpu["ate_odometry"]
    dev = max(np.linalg.norm(a[:3, 3] - b[:3, 3]) for a, b in zip(gpu["poses"], orc["poses"]))
    assert dev < 1e-3, dev
