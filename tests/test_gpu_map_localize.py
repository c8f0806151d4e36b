"""Scans localised in the corrected map on the GPU (qn_kf_map_localize / qn_kf_map_localize_c2f) on the ray-cast street scene of the other map tests: four scans
of 16 x 300 rays, the map built from the true poses at leaf 0.3.

What is pinned bit for bit: the scan cloud to qn_kf_assemble_batch of the keyframe alone with the identity, the crop to the twin (qn_amd/maplocalize.py) on the
downloaded map, every record to qn_gicp_align_batch_guess / qn_coarse_to_fine_align_batch on the downloaded clouds, the verify clouds to the twin's transform,
the overlap to qn_kf_overlap_batch on the same clouds.

The record tests crop with RADIUS = 12 m, far inside the scans' reach (100 m), so every crop is a real subset of the map; the fitness score is then large
(scan points beyond the crop have no partner) and the valid flag is not asked of them.  The sanity and overlap tests crop with WIDE = 150 m, which holds
everything a scan can see.

Sanity: every scan starts SHIFT = 0.5 m / YAW = 3 degrees away from its true pose and must end valid and nearer to it in translation and in rotation.  On the
CPU the oracle (the reference's Nano-GICP, k = 15, 32 iterations, max_corr_dist 18, trans_eps 0.01; the oracle's own voxel grid of the same four scans and of
the map, 9313 points; the crop by the twin at 150 m; the same guess) converges for all four scans from that displacement in 3 iterations: guess errors
0.5000 m / 3.000 deg, oracle results 0.00033 / 0.00146 / 0.00131 / 0.00220 m with rotation errors below 1e-5 deg, scores 0.0050 / 0.0047 / 0.0056 / 0.0046,
far below the threshold 1.5 - so the displacement was not shrunk."""
import ctypes as C
import math
import numpy as np
import pytest
from qn_amd import maplocalize as ml, synth

pytestmark = pytest.mark.gpu
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
LEAF, RADIUS, WIDE, MAX_CORR, CAP, THR = 0.3, 12.0, 150.0, 18.0, 60000, 1.5
SHIFT, YAW = 0.5, 3.0


def displaced(P, shift=SHIFT, yaw_deg=YAW):
    """the pose P with the sensor moved by `shift` metres (along 0.6, 0.8, 0 of its own frame) and turned by yaw_deg about its z axis"""
    a = math.radians(yaw_deg); D = np.eye(4)
    D[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]; D[:3, 3] = (0.6 * shift, 0.8 * shift, 0.0)
    return np.asarray(P, np.float64) @ D


def _ctx(engine, cap=CAP):
    ctx = engine.Context(cap)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    return ctx


@pytest.fixture(scope="module")
def scene():
    from qn_amd import engine
    store = engine.KeyframeStore()
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]
    ctx = _ctx(engine)
    yield dict(store=store, ctx=ctx, ids=ids, params=engine.LocalizeParams(RADIUS, LEAF, THR, 0), wide=engine.LocalizeParams(WIDE, LEAF, THR, 0))
    ctx.close(); store.close()


def _map(st):
    store = st["store"]
    n = store.build_map(st["ids"], POSES, LEAF)
    assert 3000 <= n <= 40000, n
    return store.download_map(n)


def _grec(r, v, s):
    return (int(s), bool(v), r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def _crec(o):
    return (o["status"], o["valid"], o["iterations"], o["converged"], o["score"], o["T"].tobytes(), o["T_quatro"].tobytes(), o["T_gicp"].tobytes())


def _clouds(st, m, j, G, radius=RADIUS):
    """pair j's two clouds as the record serves them, the scan pinned to the keyframe's own voxel grid and the crop to the twin -> (scan (n, 3), crop (k, 4))"""
    from qn_amd import engine
    store = st["store"]
    src = store.verify_cloud(j, engine.QN_VERIFY_SRC); dst = store.verify_cloud(j, engine.QN_VERIFY_DST)
    rec, _ = ml.crop(m, ml.guess_f32(G)[:3, 3], radius, ml.SPHERE)
    assert len(rec) > 0 and dst.tobytes() == np.ascontiguousarray(rec[:, :3]).tobytes()
    return src, rec


def _reference(engine, ctx, src, crop, G):
    """gicp_align_batch of the downloaded clouds (host memory, both as float4 records) from the guess -> the record tuple"""
    s4 = np.ones((len(src), 4), np.float32); s4[:, :3] = src
    r, v, s = engine.gicp_align_batch(ctx, [(s4, len(s4), np.ascontiguousarray(crop), len(crop), 16, 0)], THR, guesses=[G])
    return _grec(r[0], v[0], s[0])


def test_one_pair_equals_the_batch_registration_of_its_clouds(scene):
    from qn_amd import engine
    st = scene; store, ctx = st["store"], st["ctx"]
    m = _map(st)
    G = displaced(POSES[1])
    out, stats = store.map_localize(ctx, [st["ids"][1]], [G], st["params"])
    assert (stats["n_map"], stats["n_pairs"], stats["n_scans"], stats["n_crops"], stats["passes"]) == (len(m), 1, 1, 1, 1)
    src, crop = _clouds(st, m, 0, G)
    assert stats["crop_points"] == len(crop) and 0 < len(crop) < len(m)
    (ap, an, ast), = store.assemble_batch([[st["ids"][1]]], [[np.eye(4)]], LEAF)
    seg = store.download_batch(0, an) if an else None
    assert ast == 0 and an == len(src) and np.ascontiguousarray(seg[:, :3]).tobytes() == src.tobytes()      # the keyframe alone in its sensor frame at the leaf
    got = _grec(out[0]["record"], out[0]["valid"], out[0]["status"])
    assert got == _reference(engine, ctx, src, crop, G)
    assert out[0]["status"] == 0
    g = store.map_crop_get(0)                                        # the crop is served like a map_crop's
    assert g["xyzi"].tobytes() == crop.tobytes()


def test_pairs_of_several_queries_out_of_query_order(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    m = _map(st)
    q = [2, 0, 2, 1, 0]
    G = [displaced(POSES[2]), displaced(POSES[0], 0.3, -2.0), displaced(POSES[2], 0.4, -3.0), displaced(POSES[1], 0.2, 1.0), displaced(POSES[0])]
    out, stats = store.map_localize(ctx, [ids[k] for k in q], G, st["params"])
    assert (stats["n_pairs"], stats["n_scans"], stats["n_crops"]) == (5, 3, 5)
    for j in range(5):
        src, crop = _clouds(st, m, j, G[j])
        assert _grec(out[j]["record"], out[j]["valid"], out[j]["status"]) == _reference(engine, ctx, src, crop, G[j]), j
        assert out[j]["status"] == 0, j
    assert store.verify_cloud(0, engine.QN_VERIFY_SRC).tobytes() == store.verify_cloud(2, engine.QN_VERIFY_SRC).tobytes()


def test_two_headings_at_one_position_share_the_crop(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    m = _map(st)
    G = [displaced(POSES[1], 0.0, 3.0), displaced(POSES[1], 0.0, -3.0)]
    assert np.array_equal(G[0][:3, 3], G[1][:3, 3])
    out, stats = store.map_localize(ctx, [ids[1], ids[1]], G, st["params"])
    assert (stats["n_pairs"], stats["n_scans"], stats["n_crops"]) == (2, 1, 1)
    ptr = [C.c_void_p(), C.c_void_p()]; n = C.c_uint32()
    for j in range(2):
        assert store._l.qn_kf_verify_cloud(store.h, C.c_uint32(j), C.c_int(engine.QN_VERIFY_DST), C.byref(ptr[j]), C.byref(n)) == 0
        src, crop = _clouds(st, m, j, G[j])
        assert _grec(out[j]["record"], out[j]["valid"], out[j]["status"]) == _reference(engine, ctx, src, crop, G[j]), j
    assert ptr[0].value == ptr[1].value and stats["crop_points"] == n.value
    with pytest.raises(engine.EngineError):
        store.map_crop_get(1)


def test_statuses_and_refusals(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids, P = st["store"], st["ctx"], st["ids"], st["params"]
    m = _map(st)
    far = np.eye(4); far[:3, 3] = (1000.0, 0.0, 0.0)
    G = [displaced(POSES[0]), far, displaced(POSES[3])]
    out, stats = store.map_localize(ctx, [ids[0], ids[1], ids[3]], G, P)
    assert [o["status"] for o in out] == [0, engine.QN_ERR_EMPTY_CLOUD, 0] and not out[1]["valid"]
    assert stats["n_crops"] == 3
    for j in (0, 2):
        src, crop = _clouds(st, m, j, G[j])
        assert _grec(out[j]["record"], out[j]["valid"], out[j]["status"]) == _reference(engine, ctx, src, crop, G[j]), j
    with pytest.raises(engine.EngineError):
        store.verify_cloud(1, engine.QN_VERIFY_FINAL)                # nothing was registered for the pair
    small = _ctx(engine, 256)                                        # a context that takes fewer points than a scan has
    try:
        out, _ = store.map_localize(small, [ids[0]], [G[0]], P)
        assert out[0]["status"] == engine.QN_ERR_CAPACITY and not out[0]["valid"]
    finally:
        small.close()
    # ---- whole-call refusals: before anything runs, the record of the call above stays served
    keep = store.verify_cloud(0, engine.QN_VERIFY_SRC)
    L = store._l
    q = np.array([ids[0]], np.int32); g = np.ascontiguousarray(G[0].reshape(1, 16)); res = (engine.GicpResult * 1)(); v = np.zeros(1, np.int32); s = np.zeros(1, np.int32)
    pq, pg, pv, ps = (a.ctypes.data_as(C.c_void_p) for a in (q, g, v, s))

    def call(params=P, query=pq, guess=pg, n=1, results=res, valid=pv, status=ps, context=ctx.h):
        return L.qn_kf_map_localize(store.h, context, C.byref(params) if params is not None else None, query, guess, C.c_uint32(n), results, valid, status, None)
    I = engine.QN_ERR_INVALID_ARG
    assert call(params=None) == I and call(query=None) == I and call(guess=None) == I and call(n=0) == I and call(results=None) == I
    assert call(valid=None) == I and call(status=None) == I and call(context=None) == I
    for bad in (engine.LocalizeParams(0.0, LEAF, THR, 0), engine.LocalizeParams(float("nan"), LEAF, THR, 0), engine.LocalizeParams(RADIUS, 0.0, THR, 0),
                engine.LocalizeParams(RADIUS, LEAF, float("nan"), 0), engine.LocalizeParams(RADIUS, LEAF, THR, 2)):
        assert call(params=bad) == I
    r = engine.LocalizeParams(RADIUS, LEAF, THR, 0); r.reserved = 1
    assert call(params=r) == I
    for bad_id in (-1, len(ids)):
        b = np.array([bad_id], np.int32)
        assert call(query=b.ctypes.data_as(C.c_void_p)) == I
    for k, val in ((5, np.nan), (3, np.inf), (12, 1e-9), (15, 2.0)):
        b = g.copy(); b[0, k] = val
        assert call(guess=b.ctypes.data_as(C.c_void_p)) == I, k
    Tt = np.zeros((1, 4, 4))
    assert L.qn_kf_map_localize_c2f(store.h, ctx.h, C.byref(P), pq, pg, C.c_uint32(1), res, None, None, pv, ps, None) == I
    assert store.verify_cloud(0, engine.QN_VERIFY_SRC).tobytes() == keep.tobytes()
    empty = engine.KeyframeStore()
    try:
        kid = empty.add(np.zeros((3, 3), np.float32))
        b = np.array([kid], np.int32)
        assert L.qn_kf_map_localize(empty.h, ctx.h, C.byref(P), b.ctypes.data_as(C.c_void_p), pg, C.c_uint32(1), res, pv, ps, None) == engine.QN_ERR_NOT_READY
    finally:
        empty.close()


def test_verify_record_serves_the_clouds_and_the_overlap(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    m = _map(st)
    G = [displaced(POSES[2]), displaced(POSES[3], 0.3, -2.0)]
    out, _ = store.map_localize(ctx, [ids[2], ids[3]], G, st["wide"])
    pairs = []
    for j in range(2):
        src, crop = _clouds(st, m, j, G[j], WIDE)
        fin = store.verify_cloud(j, engine.QN_VERIFY_FINAL)
        assert fin.tobytes() == ml.transform_final(src, np.array(out[j]["record"].T, np.float32).reshape(4, 4)).tobytes(), j
        with pytest.raises(engine.EngineError):
            store.verify_cloud(j, engine.QN_VERIFY_COARSE)           # the GICP form has no coarse stage
        pf, pd, nf, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        assert store._l.qn_kf_verify_cloud(store.h, C.c_uint32(j), C.c_int(engine.QN_VERIFY_FINAL), C.byref(pf), C.byref(nf)) == 0
        assert store._l.qn_kf_verify_cloud(store.h, C.c_uint32(j), C.c_int(engine.QN_VERIFY_DST), C.byref(pd), C.byref(nd)) == 0
        pairs.append((pf.value, nf.value, pd.value, nd.value))
    got = store.verify_overlap(0.5, n_pairs=2)
    want = store.overlap_batch(pairs, 0.5)
    assert got == want and all(o["status"] == 0 for o in got)
    for o in got:                                                    # the map explains the scan; the scan sees a part of the neighbourhood
        a, b = o["a_to_b"], o["b_to_a"]
        assert a["inliers"] > 0.9 * a["n"] and b["inliers"] < 0.8 * b["n"]


def test_a_filtered_map_leaves_the_record_and_the_next_crop_ends_it(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    _map(st)
    G = [displaced(POSES[1])]
    out, stats = store.map_localize(ctx, [ids[1]], G, st["params"])
    src = store.verify_cloud(0, engine.QN_VERIFY_SRC); dst = store.verify_cloud(0, engine.QN_VERIFY_DST); fin = store.verify_cloud(0, engine.QN_VERIFY_FINAL)
    store.map_outliers(engine.OutlierParams())
    _, left = store.map_remove_outliers()
    assert left < stats["n_map"]
    assert store.verify_cloud(0, engine.QN_VERIFY_SRC).tobytes() == src.tobytes() and store.verify_cloud(0, engine.QN_VERIFY_DST).tobytes() == dst.tobytes()
    assert store.verify_cloud(0, engine.QN_VERIFY_FINAL).tobytes() == fin.tobytes()
    assert store.map_crop_get(0)["n"] == len(dst)
    _, stats2 = store.map_localize(ctx, [ids[1]], G, st["params"])
    assert stats2["generation"] > stats["generation"] and stats2["n_map"] == left      # the old record's generation said which map it came from
    store.map_crop([(0.0, 0.0, 0.0)], 5.0)
    for which in (engine.QN_VERIFY_SRC, engine.QN_VERIFY_DST, engine.QN_VERIFY_FINAL):
        with pytest.raises(engine.EngineError) as ei:
            store.verify_cloud(0, which)
        assert ei.value.status == engine.QN_ERR_NOT_READY


def test_every_scan_ends_nearer_to_its_true_pose_than_it_started(scene):
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    _map(st)
    G = [displaced(P) for P in POSES]
    out, _ = store.map_localize(ctx, ids, G, st["wide"])
    for j, P in enumerate(POSES):
        gt, gr = synth.pose_error(G[j], P)
        et, er = synth.pose_error(out[j]["T"], P)
        print("scan %d: guess %.4f m / %.3f deg -> %.4f m / %.3f deg, score %.4f, %d iterations" % (j, gt, math.degrees(gr), et, math.degrees(er), out[j]["score"], out[j]["iterations"]))
        assert abs(gt - SHIFT) < 1e-9 and abs(math.degrees(gr) - YAW) < 1e-6
        assert out[j]["status"] == 0 and out[j]["valid"], j
        assert et < gt and er < gr, (j, et, er)


def test_coarse_to_fine_equals_the_batch_of_its_clouds(scene):
    from qn_amd import engine
    st = scene; store, ctx, ids = st["store"], st["ctx"], st["ids"]
    m = _map(st)
    G = [displaced(POSES[1]), displaced(POSES[2], 0.3, -2.0)]
    out, stats = store.map_localize_c2f(ctx, [ids[1], ids[2]], G, st["params"])
    assert (stats["n_pairs"], stats["n_scans"], stats["n_crops"]) == (2, 2, 2)
    for j in range(2):
        src, crop = _clouds(st, m, j, G[j])
        s4 = np.ones((len(src), 4), np.float32); s4[:, :3] = src
        want = engine.coarse_to_fine_align_batch([ctx], [(s4, len(s4), np.ascontiguousarray(crop), len(crop), 16, 0)], THR)
        assert _crec(out[j]) == _crec(want[0]), j

