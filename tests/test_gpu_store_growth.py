"""A result buffer of the keyframe store's extensions regrown under a result that is still readable: the overlap's per-point results, the free-space
classes, the static map's votes and kept records, and the arena qn_kf_verify_cloud computes into.  Each test walks ONE store through three calls - a small
one, one whose total is more than half again the first (the buffer has to be allocated anew; the arena is sized exactly, so any larger call moves it), the
small one again - and after every call compares the records and the per-point read-back bit for bit with the specification: the numpy twins
qn_amd/overlap.py, freespace.py and staticmap.py, and for qn_kf_verify_cloud the two transforms restated here in the order DESIGN.md gives
(COARSE: f64, ((T0 x + T1 y) + T2 z) + T3, rounded to f32; FINAL: that through the GICP T in f32, T0 x + (T1 y + (T2 z + T3))).  The third call's results
must also equal the first's.

Sizes: keyframes of 64 and of 4096 records (two tiles of the range-image kernels: FS_TILE = FS_BLOCK * FS_ITERS = 512 * 4 = 2048 records), so the totals are 128 / 192 records against 8192 / 12288; the street
revisits (12, 2) and (13, 3) of tests/test_gpu_sc_verify.py for the verify record, one pair against two."""
import math
import os
import sys
import numpy as np
import pytest
from qn_amd import freespace as fs, overlap as ov, staticmap as sm, synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SMALL, LARGE = 64, 4096
FIELDS = ("n", "n_finite", "in_fov", "observed", "seen_through", "occluded", "agree")


def _shell(seed, n, radius):
    """n records on a noisy shell around the sensor, inside the image's field of view mostly: a surface the other keyframes see nearer or farther"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-math.pi, math.pi, n); el = rng.uniform(-0.45, 0.45, n)
    r = radius + rng.normal(0, 0.4, n)
    a = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)
    a[1] = [np.nan, 1, 1]; a[2] = [0.1, 0.1, 0.0]                     # a non-finite record and one inside min_range
    return a


@pytest.fixture()
def ranged():
    """one store: three keyframes of SMALL records, three of LARGE, range images of all"""
    from qn_amd import engine
    store = engine.KeyframeStore()
    small = [store.add(_shell(10 + k, SMALL, 6.0 + 1.0 * k)) for k in range(3)]
    large = [store.add(_shell(20 + k, LARGE, 6.0 + 1.0 * k)) for k in range(3)]
    p = engine.RangeParams(n_rows=16, n_cols=48, el_lo=-0.4, el_hi=0.4, min_range=0.5, window_rows=1, window_cols=1, tol_abs=0.3, tol_rel=0.02)
    store.range_set_params(p)
    assert store.range_describe(small + large) == [0] * 6
    clouds = {i: store.keyframe(i) for i in small + large}
    yield dict(store=store, small=small, large=large, p=p.twin(), clouds=clouds)
    store.close()


def _poses(n):
    return [synth.sensor_pose(0.4 * k, -0.3 * k, 0.05 * k) for k in range(n)]


def test_overlap_results_regrown():
    import torch
    from qn_amd import engine
    store = engine.KeyframeStore()
    rng = np.random.default_rng(3)

    def pair(n):
        a = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
        b = (a[rng.permutation(n)] + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
        a4 = np.ones((n, 4), np.float32); a4[:, :3] = a
        b4 = np.ones((n, 4), np.float32); b4[:, :3] = b
        return a, b, torch.from_numpy(a4).cuda(), torch.from_numpy(b4).cuda()

    small, large = [pair(SMALL)], [pair(LARGE), pair(LARGE + 1)]
    radius = 0.8

    def step(pairs, what):
        recs = store.overlap_batch([(da.data_ptr(), len(a), db.data_ptr(), len(b)) for a, b, da, db in pairs], radius)
        out = []
        for slot, ((a, b, _, _), rec) in enumerate(zip(pairs, recs)):
            assert rec["status"] == 0, (what, slot)
            for d, key, x, y in ((0, "a_to_b", a, b), (1, "b_to_a", b, a)):
                nn_d2, nn_idx = ov.nearest(x, y, radius)
                want = ov.record(x, nn_d2)
                got = rec[key]
                d2, idx = store.overlap_points(slot, d)
                print(what, slot, key, {k: got[k] for k in ("n", "n_finite", "inliers")}, "sum_d2", got["sum_d2"])
                assert (got["n"], got["n_finite"], got["inliers"]) == (want["n"], want["n_finite"], want["inliers"]), (what, slot, key)
                assert np.array_equal(idx, nn_idx) and np.array_equal(d2.view(np.uint32), nn_d2.view(np.uint32)), (what, slot, key)
                exact = math.fsum(float(v) for v in nn_d2[np.isfinite(nn_d2)])  # (the bound of tests/test_gpu_overlap.py: the order of the f64 sum is free)
                assert abs(got["sum_d2"] - exact) <= 1e-12 * exact, (what, slot, key, got["sum_d2"], exact)
                assert 0 < got["inliers"] < got["n"], (what, slot, key)       # (both outcomes occur)
                out.append((got, d2.tobytes(), idx.tobytes()))
        return out

    try:
        first = step(small, "small")
        step(large, "large")
        assert step(small, "small again") == first
    finally:
        store.close()


def test_freespace_classes_regrown(ranged):
    w = ranged; store, p, S, L = w["store"], w["p"], w["small"], w["large"]
    im = {i: fs.range_images(c, p) for i, c in w["clouds"].items()}

    def step(q, c, what):
        T = [synth.sensor_pose(0.5, -0.2, 0.1 * (j + 1)) for j in range(len(q))]
        recs = store.freespace_batch(q, c, T)
        out = []
        for slot, (qi, ci, Ti, rec) in enumerate(zip(q, c, T, recs)):
            want = fs.freespace(w["clouds"][qi], w["clouds"][ci], Ti, p, points=True, q_images=im[qi], c_images=im[ci])
            assert rec["status"] == 0, (what, slot)
            for d, key in ((0, "q_in_c"), (1, "c_in_q")):
                got = {f: rec[key][f] for f in FIELDS}
                print(what, (qi, ci), key, got)
                assert got == {f: want[key][f] for f in FIELDS}, (what, qi, ci, key)
                cls = store.freespace_points(slot, d)
                assert cls.dtype == np.uint8 and np.array_equal(cls, want[key]["classes"]), (what, qi, ci, key)
                assert got["observed"] > 0 and got["n_finite"] == got["n"] - 1, (what, qi, ci, key)
                out.append((got, cls.tobytes()))
        return out

    first = step([S[0]], [S[1]], "small")
    big = step([L[0], L[2]], [L[1], L[0]], "large")
    assert all(sum(r[0][k] for r in big) > 0 for k in ("seen_through", "occluded", "agree"))      # (every class occurs)
    assert step([S[0]], [S[1]], "small again") == first


def test_static_votes_and_kept_records_regrown(ranged):
    w = ranged; store, p, S, L = w["store"], w["p"], w["small"], w["large"]
    im = {i: fs.range_images(c, p) for i, c in w["clouds"].items()}
    poses = _poses(3)

    def step(ids, what):
        wit = sm.window_witnesses(ids, 2)
        got = store.static_classify(ids, poses, witnesses=wit)
        want = sm.classify(w["clouds"], ids, poses, wit[0], wit[1], p, images=im)
        out = []
        for e, x in enumerate(want):
            st, ag, rm = store.static_points(e)
            assert np.array_equal(st, x["seen_through"]) and np.array_equal(ag, x["agree"]) and np.array_equal(rm, x["removed"].astype(np.uint8)), (what, e)
            assert int(got["removed"][e]) == int(x["removed"].sum()) and got["status"][e] == 0, (what, e)
            out.append((st.tobytes(), ag.tobytes(), rm.tobytes()))
        print(what, "removed per entry", got["removed"].tolist())
        # the kept records, through the map built of them: against build_map of the twin's kept records on a store of its own
        n = store.build_map_static(0.5)
        got_map = store.download_map(n).tobytes()
        twin_ids = [other.add(k[:, :3]) for k in sm.static_clouds(w["clouds"], ids, want)]
        n = other.build_map(twin_ids, poses, 0.5)
        assert other.download_map(n).tobytes() == got_map, what
        out.append(got_map)
        return out, want

    from qn_amd import engine
    other = engine.KeyframeStore()
    try:
        first, _ = step(S, "small")
        _, want = step(L, "large")
        assert sum(int(x["removed"].sum()) for x in want) > 0 and sum(int(x["agree"].sum()) for x in want) > 0      # (both votes occur)
        again, _ = step(S, "small again")
        assert again == first
    finally:
        other.close()


def test_verify_cloud_arena_regrown():
    from qn_amd import engine
    import test_gpu_sc_verify as scv
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    store = engine.KeyframeStore()
    ctx = engine.Context(60000)
    try:
        g = engine.NanoGICP(ctx)
        g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(scv.MAX_CORR); g.setTransformationEpsilon(0.01); g.bind()
        engine.Quatro(ctx)
        which = [2, 3, 12, 13]                                             # two places and their revisits: keyframes 0 .. 3 of this store
        ids = [int(i) for i in store.add_lidar_scans(prims, sen, [poses[k] for k in which], [100 + k for k in which])]
        assert store.quatro_describe(ctx, ids, 0.3) == [0] * 4

        def step(qs, cs, what):
            recs = store.verify_loop_pairs_c2f(ctx, qs, cs)
            out = []
            for j, r in enumerate(recs):
                assert r["status"] == 0 and r["valid"], (what, j, r)
                src = store.verify_cloud(j, engine.QN_VERIFY_SRC)
                T = r["T_quatro"]; x, y, z = (src[:, i].astype(np.float64) for i in range(3))
                coarse = np.stack([(((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]).astype(np.float32) for k in range(3)], 1)
                G = np.array(r["record"].T, np.float32).reshape(4, 4); cx, cy, cz = coarse[:, 0], coarse[:, 1], coarse[:, 2]
                final = np.stack([G[k, 0] * cx + (G[k, 1] * cy + (G[k, 2] * cz + G[k, 3])) for k in range(3)], 1)
                assert final.dtype == np.float32
                got_c, got_f = store.verify_cloud(j, engine.QN_VERIFY_COARSE), store.verify_cloud(j, engine.QN_VERIFY_FINAL)
                print(what, j, "n", len(src), "coarse moved", float(np.abs(coarse - src).max()), "final moved", float(np.abs(final - coarse).max()))
                assert len(src) > 1000 and np.array_equal(got_c.view(np.uint32), coarse.view(np.uint32)), (what, j)
                assert np.array_equal(got_f.view(np.uint32), final.view(np.uint32)), (what, j)
                # COARSE is still what it was after FINAL was computed beside it
                assert np.array_equal(store.verify_cloud(j, engine.QN_VERIFY_COARSE).view(np.uint32), coarse.view(np.uint32)), (what, j)
                out.append((np.asarray(T).tobytes(), G.tobytes(), got_c.tobytes(), got_f.tobytes()))
            return out

        first = step([2], [0], "one pair")
        step([2, 3], [0, 1], "two pairs")
        assert step([2], [0], "one pair again") == first
    finally:
        ctx.close(); store.close()
