"""Range images and the free-space (see-through) check on the GPU (qn_kf_range_* / qn_kf_freespace_*) against their specification, the numpy twin
qn_amd/freespace.py.  Bit for bit: near and far of every keyframe, every count of both directions, every point's class byte; a pair alone against the same
pair inside a batch of 16, and two runs of one call.

The scenario at the end shows what the figure is for, on the street scene of tests/test_gpu_sc_verify.py: the revisit (12, 2) verified by verify_loop_pairs
from its true Scan Context heading, and the same pair from that heading plus 180 degrees, each transform then checked against the raw scans' range images
(32 x 720, window 1 x 1, 0.3 m + 2 %).  Share of the observed points seen through (12 in 2, 2 in 12):
not recorded yet - the test prints them (true / wrong: fraction q in c, fraction c in q, valid, score, observed points).
Only the ordering is asserted."""
import math
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import freespace as fs, scancontext as sc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SEN = synth.SpinningLidar(n_beams=32, n_cols=720)
FIELDS = ("n", "n_finite", "in_fov", "observed", "seen_through", "occluded", "agree")


def _added_clouds():
    rng = np.random.default_rng(9)
    a = rng.normal(0, 15, (30000, 3)).astype(np.float32); a[:, 2] *= 0.15
    a[5] = [np.nan, 1, 1]; a[77] = [3, np.inf, 0]; a[1234] = [1, 2, -np.inf]; a[20000] = [0, 0, 0]; a[20001] = [0, 0, 5]; a[20002] = [4, 0, 0]; a[20003] = [-4, 0, 0]
    gated = rng.normal(0, 0.4, (500, 3)).astype(np.float32)                         # everything inside min_range: empty after the gates
    gated[3] = [np.nan, np.nan, np.nan]; gated[4] = [0.5, 0.5, 30.0]                # (and one far above the field of view)
    dense = rng.normal(0, 8, (120000, 3)).astype(np.float32); dense[:, 2] *= 0.1    # many points per pixel: the atomics' min / max at work
    return [a, gated, np.zeros((0, 3), np.float32), dense]


@pytest.fixture(scope="module")
def world():
    from qn_amd import engine
    import test_gpu_sc_verify as scv
    prims, poses = scv._street()
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, SEN, poses, np.arange(len(poses)) + 100)]
    added = _added_clouds()
    ids += [store.add(c) for c in added]
    clouds = {i: store.keyframe(i) for i in ids}
    params = engine.RangeParams.for_sensor(SEN)
    store.range_set_params(params)
    status = store.range_describe(ids)
    yield dict(store=store, ids=ids, clouds=clouds, poses=poses, params=params, status=status, n_street=len(poses), prims=prims)
    store.close()


def _images_equal(got, want, what):
    for g, w, name in zip(got, want, ("near", "far")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


def test_images_equal_the_twin(world):
    from qn_amd import engine
    store, p = world["store"], world["params"].twin()
    ns = world["n_street"]
    assert world["status"] == [0] * ns + [0, engine.QN_ERR_EMPTY_CLOUD, engine.QN_ERR_EMPTY_CLOUD, 0]
    for i in world["ids"]:
        want = fs.range_images(world["clouds"][i], p)
        _images_equal(store.range_images(i), want, i)
        if i < ns:
            assert np.isfinite(want[0]).sum() > 5000
    gated = store.range_images(world["ids"][ns + 1])
    assert np.isinf(gated[0]).all() and (gated[1] == 0).all()
    # describing again (a subset, an id twice) replaces with the same bits and leaves the others alone
    assert store.range_describe([3, ns, 3]) == [0, 0, 0]
    for i in (3, ns, 4):
        _images_equal(store.range_images(i), fs.range_images(world["clouds"][i], p), i)


def _check(world, recs, q, c, T, p, what):
    """every count and every class of a call against the twin"""
    store = world["store"]
    im = {}
    for slot, (qi, ci, Ti, rec) in enumerate(zip(q, c, T, recs)):
        for k in (qi, ci):
            if k not in im:
                im[k] = fs.range_images(world["clouds"][k], p)
        want = fs.freespace(world["clouds"][qi], world["clouds"][ci], Ti, p, points=True, q_images=im[qi], c_images=im[ci])
        for d, key in ((0, "q_in_c"), (1, "c_in_q")):
            got = rec[key]
            print(what, (qi, ci), key, {f: got[f] for f in FIELDS}, "see-through %.4f" % fs.see_through_fraction(got))
            assert {f: got[f] for f in FIELDS} == {f: want[key][f] for f in FIELDS}, (what, qi, ci, key)
            cls = store.freespace_points(slot, d)
            assert cls.dtype == np.uint8 and np.array_equal(cls, want[key]["classes"]), (what, qi, ci, key, int((cls != want[key]["classes"]).sum()))
            assert got["seen_through"] + got["occluded"] + got["agree"] == got["observed"] <= got["in_fov"] <= got["n_finite"] <= got["n"]


def _true(poses, q, c):
    return np.linalg.inv(poses[c]) @ poses[q]


def _rz(a):
    T = np.eye(4); T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    return T


def _pairs(world):
    """revisits at their true pose (0.4 m apart), neighbours 12 m and more apart at theirs, the identity, a 180 degree wrong transform, a shifted one, and pairs with the added clouds"""
    poses, ns = world["poses"], world["n_street"]
    A, G, E, D = world["ids"][ns:ns + 4]
    q = [12, 13, 10, 4, 12, 12, 11, A, 3, G, E, D]
    c = [2, 3, 5, 7, 2, 2, 1, 3, A, 2, 5, 2]
    T = [_true(poses, 12, 2), _true(poses, 13, 3), _true(poses, 10, 5), _true(poses, 4, 7), np.eye(4), _rz(math.pi) @ _true(poses, 12, 2),
         synth.sensor_pose(2.0, -3.0, 0.2, 0.1) @ _true(poses, 11, 1), np.eye(4), synth.sensor_pose(1.0, 0.0, 1.0, 0.0), np.eye(4), np.eye(4), _rz(0.3)]
    return q, c, T


def test_batch_equals_the_twin(world):
    from qn_amd import engine
    store = world["store"]
    q, c, T = _pairs(world)
    recs = store.freespace_batch(q, c, T)
    assert [r["status"] for r in recs] == [0] * 10 + [engine.QN_ERR_EMPTY_CLOUD, 0]
    _check(world, recs, q, c, T, world["params"].twin(), "32x720")
    # a true revisit is hardly seen through, the same pair turned by 180 degrees is
    assert fs.see_through_fraction(recs[0]["q_in_c"]) < 0.01 and fs.see_through_fraction(recs[5]["q_in_c"]) > fs.see_through_fraction(recs[0]["q_in_c"])
    assert recs[0]["q_in_c"]["observed"] > 10000
    # a scan against itself through the identity: nothing seen through, nothing occluded (the pair (q, q) is refused, so through a second copy)
    copy = store.add(world["clouds"][12][:, :3])
    world["clouds"][copy] = store.keyframe(copy)
    assert store.range_describe([copy]) == [0]
    r, = store.freespace_batch([12], [copy], [np.eye(4)])
    for key in ("q_in_c", "c_in_q"):
        assert r[key]["seen_through"] == 0 and r[key]["occluded"] == 0 and r[key]["agree"] == r[key]["observed"] == r[key]["in_fov"] > 20000


@pytest.mark.parametrize("kw", [dict(window_rows=2, window_cols=3), dict(window_rows=0, window_cols=0), dict(tol_abs=0.05, tol_rel=0.0), dict(tol_abs=1.0, tol_rel=0.1)])
def test_another_window_and_another_tolerance(world, kw):
    from qn_amd import engine
    store = world["store"]
    p = engine.RangeParams.for_sensor(SEN, **kw)
    store.range_set_params(p)                                   # the images do not depend on these: they stay
    try:
        _images_equal(store.range_images(12), fs.range_images(world["clouds"][12], world["params"].twin()), 12)
        q, c, T = _pairs(world)
        sel = [0, 2, 5, 6, 8]
        q, c, T = [q[i] for i in sel], [c[i] for i in sel], [T[i] for i in sel]
        _check(world, store.freespace_batch(q, c, T), q, c, T, p.twin(), str(kw))
    finally:
        store.range_set_params(world["params"])


@pytest.mark.parametrize("shape", [(128, 8192, 1, 2), (1, 1, 0, 0), (64, 1800, 1, 1), (1024, 37, 3, 1)])
def test_other_image_shapes_on_a_store_of_their_own(world, shape):
    """8192 columns: the column table is read from global memory rather than staged in LDS; 1 x 1: the degenerate image"""
    from qn_amd import engine
    nr, nc, wr, wc = shape
    p = engine.RangeParams(n_rows=nr, n_cols=nc, el_lo=math.radians(-16.0), el_hi=math.radians(15.0), min_range=1.0, window_rows=wr, window_cols=wc)
    store = engine.KeyframeStore()
    try:
        ns = world["n_street"]
        src = [12, 2, world["ids"][ns], world["ids"][ns + 3]]
        ids = [store.add(world["clouds"][i][:, :3]) for i in src]
        w = dict(store=store, clouds={k: store.keyframe(k) for k in ids})
        store.range_set_params(p)
        got = store.range_params()
        assert (got.n_rows, got.n_cols, got.window_rows, got.window_cols, got.el_lo, got.tol_abs) == (nr, nc, wr, wc, p.el_lo, 0.3)
        assert store.range_describe(ids) == [0] * 4
        for k in ids:
            _images_equal(store.range_images(k), fs.range_images(w["clouds"][k], p.twin()), (shape, k))
        q, c, T = [0, 2, 3], [1, 3, 0], [_true(world["poses"], 12, 2), np.eye(4), _rz(1.0)]
        _check(w, store.freespace_batch(q, c, T), q, c, T, p.twin(), str(shape))
    finally:
        store.close()


def test_a_pair_alone_in_a_batch_and_again(world):
    store = world["store"]
    q, c, T = _pairs(world)
    strip = lambda recs: [(r["q_in_c"], r["c_in_q"], r["status"]) for r in recs]
    one = strip(store.freespace_batch(q, c, T))
    assert strip(store.freespace_batch(q, c, T)) == one
    alone = [strip(store.freespace_batch([q[j]], [c[j]], [T[j]]))[0] for j in range(len(q))]
    assert alone == one
    order = [3, 1, 0, 2, 5, 0, 6, 3, 0, 8, 11, 2, 1, 7, 9, 5]                  # a batch of 16
    big = strip(store.freespace_batch([q[i] for i in order], [c[i] for i in order], [T[i] for i in order]))
    assert big == [one[i] for i in order]
    pts = [store.freespace_points(8, d) for d in (0, 1)]                      # pair 0 at slot 8 of the batch
    store.freespace_batch([q[0]], [c[0]], [T[0]])
    for d in (0, 1):
        assert np.array_equal(pts[d], store.freespace_points(0, d))


def test_refused_calls_change_nothing(world):
    from qn_amd import engine
    store, ns = world["store"], world["n_street"]
    q, c, T = _pairs(world)
    store.freespace_batch(q[:3], c[:3], T[:3])
    before_pts = [store.freespace_points(s, d) for s in range(3) for d in (0, 1)]
    before_img = [store.range_images(i) for i in (2, 12, world["ids"][ns])]
    late = store.add(world["clouds"][2][:, :3])                            # a keyframe without images
    bad_T = np.eye(4); bad_T[1, 3] = np.nan
    inf_T = np.eye(4); inf_T[0, 0] = np.inf
    for args in (([], [], np.zeros((0, 4, 4))), ([12], [12], [np.eye(4)]), ([12], [-1], [np.eye(4)]), ([late + 1], [2], [np.eye(4)]), ([12], [late], [np.eye(4)]),
                 ([late], [2], [np.eye(4)]), ([12], [2], [bad_T]), ([12, 13], [2, 3], [np.eye(4), inf_T])):
        with pytest.raises(engine.EngineError) as e:
            store.freespace_batch(*args)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, args
    n = 32768
    with pytest.raises(engine.EngineError) as e:
        store.freespace_batch(np.full(n, 12), np.full(n, 2), np.tile(np.eye(4), (n, 1, 1)))
    assert e.value.status == engine.QN_ERR_CAPACITY
    with pytest.raises(engine.EngineError) as e:
        store.range_images(late)
    assert e.value.status == engine.QN_ERR_NOT_READY
    for bad in ([], [-1], [late + 1]):
        with pytest.raises(engine.EngineError) as e:
            store.range_describe(bad)
        assert e.value.status == engine.QN_ERR_INVALID_ARG
    for kw in (dict(el_lo=0.3, el_hi=0.2), dict(el_lo=-1.6), dict(el_hi=1.6), dict(n_rows=0), dict(n_cols=0), dict(n_rows=1025), dict(n_cols=8193), dict(tol_abs=-0.1),
               dict(tol_rel=float("nan")), dict(tol_abs=float("inf")), dict(min_range=-1.0), dict(window_rows=64), dict(n_cols=6, window_cols=3), dict(el_lo=float("nan"))):
        with pytest.raises(engine.EngineError) as e:
            store.range_set_params(**kw)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, kw
    got = store.range_params()
    assert (got.n_rows, got.n_cols, got.el_lo, got.el_hi) == (32, 720, world["params"].el_lo, world["params"].el_hi)
    store._freespace_n = [(len(world["clouds"][a]), len(world["clouds"][b])) for a, b in zip(q[:3], c[:3])]      # (the wrapper's own bookkeeping of the refused calls)
    for x, y in zip(before_pts, [store.freespace_points(s, d) for s in range(3) for d in (0, 1)]):
        assert np.array_equal(x, y)
    for x, i in zip(before_img, (2, 12, world["ids"][ns])):
        _images_equal(store.range_images(i), x, i)
    l = engine.lib()
    out = np.zeros(8, np.uint8)
    import ctypes as C
    assert l.qn_kf_freespace_points(store.h, C.c_uint32(3), C.c_int(0), out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_freespace_points(store.h, C.c_uint32(0), C.c_int(2), out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG


def test_points_before_any_call_are_not_ready_and_new_parameters_discard_the_images(world):
    from qn_amd import engine
    store = engine.KeyframeStore()
    try:
        a = store.add(world["clouds"][12][:, :3]); b = store.add(world["clouds"][2][:, :3])
        store._freespace_n = [(1, 1)]
        with pytest.raises(engine.EngineError) as e:
            store.freespace_points(0, 0)
        assert e.value.status == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as e:
            store.range_images(a)
        assert e.value.status == engine.QN_ERR_NOT_READY
        p = engine.RangeParams.for_sensor(SEN)
        store.range_set_params(p)
        assert store.range_describe([a, b]) == [0, 0]
        T = _true(world["poses"], 12, 2)
        first, = store.freespace_batch([a], [b], [T])
        store.range_set_params(engine.RangeParams.for_sensor(SEN, tol_abs=0.2))          # not the images' business
        store.range_images(a)
        for kw in (dict(min_range=3.0), dict(n_rows=31), dict(el_hi=p.el_hi + 0.01)):
            q = engine.RangeParams.for_sensor(SEN)
            for k, v in kw.items():
                setattr(q, k, v)
            store.range_set_params(q)
            for k in (a, b):
                with pytest.raises(engine.EngineError) as e:
                    store.range_images(k)
                assert e.value.status == engine.QN_ERR_NOT_READY, kw
            with pytest.raises(engine.EngineError) as e:
                store.freespace_batch([a], [b], [T])
            assert e.value.status == engine.QN_ERR_INVALID_ARG
            assert store.range_describe([a, b]) == [0, 0]
            _images_equal(store.range_images(a), fs.range_images(world["clouds"][12][:, :3], q.twin()), kw)
        store.range_set_params(p)
        assert store.range_describe([b, a]) == [0, 0]
        again, = store.freespace_batch([a], [b], [T])
        assert again == first
    finally:
        store.close()


def test_an_accepted_transform_is_seen_through_less_than_a_wrong_one(world):
    """revisit (12, 2) by verify_loop_pairs: its Scan Context heading against that heading turned by 180 degrees (figures: module docstring)"""
    from qn_amd import engine
    import test_gpu_submap_verify as sv
    store = world["store"]
    pp = sv._perturbed(world["poses"])
    ctx = sv._ctx(engine, lanes=2)
    try:
        y = sv._yaw(world["poses"], 12, 2)
        figs = {}
        for name, yaw in (("true", y), ("wrong", y + math.pi)):
            r, = store.verify_loop_pairs(ctx, [12], [2], [yaw], pp, sv.RANGE, sv.LEAF, sv.THR)
            T = np.array(r["record"].T64).reshape(4, 4)
            f, = store.freespace_batch([12], [2], [T])
            figs[name] = (fs.see_through_fraction(f["q_in_c"]), fs.see_through_fraction(f["c_in_q"]), r["valid"], r["score"], f["q_in_c"]["observed"], f["c_in_q"]["observed"])
            print(name, figs[name])
            _check(world, [f], [12], [2], [T], world["params"].twin(), name)
        assert figs["true"][2]
        assert figs["true"][0] < figs["wrong"][0] and figs["true"][1] < figs["wrong"][1]
    finally:
        ctx.close()


def test_the_three_kernels_have_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_range_bin", "k_freespace_check", "k_freespace_reduce"):
        rows = [l for l in out.splitlines() if re.search(r"\b%s\b" % k, l)]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows
