"""The specification of the static map, qn_amd/staticmap.py, on a ray-cast stream with one moving box: 12 scans of a 32 x 900 spinning LiDAR driving past
120 m of static primitives, and a 4 x 2 x 1.5 m box that is somewhere else in every scan.  No GPU needed.

Conditions on the rule itself (not measurements of an implementation): with the +-W neighbours in the list as witnesses and the default rule (2, 1), at most
0.1 % of the static records may be removed and at least 60 % of the box's records must be.  The test prints the shares it finds."""
import numpy as np
import pytest
from qn_amd import freespace as fs, scancontext as sc, staticmap as sm, synth

S = 12
SEN = synth.SpinningLidar(n_beams=32, n_cols=900)


def box_at(s):
    return -20.0 + 3.5 * s, 6.0


@pytest.fixture(scope="module")
def stream():
    static = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    p = fs.Params.for_sensor(SEN)
    tabs = fs.tables(p)
    poses = [synth.sensor_pose(-8.0 + 1.5 * s, 0.3 * np.sin(0.5 * s), 0.05 * s) for s in range(S)]
    clouds, dyn = {}, {}
    for s in range(S):
        bx, by = box_at(s)
        box = np.array([(synth.PRIM_BOX, (bx, by, 4.0, 2.0, 1.5, 0.0))], dtype=synth.PRIM_DTYPE)
        c = synth.lidar_scan(np.concatenate([static, box]), SEN, poses[s], 100 + s)
        w = fs.transform(c, poses[s])
        clouds[s] = c
        dyn[s] = (np.abs(w[:, 0] - bx) < 2.15) & (np.abs(w[:, 1] - by) < 1.15) & (w[:, 2] < 1.65) & (w[:, 2] > 0.08)      # the box's records (not the ground under it)
    images = {s: fs.range_images(clouds[s], p, tabs) for s in range(S)}
    return dict(p=p, tabs=tabs, poses=poses, clouds=clouds, dyn=dyn, images=images, ids=list(range(S)))


def _classify(st, wit, rule=None):
    return sm.classify(st["clouds"], st["ids"], st["poses"], wit[0], wit[1], st["p"], rule, images=st["images"])


@pytest.fixture(scope="module")
def w2(stream):
    wit = sm.window_witnesses(stream["ids"], 2)
    return wit, _classify(stream, wit)


def test_static_records_stay_and_the_moving_box_goes(stream, w2):
    _, res = w2
    ns = rs = nd = rd = 0
    for s in range(S):
        d, r = stream["dyn"][s], res[s]["removed"]
        ns += int((~d).sum()); rs += int((r & ~d).sum()); nd += int(d.sum()); rd += int((r & d).sum())
    print("static removed %d of %d (%.4f %%), box removed %d of %d (%.1f %%)" % (rs, ns, 100.0 * rs / ns, rd, nd, 100.0 * rd / nd))
    assert nd > 1000 and ns > 200000
    assert rs <= 0.001 * ns                                         # (a)
    assert rd >= 0.6 * nd                                           # (b)


def test_no_witness_and_an_unreachable_threshold_remove_nothing(stream):
    none = (np.zeros(S + 1, np.uint32), np.zeros(0, np.uint32))
    for r in _classify(stream, none):                               # (c)
        assert not r["removed"].any() and not r["seen_through"].any() and not r["agree"].any()
    wit = sm.window_witnesses(stream["ids"][:5], 2)
    sub = dict(stream, ids=stream["ids"][:5], poses=stream["poses"][:5])
    loose = _classify(sub, wit, sm.StaticParams(1, 0))
    assert sum(int(r["removed"].sum()) for r in loose) > 0
    most = int(np.diff(wit[0]).max())
    for r in _classify(sub, wit, sm.StaticParams(most + 1, 0)):     # (d)
        assert not r["removed"].any()


def test_votes_equal_a_brute_force_loop_over_the_loop_check(stream, w2):
    (off, wit), res = w2
    for e in (0, 5, 11):                                            # (e)
        st = np.zeros(len(stream["clouds"][e]), np.int64); ag = np.zeros_like(st)
        for w in wit[off[e]:off[e + 1]]:
            M = sc.relative_pose(stream["poses"][w], stream["poses"][e])
            near, far = stream["images"][int(w)]
            cls = fs.direction(stream["clouds"][e], M, near, far, stream["p"], points=True, tabs=stream["tabs"])["classes"]
            st += cls == 2; ag += cls == 4
        assert res[e]["seen_through"].dtype == np.uint8 and res[e]["agree"].dtype == np.uint8
        assert np.array_equal(res[e]["seen_through"], st) and np.array_equal(res[e]["agree"], ag)
        assert np.array_equal(res[e]["removed"], (st >= 2) & (st > ag))
    kept = sm.static_clouds(stream["clouds"], stream["ids"], res)
    assert all(np.array_equal(k, stream["clouds"][e][~res[e]["removed"]]) for e, k in enumerate(kept))


def test_the_rule_is_integers_only():
    st = np.array([0, 1, 2, 2, 3, 255, 255, 2], np.uint8); ag = np.array([0, 0, 0, 2, 2, 254, 255, 1], np.uint8)
    assert sm.removed(st, ag).tolist() == [False, False, True, False, True, True, False, True]
    assert sm.removed(st, ag, sm.StaticParams(1, 0)).tolist() == [False, True, True, True, True, True, True, True]
    assert sm.removed(st, ag, sm.StaticParams(3, 2)).tolist() == [False, False, False, False, False, False, False, False]
    assert sm.removed(st, ag, sm.StaticParams(2, 0xFFFFFFFF)).tolist() == [False, False, True, False, False, False, False, False]
    for bad in (sm.StaticParams(0, 1), sm.StaticParams(1, -1), sm.StaticParams(1 << 32, 1)):
        with pytest.raises(ValueError):
            sm.removed(st, ag, bad)


def test_a_non_finite_record_is_never_removed(stream):
    c = stream["clouds"][5].copy()
    c[10, 0] = np.nan; c[11, 2] = np.inf; c[12, :3] = -np.inf
    clouds = dict(stream["clouds"]); clouds[5] = c
    wit = sm.window_witnesses(stream["ids"], 1)
    r = sm.classify(clouds, stream["ids"], stream["poses"], wit[0], wit[1], stream["p"], sm.StaticParams(1, 0), images=stream["images"])[5]
    assert not r["removed"][10:13].any() and not r["seen_through"][10:13].any() and not r["agree"][10:13].any()


def test_witnesses_against_a_plain_sort():
    rng = np.random.default_rng(3)                                  # (f)
    n = 40
    ids = rng.integers(0, 25, n)
    poses = np.tile(np.eye(4), (n, 1, 1)); poses[:, :3, 3] = rng.integers(-3, 4, (n, 3)) * 1.5      # a lattice: many exact ties
    for radius, k in ((4.0, 5), (2.0, 255), (100.0, 3), (0.0, 4), (3.0, 0)):
        off, wit = sm.witnesses(ids, poses, radius, k)
        assert off.dtype == np.uint32 and wit.dtype == np.uint32 and off[0] == 0 and len(off) == n + 1 and off[-1] == len(wit)
        for e in range(n):
            d = poses[:, :3, 3] - poses[e, :3, 3]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            want = sorted((float(d2[w]), w) for w in range(n) if ids[w] != ids[e] and d2[w] <= radius * radius)[:k]
            assert wit[off[e]:off[e + 1]].tolist() == [w for _, w in want], (radius, k, e)
    with pytest.raises(ValueError):
        sm.witnesses(ids, poses, 1.0, 256)
    with pytest.raises(ValueError):
        sm.witnesses(ids, poses[:-1], 1.0, 2)
    off, wit = sm.window_witnesses([4, 5, 4, 6], 1)
    assert off.tolist() == [0, 1, 3, 5, 6] and wit.tolist() == [1, 0, 2, 1, 3, 2]
    for bad in (([0, 1, 1, 2, 3], [1, 0, 3]), ([0, 1, 2, 3], [1, 0, 3]), ([0, 2, 1, 3, 3], [1, 0, 3]), ([0, 1, 2, 3, 3], [1, 0, 4]), ([0, 1, 2, 3, 3], [2, 0, 3])):
        with pytest.raises(ValueError):
            sm.check_witnesses([4, 5, 4, 6], *bad)
    with pytest.raises(ValueError):
        sm.check_witnesses([1, 2], [0, 256, 256], [1] * 256)
