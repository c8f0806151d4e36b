"""The two-way overlap on the GPU (qn_kf_overlap_batch / qn_kf_verify_overlap / qn_kf_overlap_points) against its specification, the numpy twin
qn_amd/overlap.py.  Bit for bit: both directions' n, n_finite and inliers, every point's nn_d2 and nn_idx; sum_d2 between two runs of a call and between a
pair alone and inside a batch of 16.  sum_d2 against math.fsum of the twin's nn_d2: 1e-12 relative, a bound on an f64 sum of at most 1e5 non-negative terms
in any order (each addition errs by at most 2^-53 of the running sum, which never exceeds the total: n 2^-53 < 1.2e-11 worst case, ~sqrt(n) 2^-53 typically),
not a measurement.

The scenario at the end shows what the figures are for, on the street scene of tests/test_gpu_sc_verify.py, submap against submap as
tests/test_gpu_submap_verify.py sets it up: the revisit (12, 2) registered from its true Scan Context heading, and the same pair from that heading plus 180
degrees.  Checked on the CPU oracle and the twin first (22124 against 26400 points, radius 0.6): true seed converged, score 0.0468, overlaps 0.9949 (aligned
source -> target) and 0.9010 (target -> source), inlier RMSE 0.194 / 0.212 m; wrong seed not converged, score 54.56, overlaps 0.3522 / 0.3138, inlier RMSE
0.298 / 0.303 m.  (At radius 0.3: 0.8522 / 0.7442 against 0.2289 / 0.1984.  The pair (13, 3) orders the same way: 0.9982 / 0.7968 against 0.5404 / 0.4277.)
Only the ordering is asserted."""
import math
import os
import sys
import numpy as np
import pytest
from qn_amd import overlap as ov, scancontext as sc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RADII = (0.15, 0.3, 0.6, 2.0)


def _dev(xyz):
    """(n, 3) -> a float4 device tensor (w = 1), kept alive by the caller"""
    import torch
    a = np.ones((len(xyz), 4), np.float32); a[:, :3] = np.asarray(xyz, np.float32)[:, :3]
    return torch.from_numpy(a).cuda()


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _pairs_arg(dev):
    return [(a.data_ptr() if len(a) else 0, len(a), b.data_ptr() if len(b) else 0, len(b)) for a, b in dev]


def _twin_unbounded(a, b):
    return ov.nearest_unbounded(a, b, block=128), ov.nearest_unbounded(b, a, block=128)


def _check_pair(store, slot, rec, a, b, unb, r, what):
    """one pair's record and per-point results against the twin (unb = _twin_unbounded(a, b), so that one brute-force pass serves every radius)"""
    assert rec["status"] == 0, what
    for d, key, x, u in ((0, "a_to_b", a, unb[0]), (1, "b_to_a", b, unb[1])):
        nn_d2, nn_idx = ov.apply_radius(u[0], u[1], r)
        want = ov.record(x, nn_d2)
        got = rec[key]
        d2, idx = store.overlap_points(slot, d)
        print(what, key, "r", r, "n", got["n"], "finite", got["n_finite"], "inliers", got["inliers"], "want", want["inliers"], "sum", got["sum_d2"],
              "fsum", math.fsum(float(v) for v in nn_d2[np.isfinite(nn_d2)]))
        assert (got["n"], got["n_finite"], got["inliers"]) == (want["n"], want["n_finite"], want["inliers"]), (what, key, r)
        assert np.array_equal(idx, nn_idx), (what, key, r, int((idx != nn_idx).sum()))
        assert np.array_equal(d2.view(np.uint32), nn_d2.view(np.uint32)), (what, key, r)
        exact = math.fsum(float(v) for v in nn_d2[np.isfinite(nn_d2)])
        assert abs(got["sum_d2"] - exact) <= 1e-12 * exact, (what, key, r, got["sum_d2"], exact)


def _uniform_pair(seed, na, nb, extent):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-extent, extent, (na, 3)).astype(np.float32); a[:, 2] *= 0.2
    b = rng.uniform(-extent, extent, (nb, 3)).astype(np.float32); b[:, 2] *= 0.2
    m = min(na, nb) // 2
    b[:m] = a[:m] + rng.normal(0, 0.2, (m, 3)).astype(np.float32)      # half of B lies near A
    return a, b


@pytest.fixture(scope="module")
def clouds():
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    out = [("uniform-a", *_uniform_pair(1, 9000, 12000, 30.0)), ("uniform-b", *_uniform_pair(2, 20000, 7000, 60.0))]
    for pid, sep in ((3, 5.0), (4, 12.0)):
        s, t, T = synth.make_lidar_pair(pid, separation=sep, sensor=sen)
        s64 = s.astype(np.float64)
        aligned = (s64 @ T[:3, :3].T + T[:3, 3]).astype(np.float32)       # the source brought onto the target: a revisit from `sep` metres away
        assert 5000 < len(s) < 40000 and 5000 < len(t) < 40000, (len(s), len(t))
        out.append(("lidar-%d" % pid, aligned, t))
    out[0][1][17] = np.nan; out[0][2][5] = [0, np.inf, 0]                 # non-finite points on both sides of one pair
    return [(name, a, b, _twin_unbounded(a, b)) for name, a, b in out]


@pytest.mark.parametrize("r", RADII)
def test_batch_equals_the_twin(store, clouds, r):
    dev = [(_dev(a), _dev(b)) for _, a, b, _ in clouds]
    recs = store.overlap_batch(_pairs_arg(dev), r)
    for slot, ((name, a, b, unb), rec) in enumerate(zip(clouds, recs)):
        _check_pair(store, slot, rec, a, b, unb, r, name)
    assert recs[0]["a_to_b"]["n_finite"] == len(clouds[0][1]) - 1 and recs[0]["b_to_a"]["n_finite"] == len(clouds[0][2]) - 1
    if r >= 0.6:
        assert all(rec["a_to_b"]["inliers"] > 1000 and rec["b_to_a"]["inliers"] > 1000 for rec in recs)


def test_sums_are_reproducible_and_do_not_depend_on_the_batch(store, clouds):
    dev = [(_dev(a), _dev(b)) for _, a, b, _ in clouds]
    args = _pairs_arg(dev)
    strip = lambda recs: [(x["a_to_b"], x["b_to_a"], x["status"]) for x in recs]
    one = strip(store.overlap_batch(args, 0.6))
    assert strip(store.overlap_batch(args, 0.6)) == one
    alone = [strip(store.overlap_batch([p], 0.6))[0] for p in args]
    assert alone == one
    order = [3, 1, 0, 2, 2, 0, 1, 3, 0, 0, 3, 2, 1, 1, 2, 3]                # a batch of 16
    big = strip(store.overlap_batch([args[i] for i in order], 0.6))
    assert big == [one[i] for i in order]
    pts = store.overlap_points(7, 1)
    store.overlap_batch([args[3]], 0.6)
    ref = store.overlap_points(0, 1)
    assert np.array_equal(pts[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(pts[1], ref[1])


def _run_one(store, a, b, r, what):
    da, db = _dev(a), _dev(b)
    rec, = store.overlap_batch(_pairs_arg([(da, db)]), r)
    _check_pair(store, 0, rec, a, b, _twin_unbounded(a, b), r, what)
    return rec


def test_cell_borders(store):
    # an integer lattice with spacing exactly r: every point has partners at distance exactly r across cell borders (and at 0: its own copy, in the second run)
    r = 0.5
    g = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-8, 9), np.arange(-3, 4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(r)
    shifted = g + np.array([r, 0, 0], np.float32)
    rec = _run_one(store, g, shifted, r, "lattice")
    assert rec["a_to_b"]["inliers"] == len(g) and rec["b_to_a"]["inliers"] == len(g)
    odd = g[(np.abs(np.round(g / r)).sum(1) % 2) == 1]; even = g[(np.abs(np.round(g / r)).sum(1) % 2) == 0]      # every partner at exactly r
    rec = _run_one(store, odd, even, r, "checkerboard")
    assert rec["a_to_b"]["inliers"] == len(odd) and rec["a_to_b"]["sum_d2"] == len(odd) * r * r
    for way in (np.float32(np.inf), np.float32(-np.inf)):                  # one cloud moved by one ulp, either way
        _run_one(store, odd, np.nextafter(even, way), r, "checkerboard ulp %s" % way)
        _run_one(store, np.nextafter(odd, way), even, r, "checkerboard ulp' %s" % way)
    # the same at a radius that is no dyadic number, and on a lattice whose spacing is that radius in f32
    r = 0.3
    h = np.stack(np.meshgrid(np.arange(-20, 21), np.arange(-20, 21), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(r)
    par = (np.abs(np.stack(np.meshgrid(np.arange(-20, 21), np.arange(-20, 21), np.arange(-2, 3), indexing="ij"), -1).reshape(-1, 3)).sum(1) % 2)
    _run_one(store, h[par == 1], h[par == 0], r, "lattice 0.3")
    _run_one(store, h[par == 1], np.nextafter(h[par == 0], np.float32(np.inf)), r, "lattice 0.3 ulp")


def test_far_from_the_origin_disjoint_boxes_one_point_and_a_wide_extent(store):
    # 76 km from the origin: an f32 ulp is 7.8 mm there, the cell coordinates are in the hundreds of thousands
    rng = np.random.default_rng(5)
    a = rng.uniform(-20, 20, (6000, 3)).astype(np.float32)
    b = (a[:4000] + rng.normal(0, 0.1, (4000, 3))).astype(np.float32)
    off = np.array([76000.0, -76000.0, 300.0], np.float32)
    for r in (0.15, 0.3):
        rec = _run_one(store, a + off, b + off, r, "76 km")
        assert rec["b_to_a"]["inliers"] > 1000
    # two clouds whose boxes do not intersect
    rec = _run_one(store, a, a + np.array([500.0, 0, 0], np.float32), 2.0, "disjoint")
    assert rec["a_to_b"]["inliers"] == 0 and rec["b_to_a"]["inliers"] == 0 and rec["a_to_b"]["sum_d2"] == 0.0
    # one point against 1e5
    big = rng.uniform(-50, 50, (100000, 3)).astype(np.float32)
    rec = _run_one(store, big[777:778] + np.float32(0.01), big, 0.3, "one point")
    assert rec["a_to_b"]["inliers"] == 1 and rec["b_to_a"]["inliers"] >= 1
    # 200 m x 200 m x 30 m at r = 0.15: 1334 x 1334 x 201 cells of edge r need 29 key bits, so the edge is widened until 26 suffice
    w = rng.uniform(0, 1, (30000, 3)).astype(np.float32) * np.array([200, 200, 30], np.float32) - np.array([100, 100, 15], np.float32)
    w[0] = [-100, -100, -15]; w[1] = [100, 100, 15]
    v = w.copy(); v[:15000] += rng.normal(0, 0.08, (15000, 3)).astype(np.float32)
    assert (200 / 0.15) ** 2 * (30 / 0.15) > 2 ** 26
    rec = _run_one(store, w, v[::-1].copy(), 0.15, "wide")
    assert rec["a_to_b"]["inliers"] > 15000


def test_empty_sides_and_refused_arguments_change_nothing(store, clouds):
    from qn_amd import engine
    _, a, b, _ = clouds[0]
    da, db = _dev(a), _dev(b)
    none = _dev(np.zeros((0, 3), np.float32))
    recs = store.overlap_batch(_pairs_arg([(da, db), (none, db), (da, none), (da, db)]), 0.3)
    zero = dict(n=0, n_finite=0, inliers=0, sum_d2=0.0)
    assert [x["status"] for x in recs] == [0, engine.QN_ERR_EMPTY_CLOUD, engine.QN_ERR_EMPTY_CLOUD, 0]
    assert recs[1]["a_to_b"] == zero and recs[1]["b_to_a"] == zero and recs[2]["a_to_b"] == zero and recs[2]["b_to_a"] == zero
    assert (recs[0]["a_to_b"], recs[0]["b_to_a"]) == (recs[3]["a_to_b"], recs[3]["b_to_a"]) and recs[0]["a_to_b"]["inliers"] > 0
    with pytest.raises(engine.EngineError) as e:
        store._overlap_n[1] = (1, 1); store.overlap_points(1, 0)
    assert e.value.status == engine.QN_ERR_NOT_READY
    before = [store.overlap_points(0, d) for d in (0, 1)] + [store.overlap_points(3, d) for d in (0, 1)]
    host = np.ones((64, 4), np.float32)
    good = _pairs_arg([(da, db)])[0]
    for pairs, r in (([], 0.3), ([good], 0.0), ([good], -0.3), ([good], float("nan")), ([good], float("inf")),
                     ([(0, 5, good[2], good[3])], 0.3),                                  # a null cloud with points
                     ([(good[0] + 4, 5, good[2], good[3])], 0.3),                        # records not 16-byte aligned
                     ([(host.ctypes.data, 64, good[2], good[3])], 0.3)):                 # a host pointer
        with pytest.raises(engine.EngineError) as e:
            store.overlap_batch(pairs, r)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, (pairs, r)
    store._overlap_n = [(len(a), len(b)), (0, 0), (0, 0), (len(a), len(b))]                  # (the wrapper's own bookkeeping of the refused calls)
    after = [store.overlap_points(0, d) for d in (0, 1)] + [store.overlap_points(3, d) for d in (0, 1)]
    for x, y in zip(before, after):
        assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1], y[1])
    for slot, d in ((4, 0), (0, 2)):
        with pytest.raises((engine.EngineError, ValueError)):
            store.overlap_points(slot, d)


# ------------------------------------------------------------------ the pairs of a verify call
@pytest.fixture(scope="module")
def street():
    from qn_amd import engine
    import test_gpu_submap_verify as sv
    import test_gpu_sc_verify as scv
    prims, poses = scv._street()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    st = engine.KeyframeStore()
    ids = [int(i) for i in st.add_lidar_scans(prims, sen, poses, np.arange(len(poses)) + 100)]
    empty = st.add(np.zeros((0, 3), np.float32))
    pp = sv._perturbed(poses)
    ctx = sv._ctx(engine, lanes=4)
    assert st.submap_describe(ctx, ids, pp, sv.RANGE, sv.LEAF) == [0] * len(ids)
    assert st.submap_describe(ctx, [empty], pp + [np.eye(4)], 0, sv.LEAF) == [engine.QN_ERR_EMPTY_CLOUD]
    assert st.quatro_describe(ctx, ids + [empty], sv.LEAF)[:len(ids)] == [0] * len(ids)
    yield dict(store=st, ctx=ctx, poses=poses, pp=pp, ids=ids, empty=empty, sv=sv)
    ctx.close(); st.close()


def _verify(st, kind, q, c, yaws):
    store, ctx, sv = st["store"], st["ctx"], st["sv"]
    if kind == "gicp":
        return store.verify_loop_pairs(ctx, q, c, yaws, st["pp"] + [np.eye(4)], sv.RANGE, sv.LEAF, sv.THR)
    if kind == "c2f":
        return store.verify_loop_pairs_c2f(ctx, q, c, sv.THR)
    if kind == "submap":
        return store.verify_loop_pairs_submap(ctx, q, c, yaws, sv.THR)
    return store.verify_loop_pairs_submap_c2f(ctx, q, c, sv.THR)


@pytest.mark.parametrize("kind", ["gicp", "c2f", "submap", "submap_c2f"])
def test_verify_overlap_equals_the_batch_on_the_pairs_clouds(street, kind):
    from qn_amd import engine
    st = street; store, sv = st["store"], st["sv"]
    q, c = [12, st["empty"], 13, 10], [2, 3, 3, 5]
    yaws = [0.0 if st["empty"] in p else sv._yaw(st["poses"], *p) for p in zip(q, c)]
    out = _verify(st, kind, q, c, yaws)
    assert out[1]["status"] == engine.QN_ERR_EMPTY_CLOUD and [o["status"] for o in out[:1] + out[2:]] == [0, 0, 0]
    key = lambda o: (o["status"], o["valid"], o["score"], o["iterations"], o["T"].tobytes())
    live = [0, 2, 3]
    cl = {j: (store.verify_cloud(j, engine.QN_VERIFY_FINAL), store.verify_cloud(j, engine.QN_VERIFY_DST), store.verify_cloud(j, engine.QN_VERIFY_SRC)) for j in live}
    R = 0.6
    recs = store.verify_overlap(R, n_pairs=4)
    assert recs[1]["status"] == engine.QN_ERR_NOT_READY and recs[1]["a_to_b"] == dict(n=0, n_finite=0, inliers=0, sum_d2=0.0) and recs[1]["b_to_a"] == recs[1]["a_to_b"]
    pts = {j: [store.overlap_points(j, d) for d in (0, 1)] for j in live}
    # the verify record serves the same clouds afterwards
    for j in live:
        for which, before in zip((engine.QN_VERIFY_FINAL, engine.QN_VERIFY_DST, engine.QN_VERIFY_SRC), cl[j]):
            assert np.array_equal(store.verify_cloud(j, which).view(np.uint32), before.view(np.uint32)), (kind, j, which)
    with pytest.raises(engine.EngineError) as e:
        store.verify_cloud(1, engine.QN_VERIFY_FINAL)
    assert e.value.status == engine.QN_ERR_NOT_READY
    # another order, a subset
    perm = store.verify_overlap(R, pairs=[3, 0, 1, 2])
    assert [(x["a_to_b"], x["b_to_a"], x["status"]) for x in perm] == [(recs[j]["a_to_b"], recs[j]["b_to_a"], recs[j]["status"]) for j in (3, 0, 1, 2)]
    sub = store.verify_overlap(R, pairs=[2])
    assert (sub[0]["a_to_b"], sub[0]["b_to_a"]) == (recs[2]["a_to_b"], recs[2]["b_to_a"])
    for bad in ([4], [0, 0], []):
        with pytest.raises(engine.EngineError) as e:
            store.verify_overlap(R, pairs=bad)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, bad
    with pytest.raises(engine.EngineError) as e:
        store.verify_overlap(R, n_pairs=3)
    assert e.value.status == engine.QN_ERR_INVALID_ARG
    # the batch call on the downloaded clouds
    dev = [(_dev(cl[j][0]), _dev(cl[j][1])) for j in live]
    want = store.overlap_batch(_pairs_arg(dev), R)
    for k, j in enumerate(live):
        print(kind, (q[j], c[j]), "valid", out[j]["valid"], "score", out[j]["score"], "overlap", ov.overlap_fraction(recs[j]["a_to_b"]), ov.overlap_fraction(recs[j]["b_to_a"]),
              "rmse", ov.inlier_rmse(recs[j]["a_to_b"]), ov.inlier_rmse(recs[j]["b_to_a"]))
        assert (recs[j]["a_to_b"], recs[j]["b_to_a"], recs[j]["status"]) == (want[k]["a_to_b"], want[k]["b_to_a"], 0), (kind, j)
        assert recs[j]["a_to_b"]["n"] == len(cl[j][0]) and recs[j]["b_to_a"]["n"] == len(cl[j][1])
        for d in (0, 1):
            w = store.overlap_points(k, d)
            assert np.array_equal(w[0].view(np.uint32), pts[j][d][0].view(np.uint32)) and np.array_equal(w[1], pts[j][d][1])
    # and the verify call itself gives the records it gave
    again = _verify(st, kind, q, c, yaws)
    assert [key(o) for o in again] == [key(o) for o in out]


def test_verify_overlap_without_a_record_is_not_ready():
    from qn_amd import engine
    s = engine.KeyframeStore()
    with pytest.raises(engine.EngineError) as e:
        s.verify_overlap(0.3, n_pairs=1)
    assert e.value.status == engine.QN_ERR_NOT_READY
    with pytest.raises(engine.EngineError) as e:
        s._overlap_n = [(1, 1)]; s.overlap_points(0, 0)
    assert e.value.status == engine.QN_ERR_NOT_READY
    s.close()


def test_a_true_alignment_overlaps_more_than_a_wrong_one(street):
    """revisit (12, 2), submap against submap: its Scan Context heading against that heading turned by 180 degrees (figures of the CPU run: module docstring)"""
    st = street; store, sv = st["store"], st["sv"]
    y = sv._yaw(st["poses"], 12, 2)
    figs = {}
    for name, yaw in (("true", y), ("wrong", y + math.pi)):
        r, = _verify(st, "submap", [12], [2], [yaw])
        o, = store.verify_overlap(0.6, n_pairs=1)
        figs[name] = (ov.overlap_fraction(o["a_to_b"]), ov.overlap_fraction(o["b_to_a"]), ov.inlier_rmse(o["a_to_b"]), ov.inlier_rmse(o["b_to_a"]), r["valid"], r["score"])
        print(name, figs[name])
    assert figs["true"][4]
    assert figs["true"][0] > figs["wrong"][0] and figs["true"][1] > figs["wrong"][1]
