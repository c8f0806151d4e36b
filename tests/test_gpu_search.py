"""The building blocks of the cooperative neighbour search (csrc/qn_device.cuh) called directly through qn_debug_search on the clouds and queries of
tests/search_cases.py, against the references of tests/search_checks.py: Best1 with and without UNIQUE and its finish<1 | 2 | 4> lane for lane; BestK<16 | 20 |
24 | 32> with its lazy queue and finish<4>, wave_search<4, BestK<KMAX>> and lane_ball_knn<KMAX> against the brute-force list; tile_box_d2,
cap_of, cap_extent, cap_face_dist, cell_coord and cell_key bit for bit, and tile_box_d2 against the device's own grid; divmod_small against / and %; what
stream_box delivers in row mode, tile mode and tile mode pruned by a ball; what build_clusters with stream_clusters<1 | 4> hands every lane, first walk and
REUSE walk; for_each_in_ball_cells, _group<8> and _group_pre<8 | 16> (csrc/qn_ball_walk.cuh) position for position; wave_search<4, Best1>, wave_search_single and wave_search_far16 against the brute
force, and the bound min(sqrt(second), d_unseen) they return against the exact distance to every other point.  The maxima and counts are printed."""
import ctypes as C
import numpy as np
import pytest
import search_cases as sc
import search_checks as chk

pytestmark = pytest.mark.gpu
F = np.float32
INF_BITS = 0x7f800000
BOUND = 1.0 + 4.0 * chk.U24          # what the comment above track_bound_holds grants the stored bound over the exact distance


@pytest.fixture(scope="module")
def dev():
    """one context per cloud with the cloud as its target (grid 1) under the cloud's `cell`, and the grid as the device built it"""
    from qn_amd import engine
    made = {}

    def get(name):
        if name not in made:
            c = engine.Context(4096)
            c.debug_set("cell", sc.CELLS[name])
            engine.NanoGICP(c).setInputTarget(sc.cloud(name))
            g = sc.grid(name)
            w = c.debug_search(c.DS_DUMP, 1, [], g.n, g.ncells, g.ncells + 1 + 4 * g.n)
            cs = w[:g.ncells + 1].astype(np.int64); p = w[g.ncells + 1:].reshape(-1, 4)
            made[name] = (c, cs, chk.fbits(p[:, :3]), p[:, 3].astype(np.int64))
        return made[name]
    yield get
    for c, *_ in made.values():
        c.close()


def recs8(q, r, w4, w5=0):
    a = np.zeros((len(q), 8), dtype=np.uint32)
    a[:, :3] = chk.bits(q); a[:, 3] = chk.bits(r); a[:, 4] = w4; a[:, 5] = w5
    return a


def keys_of(out):
    return out[:, 0].astype(np.uint64) | (out[:, 1].astype(np.uint64) << np.uint64(32))


def check_bound(label, truth, key, second_bits, du_bits):
    """min(sqrt(second), d_unseen) <= D (1 + 4 u), D the exact distance to the nearest point other than the key's (no key: the nearest at all)"""
    idx = np.where(key == np.uint64(chk.INF_KEY), -1, (key & np.uint64(0xffffffff)).astype(np.int64))
    D = chk.distance_to_the_others(truth, idx)
    bound = np.minimum(np.sqrt(chk.fbits(second_bits)), chk.fbits(du_bits)).astype(np.float64)
    assert not np.isnan(bound).any(), label
    pos = D > 0
    ratio = float((bound[pos] / D[pos]).max()) if pos.any() else 0.0
    finite = int(np.isfinite(bound).sum())
    print("%s: max bound / D = %.9f over %d queries (%d finite bounds, %d with D = 0)" % (label, ratio, len(D), finite, int((~pos).sum())))
    bad = np.flatnonzero(bound > D * BOUND)
    assert len(bad) == 0, (label, len(bad), bad[:8], bound[bad[:8]], D[bad[:8]])
    return ratio


# ------------------------------------------------------------------ the grid itself
@pytest.mark.parametrize("name", sc.CLOUDS)
def test_grid_numbers_and_placement_equal_the_restatement(dev, name):
    c, cs, p, idx = dev(name)
    g = sc.grid(name); info = c.grid_info(1)
    assert (info["origin"] == g.o.astype(np.float64)).all() and info["cell"] == float(g.cell) and tuple(info["dims"]) == tuple(g.dims) and info["eps"] == float(g.eps)
    assert cs[0] == 0 and cs[-1] == g.n and (np.diff(cs) >= 0).all()
    assert sorted(idx) == list(range(g.n)) and (chk.bits(p) == chk.bits(sc.cloud(name)[idx])).all()
    key_dev = np.searchsorted(cs, np.arange(g.n), side="right") - 1
    assert (key_dev == g.cell_key(g.cells(p))).all()


# ------------------------------------------------------------------ sinks
@pytest.mark.parametrize("unique", (False, True))
def test_best1_every_lane_equals_the_restatement(dev, unique):
    c = dev("lattice")[0]
    lanes_checked = 0
    for L in (0, 1, 5, 17):
        rec, fin = sc.best1_waves(200 + L, L)
        if unique and L != 5:
            rec = sc.make_unique(rec)                                 # (L = 5 keeps its repeated indices: UNIQUE then counts the repeat as another point)
        W = rec.shape[0]
        lanes = [[chk.best1_serial([(bool(r[0]), chk.f1(r[1]), int(r[2])) for r in rec[w, :, l]], unique) for l in range(64)] for w in range(W)]
        words = np.concatenate([rec.reshape(W, -1), fin], axis=1)
        for S in (1, 2, 4):
            out = c.debug_search(c.DS_BEST1, 1, words, W, S | (int(unique) << 8) | (L << 16), 256 * W).reshape(W, 64, 4)
            for w in range(W):
                want = chk.best1_finish(lanes[w], S, fin[w] != 0)
                wk = np.array([k for k, _, _ in want], dtype=np.uint64)
                assert (keys_of(out[w]) == wk).all(), (L, S, w, np.flatnonzero(keys_of(out[w]) != wk)[:8])
                assert (out[w, :, 2] == chk.bits(np.array([s for _, s, _ in want], dtype=np.float32))).all(), (L, S, w, "second")
                assert (out[w, :, 3] == chk.bits(np.array([b for _, _, b in want], dtype=np.float32))).all(), (L, S, w, "bd")
                lanes_checked += 64
    print("Best1 UNIQUE %s: %d lanes equal" % (unique, lanes_checked))


@pytest.mark.parametrize("kmax", sc.KMAXES)
def test_bestk_every_lane_equals_the_restatement(dev, kmax):
    c = dev("lattice")[0]
    lanes = 0
    for L in (0, 1, 15, 16, 17, 33):
        rec, fin = sc.bestk_waves(400 + L, L)
        words = np.concatenate([rec.reshape(3, -1), fin], axis=1)
        for k in sc.ks_of(kmax):
            for S in ((4, 1) if L == 17 else (4,)):
                out = c.debug_search(c.DS_BESTK, 1, words, 3, kmax | (k << 8) | (S << 14) | (L << 17), 3 * 64 * (2 * k + 4)).reshape(3, 64, 2 * k + 4)
                for w in range(3):
                    want = chk.bestk_wave_serial(sc.bestk_steps(rec[w]), k, S, fin[w] != 0)
                    got = out[w, :, 0:2 * k:2].astype(np.uint64) | (out[w, :, 1:2 * k:2].astype(np.uint64) << np.uint64(32))
                    assert (got == np.array([e for e, _, _ in want], dtype=np.uint64)).all(), (L, k, S, w)
                    assert (keys_of(out[w, :, 2 * k:]) == np.array([x for _, x, _ in want], dtype=np.uint64)).all(), (L, k, S, w, "w")
                    assert (out[w, :, 2 * k + 2] == np.array([f for _, _, f in want])).all(), (L, k, S, w, "found")
                    lanes += 64
    print("BestK<%d>: %d lanes equal" % (kmax, lanes))


def klist(out, k):
    return out[:, 0:2 * k:2].astype(np.uint64) | (out[:, 1:2 * k:2].astype(np.uint64) << np.uint64(32))


@pytest.mark.parametrize("name", sc.CLOUDS)
@pytest.mark.parametrize("kmax", sc.KMAXES)
def test_wave_search_knn_certifies_the_brute_force_list(dev, name, kmax):
    c = dev(name)[0]; q = sc.queries(name); want = sc.truth_k(name); g = sc.grid(name)
    for k in sc.ks_of(kmax):
        r = sc.first_radii(name, 6 + k)
        kth = np.sqrt(chk.fbits((want[:, k - 1] >> np.uint64(32)).astype(np.uint32)).astype(np.float64))
        capf = np.where(np.arange(len(q)) % 2 == 0, np.inf, kth * 1.01 + 4 * float(g.eps)).astype(np.float32)      # half under a proven cap on the k-th distance
        r = np.minimum(r, capf)
        rec = recs8(q, r, chk.bits(capf), 1)
        out = c.debug_search(c.DS_WAVE_SEARCH_K, 1, rec, len(q), 64 | (kmax << 8) | (k << 16), (2 * k + 4) * len(q)).reshape(-1, 2 * k + 4)
        assert (out[:, 2 * k + 1] == 1).all() and (out[:, 2 * k + 3] == k).all(), (k, "uncertified")
        assert (klist(out, k) == want[:, :k]).all(), (k, np.flatnonzero((klist(out, k) != want[:, :k]).any(axis=1))[:8])
        assert (chk.fbits(out[:, 2 * k + 2]) <= capf).all(), (k, "r past r_cap")
        for rounds in (1, 2):
            cut = c.debug_search(c.DS_WAVE_SEARCH_K, 1, rec, len(q), rounds | (kmax << 8) | (k << 16), (2 * k + 4) * len(q)).reshape(-1, 2 * k + 4)
            cert = cut[:, 2 * k + 1] == 1
            if rounds == 1:
                assert (~cert).sum() >= 1, (k, cert.sum())            # (the 0.3-cell first radii cannot hold a point with room to spare)
            assert (klist(cut[cert], k) == want[cert, :k]).all(), (k, rounds)
            assert (chk.fbits(cut[:, 2 * k + 2]) <= capf).all(), (k, rounds, "r past r_cap")
    print("wave_search<4, BestK<%d>> %s: %d queries, k in %s, 64, 1 and 2 rounds" % (kmax, name, len(q), sc.ks_of(kmax)))


@pytest.mark.parametrize("name", sc.CLOUDS)
@pytest.mark.parametrize("kmax", sc.KMAXES)
def test_lane_ball_knn_finds_the_brute_force_list(dev, name, kmax):
    c = dev(name)[0]; q = sc.queries(name); want = sc.truth_k(name)
    for k in sc.ks_of(kmax):
        r = sc.first_radii(name, 8 + k)
        out = c.debug_search(c.DS_LANE_BALL_KNN, 1, recs8(q, r, 0), len(q), kmax | (k << 8), (2 * k + 4) * len(q)).reshape(-1, 2 * k + 4)
        assert (out[:, 2 * k] == k).all()
        assert (klist(out, k) == want[:, :k]).all(), (k, np.flatnonzero((klist(out, k) != want[:, :k]).any(axis=1))[:8])


# ------------------------------------------------------------------ bounds
def bounds_call(c, t, q, r, f):
    a = np.zeros((len(q), 8), dtype=np.uint32)
    a[:, :3] = t; a[:, 3:6] = chk.bits(q); a[:, 6] = chk.bits(r); a[:, 7] = chk.bits(f)
    out = [c.debug_search(c.DS_BOUNDS, 1, a[i:i + 65536], len(a[i:i + 65536]), 0, 16 * len(a[i:i + 65536])).reshape(-1, 16) for i in range(0, len(a), 65536)]
    return np.concatenate(out)


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_bounds_equal_the_f32_restatement_bit_for_bit(dev, name):
    c = dev(name)[0]; g = sc.grid(name)
    q = np.concatenate([sc.queries(name), sc.cloud(name)[:600]])
    rng = np.random.default_rng(7)
    t = np.stack([rng.integers(0, int(n), len(q)) for n in g.tdims], axis=1)
    own = g.tile_of(g.cells(q)); t[::3] = own[::3]
    o2, S = g.cap_of(q)
    near = np.sqrt(S) * rng.choice(np.array([1.0, 1.000001, 1.01, 2.0], dtype=np.float32), len(q))
    r = np.where(rng.uniform(size=len(q)) < 0.5, near + F(0.01), rng.uniform(0.05, 30, len(q))).astype(np.float32)
    f = rng.uniform(0, 40, len(q)).astype(np.float32)
    out = bounds_call(c, t, q, r, f)
    differ = {"tile_box_d2": int((out[:, 0] != chk.bits(g.tile_box_d2(t, q))).sum()), "cap_of": int((out[:, 1:4] != chk.bits(o2)).sum() + (out[:, 4] != chk.bits(S)).sum())}
    for a in range(3):
        differ["cap_extent %d" % a] = int((out[:, 5 + a] != chk.bits(g.cap_extent(o2, S, r, a))).sum())
        differ["cap_face_dist %d" % a] = int((out[:, 8 + a] != chk.bits(g.cap_face_dist(o2, S, f, a))).sum())
    cells = g.cells(q)
    differ["cell_coord"] = int((out[:, 11:14].astype(np.int64) != cells).sum())
    differ["cell_key"] = int((out[:, 14].astype(np.int64) != g.cell_key(cells)).sum())
    assert not any(differ.values()), {k: v for k, v in differ.items() if v}      # (every function named, so that a failure says which one broke)
    print("%s: %d records, 15 words each, equal" % (name, len(q)))


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_tile_box_d2_is_below_every_point_the_device_put_in_the_tile(dev, name):
    c, cs, p, idx = dev(name); g = sc.grid(name)
    q = np.concatenate([sc.queries(name), sc.cloud(name)[::4]])
    nt = int(np.prod(g.tdims))
    tl = np.arange(nt)
    t3 = np.stack([tl % g.tdims[0], (tl // g.tdims[0]) % g.tdims[1], tl // (g.tdims[0] * g.tdims[1])], axis=1)
    tb = chk.fbits(bounds_call(c, np.repeat(t3, len(q), axis=0), np.tile(q, (nt, 1)), np.ones(nt * len(q), dtype=np.float32), np.ones(nt * len(q), dtype=np.float32))[:, 0]).reshape(nt, len(q))
    d2 = chk.sqdist32(q, p)                                           # (Q, sorted points)
    pairs = 0
    for t in range(nt):
        a, b = cs[t * 128], cs[(t + 1) * 128]
        if b > a:
            assert (tb[t] <= d2[:, a:b].min(axis=1)).all(), (name, t)
            pairs += len(q)
    print("%s: tile_box_d2 <= the nearest point of the tile for %d (query, occupied tile) pairs" % (name, pairs))


def test_divmod_small_equals_division_on_the_whole_sweep(dev):
    c = dev("lattice")[0]
    out = c.debug_search(c.DS_DIVMOD, 1, [], 0, 0, 6).view(np.uint64)
    d = np.arange(1, 1 << 22, dtype=np.int64)
    top = ((1 << 22) - 1) // d * d
    expect = 128 * (1 << 22) + 5 * len(d) + int((top + 1 < (1 << 22)).sum()) + int((top - 1 >= 0).sum())
    print("divmod_small: %d mismatches in %d pairs" % (int(out[0]), int(out[1])))
    assert int(out[1]) == expect
    assert int(out[0]) == 0 and int(out[2]) == (1 << 64) - 1, (int(out[0]), int(out[2]) >> 22, int(out[2]) & ((1 << 22) - 1))


# ------------------------------------------------------------------ stream_box
def stream_call(c, boxes, mode, centre=None, r2=None, cap=4096):
    a = np.zeros((len(boxes), 12), dtype=np.uint32)
    a[:, :6] = np.array(boxes); a[:, 6] = mode
    if centre is not None:
        a[:, 7:10] = chk.bits(centre); a[:, 10] = chk.bits(r2)
    out = c.debug_search(c.DS_STREAM_BOX, 1, a, len(a), cap, (4 + cap) * len(a)).reshape(len(a), 4 + cap)
    assert (out[:, 1] == 0).all(), "overflow"
    assert (out[:, 0] == out[:, 2]).all(), "the stream's return value is the number it delivered"
    return [row[4:4 + row[0]].astype(np.int64) for row in out]


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_stream_box_rows_deliver_every_point_of_the_box_once(dev, name):
    c = dev(name)[0]; g = sc.grid(name); pts = sc.cloud(name)
    got = stream_call(c, sc.boxes(name), 0)
    total = 0
    for box, d in zip(sc.boxes(name), got):
        bp = chk.box_points(g, pts, box)
        assert len(np.unique(d)) == len(d), (box, "a point twice")
        assert len(d) == len(bp) and (np.sort(d) == bp).all(), box
        total += len(d)
    assert (np.sort(got[0]) == np.arange(g.n)).all()                  # the whole grid
    print("%s: %d boxes, %d candidates" % (name, len(got), total))


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_stream_box_tiles_deliver_the_box_once_and_never_drop_a_point_of_the_ball(dev, name):
    c = dev(name)[0]; g = sc.grid(name); pts = sc.cloud(name)
    wide = [chk.widen(g, b) for b in sc.boxes(name)]
    for box, d in zip(wide, stream_call(c, wide, 1)):
        assert len(np.unique(d)) == len(d) and sorted(d) == list(chk.box_points(g, pts, box)), box
    rng = np.random.default_rng(9)
    q = sc.queries(name)[rng.choice(len(sc.queries(name)), len(wide))]
    dropped = 0
    for rr in (0.4, 1.5, 6.0):
        r2 = np.full(len(wide), F(rr * sc.CELLS[name]) ** 2, dtype=np.float32)
        for box, d, qq, r2_ in zip(wide, stream_call(c, wide, 2, q, r2), q, r2):
            inbox = chk.box_points(g, pts, box)
            assert len(np.unique(d)) == len(d) and np.isin(d, inbox).all(), (box, "outside the widened box, or twice")
            ball = inbox[chk.sqdist32(qq[None], pts[inbox])[0] <= r2_]
            assert np.isin(ball, d).all(), (box, qq, rr, "a point of the ball was not delivered")
            dropped += len(inbox) - len(d)
    assert dropped > 0                                                # the pruning pruned
    print("%s: %d boxes x 3 radii, %d candidates pruned, none of them in its ball" % (name, len(wide), dropped))


@pytest.mark.parametrize("name", sc.CLOUDS)
@pytest.mark.parametrize("S", (1, 4))
def test_stream_clusters_deliver_each_box_once_and_the_reuse_walk_repeats_the_first(dev, name, S):
    c = dev(name)[0]; g = sc.grid(name); pts = sc.cloud(name)
    Q, R, T = sc.cluster_waves(name, S)
    W = len(Q); cap = 4096
    a = np.zeros((W, 64, 8), dtype=np.uint32)
    a[:, :, :3] = chk.bits(Q); a[:, :, 3] = chk.bits(R); a[:, :, 4] = T
    stride = 8 + 64 * (4 + 2 * cap)
    out = c.debug_search(c.DS_STREAM_CLUSTERS, 1, a, W, cap | (S << 24), W * stride).reshape(W, stride)
    reused = walked = tiled = delivered = 0
    for w in range(W):
        hdr = out[w, :8]; lanes = out[w, 8:].reshape(64, 4 + 2 * cap)
        cid, cl = chk.clusters_restated(g, Q[w], R[w], T[w], S)
        assert hdr[4] == 0, "overflow"
        assert hdr[0] == len(cl) and (lanes[:, 0].astype(np.int32) == cid).all(), (w, "clusters")
        assert (lanes[T[w], 1] == np.array([cl[i][1] for i in cid[T[w]]])).all(), (w, "tile mode")
        want = [chk.box_points(g, pts, box) for box, _ in cl]
        assert hdr[2] == hdr[3] == sum(len(v) for v in want), (w, "stream length")
        assert (lanes[~T[w], 2:4] == 0).all(), (w, "a lane that is not open accepted a candidate")
        assert (lanes[:, 2] == lanes[:, 3]).all() and (lanes[:, 4:4 + cap] == lanes[:, 4 + cap:]).all(), (w, "the REUSE walk differs from the first")
        for l in np.flatnonzero(T[w][:64 // S]):                      # a query's S sub-slots together: every point of its cluster's box, each once
            got = np.concatenate([lanes[l + s * (64 // S), 4:4 + lanes[l + s * (64 // S), 2]] for s in range(S)]).astype(np.int64)
            assert len(got) == len(want[cid[l]]) and (np.sort(got) == want[cid[l]]).all(), (w, l)
            delivered += len(got)
        reused += hdr[1] <= 64; walked += hdr[1] > 64; tiled += any(t for _, t in cl)
    assert reused >= 1 and (walked >= 1 or name == "lattice"), (reused, walked)      # both forms of the second walk are run (the lattice's whole grid is 30 segments)
    if name == "slabs":
        assert tiled >= 1
    print("stream_clusters<%d> %s: %d waves (%d reuse their table, %d in tile mode), %d candidates accepted" % (S, name, W, reused, tiled, delivered))


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_ball_walks_deliver_the_restated_sequences_and_group_pre_equals_group(dev, name):
    c, cs, p, idx = dev(name); g = sc.grid(name)
    q, r, on = sc.ball_queries(name)
    cap = 2048
    a = recs8(q, r, on.astype(np.uint32))

    def run(variant, fg):
        lanes = (len(q) * fg + 63) // 64 * 64
        o = c.debug_search(c.DS_BALL_CELLS, 1, a, len(q), cap | (variant << 24), lanes * (2 + cap)).reshape(lanes, 2 + cap)
        assert (o[:, 1] == 0).all(), "overflow"
        return [[o[i * fg + gl, 2:2 + o[i * fg + gl, 0]].tolist() for gl in range(fg)] for i in range(len(q))]
    one, grp, pre8, pre16 = run(0, 1), run(1, 8), run(2, 8), run(3, 16)
    small = big = 0
    for i in range(len(q)):
        if not on[i]:
            assert one[i] == [[]] and grp[i] == [[]] * 8 and pre8[i] == [[]] * 8 and pre16[i] == [[]] * 16, (i, "a query that is not on saw a point")
            continue
        w1, nseg = chk.ball_walk_restated(g, cs, q[i], r[i], 1)
        assert one[i] == w1, (i, "for_each_in_ball_cells")
        box = chk.ball_box(g, q[i], r[i])
        assert sorted(idx[one[i][0]]) == list(chk.box_points(g, sc.cloud(name), box)), (i, "not the points of the box, each once")
        assert grp[i] == chk.ball_walk_restated(g, cs, q[i], r[i], 8)[0], (i, "_group<8>")
        assert pre8[i] == grp[i], (i, nseg, "_group_pre<8> differs from _group<8>")
        assert pre16[i] == chk.ball_walk_restated(g, cs, q[i], r[i], 16)[0], (i, nseg, "_group_pre<16>")
        small += nseg <= 80; big += nseg > 80
    assert small >= 10 and (big >= 10 or name == "lattice"), (small, big)      # the table and the fallback past QN_SEG_CAP (the lattice's grid, 8 x 6 x 5 cells, has no box of 80 segments)
    print("ball walks %s: %d boxes of <= 80 segments, %d of more, %d queries not on" % (name, small, big, int((~on).sum())))


# ------------------------------------------------------------------ searches
@pytest.mark.parametrize("name", sc.CLOUDS)
def test_wave_search_certifies_the_brute_force_neighbour(dev, name):
    c = dev(name)[0]; q = sc.queries(name); truth = sc.truth(name); g = sc.grid(name)
    r = sc.first_radii(name, 3)
    cap = np.full(len(q), INF_BITS, dtype=np.uint32)
    seeded = np.arange(len(q)) % 3 == 0                               # a proven cap: comfortably above the neighbour's distance
    cap[seeded] = chk.bits((truth[2][seeded] * 1.01 + 4 * float(g.eps)).astype(np.float32))
    r = np.where(seeded, np.minimum(r, chk.fbits(cap)), r).astype(np.float32)
    out = c.debug_search(c.DS_WAVE_SEARCH1, 1, recs8(q, r, cap, 1), len(q), 64, 8 * len(q)).reshape(-1, 8)
    assert (out[:, 4] == 1).all(), ("uncertified", np.flatnonzero(out[:, 4] != 1)[:8])
    assert (keys_of(out) == truth[0]).all(), np.flatnonzero(keys_of(out) != truth[0])[:8]
    check_bound("wave_search<4, Best1> %s, 64 rounds" % name, truth, keys_of(out), out[:, 2], out[:, 3])


@pytest.mark.parametrize("name", sc.CLOUDS)
@pytest.mark.parametrize("rounds", (1, 2))
def test_wave_search_cut_short_is_exact_where_certified_and_bounded_everywhere(dev, name, rounds):
    c = dev(name)[0]; q = sc.queries(name); truth = sc.truth(name); g = sc.grid(name)
    r = sc.first_radii(name, 4)
    capf = np.where(np.arange(len(q)) % 2 == 0, np.inf, truth[2] * 1.01 + 4 * float(g.eps)).astype(np.float32)
    r = np.minimum(r, capf)
    active = (np.arange(len(q)) % 7 != 3).astype(np.uint32)           # idle lanes beside working ones
    out = c.debug_search(c.DS_WAVE_SEARCH1, 1, recs8(q, r, chk.bits(capf), active), len(q), rounds, 8 * len(q)).reshape(-1, 8)
    on = active != 0
    assert (out[~on, 4] == 0).all() and (keys_of(out[~on]) == np.uint64(chk.INF_KEY)).all()
    cert = on & (out[:, 4] == 1)
    # both paths are run: one round leaves the small first radii uncertified in every cloud; two rounds certify whatever found a point in the first (the second
    # uses that point's distance), so only the slabs' gap queries - an empty box twice - stay open
    assert cert.sum() > 100, cert.sum()
    if rounds == 1 or name == "slabs":
        assert (on & ~cert).sum() >= 1
    assert (keys_of(out[cert]) == truth[0][cert]).all()
    assert (chk.fbits(out[on, 5]) <= capf[on]).all()
    sub = tuple(t[on] for t in truth)
    check_bound("wave_search<4, Best1> %s, %d round(s), %d of %d certified" % (name, rounds, cert.sum(), on.sum()), sub, keys_of(out[on]), out[on, 2], out[on, 3])


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_wave_search_single_finds_the_brute_force_neighbour(dev, name):
    c = dev(name)[0]; q = sc.queries(name); truth = sc.truth(name); g = sc.grid(name)
    r = sc.first_radii(name, 5)
    capf = np.where(np.arange(len(q)) % 3 != 0, np.inf, truth[2] * 1.01 + 4 * float(g.eps)).astype(np.float32)      # a third under a proven cap, as k_nn_search's seeded entries
    r = np.minimum(r, capf)
    out = c.debug_search(c.DS_WAVE_SEARCH_SINGLE, 1, recs8(q, r, chk.bits(capf)), len(q), 0, 8 * len(q)).reshape(-1, 8)
    assert (keys_of(out) == truth[0]).all(), np.flatnonzero(keys_of(out) != truth[0])[:8]
    assert (out[:, 4] >= 1).all() and (out[:, 4] <= 160).all(), "a search ran into its round limit"
    capped = np.isfinite(capf)
    assert (chk.fbits(out[capped, 7]) <= np.maximum(capf[capped], r[capped])).all(), "the last radius went past the cap"
    check_bound("wave_search_single %s" % name, truth, keys_of(out), out[:, 2], out[:, 3])
    far = truth[2] > 6 * sc.CELLS[name]
    shells = far & (out[:, 4] >= 2) & (out[:, 6] > 128)               # more than one round, more segments than a row-mode round may have: tile rounds that carried on
    print("wave_search_single %s: rounds 1..%d, %d of the %d queries with a neighbour beyond 6 cells took two or more rounds over more than 128 segments" % (name, out[:, 4].max(), shells.sum(), far.sum()))
    if name == "slabs":
        assert shells.sum() >= 20


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_wave_search_far16_finds_every_members_neighbour(dev, name):
    c = dev(name)[0]
    slots, rad, mem, truth = sc.far16_waves(name)
    out = c.debug_search(c.DS_WAVE_SEARCH_FAR16, 1, recs8(slots, rad, mem.astype(np.uint32)), len(slots), 0, 8 * len(slots)).reshape(-1, 8)
    assert (out[:, 4] == mem).all()
    assert (keys_of(out[~mem]) == np.uint64(chk.INF_KEY)).all()       # a slot that is no member is left alone
    assert (keys_of(out[mem]) == truth[0][mem]).all(), np.flatnonzero(mem)[keys_of(out[mem]) != truth[0][mem]][:8]
    per_m = np.repeat(mem.reshape(-1, 16).sum(axis=1), 16)
    assert sorted(set(per_m)) == sorted(sc.FAR_M)
    sub = tuple(t[mem] for t in truth)
    check_bound("wave_search_far16 %s, %d members in %d waves" % (name, mem.sum(), len(mem) // 16), sub, keys_of(out[mem]), out[mem, 2], out[mem, 3])


# ------------------------------------------------------------------ refusals
def test_bad_records_are_refused_before_any_launch(dev):
    from qn_amd import engine
    c = dev("seams")[0]; g = sc.grid("seams")
    L = engine.lib()
    L.qn_debug_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    out = np.full(4096, 7, dtype=np.uint32)

    def call(which, grid, a, n, arg):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        return L.qn_debug_search(c.h, which, grid, a.ctypes.data_as(C.c_void_p), n, arg, out.ctypes.data_as(C.c_void_p))
    q = np.array([[1, 2, 3]], dtype=np.float32)
    ok = recs8(q, F(1), INF_BITS, 1)
    bad = []
    for col, word in ((0, 0x7fc00000), (1, INF_BITS), (2, 0xff800000), (3, 0), (3, 0x7fc00000), (3, chk.b1(-1.0)), (3, INF_BITS), (4, 0x7fc00000), (4, 0)):
        a = ok.copy(); a[0, col] = word; bad.append(a)
    for a in bad:
        assert call(c.DS_WAVE_SEARCH1, 1, a, 1, 64) == engine.QN_ERR_INVALID_ARG
    for a in bad[:7]:
        assert call(c.DS_WAVE_SEARCH_SINGLE, 1, a, 1, 0) == engine.QN_ERR_INVALID_ARG
        assert call(c.DS_WAVE_SEARCH_FAR16, 1, np.repeat(a, 16, axis=0), 16, 0) == engine.QN_ERR_INVALID_ARG
    for rounds in (0, 65):
        assert call(c.DS_WAVE_SEARCH1, 1, ok, 1, rounds) == engine.QN_ERR_INVALID_ARG
    assert call(c.DS_WAVE_SEARCH_FAR16, 1, np.repeat(ok, 8, axis=0), 8, 0) == engine.QN_ERR_INVALID_ARG          # not whole waves
    assert call(c.DS_WAVE_SEARCH1, 1, ok, 0, 64) == engine.QN_ERR_INVALID_ARG and call(c.DS_WAVE_SEARCH1, 1, ok, (1 << 16) + 1, 64) == engine.QN_ERR_INVALID_ARG
    assert call(c.DS_WAVE_SEARCH1, 2, ok, 1, 64) == engine.QN_ERR_INVALID_ARG and call(8, 1, ok, 1, 64) == engine.QN_ERR_INVALID_ARG
    assert call(c.DS_WAVE_SEARCH1, 0, ok, 1, 64) == engine.QN_ERR_NOT_READY                                       # no source cloud was set
    nx, ny, nz = (int(v) for v in g.dims)
    for box, mode in (((0, nx, 0, 0, 0, 0), 0), ((3, 2, 0, 0, 0, 0), 0), ((0, 0, 0, ny, 0, 0), 0), ((0, 0, 0, 0, 0, nz), 0), ((1, 7, 0, 3, 0, 3), 1), ((0, 6, 0, 3, 0, 3), 1), ((0, 7, 0, 3, 0, 3), 3)):
        a = np.zeros((1, 12), dtype=np.uint32); a[0, :6] = box; a[0, 6] = mode
        assert call(c.DS_STREAM_BOX, 1, a, 1, 64) == engine.QN_ERR_INVALID_ARG, box
    a = np.zeros((1, 12), dtype=np.uint32); a[0, :6] = (0, 7, 0, 3, 0, 3)
    assert call(c.DS_STREAM_BOX, 1, a, 1, 0) == engine.QN_ERR_INVALID_ARG and call(c.DS_STREAM_BOX, 1, a, 1, (1 << 16) + 1) == engine.QN_ERR_INVALID_ARG
    b = np.zeros((1, 8), dtype=np.uint32); b[0, 6] = chk.b1(1.0)
    for col, word in ((0, int(g.tdims[0])), (1, int(g.tdims[1])), (2, int(g.tdims[2])), (3, INF_BITS), (6, 0)):
        a = b.copy(); a[0, col] = word
        assert call(c.DS_BOUNDS, 1, a, 1, 0) == engine.QN_ERR_INVALID_ARG
    assert call(c.DS_BEST1, 1, np.zeros(64), 1, 3) == engine.QN_ERR_INVALID_ARG and call(c.DS_BEST1, 1, np.zeros(64), 1, 1 | (65 << 16)) == engine.QN_ERR_INVALID_ARG
    assert call(c.DS_DUMP, 1, ok, g.n + 1, g.ncells) == engine.QN_ERR_INVALID_ARG
    assert (out == 7).all()


def test_overflow_word_is_raised_and_nothing_is_written_past_the_capacity(dev):
    c = dev("seams")[0]; g = sc.grid("seams")
    a = np.zeros((2, 12), dtype=np.uint32); a[0, :6] = (0, g.dims[0] - 1, 0, g.dims[1] - 1, 0, g.dims[2] - 1); a[1, :6] = (8, 8, 4, 4, 3, 3)
    out = c.debug_search(c.DS_STREAM_BOX, 1, a, 2, 100, 2 * 104).reshape(2, 104)
    alone = c.debug_search(c.DS_STREAM_BOX, 1, a[1:], 1, 100, 104)
    assert tuple(out[0, :3]) == (g.n, 1, g.n) and len(np.unique(out[0, 4:])) == 100
    assert 0 < alone[0] < 100 and alone[1] == 0 and (out[1] == alone).all()      # the record behind the overflowing one is what it is alone
