"""The Scan Context twin (qn_amd/scancontext.py) on the edge cases of tests/sc_edge_cases.py, without a GPU:
  - against what the cases state by construction: bins, dropped records, bin values, D == 0.0 and the shift of rolled periodic descriptors, the tie
    classes and their order, the rows of the chunk-seam queries;
  - against a scalar restatement of the definition in include/qn_engine.h (one point, one column, one candidate at a time, Python floats, no numpy vector
    operation): descriptor, ring key, column norms, every distance and shift, every query result, bit for bit;
  - bins() against plain geometry (atan2, hypot) on 200k uniform points per shape, away from the edges;
  - and the cases against what they claim: the seams are crossed under the restated constants."""
import math
import os
import struct
import sys
import numpy as np
import pytest
from qn_amd import scancontext as sc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sc_edge_cases as ec


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same3(got, want, what):
    for g, w, name in zip(got, want, ("descriptor", "ring key", "column norms")):
        g = np.asarray(g, np.float32 if name == "descriptor" else np.float64)
        w = np.asarray(w, np.float32 if name == "descriptor" else np.float64)
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, name, np.argwhere(_bits(g) != _bits(w))[:6].tolist())


# ---- the definition (include/qn_engine.h, "loop candidates by Scan Context"), one thing at a time
def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def s_bin(x, y, z, p, tabs):
    """-> None (dropped) or (ring, sector, value)"""
    e, c, s = tabs
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)) or (x == 0.0 and y == 0.0):
        return None
    r2 = x * x + y * y
    if r2 >= e[p.n_rings]:
        return None
    ring = 0
    for i in range(1, p.n_rings):
        if r2 >= e[i]:
            ring += 1
    lower = not (y > 0.0 or (y == 0.0 and x > 0.0))                  # p in [pi, 2 pi)
    sector = 0
    for j in range(1, p.n_sectors):
        b_upper = s[j] > 0.0 or (s[j] == 0.0 and c[j] > 0.0)
        if (lower and b_upper) or (lower != b_upper and c[j] * y - s[j] * x >= 0.0):
            sector += 1
    return ring, sector, f32(z + p.lidar_height)


def s_descriptor(cloud, p):
    """-> (d [nr][ns] floats, rk [nr], cn [ns], ss [ns])"""
    tabs = ec.table_values(p)
    d = [[None] * p.n_sectors for _ in range(p.n_rings)]
    seen = set()
    for rec in np.asarray(cloud, np.float32).astype(np.float64).tolist():
        if tuple(rec) in seen:                                       # a repeated record changes no maximum
            continue
        seen.add(tuple(rec))
        b = s_bin(rec[0], rec[1], rec[2], p, tabs)
        if b is not None and (d[b[0]][b[1]] is None or b[2] > d[b[0]][b[1]]):
            d[b[0]][b[1]] = b[2]
    d = [[0.0 if v is None else v for v in row] for row in d]        # a bin with no point is 0
    return (d,) + s_keys(d)


def s_keys(d):
    nr, ns = len(d), len(d[0])
    rk = []
    for i in range(nr):
        acc = 0.0
        for j in range(ns):
            acc = acc + d[i][j]
        rk.append(acc / ns)
    ss = []
    for j in range(ns):
        acc = 0.0
        for i in range(nr):
            acc = acc + d[i][j] * d[i][j]
        ss.append(acc)
    return rk, [math.sqrt(v) for v in ss], ss


_PAIRS = {}


def s_distance(q, c):
    """q, c = s_descriptor results -> (D, shift); identical pairs are evaluated once"""
    key = (repr(q[0]), repr(c[0]))
    if key in _PAIRS:
        return _PAIRS[key]
    nr, ns = len(q[0]), len(q[0][0])
    qcol = [[q[0][i][j] for i in range(nr)] for j in range(ns)]
    ccol = [[c[0][i][j] for i in range(nr)] for j in range(ns)]
    qs, cs = q[3], c[3]
    qj = [j for j in range(ns) if qs[j] != 0.0]
    best, shift = None, 0
    for s in range(ns):
        total, cnt = 0.0, 0
        for j in qj:
            k = (j + s) % ns
            if cs[k] != 0.0:
                dot = 0.0
                for a, b in zip(qcol[j], ccol[k]):
                    dot = dot + a * b
                total = total + (1.0 - dot / math.sqrt(qs[j] * cs[k]))
                cnt += 1
        D = total / cnt if cnt else 1.0
        if best is None or D < best:
            best, shift = D, s
    _PAIRS[key] = (best, shift)
    return best, shift


def s_query(descs, q, stamps, tdiff, top_k, prefilter=0):
    cand = [c for c in sorted(descs) if c != q and stamps[q] - stamps[c] > tdiff]
    if prefilter:
        def rkd(c):
            acc = 0.0
            for a, b in zip(descs[q][1], descs[c][1]):
                acc = acc + (a - b) * (a - b)
            return acc
        cand = sorted(cand, key=lambda c: (rkd(c), c))[:prefilter]
    rows = sorted(((s_distance(descs[q], descs[c]), c) for c in cand), key=lambda r: (r[0][0], r[1]))[:top_k]
    return [(c, D, sh) for (D, sh), c in rows]


def _same_rows(got, want, what):
    assert [r[0] for r in got] == [r[0] for r in want] and [r[2] for r in got] == [r[2] for r in want], (what, got[:8], want[:8])
    assert [struct.pack("d", r[1]) for r in got] == [struct.pack("d", r[1]) for r in want], (what, got[:8], want[:8])


def _scalar_of(twin3, p):
    """the scalar structures of a descriptor the twin gave (for the distance restatement)"""
    d = [[float(v) for v in row] for row in np.asarray(twin3[0], np.float64)]
    return (d,) + s_keys(d)


# ---- the cases cross the seams they name
def test_the_seams_are_crossed_under_the_restated_constants():
    assert [ec.waves(*s) for s in ((20, 60), (30, 128), (50, 100), (64, 100), (64, 128), (8, 128), (8, 120))] == [4, 4, 3, 2, 1, 4, 4]
    assert ec.stage_bytes(30, 128) == 16384 and 4 * ec.stage_bytes(30, 128) == 65536
    assert set(ec.TILE_COUNTS) >= {ec.SC_BIN_BLOCK - 1, ec.SC_BIN_BLOCK, ec.SC_BIN_BLOCK + 1, ec.SC_BIN_TILE - 1, ec.SC_BIN_TILE, ec.SC_BIN_TILE + 1,
                                   2 * ec.SC_BIN_TILE, 2 * ec.SC_BIN_TILE + 1}
    assert ec.DESCRIBE_COUNT > ec.SC_DESCRIBE_CHUNK
    cap = 0
    for n in ec.GROWTH_STEPS:                                       # every step outgrows the capacity the step before left
        assert n > cap
        cap = max(n, 2 * cap, ec.SC_MIN_CAP)
    assert ec.query_chunk(ec.ROWCAP_NQ, ec.ROWCAP_KEYFRAMES, 0, 1) == ec.SC_MAX_ROWS < ec.ROWCAP_NQ
    q, qc = ec.scratch_queries()
    assert len(q) > qc == ec.query_chunk(len(q), ec.SCRATCH_N, ec.SCRATCH_P, ec.SCRATCH_K) and 14000 < qc < 16000 and qc < ec.SC_MAX_ROWS
    assert ec.GROWTH_STEPS[-1] == ec.SCRATCH_N
    w = ec.SelectWorld()
    assert len(w.a_ids) + len(w.a2_ids) >= 300 and w.a_ids[252:255] == [254, 255, 256] and w.count > ec.SC_SEL_MAX


# ---- knife edges
KNIVES = {k.name: k for k in ec.knives()}


@pytest.mark.parametrize("name", sorted(KNIVES))
def test_the_twin_bins_knife_edge_records_as_the_geometry_states(name):
    k = KNIVES[name]
    ring, sector, keep = sc.bins(k.cloud, k.params)
    want = k.bins
    assert keep.tolist() == [w[2] for w in want], name
    assert sector.tolist() == [w[1] for w in want], (name, [i for i, w in enumerate(want) if sector[i] != w[1]][:8])
    assert [r for r, w in zip(ring.tolist(), want) if w[2]] == [w[0] for w in want if w[2]], name
    for at, r, s, kp in k.pinned:
        assert bool(keep[at]) == kp, (name, at, k.cloud[at])
        assert r is None or ring[at] == r, (name, at, k.cloud[at], int(ring[at]), r)
        assert s is None or sector[at] == s, (name, at, k.cloud[at], int(sector[at]), s)
    if k.desc is not None:
        d = ec.dense(k.desc, k.params)
        assert np.array_equal(_bits(sc.descriptor(k.cloud, k.params)[0]), _bits(d)), name
    tabs = ec.table_values(k.params)
    for i, (x, y, z) in enumerate(k.cloud.astype(np.float64).tolist()):
        b = s_bin(x, y, z, k.params, tabs)
        assert (b is not None) == bool(keep[i]) and (b is None or (b[0], b[1]) == (ring[i], sector[i])), (name, i)
    _same3(s_descriptor(k.cloud, k.params)[:3], sc.descriptor(k.cloud, k.params), name)


def test_the_knife_edge_records_sit_on_their_edges():
    """conditions on the inputs: the diagonal family has records whose cross product is exactly 0 and records on both sides of the boundary; the
    neighbours of an on-edge record fall on both sides"""
    for ns in ec.DIAGONAL_NS:
        k = KNIVES["diagonal-%d" % ns]
        _, c, s = ec.table_values(k.params)
        j = ns // 8
        zero = [rec for rec in k.cloud.astype(np.float64).tolist() if rec[0] > 0 and rec[1] > 0 and c[j] * rec[1] - s[j] * rec[0] == 0.0]
        assert len(zero) >= 3, (ns, zero)
        first = [b[1] for b, rec in zip(k.bins, k.cloud.tolist()) if rec[0] > 0 and rec[1] > 0]
        assert set(first) == {j - 1, j}, (ns, set(first))
    py = KNIVES["pythagoras"]
    rings = [b[0] for b in py.bins]
    assert rings[0:5] == [5, 4, 5, 4, 5]
    assert [b[2] for b in py.bins[35:40]] == [False, True, False, True, False]
    odd = KNIVES["odd-ring-width"]
    assert len({b[0] for b in odd.bins if b[2]}) == 7                 # both sides of every edge: all seven rings


def test_tile_seam_keyframes():
    for a, want in ec.tile_keyframes():
        d = ec.dense(want)
        tw = sc.descriptor(a, ec.DEFAULT)
        assert np.array_equal(_bits(tw[0]), _bits(d)), len(a)
        _same3(tw, (d,) + ec.keys_of(d), len(a))
        _same3(s_descriptor(a, ec.DEFAULT)[:3], tw, len(a))


# ---- distances
_WORLDS = {}


def dist_world(shape):
    if shape not in _WORLDS:
        w = ec.DistWorld(*shape)
        w.twin = {m: sc.descriptor(c, w.params) for m, c in enumerate(w.clouds)}
        _WORLDS[shape] = w
    return _WORLDS[shape]


@pytest.mark.parametrize("shape", sorted(ec.DIST_SHAPES))
def test_rolled_periodic_descriptors_are_at_zero_at_the_stated_shift(shape):
    w = dist_world(shape)
    for m, v in enumerate(w.values):
        _same3(w.twin[m], (np.asarray(v, np.float32),) + ec.keys_of(v), (shape, m))      # the cloud's descriptor is the stated one
    scal = {m: _scalar_of(w.twin[m], w.params) for m in w.twin}
    _same3(s_descriptor(w.clouds[1], w.params)[:3], w.twin[1], (shape, "scalar descriptor"))
    for m in range(1, w.count):
        got = sc.distance(w.twin[0], w.twin[m])
        if m in w.rolled:
            assert got == (0.0, w.rolled[m] % w.period), (shape, m, w.rolled[m], got)
        else:
            assert got[0] > 1e-3, (shape, m, got)
        sd = s_distance(scal[0], scal[m])
        assert struct.pack("d", sd[0]) == struct.pack("d", got[0]) and sd[1] == got[1], (shape, m, sd, got)
    pb = w.per_block
    for n, pre in [(pb - 1, 0), (pb, 0), (pb + 1, 0), (pb + 2, pb - 1), (pb + 2, pb), (pb + 2, pb + 1)]:
        descs = {m: w.twin[m] for m in range(n)}
        res = sc.query(descs, 0, w.stamps, w.tdiff, n, prefilter=pre)
        zero = w.zero_class(range(1, n))
        assert res[:len(zero)] == zero and len(res) == (min(pre, n - 1) if pre else n - 1), (shape, n, pre, res[:4], zero[:4])
        _same_rows(s_query({m: scal[m] for m in range(n)}, 0, w.stamps, w.tdiff, n, prefilter=pre), res, (shape, n, pre))


def test_equal_minima_in_one_lane_and_in_two():
    """the shapes and rolls the shift minimum is tested at: (Nr, Ns, period, roll)"""
    for nr, ns, p, k in ((8, 128, 64, 5), (8, 120, 60, 2), (8, 120, 60, 10), (30, 128, 64, 63)):
        w = dist_world((nr, ns))
        assert w.period == p and k in w.rolled.values()
        m = [i for i, r in w.rolled.items() if r == k][0]
        assert sc.distance(w.twin[0], w.twin[m]) == (0.0, k % p)
        q = w.twin[0][0].astype(np.float64)
        assert np.array_equal(np.roll(q, k, axis=1), np.roll(q, k % p + p, axis=1))      # the second minimum, one period on


# ---- selection
@pytest.fixture(scope="module")
def sel():
    w = ec.SelectWorld()
    memo = {}
    w.twin = {}
    for i, c in enumerate(w.clouds):
        key = c.tobytes()
        if key not in memo:
            memo[key] = sc.descriptor(c, ec.DEFAULT)
        w.twin[i] = memo[key]
    smemo = {}
    w.scal = {}
    for i, c in enumerate(w.clouds):
        key = c.tobytes()
        if key not in smemo:
            smemo[key] = s_descriptor(c, ec.DEFAULT)
            _same3(smemo[key][:3], memo[key], ("select", i))
        w.scal[i] = smemo[key]
    return w


def test_the_tie_classes_are_what_the_world_states(sel):
    w = sel
    q = w.twin[699]
    DA, DA2, DB = (sc.distance(q, w.twin[i]) for i in (0, 400, 100))
    assert DA == DA2 and 0.0 < DA[0] < DB[0] and sc.distance(q, w.twin[690]) == (0.0, 0)
    rk = [sc.ringkey_distance(q[1], w.twin[i][1]) for i in (690, 400, 0, 100)]
    assert rk[0] == 0.0 and rk[0] < rk[1] < rk[2] < rk[3], rk
    assert sc.distance(w.twin[w.q_empty], w.twin[700]) == (1.0, 0) and sc.distance(q, w.twin[w.q_empty]) == (1.0, 0)


@pytest.mark.parametrize("top_k,prefilter", [(255, 0), (256, 0), (257, 0), (300, 0), (300, 305), (300, 306), (300, 307), (256, 306), (1024, 0), (1024, 1024)])
def test_ties_across_id_256(sel, top_k, prefilter):
    """selection "ties" and "strict-tdiff\""""
    w = sel
    st = w.tie_stamps()
    descs = {i: w.twin[i] for i in range(w.count)}
    res = sc.query(descs, 699, st, 2.0, top_k, prefilter=prefilter)
    head = w.tie_prefix(top_k, prefilter)
    assert [r[0] for r in res[:len(head)]] == head, (res[:3], head[:3])
    assert len(res) == min(top_k, prefilter or 697, 697)
    assert 697 not in [r[0] for r in res] and 698 not in [r[0] for r in res]              # 699 - 697 == tdiff: not admissible
    if not prefilter and top_k in (255, 256, 257):
        assert res[-1][0] == top_k - 1                                # ids 254, 255, 256: the want-th entry inside the tie class
    if top_k == 1024 and not prefilter:
        b = [i for i in range(697) if w.kind[i] == "B"]
        assert [r[0] for r in res] == [690, 691] + sorted(w.a_ids + w.a2_ids) + b
    _same_rows(s_query({i: w.scal[i] for i in range(w.count)}, 699, st, 2.0, top_k, prefilter=prefilter), res, (top_k, prefilter))


def test_empty_candidates_low_byte_keys_and_decades(sel):
    w = sel
    descs = {i: w.twin[i] for i in range(w.count)}
    scal = {i: w.scal[i] for i in range(w.count)}
    # every candidate empty: D == 1.0, shift 0, the lowest ids
    st = w.stamps_for(w.q_empty, w.empties)
    for k in (255, 256, 257, 300):
        res = sc.query(descs, w.q_empty, st, 1.0, k)
        assert res == [(c, 1.0, 0) for c in w.empties[:k]]
        _same_rows(s_query(scal, w.q_empty, st, 1.0, k), res, ("empties", k))
    # 1 .. 40 f32 steps: the order is the order of the steps, exhaustive and through a prefilter that keeps 16
    st = w.stamps_for(w.q_ulp, w.ulp_ids + w.empties[:5])
    by_m = sorted(w.ulp_ids, key=lambda c: w.ulp_of[c])
    for k, pre in ((40, 0), (7, 0), (45, 0), (16, 16), (5, 16)):
        res = sc.query(descs, w.q_ulp, st, 1.0, k, prefilter=pre)
        want = (by_m[:pre] if pre else by_m + w.empties[:5])[:k]
        assert [r[0] for r in res] == want, (k, pre)
        _same_rows(s_query(scal, w.q_ulp, st, 1.0, k, prefilter=pre), res, ("ulps", k, pre))
    keys = [sc.distance(w.twin[w.q_ulp], w.twin[c])[0] for c in by_m]
    assert all(a < b for a, b in zip(keys, keys[1:])) and (keys[-1] - keys[0]) / keys[0] < 1e-3       # the keys differ in their low bytes only
    # ring-key distances over 15 decades: the prefilter keeps the nearest by exponent
    st = w.stamps_for(w.q_dec, w.dec_ids)
    by_e = sorted(w.dec_ids, key=lambda c: w.dec_of[c])
    rk = [sc.ringkey_distance(w.twin[w.q_dec][1], w.twin[c][1]) for c in by_e]
    assert all(a < b for a, b in zip(rk, rk[1:])) and rk[-1] / rk[0] > 1e15
    for k, pre in ((33, 0), (10, 10), (33, 20), (4, 31)):
        res = sc.query(descs, w.q_dec, st, 1.0, k, prefilter=pre)
        listed = set(by_e[:pre] if pre else by_e)
        assert len(res) == min(k, len(listed)) and {r[0] for r in res} <= listed and (k < len(listed) or {r[0] for r in res} == listed), (k, pre)
        _same_rows(s_query(scal, w.q_dec, st, 1.0, k, prefilter=pre), res, ("decades", k, pre))


# ---- chunk seams
def test_tiny_indexed_keyframes():
    n = ec.DESCRIBE_COUNT
    cloud = np.concatenate([ec.tiny_cloud(i) for i in range(n)])
    ring, sector, keep = sc.bins(cloud, ec.DEFAULT)
    want = [ec.tiny_bin(i) for i in range(n)]
    assert keep.all() and ring.tolist() == [b[0] for b in want] and sector.tolist() == [b[1] for b in want]
    assert len(set(want)) == n                                        # distinct: a descriptor written to the wrong slot shows
    for i in (0, 1199, 1200, ec.SC_DESCRIBE_CHUNK - 1, ec.SC_DESCRIBE_CHUNK, n - 1):
        r, s, v = want[i]
        tw = sc.descriptor(ec.tiny_cloud(i), ec.DEFAULT)
        _same3(tw, tiny_descriptor(i), i)
        _same3(s_descriptor(ec.tiny_cloud(i), ec.DEFAULT)[:3], tw, i)
    for q, c in ((8196, 16), (8196, 17), (150, 10), (150, 149), (1300, 100), (7, 1207)):
        d = sc.distance(sc.descriptor(ec.tiny_cloud(q)), sc.descriptor(ec.tiny_cloud(c)))
        assert d == ec.tiny_pair(q, c), (q, c, d)


def tiny_descriptor(i, rings=20):
    r, s, v = ec.tiny_bin(i, rings)
    d = np.zeros((20, 60), np.float32); d[r, s] = v
    rk = np.zeros(20); rk[r] = v / 60.0
    cn = np.zeros(60); cn[s] = v
    return d, rk, cn


@pytest.mark.parametrize("which", ["rowcap", "scratch"])
def test_chunk_seam_query_rows(which):
    if which == "rowcap":
        queries, n_kf, k, rings, pre = ec.rowcap_queries(), ec.ROWCAP_KEYFRAMES, 1, ec.ROWCAP_RINGS, 0
        seam = ec.SC_MAX_ROWS
    else:
        (queries, seam), n_kf, k, rings, pre = ec.scratch_queries(), ec.SCRATCH_N, ec.SCRATCH_K, 20, ec.SCRATCH_P
    ids, D, sh, n = ec.tiny_rows(queries, n_kf, k, rings)
    descs = {i: sc.descriptor(ec.tiny_cloud(i, rings), ec.DEFAULT) for i in range(n_kf)}
    scal = {i: _scalar_of(descs[i], ec.DEFAULT) for i in range(n_kf)}
    stamps = np.arange(n_kf, dtype=np.float64)
    assert len(queries) > seam
    memo = {}
    for row in sorted({0, seam - 1, seam, len(queries) - 1} | set(range(0, len(queries), 4001 if which == "scratch" else 1))):
        q = int(queries[row])
        if q not in memo:
            memo[q] = sc.query(descs, q, stamps, 0.5, k, prefilter=pre)
            _same_rows(s_query(scal, q, stamps, 0.5, k, prefilter=pre), memo[q], (which, q))
        want = memo[q]
        assert n[row] == len(want) and [(int(a), float(b), int(c)) for a, b, c in zip(ids[row, :n[row]], D[row, :n[row]], sh[row, :n[row]])] == want, (which, row, q)
        assert (ids[row, n[row]:] == -1).all() and np.isnan(D[row, n[row]:]).all() and (sh[row, n[row]:] == -1).all()
    if which == "rowcap":
        assert n.min() == 0 and n.max() == 1 and set(np.unique(D[n > 0, 0]).tolist()) == {0.0, 1.0}
    else:
        assert (n == 3).all() and (D == 0.0).all() and len(set(int(q) for q in queries)) == 100


# ---- bins() against plain geometry
@pytest.mark.parametrize("shape", [(20, 60, 80.0), (7, 13, 25.0), (64, 128, 120.0), (3, 360, 10.0)])
def test_bins_follow_atan2_and_hypot_away_from_the_edges(shape):
    nr, ns, R = shape
    p = sc.Params(n_rings=nr, n_sectors=ns, max_radius=R)
    n = 200000
    xy = np.random.default_rng(nr * 1000 + ns).uniform(-1.1 * R, 1.1 * R, (n, 2)).astype(np.float32)
    ring, sector, keep = sc.bins(np.c_[xy, np.ones(n, np.float32)], p)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    w = 2.0 * math.pi / ns
    az = np.arctan2(y, x) % (2.0 * math.pi)
    fr = np.hypot(x, y) / (R / nr)
    clear = (np.abs(az - np.round(az / w) * w) > 1e-9) & (np.abs(fr - np.round(fr)) > 1e-9)
    left_out = int(n - clear.sum())
    print(shape, "left out", left_out, "of", n)
    assert left_out <= n // 1000
    inside = fr < nr
    assert np.array_equal(keep[clear], inside[clear])
    m = clear & inside
    assert m.sum() > n // 2
    bad = np.flatnonzero(m & ((sector != np.floor(az / w).astype(np.int64)) | (ring != np.floor(fr).astype(np.int64))))
    assert len(bad) == 0, (shape, len(bad), xy[bad[:5]].tolist())
