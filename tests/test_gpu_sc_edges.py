"""The Scan Context kernels (csrc/qn_sc.hip: k_sc_bin, k_sc_finish, k_sc_ringkey, k_sc_dist, k_sc_select, k_sc_gather and the chunk loops of
qn_kf_sc_describe / qn_kf_sc_query) on the edge cases of tests/sc_edge_cases.py: bit for bit against the numpy twin qn_amd/scancontext.py (descriptor,
ring key and column norms as bit patterns; ids, D bits, shifts, n_out and the padding -1 / NaN / -1 of every row) and against what the cases state by
construction (tests/test_sc_edges_cpu.py holds the twin to the same statements and to a scalar restatement of the definition, without a GPU).

What the cases reach that ray-cast and uniform clouds do not:
  knife edges   records ON ring edges off the axes (Pythagorean triples), at r2 == max_radius^2, around ring edges that are not representable, on the 45
                degree boundary (the cross product exactly 0 for some), on both sides of the x axis by a subnormal, each with its f32 neighbours; bin
                values at the f32 rounding ties of z + lidar_height, a negative maximum, a present value of 0.
  tile seams    keyframes of 1 .. 8193 records in ONE describe call whose deciding record is the last one or the first of the last tile of k_sc_bin.
  distances     every `waves` value of k_sc_dist (4, 4 at exactly 64 KB of LDS, 3, 2, 1) at per_block - 1, per_block, per_block + 1 slots, exhaustive and
                through the prefilter; equal minima over the shifts in one lane (s and s + 64) and in different lanes.
  selection     300 and more candidates at one D with the want-th entry at ids 254 .. 256 and 299, the same behind a prefilter whose own cut falls in a
                ring-key tie across id 256 and which lists D ties out of id order; all candidates empty (D == 1.0); keys that differ in their low bytes
                only; ring-key distances over 19 decades; a candidate exactly tdiff older than the query.
  chunk seams   8192 + 5 keyframes in one describe call; descriptor storage grown twice with every old slot re-read; 65535 + 3 query rows (the grid's row
                cap) and qc + 7 rows under the 256 MB scratch cap (qc about 14.9k), the rows on both sides of each chunk boundary checked by name.
One store per shape; every input is within the documented limits."""
import ctypes as C
import os
import sys
import time
import numpy as np
import pytest
from qn_amd import scancontext as sc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sc_edge_cases as ec

pytestmark = pytest.mark.gpu


def _store(p=None, prefilter=0):
    from qn_amd import engine
    store = engine.KeyframeStore()
    if p is not None:
        store.sc_set_params(n_rings=p.n_rings, n_sectors=p.n_sectors, max_radius=p.max_radius, lidar_height=p.lidar_height, ringkey_prefilter=prefilter)
    return store


def _set(store, p, prefilter=0):
    store.sc_set_params(n_rings=p.n_rings, n_sectors=p.n_sectors, max_radius=p.max_radius, lidar_height=p.lidar_height, ringkey_prefilter=prefilter)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same3(got, want, what):
    for g, w, name in zip(got, want, ("descriptor", "ring key", "column norms")):
        w = np.asarray(w, g.dtype)
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, name, np.argwhere(_bits(g) != _bits(w))[:6].tolist())


def _query(store, queries, stamps, tdiff, k):
    """qn_kf_sc_query with the padding kept -> (ids [nq, k], D, shift, n); the output buffers start out with values no row may keep"""
    q = np.ascontiguousarray(queries, np.int32); st = np.ascontiguousarray(stamps, np.float64)
    nq = len(q)
    ids = np.full(nq * k, 7777, np.int32); D = np.full(nq * k, 7777.0); sh = np.full(nq * k, 7777, np.int32); n = np.full(nq, 7777, np.uint32)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = store._l.qn_kf_sc_query(store.h, v(q), C.c_uint32(nq), v(st), C.c_uint32(len(st)), C.c_double(tdiff), C.c_uint32(k), v(ids), v(D), v(sh), v(n))
    assert rc == 0, rc
    return ids.reshape(nq, k), D.reshape(nq, k), sh.reshape(nq, k), n


def _arrays(rows_per_query, k):
    """twin / by-construction rows [(id, D, shift)] per query -> the padded arrays the engine must return"""
    nq = len(rows_per_query)
    ids = np.full((nq, k), -1, np.int32); D = np.full((nq, k), np.nan); sh = np.full((nq, k), -1, np.int32); n = np.zeros(nq, np.uint32)
    for r, rows in enumerate(rows_per_query):
        n[r] = len(rows)
        for c, (i, d, s) in enumerate(rows):
            ids[r, c] = i; D[r, c] = d; sh[r, c] = s
    return ids, D, sh, n


def _same_result(got, want, what, rows=None):
    sel = slice(None) if rows is None else rows
    gi, gd, gs, gn = (a[sel] for a in got)
    wi, wd, ws, wn = want
    assert np.array_equal(gn, wn), (what, "n_out", np.flatnonzero(gn != wn)[:8].tolist())
    bad = np.flatnonzero((gi != wi).any(1) | (gs != ws).any(1) | (_bits(gd) != _bits(np.ascontiguousarray(wd))).any(1))
    assert len(bad) == 0, (what, "rows", bad[:8].tolist(), gi[bad[:2]].tolist(), wi[bad[:2]].tolist(), gd[bad[:2]].tolist(), wd[bad[:2]].tolist(),
                           gs[bad[:2]].tolist(), ws[bad[:2]].tolist())


def _by_bins(k):
    """the descriptor of a knife cloud from its exact bins: the maximum over a bin's kept records of (f32)((f64)z + lidar_height)"""
    p = k.params
    best = {}
    for (ring, sector, keep), rec in zip(k.bins, k.cloud):
        if keep:
            v = np.float32(np.float64(rec[2]) + p.lidar_height)
            best[(ring, sector)] = max(best.get((ring, sector), v), v)
    return ec.dense(best, p)


# ---- knife edges and tile seams
def test_knife_edge_clouds():
    store = _store()
    for k in ec.knives():
        _set(store, k.params)
        kid = store.add(k.cloud)
        store.sc_describe([kid])
        got = store.sc_descriptor(kid)
        _same3(got, sc.descriptor(k.cloud, k.params), k.name)
        d = _by_bins(k)
        _same3(got, (d,) + ec.keys_of(d), (k.name, "by construction"))
        if k.desc is not None:
            assert np.array_equal(_bits(got[0]), _bits(ec.dense(k.desc, k.params))), (k.name, "stated values")
        # every record as a keyframe of its own, all in one describe call: the descriptor is the record's bin (or nothing, when it is dropped)
        singles = ec.single_records(k)
        ids = [store.add(a) for a, _ in singles]
        store.sc_describe(ids)
        wrong = []
        for at, (sid, (a, want)) in enumerate(zip(ids, singles)):
            d = store.sc_descriptor(sid)[0]
            if not np.array_equal(_bits(d), _bits(ec.dense(want, k.params))):
                wrong.append((at, a[0].tolist(), [(int(i), int(j), float(d[i, j])) for i, j in zip(*np.nonzero(d))], want))
        assert not wrong, (k.name, "(record, xyz, engine bins, exact bin):", wrong[:8], len(wrong))
        for at, r, s_, kp in k.pinned:
            d = store.sc_descriptor(ids[at])[0]
            nz = list(zip(*np.nonzero(d)))
            if not kp:
                assert not nz, (k.name, at, "dropped by the geometry")
            elif nz:                                                 # (a present value of 0 leaves nothing to see)
                assert (r is None or nz[0][0] == r) and (s_ is None or nz[0][1] == s_), (k.name, at, nz, r, s_)
    store.close()


def test_tile_seams_of_the_binning_in_one_launch():
    store = _store()
    cases = ec.tile_keyframes()
    ids = [store.add(a) for a, _ in cases]
    store.sc_describe(ids[::-1] + ids)                               # the long keyframes first in the launch, repeats ignored
    for kid, (a, want) in zip(ids, cases):
        d = ec.dense(want)
        got = store.sc_descriptor(kid)
        _same3(got, (d,) + ec.keys_of(d), (len(a), "by construction"))
        _same3(got, sc.descriptor(a, ec.DEFAULT), len(a))
    store.close()


# ---- distances: every waves value, per_block - 1 / per_block / per_block + 1 slots
@pytest.mark.parametrize("shape", sorted(ec.DIST_SHAPES))
def test_distance_shapes(shape):
    w = ec.DistWorld(*shape)
    pb = w.per_block
    store = _store(w.params)
    twin = {}
    n = 0
    for N, pre in [(pb - 1, 0), (pb, 0), (pb + 1, 0), (pb + 2, pb - 1), (pb + 2, pb), (pb + 2, pb + 1)]:
        new = [store.add(w.clouds[m]) for m in range(n, N)]
        assert new == list(range(n, N))
        if new:
            store.sc_describe(new)
        for m in new:
            twin[m] = sc.descriptor(w.clouds[m], w.params)
            _same3(store.sc_descriptor(m), twin[m], (shape, m))
            assert np.array_equal(_bits(store.sc_descriptor(m)[0]), _bits(np.asarray(w.values[m], np.float32))), (shape, m, "stated descriptor")
        n = N
        _set(store, w.params, pre)
        st = w.stamps[:N]
        got = _query(store, [0, 1], st, w.tdiff, N)
        want = [sc.query(twin, q, st, w.tdiff, N, prefilter=pre) for q in (0, 1)]
        _same_result(got, _arrays(want, N), (shape, N, pre))
        zero = w.zero_class(range(1, N))
        assert len(zero) >= 1 and [(int(a), float(b), int(c)) for a, b, c in zip(got[0][0], got[1][0], got[2][0])][:len(zero)] == zero, (shape, N, pre, "by construction")
    store.close()


# ---- selection
@pytest.fixture(scope="module")
def sel():
    w = ec.SelectWorld()
    store = _store()
    ids = [store.add(c) for c in w.clouds]
    assert ids == list(range(w.count))
    store.sc_describe(ids)
    memo = {}
    w.twin = {}
    for i, c in enumerate(w.clouds):
        key = c.tobytes()
        if key not in memo:
            memo[key] = sc.descriptor(c, ec.DEFAULT)
            _same3(store.sc_descriptor(i), memo[key], ("select", i))
        w.twin[i] = memo[key]
    w.store = store
    yield w
    store.close()


def _rows(got, row=0):
    ids, D, sh, n = got
    return [(int(a), float(b), int(c)) for a, b, c in zip(ids[row, :n[row]], D[row, :n[row]], sh[row, :n[row]])]


@pytest.mark.parametrize("top_k,prefilter", [(255, 0), (256, 0), (257, 0), (300, 0), (300, 305), (300, 306), (300, 307), (256, 306), (1024, 0), (1024, 1024)])
def test_ties_across_id_256(sel, top_k, prefilter):
    w = sel
    _set(w.store, ec.DEFAULT, prefilter)
    st = w.tie_stamps()
    got = _query(w.store, [699], st, 2.0, top_k)
    want = sc.query(w.twin, 699, st, 2.0, top_k, prefilter=prefilter)
    _same_result(got, _arrays([want], top_k), (top_k, prefilter))
    head = w.tie_prefix(top_k, prefilter)
    assert got[0][0, :len(head)].tolist() == head, "by construction"
    assert int(got[3][0]) == min(top_k, prefilter or 697, 697) and 697 not in got[0][0].tolist()
    if not prefilter and top_k in (255, 256, 257):
        assert int(got[0][0, -1]) == top_k - 1
    if top_k == 1024 and not prefilter:
        b = [i for i in range(697) if w.kind[i] == "B"]
        assert got[0][0, :697].tolist() == [690, 691] + sorted(w.a_ids + w.a2_ids) + b
        assert (got[0][0, 697:] == -1).all() and np.isnan(got[1][0, 697:]).all() and (got[2][0, 697:] == -1).all()


def test_empty_candidates_low_byte_keys_and_decades(sel):
    w = sel
    _set(w.store, ec.DEFAULT, 0)
    st = w.stamps_for(w.q_empty, w.empties)
    for k in (255, 256, 257, 300):
        got = _query(w.store, [w.q_empty], st, 1.0, k)
        _same_result(got, _arrays([[(c, 1.0, 0) for c in w.empties[:k]]], k), ("empties", k))
    by_m = sorted(w.ulp_ids, key=lambda c: w.ulp_of[c])
    st = w.stamps_for(w.q_ulp, w.ulp_ids + w.empties[:5])
    for k, pre in ((40, 0), (7, 0), (45, 0), (16, 16), (5, 16)):
        _set(w.store, ec.DEFAULT, pre)
        got = _query(w.store, [w.q_ulp], st, 1.0, k)
        _same_result(got, _arrays([sc.query(w.twin, w.q_ulp, st, 1.0, k, prefilter=pre)], k), ("ulps", k, pre))
        assert [r[0] for r in _rows(got)] == (by_m[:pre] if pre else by_m + w.empties[:5])[:k], ("ulps", k, pre, "by construction")
    by_e = sorted(w.dec_ids, key=lambda c: w.dec_of[c])
    st = w.stamps_for(w.q_dec, w.dec_ids)
    for k, pre in ((33, 0), (10, 10), (33, 20), (4, 31)):
        _set(w.store, ec.DEFAULT, pre)
        got = _query(w.store, [w.q_dec], st, 1.0, k)
        _same_result(got, _arrays([sc.query(w.twin, w.q_dec, st, 1.0, k, prefilter=pre)], k), ("decades", k, pre))
        listed = set(by_e[:pre] if pre else by_e)
        found = {r[0] for r in _rows(got)}
        assert len(found) == min(k, len(listed)) and found <= listed, ("decades", k, pre, "by construction")


# ---- chunk seams
def _tiny_descriptors(n, rings=20):
    d = np.zeros((n, 20, 60), np.float32); rk = np.zeros((n, 20)); cn = np.zeros((n, 60))
    for i in range(n):
        r, s, v = ec.tiny_bin(i, rings)
        d[i, r, s] = v; rk[i, r] = v / 60.0; cn[i, s] = v
    return d, rk, cn


def _check_tiny(store, ids, want, what):
    for i in ids:
        _same3(store.sc_descriptor(i), (want[0][i], want[1][i], want[2][i]), (what, i))


def test_more_than_8192_keyframes_in_one_describe():
    n = ec.DESCRIBE_COUNT
    store = _store()
    t0 = time.perf_counter()
    ids = [store.add(ec.tiny_cloud(i)) for i in range(n)]
    t1 = time.perf_counter()
    store.sc_describe(ids)
    t2 = time.perf_counter()
    want = _tiny_descriptors(n)
    _check_tiny(store, ids, want, "describe chunk")
    t3 = time.perf_counter()
    print("describe-chunk: add %d keyframes %.1f ms, describe %.2f ms, read back %.1f ms" % (n, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
    for i in (0, ec.SC_DESCRIBE_CHUNK - 1, ec.SC_DESCRIBE_CHUNK, n - 1):
        _same3(store.sc_descriptor(i), sc.descriptor(ec.tiny_cloud(i), ec.DEFAULT), ("twin", i))
    q = n - 1
    got = _query(store, [q], np.arange(n, dtype=np.float64), 0.5, 5)
    rows = ec.tiny_query(q, range(q), 5)
    assert [r[1] for r in rows] == [0.0] * 5
    _same_result(got, _arrays([rows], 5), "query over 8197 slots")
    store.close()


def test_growth_keeps_every_slot_and_the_scratch_cap_chunks_the_queries():
    store = _store()
    want = _tiny_descriptors(ec.GROWTH_STEPS[-1])
    have = 0
    for n in ec.GROWTH_STEPS:
        new = [store.add(ec.tiny_cloud(i)) for i in range(have, n)]
        store.sc_describe(new)
        have = n
        _check_tiny(store, range(n), want, ("growth to", n))       # every earlier slot again, after the copy into the grown storage
    _set(store, ec.DEFAULT, ec.SCRATCH_P)
    queries, qc = ec.scratch_queries()
    assert len(queries) > qc
    t0 = time.perf_counter()
    got = _query(store, queries, np.arange(ec.SCRATCH_N, dtype=np.float64), 0.5, ec.SCRATCH_K)
    print("scratch-cap query: %d rows (qc %d) %.2f ms" % (len(queries), qc, 1e3 * (time.perf_counter() - t0)))
    _same_result(got, ec.tiny_rows(queries, ec.SCRATCH_N, ec.SCRATCH_K), "scratch cap, by construction")
    twin = {i: sc.descriptor(ec.tiny_cloud(i), ec.DEFAULT) for i in range(ec.SCRATCH_N)}
    st = np.arange(ec.SCRATCH_N, dtype=np.float64)
    for row in (0, qc - 1, qc, len(queries) - 1):
        rows = sc.query(twin, int(queries[row]), st, 0.5, ec.SCRATCH_K, prefilter=ec.SCRATCH_P)
        _same_result(got, _arrays([rows], ec.SCRATCH_K), ("scratch cap, twin, row", row), rows=slice(row, row + 1))
    store.close()


def test_more_query_rows_than_one_grid_takes():
    store = _store()
    n_kf, rings = ec.ROWCAP_KEYFRAMES, ec.ROWCAP_RINGS
    ids = [store.add(ec.tiny_cloud(i, rings)) for i in range(n_kf)]
    store.sc_describe(ids)
    queries = ec.rowcap_queries()
    st = np.arange(n_kf, dtype=np.float64)
    t0 = time.perf_counter()
    got = _query(store, queries, st, 0.5, 1)
    print("row-cap query: %d rows %.2f ms" % (len(queries), 1e3 * (time.perf_counter() - t0)))
    _same_result(got, ec.tiny_rows(queries, n_kf, 1, rings), "row cap, by construction")
    twin = {i: sc.descriptor(ec.tiny_cloud(i, rings), ec.DEFAULT) for i in range(n_kf)}
    per_q = {q: sc.query(twin, q, st, 0.5, 1) for q in range(n_kf)}
    _same_result(got, _arrays([per_q[int(q)] for q in queries], 1), "row cap, twin")
    for row in (ec.SC_MAX_ROWS - 1, ec.SC_MAX_ROWS, len(queries) - 1):
        assert _rows(got, row) == per_q[int(queries[row])], row
    store.close()
