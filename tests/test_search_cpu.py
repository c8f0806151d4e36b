"""The references of tests/search_checks.py against each other and against exact arithmetic, on the clouds and queries of tests/search_cases.py - what
tests/test_gpu_search.py then holds the device to.  No GPU."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import search_cases as sc
import search_checks as chk

F = np.float32


def _tile_bound_violations(name, **variant):
    """pairs (query, point) whose f32 sqdist is BELOW the restated tile_box_d2 of the tile the restated grid puts the point in"""
    g, pts, q = sc.grid(name), sc.cloud(name), np.concatenate([sc.queries(name), sc.cloud(name)])
    t = g.tile_of(g.cells(pts))                                       # (N, 3)
    tb = g.tile_box_d2(t[None, :, :], q[:, None, :], **variant)       # (Q, N)
    return int((tb > chk.sqdist32(q, pts)).sum()), tb.size


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_tile_box_d2_is_a_lower_bound_of_every_pair(name):
    bad, total = _tile_bound_violations(name)
    print("%s: tile_box_d2 <= sqdist on %d pairs" % (name, total))
    assert bad == 0


def test_tile_box_d2_without_its_shrink_is_caught():
    """a point one ulp below a tile face that the f32 cell arithmetic rounds INTO the tile, queried from where it lies: the unshrunk box is too far"""
    assert sum(_tile_bound_violations(name, shrink=False)[0] for name in sc.CLOUDS) > 0


@pytest.mark.parametrize("name", sc.CLOUDS)
def test_cap_bounds_hold_against_exact_arithmetic(name):
    g, q = sc.grid(name), sc.queries(name)
    rng = np.random.default_rng(5)
    o_exact = g.exact_outside(q)
    o2, S = g.cap_of(q)
    out = o_exact.sum(axis=1) > 0
    assert out.sum() >= 100
    worst_e, worst_f = np.inf, 0.0
    for mult in (1.0, 1.0 + 1e-6, 1.01, 1.5, 4.0):
        for axis in range(3):
            rest = (o_exact ** 2).sum(axis=1) - o_exact[:, axis] ** 2
            r = (np.sqrt((o_exact ** 2).sum(axis=1)) * mult + rng.uniform(0, 1, len(q)) * (mult > 1.2)).astype(np.float32)
            r = np.maximum(r, F(0.05))
            half = np.sqrt(np.maximum(r.astype(np.float64) ** 2 - rest, 0.0))
            e = g.cap_extent(o2, S, r, axis).astype(np.float64)
            assert (e >= half).all(), (name, mult, axis)
            worst_e = min(worst_e, (e - half).min())
            f = rng.uniform(0, 40, len(q)).astype(np.float32)
            d = g.cap_face_dist(o2, S, f, axis).astype(np.float64)
            exact = np.sqrt(f.astype(np.float64) ** 2 + rest)
            assert (d <= exact).all(), (name, mult, axis)
            worst_f = max(worst_f, (d / np.maximum(exact, 1e-300)).max())
    print("%s: cap_extent - exact >= %.3g, cap_face_dist / exact <= %.9f" % (name, worst_e, worst_f))


def test_cap_bounds_without_their_slack_are_caught():
    """sqrtf alone rounds to nearest: on a few thousand queries it lands above the exact value for the face distance, below it for the extent"""
    bad_f = bad_e = 0
    for name in ("seams", "shifted"):
        g, q = sc.grid(name), sc.queries(name)
        o_exact = g.exact_outside(q); o2, S = g.cap_of(q)
        for axis in range(3):
            rest = (o_exact ** 2).sum(axis=1) - o_exact[:, axis] ** 2
            for f0 in (0.5, 3.0, 17.0):
                f = np.full(len(q), f0, dtype=np.float32)
                bad_f += int((g.cap_face_dist(o2, S, f, axis, down=False).astype(np.float64) > np.sqrt(f.astype(np.float64) ** 2 + rest))[rest > 0].sum())
                r = (np.sqrt((o_exact ** 2).sum(axis=1)) + f0).astype(np.float32)
                half = np.sqrt(np.maximum(r.astype(np.float64) ** 2 - rest, 0.0))
                bad_e += int((g.cap_extent(o2, S, r, axis, up=False).astype(np.float64) < half)[rest > 0].sum())
    assert bad_f > 0 and bad_e > 0, (bad_f, bad_e)


@pytest.mark.parametrize("unique", (False, True))
def test_best1_serial_equals_the_sorted_statement(unique):
    n = 0
    for L in (0, 1, 2, 7, 33):
        rec, fin = sc.best1_waves(100 + L, L)
        if unique:
            rec = sc.make_unique(rec)
        for w in range(rec.shape[0]):
            for lane in range(0, 64, 5):
                seq = [(bool(r[0]), chk.f1(r[1]), int(r[2])) for r in rec[w, :, lane]]
                a, b = chk.best1_serial(seq, unique), chk.best1_sorted(seq, unique)
                assert a[0] == b[0] and chk.bits(a[1]) == chk.bits(b[1]) and chk.bits(a[2]) == chk.bits(b[2]), (L, w, lane, a, b)
                n += 1
    print("Best1 serial against sorted, UNIQUE %s: %d lanes" % (unique, n))


def test_best1_that_keeps_the_higher_index_on_ties_is_caught():
    rec, _ = sc.best1_waves(107, 7)
    differ = 0
    for w in range(rec.shape[0]):
        for lane in range(64):
            seq = [(bool(r[0]), chk.f1(r[1]), int(r[2])) for r in rec[w, :, lane]]
            differ += chk.best1_serial(seq, False, keep_higher_on_ties=True)[0] != chk.best1_sorted(seq, False)[0]
    assert differ > 100


def test_best1_finish_from_the_merged_records():
    """finish<S> restated lane by lane gives what ONE sink would give on the union of the sub-slots' records (each point in one sub-slot only)"""
    rec, _ = sc.best1_waves(133, 9)
    rec = sc.make_unique(rec)
    for S in (2, 4):
        for w in range(0, rec.shape[0], 3):
            seqs = [[(bool(r[0]), chk.f1(r[1]), int(r[2])) for r in rec[w, :, lane]] for lane in range(64)]
            lanes = [chk.best1_sorted(s, True) for s in seqs]
            got = chk.best1_finish(lanes, S, [True] * 64)
            for l in range(64):
                grp = [l ^ x for x in ((0, 32) if S == 2 else (0, 16, 32, 48))]
                want = chk.best1_sorted([r for g in grp for r in seqs[g]], True)
                assert got[l][0] == want[0] and chk.bits(got[l][1]) == chk.bits(want[1]), (S, w, l)


def test_bestk_serial_equals_the_sorted_statement_and_a_short_merge_is_caught():
    """the lazy queue, the wave-wide flushes and finish<4> give every `on` query the first k of the sorted union of its four sub-slots' keys; a query that is
    not `on` keeps each sub-slot's own first k"""
    checked = caught = 0
    for kmax in sc.KMAXES:
        for k in sc.ks_of(kmax):
            for L in (0, 1, 16, 17, 33):
                rec, fin = sc.bestk_waves(300 + L, L)
                for w in range(3):
                    steps = sc.bestk_steps(rec[w]); on = fin[w] != 0
                    got = chk.bestk_wave_serial(steps, k, 4, on)
                    short = chk.bestk_wave_serial(steps, k, 4, on, merge_from=1)
                    for l in range(64):
                        grp = [l, l ^ 32, l ^ 16, l ^ 48] if (on[l] and l < 16) else ([l, l ^ 32] if (on[l] and l < 32) else [l])
                        want, found = chk.bestk_sorted([key for g in grp for row in steps for o, key in [row[g]] if o], k)
                        assert got[l][0] == want and got[l][2] == found, (kmax, k, L, w, l)
                        if on[l]:
                            assert got[l][1] == got[l & 15][1] == (got[l & 15][0][k - 1] if got[l & 15][2] == k else chk.INF_KEY)
                        caught += short[l][0] != want
                        checked += 1
    assert caught > 1000
    print("BestK serial against sorted: %d lanes" % checked)


@pytest.mark.parametrize("S", (1, 4))
def test_cluster_and_walk_restatements_cover_their_boxes(S):
    """every open lane is in one cluster, its ball box lies inside its cluster's box, and a cluster's members are within 8 x 4 x 4 cells of its first; the walk
    restated from a cell_start built here deals every position of the box to exactly one lane of the group"""
    for name in ("seams", "slabs"):
        g = sc.grid(name); pts = sc.cloud(name)
        Q, R, T = sc.cluster_waves(name, S)
        tiled = 0
        for w in range(len(Q)):
            cid, cl = chk.clusters_restated(g, Q[w], R[w], T[w], S)
            assert ((cid >= 0) == T[w]).all() and set(cid[T[w]]) == set(range(len(cl)))
            bb = chk.ball_box(g, Q[w], R[w]); c = g.cells(Q[w])
            for l in np.flatnonzero(T[w]):
                box = cl[cid[l]][0]
                assert all(box[2 * a] <= bb[l][2 * a] and bb[l][2 * a + 1] <= box[2 * a + 1] for a in range(3))
                first = c[np.flatnonzero(cid == cid[l])[0]]
                assert (np.abs(c[l] - first) <= (8, 4, 4)).all()
            tiled += any(t for _, t in cl)
        assert tiled >= 1 or name == "seams"
        order = np.argsort(g.cell_key(g.cells(pts)), kind="stable")
        cs = np.searchsorted(g.cell_key(g.cells(pts))[order], np.arange(g.ncells + 1))
        q, r, on = sc.ball_queries(name)
        for i in range(0, len(q), 7):
            one, nseg = chk.ball_walk_restated(g, cs, q[i], r[i], 1)
            assert sorted(order[one[0]]) == list(chk.box_points(g, pts, chk.ball_box(g, q[i], r[i])))
            for fg in (8, 16):
                lanes, _ = chk.ball_walk_restated(g, cs, q[i], r[i], fg)
                assert sorted(u for l in lanes for u in l) == sorted(one[0])


def test_row_split_by_reciprocal_is_exact():
    """the row -> (y, z) split of for_each_in_ball_cells_group_pre: (int)(((float)r + 0.5f) * (1.0f / ny)) == r / ny for every ny <= 80, r < 80 (its 80-entry
    table) and well beyond"""
    ny, r = np.meshgrid(np.arange(1, 200), np.arange(4096), indexing="ij")
    assert (chk.row_split_f32(r, ny) == r // ny).all()
    wrong = ((r.astype(np.float32)) * (F(1.0) / ny.astype(np.float32))).astype(np.int64)                       # without the half: caught
    assert (wrong != r // ny).any()


def test_brute_force_orders_ties_by_index_and_excludes_only_the_winner():
    pts = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [3, 0, 0]], dtype=np.float32)
    t = chk.brute_force(np.zeros((1, 3), dtype=np.float32), pts)
    assert int(t[0][0]) == (chk.b1(1.0) << 32) | 0 and t[2][0] == 1.0 and t[3][0] == 1.0
    assert chk.distance_to_the_others(t, [0])[0] == 1.0 and chk.distance_to_the_others(t, [-1])[0] == 1.0
    t = chk.brute_force(np.array([[3, 0, 0]], dtype=np.float32), pts)
    assert int(t[0][0]) == 4 and chk.distance_to_the_others(t, [4])[0] == 2.0 and chk.distance_to_the_others(t, [0])[0] == 0.0


def test_grid_restatement_has_the_dimensions_the_cases_are_built_for():
    assert tuple(sc.grid("seams").dims) == (17, 9, 9) and tuple(sc.grid("shifted").dims) == (17, 9, 9) and tuple(sc.grid("slabs").dims) == (40, 16, 16)
    for name in sc.CLOUDS:
        g = sc.grid(name)
        c = g.cells(sc.cloud(name))
        assert (c >= 0).all() and (c < g.dims).all() and len(np.unique(g.cell_key(c))) > 50
        assert len(sc.cloud(name)) <= 4000 and len(sc.queries(name)) <= 2000
    d = sc.cloud("seams")
    assert len(d) - len(np.unique(d, axis=0)) >= 40                   # exact duplicates


def test_device_entry_is_exported_wrapped_and_refuses_a_null_context():
    from qn_amd import engine
    import test_capi_symbols
    assert "qn_debug_search" in test_capi_symbols.declared_symbols() and callable(engine.Context.debug_search)
    L = engine.lib()
    L.qn_debug_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    a = np.ones(256, dtype=np.uint32); out = np.full(256, 7, dtype=np.uint32)
    for which in range(8):
        assert L.qn_debug_search(None, which, 1, a.ctypes.data_as(C.c_void_p), 1, 1, out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert (out == 7).all()


def test_no_product_path_calls_the_debug_entry():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-lio-sam-qn_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".cuh", ".h", ".inc")))
    text = {f: re.sub(r"//.*", "", open(os.path.join(csrc, f)).read()) for f in names}
    assert {f for f, t in text.items() if "debug_launch_search" in t} == {"qn_engine.hip", "qn_search_debug.hip"}
    assert {f for f, t in text.items() if "qn_debug_search" in t} == {"qn_engine.hip"} and text["qn_engine.hip"].count("qn_debug_search") == 1
    assert {f for f, t in text.items() if re.search(r"\bk_dbg_\w+", t)} == {"qn_search_debug.hip"}
