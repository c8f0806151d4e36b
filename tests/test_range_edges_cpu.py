"""The numpy twins of the range-image family (qn_amd/freespace.py, qn_amd/staticmap.py) on the edge cases of tests/range_edge_cases.py, without a GPU:
  - against a scalar restatement of their specification (plain Python floats, one point at a time, the bisections as the docstring of freespace.py writes
    them) on every cloud of every case: images, classes and counts of both directions, votes and removed flags;
  - against what the generators state by construction: classes, counts, votes, occupied pixels, kept records;
  - and the generators against what they claim: the knife-edge points change the predicate of their own edge when one expression is rounded once instead of
    twice, which is the only thing a contracted (fused multiply-add) build does differently.

Shares measured here with exact rationals (tests below re-measure and require at least half of each, and never less than 5 %):
  column boundary, c[j] y - s[j] x rounded once:   32.1 % at 32 x 720 (2891 of 9000 points), 32.5 % at 2 x 4608 (2924 of 9000)
  row edge, rho2 = x x + y y rounded once:         14.5 % at 32 x 720 (1101 of 7600), 7.8 % at 2 x 4608 (596 of 7600)
The row-edge construction as first described (radii not selected) gave 4.3 % (323 of 7600) and 2.8 % (213 of 7600): rho takes half of rho2's relative error
and the product rho t[i] rounds once more, so few points stay within the last bit.  knife() therefore picks up to 40 of each pair's 200 radii from a pool of
1024 by that very predicate.  The scalar restatement runs once per distinct (record, transform): tiled and repeated records are evaluated once."""
import math
import os
import sys
import numpy as np
import pytest
from qn_amd import freespace as fs, scancontext as sc, staticmap as sm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import range_edge_cases as rc

FIELDS = ("n", "n_finite", "in_fov", "observed", "seen_through", "occluded", "agree")


# ---- the specification, one point at a time
def s_tables(p):
    nr, nc, lo, hi = int(p.n_rows), int(p.n_cols), float(p.el_lo), float(p.el_hi)
    return ([math.tan(lo + float(i) * (hi - lo) / nr) for i in range(nr + 1)], [math.cos(2.0 * math.pi * j / nc) for j in range(nc)],
            [math.sin(2.0 * math.pi * j / nc) for j in range(nc)])


def s_project(x, y, z, p, tabs):
    """-> (finite, kept, row, col, r)"""
    t, c, s = tabs
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return False, False, 0, 0, 0.0
    rho2 = x * x + y * y
    rho = math.sqrt(rho2)
    r = math.sqrt(rho2 + z * z)
    lo, hi = 0, p.n_rows + 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if z >= rho * t[mid]:
            lo = mid + 1
        else:
            hi = mid
    row = lo - 1
    hp = 0 if (y > 0.0 or (y == 0.0 and x > 0.0)) else 1
    lo, hi = 1, p.n_cols
    while lo < hi:
        mid = (lo + hi) >> 1
        hb = 0 if (s[mid] > 0.0 or (s[mid] == 0.0 and c[mid] > 0.0)) else 1
        if hp > hb or (hp == hb and c[mid] * y - s[mid] * x >= 0.0):
            lo = mid + 1
        else:
            hi = mid
    return True, (r >= p.min_range and 0 <= row < p.n_rows), row, lo - 1, r


def _distinct(a):
    """-> (the distinct rows of an (n, k) array by bit pattern, the position of every row among them)"""
    a = np.ascontiguousarray(a)
    if not len(a):
        return a, np.zeros(0, np.int64)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).reshape(len(a), -1)
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    return a[first], np.asarray(inv).reshape(-1)


def s_images(cloud, p, tabs):
    near = np.full((p.n_rows, p.n_cols), np.inf, np.float32); far = np.zeros((p.n_rows, p.n_cols), np.float32)
    for x, y, z in _distinct(cloud)[0].astype(np.float64).tolist():
        fin, keep, row, col, r = s_project(x, y, z, p, tabs)
        if keep:
            with np.errstate(over="ignore"):
                r32 = np.float32(r)
            near[row, col] = min(near[row, col], r32); far[row, col] = max(far[row, col], r32)
    return near, far


def s_class(x, y, z, near, far, p, tabs):
    """-> (class, finite) of a point in the images' frame"""
    fin, keep, row, col, r = s_project(x, y, z, p, tabs)
    if not keep:
        return 0, fin
    rn, rf = math.inf, 0.0
    for dr in range(-p.window_rows, p.window_rows + 1):
        if 0 <= row + dr < p.n_rows:
            for dc in range(-p.window_cols, p.window_cols + 1):
                rn = min(rn, float(near[row + dr, (col + dc) % p.n_cols])); rf = max(rf, float(far[row + dr, (col + dc) % p.n_cols]))
    tol = p.tol_abs + p.tol_rel * r
    if rn == math.inf:
        return 1, fin
    if r + tol < rn:
        return 2, fin
    if r > rf + tol:
        return 3, fin
    return 4, fin


def s_direction(cloud, T, near, far, p, tabs):
    """every record through T, ((T0 x + T1 y) + T2 z) + T3 in Python floats -> (classes, finite)"""
    M = [[float(v) for v in row] for row in np.asarray(T, np.float64)]
    u, inv = _distinct(cloud)
    out = []
    for x, y, z in u.astype(np.float64).tolist():
        q = [((M[k][0] * x + M[k][1] * y) + M[k][2] * z) + M[k][3] for k in range(3)]
        out.append(s_class(q[0], q[1], q[2], near, far, p, tabs))
    out = np.array(out, np.int64).reshape(-1, 2)[inv]
    return out[:, 0].astype(np.uint8), out[:, 1].astype(bool)


def s_removed(st, ag, rule):
    return np.array([int(a) >= rule[0] and int(a) > rule[1] * int(b) for a, b in zip(st, ag)], bool)


_TWIN = {}


def twin(name):
    """the twin's images, pair records and votes of a case, computed once"""
    if name not in _TWIN:
        case = rc.get(name)
        im = rc.twin_images(case)
        _TWIN[name] = dict(images=im, pairs=rc.twin_pairs(case, im), votes=rc.twin_votes(case, im) if case.entries else None)
    return _TWIN[name]


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_twin_equals_the_scalar_restatement(name):
    case, tw = rc.get(name), twin(name)
    p, tabs = case.params, s_tables(case.params)
    t, c, s = fs.tables(p)
    assert t.tolist() == tabs[0] and c.tolist() == tabs[1] and s.tolist() == tabs[2]
    images = [s_images(cl, p, tabs) for cl in case.clouds]
    for k, (got, want) in enumerate(zip(tw["images"], images)):
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, "image", k)
    for j, (q, cd, T) in enumerate(case.pairs):
        for d, (src, img, M) in enumerate(((q, cd, T), (cd, q, fs.inverse(T)))):
            cls, fin = s_direction(case.clouds[src], M, images[img][0], images[img][1], p, tabs)
            assert np.array_equal(tw["pairs"][j][d]["classes"], cls), (name, j, d, np.flatnonzero(tw["pairs"][j][d]["classes"] != cls)[:8])
            want = rc.counts_of(cls, fin)
            assert {f: tw["pairs"][j][d][f] for f in FIELDS} == want, (name, j, d)
    if case.entries:
        e = case.entries
        ids, off, wit = [int(i) for i in e["ids"]], e["wit_off"], e["wit"]
        memo = {}
        for k in range(len(ids)):
            ws = [int(w) for w in wit[off[k]:off[k + 1]]]
            key = (ids[k], np.asarray(e["poses"][k]).tobytes(), tuple((ids[w], np.asarray(e["poses"][w]).tobytes()) for w in ws))
            if key not in memo:
                st = np.zeros(len(case.clouds[ids[k]]), np.int64); ag = st.copy()
                pair = {}
                for w in ws:
                    pk = (ids[w], np.asarray(e["poses"][w]).tobytes())
                    if pk not in pair:
                        M = sc.relative_pose(e["poses"][w], e["poses"][k])
                        pair[pk] = s_direction(case.clouds[ids[k]], M, images[ids[w]][0], images[ids[w]][1], p, tabs)[0]
                    st += pair[pk] == 2; ag += pair[pk] == 4
                memo[key] = (st, ag)
            st, ag = memo[key]
            assert np.array_equal(tw["votes"][k][0], st) and np.array_equal(tw["votes"][k][1], ag), (name, "votes", k)
            for rule in case.rules:
                assert np.array_equal(sm.removed(st, ag, sm.StaticParams(*rule)), s_removed(st, ag, rule)), (name, k, rule)


@pytest.mark.parametrize("name", rc.NAMES)
def test_the_twin_gives_what_the_generators_state(name):
    case, tw = rc.get(name), twin(name)
    p = case.params
    stated = 0
    for (j, d), cls in case.expect["cls"].items():
        got = tw["pairs"][j][d]
        assert np.array_equal(got["classes"], cls), (name, j, d, np.flatnonzero(got["classes"] != cls)[:8])
        assert {f: got[f] for f in FIELDS} == rc.counts_of(cls, case.meta["finite"][(j, d)]), (name, j, d)
        stated += len(cls)
    for k, (st, ag) in case.expect["votes"].items():
        assert np.array_equal(tw["votes"][k][0], st) and np.array_equal(tw["votes"][k][1], ag), (name, "votes", k)
        stated += len(st)
    for kf, (pix, near, far) in case.expect["pixels"].items():
        gn, gf = tw["images"][kf]
        assert np.array_equal(np.isfinite(gn), pix) and np.array_equal(gf > 0, pix), (name, "pixels", kf)
        assert np.allclose(gn[pix], near[pix], rtol=1e-5, atol=0) and np.allclose(gf[pix], far[pix], rtol=1e-5, atol=0), (name, "ranges", kf)
    for kf, kept in case.expect["kept"].items():
        assert np.array_equal(fs.project(case.clouds[kf].astype(np.float64), p)[4], kept), (name, "kept", kf)
        stated += len(kept)
    for (j, d), dropped in case.meta.get("dropped", {}).items():
        assert np.array_equal(tw["pairs"][j][d]["classes"] == 0, dropped), (name, j, d)
    if not name.startswith(("knife", "subnormals")):              # (those two are held to the scalar restatement and to the flip shares instead)
        assert stated > 0, name


def test_every_class_and_every_dropped_kind_is_in_the_seam_patterns():
    case = rc.get("seams")
    for n in rc.SEAM_COUNTS[1:]:
        assert set(rc.mixed(n, n).tolist()) == {0, 1, 2, 3, 4}, n
    a, e = rc.pattern_records(rc.EDGE, rc.mixed(65, 65))
    drop = a[e["cls"] == 0].astype(np.float64)
    assert np.isnan(drop).any(1).sum() >= 2 and (np.hypot(drop[:, 0], drop[:, 1]) == 0).sum() >= 2
    assert [len(c) for c in case.clouds[1::7]] == rc.SEAM_COUNTS
    for n, name, want in ((4097, "first-of-tile", [0, 2048, 4096]), (4097, "last-of-tile", [2047, 4095, 4096]), (513, "one-wave", list(range(64, 128))), (64, "none", [])):
        assert np.flatnonzero(rc.removal(n, name) == 2).tolist() == want, (n, name)


def test_the_launch_seams_are_crossed():
    scan = rc.get("scan-tiles")
    nt = scan.meta["tiles"]
    chunk = (nt + rc.SV_SCAN_BLOCK - 1) // rc.SV_SCAN_BLOCK
    assert chunk == 3 and nt % chunk != 0 and (nt + chunk - 1) // chunk < rc.SV_SCAN_BLOCK      # chunk >= 2, a ragged last range, threads with none
    sizes = [len(scan.clouds[i]) for i in scan.entries["ids"]]
    assert sizes.count(0) > 20 and sizes.count(1) > 500 and sizes.count(rc.FS_TILE + 1) == 1 and len(set(scan.entries["ids"])) == 5
    assert len(rc.get("many-entries").entries["ids"]) == rc.SV_CHUNK + 3
    red = rc.get("reduce-tiles")
    assert (len(red.clouds[1]) + rc.FS_TILE - 1) // rc.FS_TILE == rc.REDUCE_SLOTS + 1
    full = rc.get("full-counters")
    assert int(np.diff(full.entries["wit_off"]).max()) == rc.MAX_WITNESSES == sm.MAX_WITNESSES
    assert int(full.expect["votes"][0][0].max()) == 255 and int(full.expect["votes"][0][1].max()) == 255
    st, ag = (v.astype(np.int64) for v in full.expect["votes"][1])
    assert ((st > 0) & (ag > 0)).any()                             # a record with both counters running: the rules' product is at work
    for rule in full.rules:
        rm = s_removed(st, ag, rule)
        assert rm.any() and not rm.all(), rule


@pytest.mark.parametrize("name,col_min,row_min", [("knife-32x720", 0.20, 0.0725), ("knife-2x4608", 0.1625, 0.05)])
def test_the_knife_edge_points_sit_on_their_edges(name, col_min, row_min):
    """a condition on the inputs, with exact rationals: the share of points whose own boundary's / own edge's predicate depends on the last rounding"""
    case = rc.get(name)
    assert len(case.pairs) >= 32 and all(len(case.clouds[q]) == 200 for q, _, _ in case.pairs)
    nc, nr = case.params.n_cols, case.params.n_rows
    assert {1, nc // 4, nc // 2, nc - 1} <= {j for j, _, _ in case.meta["edges"]} and {0, nr // 2, nr} == {i for _, i, _ in case.meta["edges"]}
    cf, cn = rc.column_flip_share(case)
    rf, rn = rc.row_flip_share(case)
    print(name, "column flips %d of %d (%.1f %%)" % (cf, cn, 100.0 * cf / cn), "row flips %d of %d (%.1f %%)" % (rf, rn, 100.0 * rf / rn))
    assert cf >= col_min * cn and rf >= row_min * rn
    # the controls pushed off the row edge by tau: none of them flips
    t = fs.tables(case.params)[0]
    for (q, _, T), (j, i, shift) in zip(case.pairs, case.meta["edges"]):
        if shift == 2:
            assert not rc.row_flips(fs.transform(case.clouds[q], T), t[i]).any(), (j, i)
    # and the points of a pair fall on both sides of their edges: more than one class in nearly every pair (where sin or cos is exactly 1 the products are
    # exact and every point sits ON the edge, on one side by the definition)
    tw = twin(name)
    split = [len(set(tw["pairs"][k][0]["classes"].tolist())) >= 2 for k, (_, _, shift) in enumerate(case.meta["edges"]) if shift != 2]
    assert sum(split) >= 0.75 * len(split), (sum(split), len(split))


def test_zero_tolerance_yields_every_class():
    case = rc.get("zero-tolerance")
    cls = case.expect["cls"][(0, 0)]
    n = len(cls)
    im = twin("zero-tolerance")["images"][0]
    assert n == case.params.n_rows * case.params.n_cols and np.isfinite(im[0]).all() and np.array_equal(im[0], im[1])      # one return in every pixel
    share = {k: int((cls == k).sum()) / n for k in (2, 3, 4)}
    print("zero tolerance:", share, "integer triples", case.meta["exact"])
    assert share[2] >= 0.25 and share[4] >= 0.25 and share[3] > 0.1


def test_min_range_keeps_the_equal_and_drops_the_ulp_below():
    for name in ("min-range-5", "min-range-1.25", "min-range-40"):
        case = rc.get(name)
        a = case.clouds[0].astype(np.float64)
        r = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        assert (r[:12] == case.params.min_range).all() and (r[12:] < case.params.min_range).all() and (r[12:] > case.params.min_range * (1 - 1e-6)).all()
        cls = twin(name)["pairs"][0][0]["classes"]
        assert (cls[:12] != 0).all() and (cls[12:] == 0).all()


def test_a_range_beyond_f32_leaves_near_at_inf_and_far_at_inf():
    case = rc.get("beyond-f32")
    near, far = twin("beyond-f32")["images"][0]
    r, c = case.meta["inf_pixel"]
    assert near[r, c] == np.inf and far[r, c] == np.inf and int(np.isinf(far).sum()) == 1
