"""The occupancy edge cases (tests/occupancy_edge_cases.py) on the CPU: the vectorised twin mo.classify against a scalar restatement of the specification written
here (one record at a time, its own f32 and f64 arithmetic in the documented order, mo.walk - held to exact rationals by test_map_occupancy_twin.py - for the
path, dicts for the counts); every `expect` statement against the twin; and, per knife-edge case, the evidence that it tells the named mistake from the
specification: the restatement with ONE operation changed (a contracted d2, a contracted transform, round-half-away, truncation, ties to the highest axis, a
32-bit class product) gives other counts or other voxels on exactly the records built for it.  No GPU."""
import math
import os
import sys
import numpy as np
import pytest
from qn_amd import mapoccupancy as mo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_edge_cases as oc

F = np.float32
ALL = [c.name for c in oc.all_cases()]


def walk_ties_high(A, B):
    """mo.walk with one change: a tie goes to the HIGHEST axis"""
    c = [a >> oc.S for a in A]; cend = [b >> oc.S for b in B]
    s = [(b > a) - (b < a) for a, b in zip(A, B)]
    D = [abs(b - a) for a, b in zip(A, B)]
    rem = [abs(e - k) for e, k in zip(cend, c)]
    r = [(((c[k] + 1) << oc.S) - A[k]) if s[k] > 0 else (A[k] - (c[k] << oc.S)) for k in range(3)]
    out = [tuple(c)]
    for _ in range(sum(rem)):
        best = -1
        for k in range(3):
            if rem[k] > 0 and (best < 0 or r[k] * D[best] <= r[best] * D[k]):
                best = k
        c[best] += s[best]; r[best] += oc.ONE; rem[best] -= 1
        out.append(tuple(c))
    return out


def restate(case, d2="plain", row="plain", half="even", cell="floor", ties="low", product_bits=64):
    """the specification, one record at a time -> dict(status per record, n per record (-1: no ray), ends per ray, hits, misses (dicts), cnt, classes (dict)).
    The keyword arguments name the ONE operation done differently (the defaults are the specification)."""
    p = case.params
    lo2, hi2 = F(np.float64(p.min_range) * np.float64(p.min_range)), F(np.float64(p.max_range) * np.float64(p.max_range))
    inv = 1.0 / float(p.voxel)

    def fixed(w):
        t = w * inv
        if not abs(t) < 1048576.0:
            raise mo.CapacityError("a ray end of 2^20 voxels or more from the origin")
        q = t * 1024.0
        return round(q) if half == "even" else int(math.copysign(math.floor(abs(q) + 0.5), q))           # (round(): half to even, exact on a float)
    vox = (lambda a: a >> oc.S) if cell == "floor" else (lambda a: int(a / 1024))                        # (int(): towards zero)
    status, steps, ends, hits, misses = [], [], [], {}, {}
    for cloud, T in zip(case.clouds, case.poses):
        P = [[float(v) for v in T[k]] for k in range(3)]
        A = None
        for rec in cloud:
            x, y, z = F(rec[0]), F(rec[1]), F(rec[2])
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                status.append(oc.ST_NONFINITE); steps.append(-1); continue
            if d2 == "plain":
                with np.errstate(over="ignore"):
                    v = (x * x + y * y) + z * z                                                          # f32 scalars: every operation rounded to f32
            else:
                v = oc.d2_form(rec, d2)
            if v < lo2 or v > hi2:
                status.append(oc.ST_NEAR if v < lo2 else oc.ST_FAR); steps.append(-1); continue
            xd, yd, zd = float(x), float(y), float(z)
            if row == "plain":
                W = [((P[k][0] * xd + P[k][1] * yd) + P[k][2] * zd) + P[k][3] for k in range(3)]
            else:
                W = [float(oc.row_form(P[k], rec, row)) for k in range(3)]
            if A is None:
                A = [fixed(P[k][3]) for k in range(3)]
            B = [fixed(w) for w in W]
            cA, cB = tuple(vox(a) for a in A), tuple(vox(b) for b in B)
            status.append(oc.ST_RAY); ends.append((tuple(A), tuple(B)))
            hits[cB] = hits.get(cB, 0) + 1
            if cell != "floor":
                steps.append(sum(abs(b - a) for a, b in zip(cA, cB))); continue                          # (no walk is defined on truncated voxels: the hits alone)
            path = mo.walk(A, B) if ties == "low" else walk_ties_high(A, B)
            n = len(path) - 1
            assert path[0] == cA and path[-1] == cB
            steps.append(n)
            for i in range(max(n - int(p.shell), 0)):
                misses[path[i]] = misses.get(path[i], 0) + 1
    cnt = [len(status)] + [status.count(k) for k in (oc.ST_RAY, oc.ST_NONFINITE, oc.ST_NEAR, oc.ST_FAR)]
    mask = (1 << product_bits) - 1
    classes = {}
    for v in set(hits) | set(misses):
        h, m = hits.get(v, 0), misses.get(v, 0)
        classes[v] = oc.OCCUPIED if h >= p.min_hits and ((h * p.hit_weight) & mask) >= m else oc.FREE     # (h or m is not 0 here; every other voxel is UNKNOWN)
    return dict(status=status, n=steps, ends=ends, hits=hits, misses=misses, cnt=cnt, classes=classes)


def dense(r):
    """the restatement's dicts as the twin's arrays -> (hits, misses, classes, minc)"""
    if not r["ends"]:
        z = np.zeros((0, 0, 0), np.uint32)
        return z, z, z.astype(np.uint8), (0, 0, 0)
    cs = np.array([[a >> oc.S for a in A] for A, _ in r["ends"]] + [[b >> oc.S for b in B] for _, B in r["ends"]])
    lo, hi = cs.min(axis=0), cs.max(axis=0)
    shape = tuple(int(v) for v in (hi - lo + 1)[::-1])
    out = []
    for d, t in ((r["hits"], np.uint32), (r["misses"], np.uint32), (r["classes"], np.uint8)):
        a = np.zeros(shape, t)
        for (x, y, z), c in d.items():
            a[z - lo[2], y - lo[1], x - lo[0]] = c
        out.append(a)
    return out[0], out[1], out[2], tuple(int(v) for v in lo)


@pytest.mark.parametrize("name", [n for n in ALL if n not in oc.SLOW_TWIN])
def test_the_twin_equals_the_scalar_restatement(name):
    case = oc.get(name)
    want = oc.twin(name)
    r = restate(case)
    hits, misses, classes, minc = dense(r)
    s = want["stats"]
    assert [s.n_records, s.n_rays, s.n_nonfinite, s.n_near, s.n_far] == r["cnt"]
    assert want["grid"].minc == minc and want["hits"].shape == hits.shape
    assert np.array_equal(want["hits"], hits) and np.array_equal(want["misses"], misses) and np.array_equal(want["classes"], classes)
    assert (s.total_hits, s.total_misses) == (sum(r["hits"].values()), sum(r["misses"].values()))
    assert (s.occupied, s.free, s.unknown) == (int((classes == 2).sum()), int((classes == 1).sum()), int((classes == 0).sum()))
    if "rays" in case.meta:                                          # the exact ends are the integers they were built from
        built = [(A, tuple(int(v) for v in b)) for A, B in case.meta["rays"] for b in B]
        assert r["ends"] == built


@pytest.mark.parametrize("name", ALL)
def test_every_expectation_holds_for_the_twin(name):
    case = oc.get(name)
    r = oc.twin(name)
    oc.holds(case, r["hits"], r["misses"], r["classes"], r["stats"]._asdict(), r["grid"].minc)
    if "rays" in case.meta and name not in oc.SLOW_TWIN:
        A, B, _ = mo.rays(case.clouds, case.poses, case.params)
        assert np.array_equal(B, np.concatenate([b for _, b in case.meta["rays"]])) and np.array_equal(A, np.concatenate([np.tile(a, (len(b), 1)) for a, b in case.meta["rays"]]))
    for mask in oc.MASKS:                                            # the list and the slices of the twin, against their definitions on the dense arrays
        ijk, h, m = mo.voxel_list(r, mask)
        keep = ((mask >> r["classes"].astype(np.int64)) & 1) == 1
        assert len(ijk) == keep.sum() and np.array_equal(h, r["hits"][keep]) and np.array_equal(m, r["misses"][keep])
    for lo, hi in oc.slice_ranges(r["classes"].shape[0]):
        got = mo.slice2d(r["classes"], lo, hi)
        a, b = max(lo, 0), min(hi, r["classes"].shape[0] - 1)
        assert np.array_equal(got, r["classes"][a:b + 1].max(axis=0) if a <= b else np.zeros(r["classes"].shape[1:], np.uint8))


def test_refusals_on_the_twin_and_the_restatement():
    for ref in oc.refusals():
        with pytest.raises(mo.CapacityError) as ei:
            mo.classify(ref.clouds, ref.poses, ref.params)
        assert ref.message in str(ei.value), (ref.name, str(ei.value))
        if ref.message == oc.RAY_END:
            with pytest.raises(mo.CapacityError):
                restate(oc.Case(ref.name, ref.clouds, range(len(ref.clouds)), ref.poses, ref.params, {}))
    # the record that is refused is the last one alone: without it the entry is accepted
    ref = [r for r in oc.refusals() if r.name.startswith("one-record")][0]
    ok = mo.classify([ref.clouds[0][:-1]], ref.poses, ref.params)
    assert ok["stats"].n_rays == 4 * oc.OC_BLOCK and len(ref.clouds[0]) == 4 * oc.OC_BLOCK + 1


# ---- the table is the one intended
def test_octants_hold_every_sign_pattern_kind_and_origin():
    case = oc.get("octants/shell-0")
    rays = case.meta["rays"]
    signs = {tuple(int(v) for v in np.sign(b - np.asarray(A))) for A, B in rays for b in B}
    assert len(signs) == 27 and len(rays) == 48
    on_corner = [all(a % oc.ONE == 0 for a in A) for A, _ in rays]
    assert sum(on_corner) == 16
    assert {len(B) for _, B in rays} >= {64, 65, 255, 256, 257} and all(64 <= len(B) <= 257 for _, B in rays)
    cA = np.array([oc.cell(A) for A, _ in rays]); allB = np.concatenate([B for _, B in rays])
    assert (cA < 0).any() and (cA > 0).any() and (allB < 0).any() and (allB > 0).any()             # both sides of zero
    assert sum(bool((b == np.asarray(A)).all()) for A, B in rays for b in B) >= 48                  # B == A
    on_lattice = (allB % oc.ONE == 0)
    assert on_lattice.all(axis=1).sum() > 100 and (on_lattice.sum(axis=1) == 2).sum() > 100 and (on_lattice.sum(axis=1) == 1).sum() > 100      # corners, edges, faces
    d = np.concatenate([np.abs(B - np.asarray(A)) for A, B in rays])
    assert ((d[:, 0] == d[:, 1]) & (d[:, 1] == d[:, 2]) & (d[:, 0] > 0)).sum() > 100 and ((d[:, 0] == d[:, 1]) & (d[:, 0] > 0) & (d[:, 2] != d[:, 0])).sum() > 100
    # from a corner every axis heading down has r = 0
    A, B = next((A, B) for (A, B), c in zip(rays, on_corner) if c)
    assert mo.walk(A, [a - 3 * oc.ONE for a in A])[1] == tuple(a // oc.ONE - (k == 0) for k, a in enumerate(A))
    assert oc.get("octants/shell-1").params.shell == 1 and oc.get("octants/shell-1").expect["stats"]["total_misses"] < case.expect["stats"]["total_misses"]


def test_fold_lanes_layout():
    case = oc.get("fold-lanes")
    r = restate(case)
    shell = case.params.shell
    assert len(case.keyframes) == 2 and all(len(k) == 4 * oc.WAVE + 1 for k in case.keyframes) and case.params.min_range > 0
    for e in range(2):
        st = np.array(r["status"][e * 257:(e + 1) * 257]); n = np.array(r["n"][e * 257:(e + 1) * 257])
        assert np.array_equal(st, case.meta["status"][e]) and np.array_equal(n, case.meta["n"][e])
        w = [slice(64 * k, 64 * k + 64) for k in range(4)]
        assert st[0] == oc.ST_NONFINITE and (st[1:64] == oc.ST_RAY).all() and (n[1:63] == 0).all() and n[63] > shell        # lane 63 alone carves
        assert (st[w[1]] == oc.ST_RAY).all() and (n[w[1]] > shell).all()
        assert (st[w[2]] != oc.ST_RAY).all() and {oc.ST_NONFINITE, oc.ST_NEAR, oc.ST_FAR} == set(st[w[2]].tolist())
        assert (st[w[3]] == oc.ST_RAY).all() and (n[w[3]][0::2] == shell).all() and (n[w[3]][1::2] == shell + 1).all()
        assert st[256] == oc.ST_RAY and n[256] == 75
    v0 = list(case.expect["misses_at"])
    assert v0[0] != v0[1] and all(r["misses"][v] == 98 for v in v0)
    # the skipped records are well off the bounds: no contracted form changes a status
    for f in oc.D2_FORMS[1:]:
        assert restate(case, d2=f)["status"] == r["status"]


def test_many_entries_table():
    case = oc.get("many-entries")
    assert len(case.ids) == oc.SV_CHUNK + 3 and len(case.keyframes) == 3 and sorted(len(k) for k in case.keyframes) == [1, 2, 3]
    assert case.meta["tiles"] > oc.MO_SCAN_BLOCK * 32 and case.expect["stats"]["n_records"] == case.meta["records"]
    assert len({p.tobytes() for p in case.poses}) == oc.MANY_POSES + 3 and oc.SV_CHUNK % oc.MANY_POSES != 0
    r = oc.twin("many-entries")
    minc = r["grid"].minc
    assert len(case.meta["last"]) >= 3 and all(r["hits"][z - minc[2], y - minc[1], x - minc[0]] == 1 for x, y, z in case.meta["last"])


def test_shell_and_cell_seam_tables():
    assert [oc.get("shell/%d" % s).params.shell for s in oc.SHELLS] == [0, 3, 6, 7, 0xFFFFFFFF]
    assert [oc.get("shell/%d" % s).expect["stats"]["total_misses"] for s in oc.SHELLS] == [105, 30, 0, 0, 0]       # sum over n = 0 .. 6 of 5 max(n - shell, 0)
    sides = [c.expect["sides"] for c in oc.group("cell-seams")]
    assert sides == [(17, 15, 1), (16, 16, 1), (257, 1, 1), (16, 16, 3)] and len(oc.slice_ranges(3)) == 6 + 5


# ---- each knife-edge case distinguishes what it claims to
def test_range_gates_tell_a_contracted_d2():
    case = oc.get("range-gates")
    plain = restate(case)
    assert np.array_equal(plain["status"], case.meta["status"]) and set(case.meta["kinds"]) == set(oc.GATE_KINDS)
    for f in oc.D2_FORMS[1:]:
        other = restate(case, d2=f)
        changed = [i for i, (a, b) in enumerate(zip(plain["status"], other["status"])) if a != b]
        assert changed == case.meta["beaten"][f] and len(changed) >= 2, (f, changed)
        assert other["cnt"] != plain["cnt"] or other["hits"] != plain["hits"], f
        both = {case.meta["kinds"][i] for i in changed}
        assert both & {"on-lo", "on-hi"}, (f, both)                  # a kept record that the contracted form skips
    assert {k for f in oc.D2_FORMS[1:] for i in case.meta["beaten"][f] for k in [case.meta["kinds"][i]]} == set(oc.GATE_KINDS)
    off_axes = case.keyframes[0][:len(case.meta["kinds"])]
    assert (off_axes != 0).all()


def test_quantise_tells_half_away_truncation_and_a_contracted_transform():
    case = oc.get("quantise/halves")
    even = restate(case)
    assert [B[0] for _, B in even["ends"]] == list(oc.HALF_B) == list(case.meta["B_x"])
    away = restate(case, half="away")
    assert [B[0] for _, B in away["ends"]] == [1, 2, 3, -1, -2, 1024, -1025]
    moved = set(even["hits"]) ^ set(away["hits"])
    assert moved == {(0, 3, 0), (-1, 3, 0), (-1, 6, 0), (-2, 6, 0)}                                # k = -1 and k = -1025 end in the voxel below
    trunc = restate(case, cell="trunc")
    assert set(even["hits"]) ^ set(trunc["hits"]) == {(-1, 4, 0), (0, 4, 0)}                         # k = -2: B = -2 is voxel -1, not 0
    # the origin at -0.3 with voxel 0.3: fixed point -1024 exactly, voxel -1, three steps from the end's voxel 0
    case = oc.get("quantise/-0.3")
    assert restate(case)["ends"][0][0] == (-1024,) * 3 and restate(case)["n"] == [3]
    # the transform that lands on 1023.5
    case = oc.get("quantise/transform")
    plain = restate(case)
    assert all(B[0] == 1024 for _, B in plain["ends"]) and plain["hits"] == {(1, 1, 0): len(case.ids)}
    for f in oc.T_FORMS[1:]:
        other = restate(case, row=f)
        below = [i for i, (_, B) in enumerate(other["ends"]) if B[0] == 1023]
        assert below == case.meta["beaten"][f] and len(below) >= 3, (f, below)
        assert other["hits"].get((1, 1, 0), 0) == len(case.ids) - len(below) and other["hits"][(0, 1, 0)] == len(below)
        assert all(sum(abs(float(v)) > 0 for v in T[0, :3]) == 2 for T in case.poses)


def test_walks_tell_truncation_and_ties_to_the_highest_axis():
    for name in ("hand-walks/-x-y-z", "hand-walks/xz-in-step"):
        case = oc.get(name)
        low, high = restate(case), restate(case, ties="high")
        assert [v for v in case.meta["path"][:-1]] == sorted(low["misses"], key=case.meta["path"].index) and low["misses"] != high["misses"], name
    case = oc.get("hand-walks/from-a-face-down")                     # no tie on this one: the same path either way
    assert restate(case)["misses"] == restate(case, ties="high")["misses"] == {v: 1 for v in case.meta["path"][:-1]}
    case = oc.get("octants/shell-0")
    low, high, trunc = restate(case), restate(case, ties="high"), restate(case, cell="trunc")
    diff = sum(low["misses"].get(v, 0) != high["misses"].get(v, 0) for v in set(low["misses"]) | set(high["misses"]))
    assert diff > 100 and low["hits"] == high["hits"]
    assert low["hits"] != trunc["hits"] and low["hits"] == case.expect["hits"]


def test_class_rule_tells_a_32_bit_product():
    for case in oc.group("class-rule"):
        r64, r32 = restate(case), restate(case, product_bits=32)
        at = [(3 * j + 1, 0, 0) for j in range(len(oc.CLASS_TARGETS))]
        assert [(r64["hits"].get(v, 0), r64["misses"].get(v, 0)) for v in at] == oc.CLASS_TARGETS
        assert [r64["classes"][v] for v in at] == oc.CLASS_RULES[(case.params.min_hits, case.params.hit_weight)]
        wrong = [j for j, v in enumerate(at) if r64["classes"][v] != r32["classes"][v]]
        assert wrong == ([4, 7] if case.params.hit_weight == 1 << 31 else []), (case.name, wrong)        # (2, 9) and (2, 1): 2 * 2^31 is 0 in 32 bits


def test_shell_at_the_top_of_its_type():
    for s in (6, 7, 0xFFFFFFFF):
        r = restate(oc.get("shell/%d" % s))
        assert not r["misses"] and set(r["classes"].values()) == {oc.OCCUPIED}
    r = oc.twin("shell/4294967295")
    assert r["stats"].free == 0 and r["stats"].occupied == len(oc.get("shell/0").expect["hits"])
