"""The case table of the occupancy ray carving (csrc/qn_mapoccupancy.inc: k_oc_extent, k_oc_carve<FOLD>, k_oc_classify, k_dg_list_flag / _pick and k_dg_slice of csrc/qn_dense_grid.cuh, with
k_slot_fold and k_scan_rows of csrc/qn_map_compact.cuh and sv_each_chunk of csrc/qn_staticmap.hip): deterministic inputs, each built to put records ON an edge
of the arithmetic or a seam of the launch, with what the construction itself determines stated in `expect` - never taken from the twin and never from engine
output.  tests/test_occupancy_edges_cpu.py holds the twin (qn_amd/mapoccupancy.py) to a scalar restatement of the specification and to these expectations,
and shows that each knife-edge case tells the named mistake from the specification; tests/test_gpu_occupancy_edges.py holds the engine to the twin and to
them.  Pure numpy, no GPU, no random draws (integer Weyl sequences and fixed tables).

A Case: name, keyframes (the distinct f32 record arrays), ids (per entry its keyframe), poses (per entry, 4x4 f64), params (an mo.OccupancyParams) and
`expect`; `clouds` is the per-entry view keyframes[ids[e]].  expect (every key optional):
  stats        {field of OccupancyStats: value}             minc, sides      the grid's lowest voxel and (W, H, D)
  hits         {voxel: count}, complete (0 elsewhere)       misses           {voxel: count}, complete
  misses_at    {voxel: count}, some voxels                  classes_at       {voxel: class byte}, some voxels
  no_miss      True: misses is zero everywhere and every voxel is occupied or unknown
A Refusal: clouds, poses, params and the part of the message that names what was refused.

Exact ends: with voxel 1, min_range 0 (or records well inside the gates), an identity rotation, the origin O = A / 1024 and the record (B - A) / 1024 as f32,
the fixed-point ends are exactly the integers A and B while |B - A| < 2^24 and |A|, |B| < 2^30: every quotient and the one sum O + x are exact.  For such
rays n_i = sum_k |c(B)_k - c(A)_k| with c = floor(. / 1024), total_hits = n_rays, total_misses = sum max(n_i - shell, 0), the grid follows from the extremes of
c(A) and c(B), and hits is the histogram of c(B): exact_expect() states them from the integers alone.

Seams and the constant each belongs to (restated from the sources; whoever changes one there changes it here):
  OC_BLOCK = MO_BLOCK 256   records per block of k_oc_extent / k_oc_carve, voxels per block of k_oc_classify / k_dg_list_*, columns of k_dg_slice (qn_map_compact.cuh)
  WAVE 64                   the ballot of the fold, the wave reductions of the extent
  MO_SCAN_BLOCK 1024        threads of k_slot_fold and k_scan_rows: more slots than that and a thread's stride loop runs again (qn_map_compact.cuh)
  SV_CHUNK 32768            entries per launch of k_oc_extent / k_oc_carve (qn_staticmap.hip)
  S 10                      fractional bits of the fixed point (OC_S; mapoccupancy.S)
  2^20, 2^15                OC_COORD_LIMIT voxels from the origin, OC_MAX_SIDE voxels a side (mapoccupancy.COORD_LIMIT, MAX_SIDE)"""
import functools
from fractions import Fraction
import numpy as np
from qn_amd import mapoccupancy as mo

F = np.float32
OC_BLOCK = MO_BLOCK = 256
WAVE, MO_SCAN_BLOCK, SV_CHUNK, S = 64, 1024, 32768, 10
ONE = 1 << S
COORD_LIMIT, MAX_SIDE = 1 << 20, 1 << 15
assert (S, ONE, int(mo.COORD_LIMIT), mo.MAX_SIDE) == (mo.S, mo.ONE, COORD_LIMIT, MAX_SIDE)
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
UNIT = mo.OccupancyParams(1.0, 0.0, 100.0, 0, 1, 2)                  # voxel 1, no near gate, shell 0


def wi(i, m, salt=0):
    """the i-th value of the Weyl sequence of 1/golden ratio, as an integer in [0, m)"""
    return int((((i + 1 + 7919 * salt) * 0.6180339887498949) % 1.0) * m)


def pose_at(A):
    """the identity rotation at the origin A / 1024 (A: three fixed-point integers)"""
    T = np.eye(4)
    T[:3, 3] = [a / 1024.0 for a in A]
    return T


def records_to(A, B):
    """the f32 records (B - A) / 1024 of the rays from A to the rows of B"""
    d = np.asarray(B, np.int64).reshape(-1, 3) - np.asarray(A, np.int64)
    r = (d.astype(np.float64) / 1024.0).astype(F)
    assert (r.astype(np.float64) * 1024.0 == d).all() and (np.abs(np.asarray(B, np.int64)) < 1 << 30).all() and (np.abs(np.asarray(A, np.int64)) < 1 << 30).all()
    return r


def cell(v):
    """the voxel of fixed-point integers: floor(v / 1024)"""
    return np.asarray(v, np.int64) // ONE


def exact_expect(rays, shell, skipped=(0, 0, 0)):
    """rays: [(A, B (n, 3))] of the exact-end rays of every entry; skipped: the (non-finite, near, far) records beside them -> the expectations the integers
    give (see the module docstring)"""
    cA = np.concatenate([np.broadcast_to(cell(A), (len(B), 3)) for A, B in rays])
    cB = np.concatenate([cell(B).reshape(-1, 3) for _, B in rays])
    n = np.abs(cB - cA).sum(axis=1)
    lo = np.minimum(cA.min(axis=0), cB.min(axis=0)); hi = np.maximum(cA.max(axis=0), cB.max(axis=0))
    vox, cnt = np.unique(cB, axis=0, return_counts=True)
    m = len(n)
    return dict(stats=dict(n_records=m + sum(skipped), n_rays=m, n_nonfinite=skipped[0], n_near=skipped[1], n_far=skipped[2], total_hits=m,
                           total_misses=int(np.maximum(n - int(shell), 0).sum()), width=int(hi[0] - lo[0] + 1), height=int(hi[1] - lo[1] + 1),
                           depth=int(hi[2] - lo[2] + 1)),
                minc=tuple(int(v) for v in lo), sides=tuple(int(v) for v in hi - lo + 1), hits={tuple(int(x) for x in v): int(c) for v, c in zip(vox, cnt)})


class Case:
    def __init__(self, name, keyframes, ids, poses, params, expect, meta=None):
        self.name = name
        self.keyframes = [np.ascontiguousarray(k, F).reshape(-1, 3) for k in keyframes]
        self.ids = [int(i) for i in ids]
        self.poses = np.asarray(poses, np.float64).reshape(len(self.ids), 4, 4)
        self.params = mo.OccupancyParams(*params)
        self.expect = expect
        self.meta = {} if meta is None else meta

    @property
    def clouds(self):
        return [self.keyframes[i] for i in self.ids]


class Refusal:
    def __init__(self, name, clouds, poses, params, message):
        self.name, self.clouds, self.poses, self.params, self.message = name, [np.ascontiguousarray(c, F).reshape(-1, 3) for c in clouds], np.asarray(poses, np.float64), \
            mo.OccupancyParams(*params), message


def from_rays(name, rays, params, **meta):
    """one entry per (A, B): a case of exact-end rays"""
    rays = [(tuple(int(a) for a in A), np.asarray(B, np.int64).reshape(-1, 3)) for A, B in rays]
    meta["rays"] = rays
    return Case(name, [records_to(A, B) for A, B in rays], range(len(rays)), [pose_at(A) for A, _ in rays], params, exact_expect(rays, params[3]), meta)


def holds(case, hits, misses, classes, stats, minc):
    """`expect` against one result (the twin's or the engine's): hits, misses, classes (D, H, W), stats a dict, minc a tuple"""
    e = case.expect
    for f, v in e.get("stats", {}).items():
        assert stats[f] == v, (case.name, f, stats[f], v)
    if "minc" in e:
        assert tuple(minc) == e["minc"], (case.name, minc, e["minc"])
    if "sides" in e:
        assert hits.shape[::-1] == e["sides"] == misses.shape[::-1] == classes.shape[::-1], (case.name, hits.shape, e["sides"])

    def dense(d):
        a = np.zeros(hits.shape, np.uint32)
        for v, c in d.items():
            i = tuple(v[k] - minc[k] for k in (2, 1, 0))
            assert all(0 <= i[k] < a.shape[k] for k in range(3)), (case.name, "a stated voxel outside the grid", v, minc, hits.shape)
            a[i] = c
        return a
    if "hits" in e:
        assert np.array_equal(hits, dense(e["hits"])), (case.name, "hits")
    if "misses" in e:
        assert np.array_equal(misses, dense(e["misses"])), (case.name, "misses")
    for key, arr in (("misses_at", misses), ("classes_at", classes)):
        for v, c in e.get(key, {}).items():
            i = tuple(v[k] - minc[k] for k in (2, 1, 0))
            assert all(0 <= i[k] < arr.shape[k] for k in range(3)) and arr[i] == c, (case.name, key, v, c)
    if e.get("no_miss"):
        assert not misses.any() and not (classes == FREE).any() and (classes == OCCUPIED).sum() == len(e["hits"]), (case.name, "no miss")


# ---- octants: every sign pattern, every kind of tie, origins on corners and faces, both sides of zero
SIGNS = [(p % 3 - 1, p // 3 % 3 - 1, p // 9 - 1) for p in range(27)]
OCTANT_COUNTS = [64, 65, 255, 256, 257, 127, 128, 129, 63 + 64, 191, 192, 193]


def octant_origin(e):
    c = [(e * 5) % 13 - 6, (e * 7) % 11 - 5, (e * 3) % 7 - 3]                  # voxels on both sides of zero
    if e % 3 == 0:
        f = [0, 0, 0]                                                            # on a corner: r = 0 on every axis heading down
    elif e % 3 == 1:
        f = [1 + wi(3 * e + k, 1023, 1) for k in range(3)]
    else:
        g = 1 + wi(e, 1023, 2)
        f = [[g, g, 1 + wi(e, 1023, 3)], [0, g, g], [g, 0, 0]][e // 3 % 3]       # x and y in step; on a face of x; on an edge
    return tuple(ONE * c[k] + f[k] for k in range(3))


def octant_end(A, e, j):
    """ray j of entry e: its sign pattern is SIGNS[(j + e) % 27] and its kind (j // 27 + e) % 5"""
    s = SIGNS[(j + e) % 27]
    kind = (j // 27 + e) % 5
    i = 1000 * e + j
    if kind == 0:                                                                # anywhere
        d = [1 + wi(3 * i + k, 12 * ONE - 1, 4) for k in range(3)]
        return [A[k] + s[k] * d[k] for k in range(3)]
    if kind == 1:                                                                # ends on faces, edges and corners
        d = [ONE + wi(3 * i + k, 10 * ONE, 5) for k in range(3)]
        B = [A[k] + s[k] * d[k] for k in range(3)]
        mask = 1 + wi(i, 7, 6)
        return [(B[k] // ONE) * ONE if (mask >> k) & 1 and s[k] else B[k] for k in range(3)]
    if kind == 2:                                                                # |dx| = |dy| = |dz|: through corners from a corner, in step from anywhere
        m = 1 + wi(i, 5, 7)
        return [A[k] + s[k] * m * ONE for k in range(3)]
    if kind == 3:                                                                # two axes in step, the third anywhere
        m = 1 + wi(i, 6, 8)
        return [A[0] + s[0] * m * ONE, A[1] + s[1] * m * ONE, A[2] + s[2] * (1 + wi(i, 9 * ONE, 9))]
    return [A[k] + s[k] * wi(3 * i + k, 700, 10) for k in range(3)]              # short: inside the voxel or into a neighbour, zero-length axes among them


def octants(shell):
    rays = []
    for e in range(48):
        A = octant_origin(e)
        n = OCTANT_COUNTS[e] if e < len(OCTANT_COUNTS) else 64 + (e * 37) % 194
        rays.append((A, [octant_end(A, e, j) for j in range(n)]))
    return from_rays("octants/shell-%d" % shell, rays, UNIT._replace(shell=shell))


# ---- hand walks: the full path written out
def hand_walks():
    out = []
    for name, A, B, path in (
            # from a corner down all three axes: r = 0 everywhere, the tie goes x, y, z; then all three reach 1024 together, x, y, z again
            ("-x-y-z", (ONE, ONE, ONE), (-ONE, -ONE, -ONE), [(1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0), (-1, 0, 0), (-1, -1, 0), (-1, -1, -1)]),
            # x and z in step from the middle of the voxel, y still: each edge crossing goes to x first
            ("xz-in-step", (512, 300, 512), (512 + 2 * ONE, 300, 512 + 2 * ONE), [(0, 0, 0), (1, 0, 0), (1, 0, 1), (2, 0, 1), (2, 0, 2)]),
            # from a face heading down: the origin's voxel is the one above the face and the ray leaves it at once
            ("from-a-face-down", (5 * ONE, 512, 512), (512, 512, 512), [(5, 0, 0), (4, 0, 0), (3, 0, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)])):
        c = from_rays("hand-walks/" + name, [(A, [B])], UNIT, path=path)
        c.expect["misses"] = {v: 1 for v in path[:-1]}
        out.append(c)
    return out


# ---- fold-lanes: the ballot, its first lane and its popcount, wave by wave
FOLD_PARAMS = mo.OccupancyParams(1.0, 0.5, 60.0, 1, 1, 2)
ST_RAY, ST_NONFINITE, ST_NEAR, ST_FAR = 0, 1, 2, 3


def fold_entry(c0):
    """4 x 64 + 1 records from the origin voxel c0 (origin 100 / 1024 inside it on every axis) -> (A, records (257, 3) f32, status per record, n per record
    (-1: no ray), B of the rays)"""
    A = tuple(ONE * c + 100 for c in c0)
    rec = np.zeros((4 * WAVE + 1, 3), F); st = np.zeros(len(rec), np.int64); n = np.full(len(rec), -1, np.int64); B = {}

    def ray(i, d, steps):
        B[i] = [A[k] + d[k] for k in range(3)]; rec[i] = records_to(A, [B[i]])[0]; n[i] = steps
    for l in range(WAVE):
        # wave 0: a non-ray first lane, 62 rays that end in the origin's voxel, and lane 63 the only carving ray (n = 2 > shell)
        if l == 0:
            rec[l] = [np.nan, 0.7, 0.1]; st[l] = ST_NONFINITE
        elif l < 63:
            ray(l, (700 + (l % 7) * 20, 10 + l, 5 + 2 * l), 0)
        else:
            ray(l, (2 * ONE + 17, 300, 0), 2)
        # wave 1: all 64 carve
        ray(WAVE + l, ((2 + l % 4) * ONE + l, (l % 3) * ONE + 5, (l % 2) * ONE + 1), 2 + l % 4 + l % 3 + l % 2)
        # wave 2: every record skipped - non-finite, near and far, well off the bounds
        i = 2 * WAVE + l
        if l % 4 == 0:
            rec[i] = [1.0, 2.0, 3.0]; rec[i, l // 4 % 3] = [np.nan, np.inf, -np.inf][l // 12 % 3]; st[i] = ST_NONFINITE
        elif l % 4 == 1:
            rec[i] = [0.1 + 0.001 * l, -0.05, 0.02]; st[i] = ST_NEAR
        elif l % 4 == 2:
            rec[i] = [200.0, float(l), -3.0]; st[i] = ST_FAR
        else:
            rec[i] = [-0.2, 0.1, 0.1 - 0.001 * l]; st[i] = ST_NEAR
        # wave 3: n == shell (no carve) and n == shell + 1 (v_0 alone) in turn
        if l % 2 == 0:
            ray(3 * WAVE + l, (ONE, 7 * l, 3), 1)
        else:
            ray(3 * WAVE + l, (ONE + l, ONE + 2, 9), 2)
    ray(4 * WAVE, (40 * ONE + 5, 25 * ONE + 3, 10 * ONE + 1), 75)                 # alone in its block: one long ray (48.2 voxels < max_range)
    return A, rec, st, n, np.array([B[i] for i in sorted(B)], np.int64)


def fold_lanes():
    ents = [fold_entry(c0) for c0 in ((0, 0, 0), (-30, 7, -3))]
    rays = [(A, B) for A, _, _, _, B in ents]
    skipped = tuple(sum(int((st == k).sum()) for _, _, st, _, _ in ents) for k in (ST_NONFINITE, ST_NEAR, ST_FAR))
    shell = FOLD_PARAMS.shell
    expect = exact_expect(rays, shell, skipped)
    expect["misses_at"] = {tuple(int(v) for v in cell(A)): int((n > shell).sum()) for A, _, _, n, _ in ents}
    assert list(expect["misses_at"].values()) == [1 + 64 + 32 + 1] * 2
    return Case("fold-lanes", [rec for _, rec, _, _, _ in ents], [0, 1], [pose_at(A) for A, _, _, _, _ in ents], FOLD_PARAMS, expect,
                dict(rays=rays, status=[st for _, _, st, _, _ in ents], n=[n for _, _, _, n, _ in ents]))


# ---- shell: n - shell at 0, at n, and with shell at the top of its type
SHELLS = (0, 3, 6, 7, 0xFFFFFFFF)


def shell_cases():
    A = (-2 * ONE + 512, ONE + 512, 512)
    B = []
    for n in range(7):
        for v in range(5):
            a = wi(7 * n + v, n + 1, 11); b = wi(7 * n + v, n - a + 1, 12)
            steps = (a, b, n - a - b)
            s = SIGNS[(5 * n + 3 * v) % 27]
            s = [s[k] if s[k] else 1 for k in range(3)]
            B.append([A[k] + s[k] * steps[k] * ONE + wi(3 * (5 * n + v) + k, 200, 13) - 100 for k in range(3)])
    out = []
    for sh in SHELLS:
        c = from_rays("shell/%d" % sh, [(A, B)], UNIT._replace(shell=sh))
        assert sorted(set(np.abs(cell(B) - cell(A)).sum(axis=1).tolist())) == list(range(7))
        if sh >= 6:
            c.expect["no_miss"] = True
            assert c.expect["stats"]["total_misses"] == 0
        out.append(c)
    return out


# ---- exact single roundings (the contracted forms are evaluated in rationals and rounded once)
def round_to(q, bits, emin):
    """the rational q rounded half to even to a binary format of `bits` significant bits and least normal exponent emin -> a Fraction (the caller's values stay
    far below the format's overflow, except where it asks for it)"""
    q = Fraction(q)
    if q == 0:
        return q
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    elif Fraction(2) ** (e + 1) <= a:
        e += 1
    ulp = Fraction(2) ** (max(e, emin) - (bits - 1))
    t = a / ulp
    k = t.numerator // t.denominator
    rest = t - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    return (k * ulp) if q > 0 else -(k * ulp)


F32_MAX = Fraction(int(np.finfo(F).max))


def r32(q):
    """q rounded once to f32 (a Fraction; beyond the largest finite value: infinity, as a float)"""
    v = round_to(q, 24, -126)
    return v if abs(v) <= F32_MAX else (float("inf") if v > 0 else float("-inf"))


def r64(q):
    return round_to(q, 53, -1022)


D2_FORMS = ("plain", "fma(z,z,xx+yy)", "fma(x,x,yy)+zz", "fma(y,y,xx)+zz", "fma(z,z,fma(x,x,yy))", "fma(z,z,fma(y,y,xx))")


def d2_form(rec, form):
    """(x x + y y) + z z of an f32 record in f32: as written (every operation rounded), or with the named fused multiply-adds -> Fraction or +inf"""
    x, y, z = (Fraction(float(v)) for v in rec)
    inf = float("inf")

    def add(a, b):
        return inf if inf in (a, b) else r32(a + b)
    xx, yy, zz = r32(x * x), r32(y * y), r32(z * z)
    if form == "plain":
        return add(add(xx, yy), zz)
    if form == "fma(z,z,xx+yy)":
        s = add(xx, yy)
        return inf if s == inf else r32(z * z + s)
    if form == "fma(x,x,yy)+zz":
        return add(inf if yy == inf else r32(x * x + yy), zz)
    if form == "fma(y,y,xx)+zz":
        return add(inf if xx == inf else r32(y * y + xx), zz)
    inner = (inf if yy == inf else r32(x * x + yy)) if form == "fma(z,z,fma(x,x,yy))" else (inf if xx == inf else r32(y * y + xx))
    return inf if inner == inf else r32(z * z + inner)


def status_of(rec, lo2, hi2, form="plain"):
    """the record rule on one f32 record with the given d2"""
    if not all(np.isfinite(float(v)) for v in rec):
        return ST_NONFINITE
    d2 = d2_form(rec, form)
    return ST_NEAR if d2 < lo2 else (ST_FAR if d2 > hi2 else ST_RAY)


# ---- range gates: records ON the bounds whose contracted d2 falls on the other side, and the reverse
GATE_PARAMS = mo.OccupancyParams(2.0, 0.5, 60.0, 1, 1, 2)
GATE_KINDS = ("on-lo", "on-hi", "under-lo", "over-hi")         # plain == lo2 (kept) / == hi2 (kept) / one ulp below lo2 (near) / one ulp above hi2 (far)


def _d2_forms_f64(x, y, z):
    """the five contracted forms on arrays, through f64 (a product of two f32 is exact there; the sum may round twice, so this only picks candidates)"""
    X, Y, Z = (v.astype(np.float64) for v in (x, y, z))
    f = lambda v: v.astype(F)
    xx, yy, zz = x * x, y * y, z * z
    return {"fma(z,z,xx+yy)": f(Z * Z + (xx + yy)), "fma(x,x,yy)+zz": f(X * X + yy) + zz, "fma(y,y,xx)+zz": f(Y * Y + xx) + zz,
            "fma(z,z,fma(x,x,yy))": f(Z * Z + f(X * X + yy)), "fma(z,z,fma(y,y,xx))": f(Z * Z + f(Y * Y + xx))}


def gate_search(kind, pool=4000, per_form=2):
    """the first records of a fixed sequence of directions, off the axes, whose plain f32 d2 is the kind's value and whose status changes under a contracted
    form, until every form has `per_form` of them (or the pool ends) -> [(record, the forms it defeats)].  Candidates are picked with numpy; what is
    returned was evaluated in exact rationals."""
    lo2, hi2 = Fraction(1, 4), Fraction(3600)
    r = 0.5 if kind in ("on-lo", "under-lo") else 60.0
    want = {"on-lo": F(0.25), "on-hi": F(3600.0), "under-lo": np.nextafter(F(0.25), F(0)), "over-hi": np.nextafter(F(3600.0), F(4000))}[kind]
    plain = dict(zip(GATE_KINDS, (ST_RAY, ST_RAY, ST_NEAR, ST_FAR)))[kind]
    i = np.arange(1, pool + 1, dtype=np.float64)
    u = 0.15 + 0.7 * ((i * 0.6180339887498949) % 1.0); v = 2.0 * np.pi * ((i * 0.7548776662466927) % 1.0)
    w = np.sqrt(1.0 - u * u)
    x, y = (r * w * np.cos(v)).astype(F), (r * w * np.sin(v)).astype(F)
    z0 = np.sqrt(np.maximum(float(want) - x.astype(np.float64) ** 2 - y.astype(np.float64) ** 2, 0.0)).astype(F)
    cand = []
    for z in (z0, np.nextafter(z0, F(0)), np.nextafter(z0, F(100))):
        ok = (x * x + y * y) + z * z == want
        forms = _d2_forms_f64(x, y, z)
        moved = np.zeros(pool, bool)
        for d2 in forms.values():
            moved |= (d2 < F(0.25)) != (want < F(0.25)) if r == 0.5 else (d2 > F(3600.0)) != (want > F(3600.0))
        cand += [(int(k), (x[k], y[k], z[k])) for k in np.flatnonzero(ok & moved)]
    need = {f: per_form for f in D2_FORMS[1:]}
    out = []
    for _, rec in sorted(cand, key=lambda c: c[0]):
        assert d2_form(rec, "plain") == Fraction(float(want)) and status_of(rec, lo2, hi2) == plain
        beaten = [f for f in D2_FORMS[1:] if status_of(rec, lo2, hi2, f) != plain]
        if any(need[f] > 0 for f in beaten):
            for f in beaten:
                need[f] -= 1
            out.append((np.array(rec, F), beaten))
        if all(v <= 0 for v in need.values()):
            break
    return out


def range_gates():
    found = [(kind, rec, beaten) for kind in GATE_KINDS for rec, beaten in gate_search(kind)]
    below, above = np.nextafter(F(0.5), F(0)), np.nextafter(F(60), F(100))
    fixed = [([0.5, 0, 0], ST_RAY), ([60.0, 0, 0], ST_RAY), ([below, 0, 0], ST_NEAR), ([above, 0, 0], ST_FAR),        # the four axis records
             ([0, -0.5, 0], ST_RAY), ([0, 0, -60.0], ST_RAY), ([0, below, 0], ST_NEAR), ([0, 0, -above], ST_FAR),
             ([3e30, 0, 0], ST_FAR),                                                                                  # its square is infinite
             ([-0.0, 0.5, -0.0], ST_RAY), ([-0.0, -0.0, -0.0], ST_NEAR), ([-0.0, -0.0, 60.0], ST_RAY),
             ([np.nan, 1, 1], ST_NONFINITE), ([1, np.inf, 1], ST_NONFINITE), ([1, 1, -np.inf], ST_NONFINITE)]
    plain = dict(zip(GATE_KINDS, (ST_RAY, ST_RAY, ST_NEAR, ST_FAR)))
    cloud = np.array([rec for _, rec, _ in found] + [r for r, _ in fixed], F)
    status = np.array([plain[k] for k, _, _ in found] + [s for _, s in fixed])
    n = [int((status == k).sum()) for k in range(4)]
    expect = dict(stats=dict(n_records=len(cloud), n_rays=n[ST_RAY], n_nonfinite=n[ST_NONFINITE], n_near=n[ST_NEAR], n_far=n[ST_FAR], total_hits=n[ST_RAY]))
    beaten = {f: sorted(i for i, (_, _, b) in enumerate(found) if f in b) for f in D2_FORMS[1:]}
    return Case("range-gates", [cloud], [0], [np.eye(4)], GATE_PARAMS, expect, dict(status=status, kinds=[k for k, _, _ in found], beaten=beaten))


# ---- quantise: half to even at k + 0.5 fixed-point units, and a transform that lands on 1023.5
HALF_K = (0, 1, 2, -1, -2, 1023, -1025)
HALF_B = (0, 2, 2, 0, -2, 1024, -1024)                                # rint((k + 0.5)) to even


def quantise_halves():
    """origin 0, identity: record j is ((k_j + 0.5) / 1024, j + 0.5, 0.5) - exact in f32 - so its end is voxel (HALF_B[j] >> 10, j, 0)"""
    cloud = np.array([[(k + 0.5) / 1024.0, j + 0.5, 0.5] for j, k in enumerate(HALF_K)], F)
    assert all(Fraction(float(cloud[j, 0])) == Fraction(2 * k + 1, 2048) for j, k in enumerate(HALF_K))
    vox = [(b // ONE, j, 0) for j, b in enumerate(HALF_B)]
    assert [v[0] for v in vox] == [0, 0, 0, 0, -1, 1, -1]
    expect = dict(stats=dict(n_rays=7, total_hits=7, width=3, height=7, depth=1), minc=(-1, 0, 0), sides=(3, 7, 1), hits={v: 1 for v in vox})
    return Case("quantise/halves", [cloud], [0], [np.eye(4)], UNIT, expect, dict(B_x=HALF_B))


def quantise_minus_point_three():
    """voxel 0.3, the origin at -0.3 on every axis: (-0.3 * (1 / 0.3)) * 1024 rounds to -1024, voxel -1; the end 0.45 m further is in voxel 0"""
    T = np.eye(4); T[:3, 3] = -0.3
    cloud = np.array([[0.45, 0.45, 0.45]], F)
    expect = dict(stats=dict(n_rays=1, total_hits=1, width=2, height=2, depth=2, total_misses=3), minc=(-1, -1, -1), sides=(2, 2, 2), hits={(0, 0, 0): 1},
                  misses_at={(-1, -1, -1): 1})
    return Case("quantise/-0.3", [cloud], [0], [T], mo.OccupancyParams(0.3, 0.0, 100.0, 0, 1, 2), expect)


T_FORMS = ("plain", "fma(P0,x,P1y)", "fma(P1,y,P0x)")
P0, P1 = 1.0 + 2.0 ** -29 + 5 * 2.0 ** -36, 1.0 + 2.0 ** -28 + 3 * 2.0 ** -37


def row_form(P, rec, form):
    """((P0 x + P1 y) + P2 z) + P3 in f64 as written, or with one product left unrounded into the first sum -> Fraction"""
    p = [Fraction(float(v)) for v in P]; x, y, z = (Fraction(float(v)) for v in rec)
    if form == "plain":
        s = r64(r64(p[0] * x) + r64(p[1] * y))
    elif form == "fma(P0,x,P1y)":
        s = r64(p[0] * x + r64(p[1] * y))
    else:
        s = r64(p[1] * y + r64(p[0] * x))
    return r64(r64(s + r64(p[2] * z)) + p[3])


def transform_search(count=3, pool=400):
    """records (x, y, 0), x and y f32 in [1, 2), each with a pose row (P0, P1, 0, P3), P3 = (1 - 2^-11) - fl(fl(P0 x) + fl(P1 y)) (exact), so that the plain sum is
    1023.5 / 1024 exactly: B = 1024, voxel 1.  Kept: those where a contracted first sum is smaller, so that W' 1024 < 1023.5: B = 1023, voxel 0.
    -> [(record, pose, the forms it defeats)], until each form has `count`"""
    target = Fraction(2047, 2048)
    need = {f: count for f in T_FORMS[1:]}
    out = []
    for i in range(pool):
        x = F(1.0 + (((i + 1) * 0.6180339887498949) % 1.0)); y = F(1.0 + (((i + 1) * 0.7548776662466927) % 1.0))
        s = (P0 * float(x) + P1 * float(y))                                      # f64, each operation rounded
        P3 = float(target) - s
        assert Fraction(P3) == target - Fraction(s)
        row = (P0, P1, 0.0, P3)
        rec = (x, y, F(0.0))
        assert row_form(row, rec, "plain") == target
        beaten = [f for f in T_FORMS[1:] if row_form(row, rec, f) < target]
        assert all(row_form(row, rec, f) >= target - Fraction(1, 1 << 40) for f in T_FORMS[1:])
        if any(need[f] > 0 for f in beaten):
            for f in beaten:
                need[f] -= 1
            T = np.eye(4); T[0] = row; T[2, 3] = 0.5
            out.append((np.array(rec, F), T, beaten))
        if all(v <= 0 for v in need.values()):
            break
    return out


def quantise_transform():
    """one entry per found record; all of them end in voxel (1, 1, 0): W_x 1024 = 1023.5 rounds to the even 1024"""
    found = transform_search()
    n = len(found)
    expect = dict(stats=dict(n_rays=n, total_hits=n), hits={(1, 1, 0): n})
    return Case("quantise/transform", [r.reshape(1, 3) for r, _, _ in found], range(n), [T for _, T, _ in found], UNIT, expect,
                dict(beaten={f: [i for i, (_, _, b) in enumerate(found) if f in b] for f in T_FORMS[1:]}))


# ---- limits: next to 2^20 voxels from the origin, 2^15 voxels a side, and the refusals
FAR_PARAMS = mo.OccupancyParams(1.0, 0.0, 1.0e6, 1, 1, 2)
RAY_END, GRID = "a ray end of 2^20 voxels or more from the origin", "a grid of more than 2^27 voxels (or 2^15 a side)"


def limits():
    out = []
    edge = COORD_LIMIT * ONE - 3 * ONE - 512                                     # 2^20 - 3.5 voxels
    for sg in (1, -1):
        A = (sg * edge,) * 3
        c = from_rays("limits/%s2^20-3.5" % ("+" if sg > 0 else "-"), [(A, [[a + sg * (ONE + 256) for a in A]])], FAR_PARAMS)
        # 2^20 - 3.5 and 2^20 - 2.25 lie in voxels 1048572 and 1048573; their negatives in -1048573 and -1048574 (floor)
        assert c.expect["minc"] == ((1048572,) * 3 if sg > 0 else (-1048574,) * 3) and c.expect["sides"] == (2, 2, 2)
        out.append(c)
    # exactly 2^15 voxels a side: [32767, 0.25, 0.25] from (0.5, 0.5, 0.5), voxels 0 .. 32767 along x, all but the last `shell` before the end carved
    c = from_rays("limits/side-2^15", [((512, 512, 512), [[512 + 32767 * ONE, 768, 768]])], FAR_PARAMS)
    assert c.expect["sides"] == (MAX_SIDE, 1, 1) and c.expect["stats"]["total_misses"] == 32766
    c.expect["misses_at"] = {(0, 0, 0): 1, (32765, 0, 0): 1, (32766, 0, 0): 0, (32767, 0, 0): 0}
    out.append(c)
    return out


def refusals():
    at = lambda v: pose_at((int(v * ONE),) * 3)
    many = np.tile(np.array([[1.0, 0.5, -0.5]], F), (4 * OC_BLOCK + 1, 1)); many[-1] = [11.0, 0.0, 0.0]       # the last record alone, from its own block's lane 0
    return [Refusal("origin-at-2^20", [np.array([[-1.0, -1.0, -1.0]], F)], [at(COORD_LIMIT)], FAR_PARAMS, RAY_END),
            Refusal("origin-at--2^20", [np.array([[1.0, 1.0, 1.0]], F)], [at(-COORD_LIMIT)], FAR_PARAMS, RAY_END),
            Refusal("one-record-of-1025-past-2^20", [many], [at(COORD_LIMIT - 10)], FAR_PARAMS, RAY_END),
            Refusal("side-2^15+1", [np.array([[32768.0, 0.25, 0.25]], F)], [at(0.5)], FAR_PARAMS, GRID)]


# ---- many entries: a second launch of the extent and the carve, and a fold over more than 1024 * 32 tiles
MANY_KF = [np.array([[2.0, 1.0, 0.0]], F), np.array([[-1.0, 2.0, 1.0], [0.25, 0.25, 0.0]], F), np.array([[3.0, 0.0, 0.0], [0.0, -2.0, 0.0], [1.0, 1.0, 1.0]], F)]
MANY_POSES = 19                                                       # (a prime: no period of the pose table divides SV_CHUNK)


def many_entries():
    count = SV_CHUNK + 3
    table = [(512 + ONE * (t % 5), 256 + ONE * (t // 5), 768 - ONE * (t % 3)) for t in range(MANY_POSES)]
    assert len(set(table)) == MANY_POSES
    apart = [(512 + ONE * (40 + 6 * i), 512 + ONE * 40, 512 + ONE * 9) for i in range(3)]       # the last three entries: where no other ray ends
    ids = [(e * 5 + e // 9) % 3 for e in range(count)]
    origin = [table[(e + e // 100) % MANY_POSES] for e in range(count - 3)] + apart
    rays = [(A, np.asarray(A, np.int64) + np.round(MANY_KF[k].astype(np.float64) * ONE).astype(np.int64)) for A, k in zip(origin, ids)]
    expect = exact_expect(rays, 1)
    n_rec = sum(len(MANY_KF[k]) for k in ids)
    assert expect["stats"]["n_records"] == n_rec and n_rec > 2 * count - 1000
    last = {tuple(int(v) for v in cell(b)) for A, B in rays[-3:] for b in B}
    others = {tuple(int(v) for v in cell(b)) for A, B in rays[:-3] for b in B}
    assert not (last & others) and all(expect["hits"][v] >= 1 for v in last)
    return Case("many-entries", MANY_KF, ids, [pose_at(A) for A in origin], UNIT._replace(shell=1), expect,
                dict(last=sorted(last), tiles=count, records=n_rec))


# ---- class rule
CLASS_TARGETS = [(3, 6), (3, 7), (3, 5), (2, 0), (2, 9), (0, 1), (1, 0), (2, 1)]            # (hits, misses) of voxel (3 j + 1, 0, 0)
CLASS_RULES = {(1, 2): [2, 1, 2, 2, 1, 1, 2, 2],        # hits * hit_weight == misses is still occupied; 7 > 6 and 9 > 4 are free; a miss alone is free
               (3, 2): [2, 1, 2, 1, 1, 1, 1, 1],        # hits == min_hits - 1 is free, even without a miss
               (1, 1 << 31): [2, 2, 2, 2, 2, 1, 2, 2]}  # 2 * 2^31 = 2^32 >= 1: occupied (the low 32 bits of the product are 0, which would be free)


def class_rule():
    """voxel p = 3 j + 1 of one row: h rays from the middle of voxel p - 1 into p, and m rays from the middle of p into p + 1 (shell 0: each leaves one miss in
    the voxel it starts in and a hit in the next)"""
    rays, hits, misses = [], {}, {}
    add = lambda d, v, c: d.__setitem__(v, d.get(v, 0) + c)
    for j, (h, m) in enumerate(CLASS_TARGETS):
        p = 3 * j + 1
        for o, k in ((p - 1, h), (p, m)):
            if k:
                A = (o * ONE + 512, 512, 512)
                rays.append((A, [[A[0] + ONE + 3 * i, 512 + i, 512 - i] for i in range(k)]))
                add(misses, (o, 0, 0), k); add(hits, (o + 1, 0, 0), k)
    out = []
    for (min_hits, w), cls in CLASS_RULES.items():
        c = from_rays("class-rule/%d-%d" % (min_hits, w), rays, UNIT._replace(min_hits=min_hits, hit_weight=w))
        assert c.expect["hits"] == hits and all((hits.get((3 * j + 1, 0, 0), 0), misses.get((3 * j + 1, 0, 0), 0)) == t for j, t in enumerate(CLASS_TARGETS))
        c.expect["misses"] = misses
        c.expect["classes_at"] = {(3 * j + 1, 0, 0): b for j, b in enumerate(cls)}
        out.append(c)
    return out


# ---- the seams of k_oc_classify, k_dg_list_* and k_dg_slice
def cell_seams():
    out = []
    for W, H, D in ((17, 15, 1), (16, 16, 1), (257, 1, 1), (16, 16, 3)):
        A = (512, 512, 512)
        ends = [[(W - 1) * ONE + 300, (H - 1) * ONE + 700, (D - 1) * ONE + 100], [(W - 1) * ONE + 5, 40, 512], [100, (H - 1) * ONE + 9, 512],
                [(W // 2) * ONE + 1, (H // 2) * ONE + 1, (D - 1) * ONE + 1], [600, 600, 600]]
        c = from_rays("cell-seams/%dx%dx%d" % (W, H, D), [(A, ends)], UNIT._replace(max_range=1000.0))
        assert c.expect["sides"] == (W, H, D) and c.expect["minc"] == (0, 0, 0)
        out.append(c)
    assert [c.expect["sides"][0] * c.expect["sides"][1] * c.expect["sides"][2] for c in out[:3]] == [OC_BLOCK - 1, OC_BLOCK, OC_BLOCK + 1]
    return out


# ---- the table
GROUPS = {"octants": lambda: [octants(0), octants(1)], "hand-walks": hand_walks, "fold-lanes": lambda: [fold_lanes()], "shell": shell_cases,
          "range-gates": lambda: [range_gates()], "quantise": lambda: [quantise_halves(), quantise_minus_point_three(), quantise_transform()], "limits": limits,
          "many-entries": lambda: [many_entries()], "class-rule": class_rule, "cell-seams": cell_seams}
NAMES = list(GROUPS)
SLOW_TWIN = ("many-entries", "limits/side-2^15")                     # no scalar restatement of these: compared with the stated counts instead
MASKS = (1, 2, 3, 4, 5, 6, 7)


@functools.lru_cache(maxsize=None)
def group(name):
    return GROUPS[name]()


def get(name):
    """a case by its full name, e.g. 'shell/3'"""
    for c in group(name.split("/")[0]):
        if c.name == name:
            return c
    raise KeyError(name)


def all_cases():
    return [c for g in NAMES for c in group(g)]


@functools.lru_cache(maxsize=None)
def twin(name):
    """the twin's result of a case, computed once and shared (treat it as read-only)"""
    c = get(name)
    return mo.classify(c.clouds, c.poses, c.params)


def slice_ranges(D):
    """every (lo, hi) with 0 <= lo <= hi <= D - 1 (of a deep grid: all layers, the middle one and the two ends), and the clipped and the empty ranges"""
    inside = [(lo, hi) for lo in range(D) for hi in range(lo, D)] if D <= 4 else [(0, D - 1), (D // 2, D // 2), (0, 0), (D - 1, D - 1), (1, D - 2)]
    return inside + [(-5, 0), (D - 1, D + 7), (-2, D + 2), (D, D + 1), (-3, -1)]
