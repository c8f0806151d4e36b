"""The case table of the range-image family (csrc/qn_range.cuh: fs_project, fs_window, fs_class, run by k_range_bin, k_freespace_check / _reduce and
k_static_vote / _scan / _compact): deterministic inputs, each built to put records ON an edge of the arithmetic or a seam of the launch, with the expected
class bytes, counts, votes and image pixels stated BY CONSTRUCTION wherever the geometry gives them - never from the twin and never from engine output.
tests/test_range_edges_cpu.py holds the twin (qn_amd/freespace.py, qn_amd/staticmap.py) to a scalar restatement of the specification and to these
expectations on every case; tests/test_gpu_range_edges.py holds the engine to the twin and to them.  Pure numpy, no GPU, no random draws (ranges and radii
come from a Weyl sequence).

A Case: range parameters, keyframes (clouds), free-space pairs (q, c, T), optionally a static-map list (ids, poses, witnesses) with rules, and `expect`:
  cls[(pair, direction)]   the class byte of every record;          votes[entry] = (seen_through, agree);
  pixels[keyframe]         the occupied pixels of its images (bool, n_rows x n_cols), `near` / `far` the nominal ranges there (to 1e-5);
  kept[keyframe]           per record: survives the gates of the images (bool).

Seams and the constant each belongs to (restated from the sources; whoever changes one there changes it here):
  FS_BLOCK 512 / FS_TILE 2048   records per round / per block of k_range_bin, k_freespace_check, k_static_vote, k_static_compact (wave: 64)
  REDUCE_SLOTS 256              threads of k_freespace_reduce: a direction with more tiles runs its stride loop again (> 524288 records)
  SV_SCAN_BLOCK 1024            threads of k_static_scan: more tiles than that and a thread scans chunk >= 2 of them
  SV_CHUNK 32768                entries per launch of k_static_vote / k_static_compact
  MAX_WITNESSES 255             the u8 vote counters' cap"""
import math
from fractions import Fraction
import numpy as np
from qn_amd import freespace as fs, staticmap as sm

WAVE, FS_BLOCK, FS_TILE = 64, 512, 2048
REDUCE_SLOTS, SV_SCAN_BLOCK, SV_CHUNK, MAX_WITNESSES = 256, 1024, 32768, 255
SEAM_COUNTS = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097]

# window 0 x 0 throughout: a record one row or one column off meets another pixel, and the checkerboards below give that pixel another class
EDGE = fs.Params(n_rows=8, n_cols=64, el_lo=-0.8, el_hi=0.8, min_range=1.0, window_rows=0, window_cols=0)
WIDE = fs.Params(n_rows=2, n_cols=4608, el_lo=-0.5, el_hi=0.5, min_range=1.0, window_rows=0, window_cols=0)        # > 4096 columns: the table stays in global memory
KNIFE = fs.Params(n_rows=32, n_cols=720, el_lo=math.radians(-25.0), el_hi=math.radians(15.0), min_range=1.0, window_rows=0, window_cols=0)
NEAR_M, SHELL_M, FAR_M = 10.0, 30.0, 50.0                # seen through / agree / occluded against a shell at 30 m (tol = 0.3 + 0.02 r <= 1.3 m)


def with_(p, **kw):
    d = dict(p.__dict__); d.update(kw)
    return fs.Params(**d)


def weyl(n, lo, hi, salt=0):
    """n values of the Weyl sequence of 1/golden ratio in [lo, hi)"""
    return lo + (((np.arange(1, n + 1, dtype=np.float64) + salt) * 0.6180339887498949) % 1.0) * (hi - lo)


def centres(p, rows, cols, rng):
    """one f32 record at the centre of each pixel (rows[k], cols[k]) at range rng[k]: half a pixel (>= 6e-4 rad here) from every edge, f32 rounding moves it 1e-7"""
    rows = np.asarray(rows, np.float64); cols = np.asarray(cols, np.float64); rng = np.broadcast_to(np.asarray(rng, np.float64), rows.shape)
    el = p.el_lo + (rows + 0.5) * (p.el_hi - p.el_lo) / p.n_rows
    az = 2.0 * np.pi * (cols + 0.5) / p.n_cols
    return np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], axis=1).astype(np.float32)


def even_pixels(p):
    r, c = np.meshgrid(np.arange(0, p.n_rows, 2), np.arange(0, p.n_cols, 2), indexing="ij")
    return r.reshape(-1), c.reshape(-1)


def odd_pixels(p):
    """the pixels a checkerboard leaves empty: an odd row or an odd column"""
    r, c = np.meshgrid(np.arange(p.n_rows), np.arange(p.n_cols), indexing="ij")
    m = ((r | c) & 1).astype(bool)
    return r[m], c[m]


def checkerboard(p, rng=SHELL_M):
    """the shell keyframe: one record at the centre of every (even row, even column) pixel at `rng`; every odd row and odd column stays empty"""
    r, c = even_pixels(p)
    return centres(p, r, c, rng)


def parity_shell(p, rows, cols):
    """the four-class shell over the listed pixels, by the parity of (row, column): (even, even) two returns 2 m and 200 m - anything between agrees (4);
    (even, odd) empty (1); (odd, even) 200 m - seen through (2); (odd, odd) 2 m - occluded (3).  A record between 5 m and 150 m gets a different class in
    each of the four pixels around a (row edge, column boundary) crossing."""
    rows = np.asarray(rows); cols = np.asarray(cols)
    near = (rows + cols) % 2 == 0                       # (even, even) and (odd, odd) hold the 2 m return
    far = cols % 2 == 0                                 # (even, even) and (odd, even) hold the 200 m return
    return np.concatenate([centres(p, rows[near], cols[near], 2.0), centres(p, rows[far], cols[far], 200.0)])


class Case:
    def __init__(self, name, params, clouds, pairs=(), entries=None, rules=((1, 0),), expect=None, meta=None):
        self.name, self.params = name, params
        self.clouds = [np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in clouds]
        self.pairs = [(int(q), int(c), np.asarray(T, np.float64).reshape(4, 4)) for q, c, T in pairs]
        self.entries = entries                           # None or dict(ids, poses, wit_off, wit)
        self.rules = [tuple(r) for r in rules]
        self.expect = dict(cls={}, votes={}, pixels={}, kept={}) if expect is None else expect
        self.meta = {} if meta is None else meta


def witness_csr(lists):
    off = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.uint32)
    return off, np.array([w for l in lists for w in l], np.uint32)


# ---- pattern records: a requested class per record against checkerboard(p)
DROP_KINDS = ("nan", "above", "blind", "axis")


def pattern_records(p, seq, shell_m=SHELL_M):
    """-> (records (n, 3) f32, dict(cls, finite, kept, pixels, near, far)): record k has class seq[k] against checkerboard(p, shell_m) through the identity.
    2 / 4 / 3: the centre of a filled pixel at 10 / 30 / 50 m (the pixels cycle); 1: the centre of an empty pixel; 0: in turn a NaN coordinate, a point
    above the field of view, one inside min_range, one on the z axis."""
    seq = np.asarray(seq, np.uint8)
    n = len(seq)
    fr, fc = even_pixels(p); er, ec = odd_pixels(p)
    k = np.arange(n)
    rows = np.where(seq == fs.UNOBSERVED, er[k % len(er)], fr[(5 * k + 1) % len(fr)])
    cols = np.where(seq == fs.UNOBSERVED, ec[k % len(ec)], fc[(5 * k + 1) % len(fc)])
    rng = np.select([seq == fs.SEEN_THROUGH, seq == fs.OCCLUDED], [NEAR_M, FAR_M], shell_m)
    a = centres(p, rows, cols, rng)
    fin = np.ones(n, bool)
    drop = np.flatnonzero(seq == fs.DROPPED)
    for m, i in enumerate(drop):
        kind = DROP_KINDS[m % 4]
        if kind == "nan":
            a[i, m // 4 % 3] = np.nan; fin[i] = False
        elif kind == "above":
            el = 0.5 * (p.el_hi + 0.5 * math.pi); az = 0.1 * m
            a[i] = [30.0 * math.cos(el) * math.cos(az), 30.0 * math.cos(el) * math.sin(az), 30.0 * math.sin(el)]
        elif kind == "blind":
            a[i] = centres(p, [rows[i]], [cols[i]], 0.5 * p.min_range)[0]
        else:
            a[i] = [0.0, 0.0, 5.0 if m % 8 < 4 else -5.0]
    kept = seq != fs.DROPPED
    pix = np.zeros((p.n_rows, p.n_cols), bool)
    near = np.full((p.n_rows, p.n_cols), np.inf); far = np.zeros((p.n_rows, p.n_cols))
    pix[rows[kept], cols[kept]] = True
    np.minimum.at(near, (rows[kept], cols[kept]), rng[kept]); np.maximum.at(far, (rows[kept], cols[kept]), rng[kept])
    return a, dict(cls=seq.copy(), finite=fin, kept=kept, pixels=pix, near=near, far=far)


def counts_of(cls, finite):
    """the direction record of a class sequence, by the definitions in freespace.py's docstring"""
    n = [int((cls == k).sum()) for k in range(5)]
    return dict(n=len(cls), n_finite=int(finite.sum()), in_fov=n[1] + n[2] + n[3] + n[4], observed=n[2] + n[3] + n[4], seen_through=n[2], occluded=n[3], agree=n[4])


def mixed(n, salt=0):
    """a class sequence with every class and every dropped kind, no period that divides a wave"""
    k = np.arange(n) + salt
    return ((k * 7 + k // 5 + k // 67) % 5).astype(np.uint8)


REMOVALS = ("none", "all", "alternating", "one-wave", "first-of-tile", "last-of-tile")


def removal(n, name):
    """a class sequence whose class-2 records - the ones rule (1, 0) removes with one witness - follow the named pattern; the others cycle through 4, 3, 1, 0"""
    k = np.arange(n)
    rest = np.array([4, 3, 1, 0, 4], np.uint8)[(k + k // 64) % 5]
    rm = dict(none=np.zeros(n, bool), all=np.ones(n, bool), alternating=k % 2 == 0, **{"one-wave": (k >= WAVE) & (k < 2 * WAVE) if n > WAVE else k >= 0,
              "first-of-tile": k % FS_TILE == 0, "last-of-tile": (k % FS_TILE == FS_TILE - 1) | (k == n - 1)})[name]
    return np.where(rm, fs.SEEN_THROUGH, rest).astype(np.uint8)


def _add_pattern(case, seq, pair_with=None, shell_m=SHELL_M):
    a, e = pattern_records(case.params, seq, shell_m)
    kf = len(case.clouds)
    case.clouds.append(a)
    case.expect["pixels"][kf] = (e["pixels"], e["near"], e["far"]); case.expect["kept"][kf] = e["kept"]
    if pair_with is not None:
        case.expect["cls"][(len(case.pairs), 0)] = e["cls"]
        case.meta.setdefault("finite", {})[(len(case.pairs), 0)] = e["finite"]
        case.pairs.append((kf, pair_with, np.eye(4)))
    return kf, e


def _shell_expect(case, kf, rng=SHELL_M):
    p = case.params
    pix = np.zeros((p.n_rows, p.n_cols), bool); pix[::2, ::2] = True
    case.expect["pixels"][kf] = (pix, np.where(pix, rng, np.inf), np.where(pix, rng, 0.0))
    case.expect["kept"][kf] = np.ones(len(case.clouds[kf]), bool)


def seams(p=EDGE, counts=SEAM_COUNTS, name="seams"):
    """keyframe 0 the shell; per count a mixed sequence and the six removal patterns; every one a pair with the shell and an entry with the shell as witness"""
    c = Case(name, p, [checkerboard(p)])
    _shell_expect(c, 0)
    ids, wits = [0], [[]]
    c.expect["votes"][0] = (np.zeros(len(c.clouds[0]), np.uint8),) * 2
    for n in counts:
        for s, seq in enumerate([mixed(n, n)] + [removal(n, r) for r in REMOVALS]):
            kf, e = _add_pattern(c, seq, pair_with=0)
            c.expect["votes"][len(ids)] = ((seq == 2).astype(np.uint8), (seq == 4).astype(np.uint8))
            ids.append(kf); wits.append([0])
    off, wit = witness_csr(wits)
    c.entries = dict(ids=ids, poses=[np.eye(4)] * len(ids), wit_off=off, wit=wit)
    return c


def yaw(a):
    T = np.eye(4); T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    return T


def _tiny(p):
    """shell + the four tiny keyframes: 0 records, 1, 3 and 2049"""
    c = Case("", p, [checkerboard(p)])
    _shell_expect(c, 0)
    sizes = [0, 1, 3, FS_TILE + 1]
    for n in sizes:
        _add_pattern(c, np.array([2, 4, 2, 3, 1, 0, 2], np.uint8)[(np.arange(n) + 2 * n) % 7])
    return c, sizes


def scan_tiles(p=EDGE):
    """2100 entries of the four tiny keyframes (ids repeat): more than 2048 tiles, so k_static_scan's threads take chunk = 3 tiles each, 340 threads of the
    1024 have an empty range and off[nt] comes from the last one.  Entry 0 is the shell, everybody's witness.  A third of the entries stand at the identity
    (classes by construction), the others are turned by one and by two columns (twin only)."""
    c, sizes = _tiny(p)
    c.name = "scan-tiles"
    ids, poses = [0], [np.eye(4)]
    turn = [np.eye(4), yaw(2.0 * math.pi / p.n_cols), yaw(4.0 * math.pi / p.n_cols)]
    for e in range(1, 2100):
        kf = 4 if e == 1000 else (1 if e % 41 == 0 else (3 if e % 3 == 0 else 2))
        ids.append(kf); poses.append(turn[(e // 7) % 3])
    off, wit = witness_csr([[]] + [[0]] * (len(ids) - 1))
    c.entries = dict(ids=ids, poses=poses, wit_off=off, wit=wit)
    nt = sum((len(c.clouds[i]) + FS_TILE - 1) // FS_TILE for i in ids)
    c.meta["tiles"] = nt
    return c


def many_entries(p=EDGE):
    """SV_CHUNK + 3 entries of 1 to 3 records: the second launch of k_static_vote / k_static_compact holds three entries"""
    c = Case("many-entries", p, [checkerboard(p)])
    _shell_expect(c, 0)
    for n in (1, 2, 3):
        _add_pattern(c, np.array([2, 4, 2], np.uint8)[(np.arange(n) + n) % 3])
    count = SV_CHUNK + 3
    ids = [0] + [1 + (e * 5 + e // 9) % 3 for e in range(1, count)]
    off, wit = witness_csr([[]] + [[0]] * (count - 1))
    c.entries = dict(ids=ids, poses=[np.eye(4)] * count, wit_off=off, wit=wit)
    return c


def reduce_tiles(p=EDGE):
    """one query of REDUCE_SLOTS * FS_TILE + 1 pattern records (a 2048-record tile repeated): 257 tiles, thread 0 of k_freespace_reduce sums two slots"""
    c = Case("reduce-tiles", p, [checkerboard(p)])
    _shell_expect(c, 0)
    n = REDUCE_SLOTS * FS_TILE + 1
    a, e = pattern_records(p, mixed(FS_TILE, 3))
    reps = n // FS_TILE + 1
    c.clouds.append(np.tile(a, (reps, 1))[:n])
    c.expect["cls"][(0, 0)] = np.tile(e["cls"], reps)[:n]
    c.meta["finite"] = {(0, 0): np.tile(e["finite"], reps)[:n]}
    c.expect["pixels"][1] = (e["pixels"], e["near"], e["far"]); c.expect["kept"][1] = np.tile(e["kept"], reps)[:n]
    c.pairs.append((1, 0, np.eye(4)))
    return c


def full_counters(p=EDGE):
    """255 witnesses: entry 0 = 300 pattern records seen by 255 entries of the 30 m shell; entry 1 = the same keyframe seen by 128 of them and 127 entries of
    a shell at 100 m (every kept record on a filled pixel is seen through by those): class 2 -> (255, 0), class 4 -> (127, 128), class 3 -> (127, 0)"""
    c = Case("full-counters", p, [checkerboard(p), checkerboard(p, 100.0)], rules=[(255, 0), (1, 0xFFFFFFFF), (2, 1)])
    _shell_expect(c, 0); _shell_expect(c, 1, 100.0)
    kf, e = _add_pattern(c, mixed(300, 11))
    seq = e["cls"]
    ids = [kf, kf] + [0] * MAX_WITNESSES + [1] * 127
    near_w = list(range(2, 2 + MAX_WITNESSES)); far_w = list(range(2 + MAX_WITNESSES, 2 + MAX_WITNESSES + 127))
    off, wit = witness_csr([near_w, near_w[:128] + far_w] + [[]] * (len(ids) - 2))
    c.entries = dict(ids=ids, poses=[np.eye(4)] * len(ids), wit_off=off, wit=wit)
    u8 = lambda v: v.astype(np.uint8)
    on_filled = (seq >= 2)
    c.expect["votes"][0] = (u8(255 * (seq == 2)), u8(255 * (seq == 4)))
    c.expect["votes"][1] = (u8(128 * (seq == 2) + 127 * on_filled), u8(128 * (seq == 4)))
    for e_ in range(2, len(ids)):
        c.expect["votes"][e_] = (np.zeros(len(c.clouds[ids[e_]]), np.uint8),) * 2
    return c


# ---- knife edges: transformed points within a few ulps of column boundary j and row edge i
def knife_columns(p):
    nc = p.n_cols
    return sorted({1, 2, nc // 8 + 1, nc // 4, nc // 4 + 1, 3 * nc // 8, nc // 2 - 1, nc // 2, nc // 2 + 3, 5 * nc // 8 + 2, 3 * nc // 4, 3 * nc // 4 + 1, 7 * nc // 8, nc - 2, nc - 1})


def knife_rows(p):
    return [0, p.n_rows // 2, p.n_rows]


def knife_transform(tabs, j, i, shift=0):
    """diag(c[j], s[j], t[i]): (rad, rad, rad) -> (fl(c rad), fl(s rad), fl(t rad)), on boundary j's direction and on edge i's cone up to the products' rounding.
    shift: 1 adds the f64 translation tau (c, s, t)[j, i] - the sums round once more and the point stays on both; 2 adds tau (c, s, 0) - on the boundary, rho
    longer by tau, so the point leaves the row edge (a control: far from the edge nothing may flip)."""
    t, c, s = tabs
    T = np.diag([c[j], s[j], t[i], 1.0])
    if shift:
        tau = 0.001 * (1.0 + 2.0 ** -30)
        T[:3, 3] = [c[j] * tau, s[j] * tau, t[i] * tau if shift == 1 else 0.0]
    return T


def knife_radii(n, salt):
    """f32 radii 8 .. 25 m: with |t| < 0.6 the range stays between the parity shell's 2 m and 200 m"""
    return weyl(n, 8.0, 25.0, salt).astype(np.float32)


def _two_product(a):
    """a * a = p + e exactly (Dekker / Veltkamp), elementwise on f64"""
    p = a * a
    h = a * 134217729.0
    ah = h - (h - a); al = a - ah
    return p, ((ah * ah - p) + 2.0 * ah * al) + al * al


def rho2_rounded_once(x, y):
    """x x + y y with a single rounding, elementwise on f64: the exact products as double-doubles, their sum by two-sum, the tails added last (exact short of a tie
    in the 105th bit; the CPU module re-measures with rationals)"""
    p, ep = _two_product(x); q, eq = _two_product(y)
    s = p + q
    v = s - p
    es = (p - (s - v)) + (q - v)
    return s + (es + (ep + eq))


def row_flips(P, ti):
    """per transformed point: does z >= rho t[i] change when rho2 is rounded once?"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return (z >= np.sqrt(x * x + y * y) * ti) != (z >= np.sqrt(rho2_rounded_once(x, y)) * ti)


def knife(p, name, n_rec=200, n_sel=40, pool=1024):
    """keyframe 0 the parity shell around every used crossing; one pair per (column, row, shift) - at least 32 pairs - each with a query keyframe of its own:
    n_rec diagonal records (rad, rad, rad).  The radii are the first of a pool of `pool` Weyl values, except that up to n_sel of them are the pool's first
    values whose row predicate changes when rho2 is rounded once (the plain construction puts 3-4 % of its points that close to the row edge; a third of them
    sit that close to the column boundary without any selection).  The same geometry as votes through P_w = I, P_e = the transform."""
    tabs = fs.tables(p)
    J, I = knife_columns(p), knife_rows(p)
    rows = sorted({r for i in I for r in range(i - 2, i + 2) if 0 <= r < p.n_rows})
    cols = sorted({(j + d) % p.n_cols for j in J for d in range(-2, 2)})
    rr, cc = np.meshgrid(rows, cols, indexing="ij")
    c = Case(name, p, [parity_shell(p, rr.reshape(-1), cc.reshape(-1))])
    edges = []
    for a, j in enumerate(J):
        for b, i in enumerate(I):
            shift = (a + b) % 3 if (a + b) % 3 != 2 or a % 2 else 0           # mostly 0 and 1; a few controls with shift 2
            T = knife_transform(tabs, j, i, shift)
            rad = knife_radii(pool, 1000 * len(edges))
            take = np.zeros(pool, bool)
            if shift != 2:
                take[np.flatnonzero(row_flips(fs.transform(np.stack([rad, rad, rad], axis=1), T), tabs[0][i]))[:n_sel]] = True
            take[np.flatnonzero(~take)[:n_rec - int(take.sum())]] = True
            c.pairs.append((len(c.clouds), 0, T))
            c.clouds.append(np.stack([rad[take]] * 3, axis=1))
            edges.append((j, i, shift))
    c.meta["edges"] = edges
    ids = [0] + [q for q, _, _ in c.pairs]
    off, wit = witness_csr([[]] + [[0]] * len(c.pairs))
    c.entries = dict(ids=ids, poses=[np.eye(4)] + [T for _, _, T in c.pairs], wit_off=off, wit=wit)
    return c


def _as_written(c, s, x, y):
    return c * y - s * x >= 0.0


def column_flip_share(case):
    """of the case's transformed points, the share whose predicate against their OWN boundary j changes when c[j] y - s[j] x is rounded once (exact rationals)
    -> (flips, points)"""
    t, c, s = fs.tables(case.params)
    flips = total = 0
    for (q, _, T), (j, i, shift) in zip(case.pairs, case.meta["edges"]):
        P = fs.transform(case.clouds[q], T)
        for x, y in zip(P[:, 0].tolist(), P[:, 1].tolist()):
            exact = Fraction(float(c[j])) * Fraction(y) - Fraction(float(s[j])) * Fraction(x) >= 0
            flips += bool(_as_written(float(c[j]), float(s[j]), x, y)) != exact; total += 1
    return flips, total


def row_flip_share(case):
    """of the case's transformed points that sit on a row edge (shift 0 or 1), the share whose predicate z >= rho t[i] against their OWN edge i changes when
    rho2 = x x + y y is rounded once -> (flips, points)"""
    t = fs.tables(case.params)[0]
    flips = total = 0
    for (q, _, T), (j, i, shift) in zip(case.pairs, case.meta["edges"]):
        if shift == 2:
            continue
        P = fs.transform(case.clouds[q], T)
        for x, y, z in P.tolist():
            two = math.sqrt(x * x + y * y)
            one = math.sqrt(float(Fraction(x) * Fraction(x) + Fraction(y) * Fraction(y)))
            flips += (z >= two * float(t[i])) != (z >= one * float(t[i])); total += 1
    return flips, total


# ---- thresholds
def exact_triples(limit=48):
    """integer (a, b, c), a, b > 0, with a a + b b + c c a perfect square: r is an integer, exact in f32 and f64 alike"""
    out = []
    for a in range(1, limit):
        for b in range(1, limit):
            for c in range(0, limit):
                r2 = a * a + b * b + c * c
                r = math.isqrt(r2)
                if r * r == r2 and r >= 2:
                    out.append((a, b, c))
    return out


def _pixel_of(p, x, y, z, margin=1e-6):
    """the pixel of a point by atan2 (generator only; None within `margin` rad of an edge or outside the field of view)"""
    el = math.atan2(z, math.hypot(x, y)); az = math.atan2(y, x) % (2.0 * math.pi)
    fr = (el - p.el_lo) / (p.el_hi - p.el_lo) * p.n_rows; fc = az / (2.0 * math.pi) * p.n_cols
    if not (0 < fr < p.n_rows) or min(fr % 1.0, 1.0 - fr % 1.0) * (p.el_hi - p.el_lo) / p.n_rows < margin or min(fc % 1.0, 1.0 - fc % 1.0) * 2.0 * math.pi / p.n_cols < margin:
        return None
    return int(fr), int(fc) % p.n_cols


def zero_tolerance(p=EDGE):
    """tol_abs = tol_rel = 0, a scan against a copy of itself through the identity, one return per pixel: near = far = float32(r), so the class is 2, 3 or 4 as
    the f64 r is below, above or equal to float64(float32(r)).  Pixels with row + column = 0, 1 mod 5 hold an integer triple (r exact: class 4), the others a
    pixel centre at a Weyl range (2 or 3 by the rounding of its r)."""
    p0 = with_(p, tol_abs=0.0, tol_rel=0.0)
    taken, recs, exact = {}, [], []
    for a, b, c in exact_triples():
        for sa, sb, sc, sw in ((1, 1, 1, 0), (-1, 1, -1, 0), (-1, -1, 1, 1), (1, -1, -1, 1), (1, 1, -1, 0), (-1, 1, 1, 1)):
            x, y, z = (sa * a, sb * b, sc * c) if not sw else (sa * b, sb * a, sc * c)
            pix = _pixel_of(p0, x, y, z)
            if pix is not None and (pix[0] + pix[1]) % 5 < 2 and pix not in taken and math.sqrt(x * x + y * y + z * z) >= p0.min_range:
                taken[pix] = True; recs.append((x, y, z)); exact.append(True)
    rows, cols = np.meshgrid(np.arange(p0.n_rows), np.arange(p0.n_cols), indexing="ij")
    free = np.array([(r, c) for r, c in zip(rows.reshape(-1), cols.reshape(-1)) if (r, c) not in taken])
    generic = centres(p0, free[:, 0], free[:, 1], weyl(len(free), 3.0, 90.0))
    cloud = np.concatenate([np.array(recs, np.float32).reshape(-1, 3), generic])
    r64 = [math.sqrt((x * x + y * y) + z * z) for x, y, z in cloud.astype(np.float64).tolist()]
    r32 = [float(np.float32(r)) for r in r64]
    cls = np.array([2 if r < q else (3 if r > q else 4) for r, q in zip(r64, r32)], np.uint8)
    c = Case("zero-tolerance", p0, [cloud, cloud.copy()], pairs=[(0, 1, np.eye(4))])
    c.expect["cls"][(0, 0)] = cls; c.expect["cls"][(0, 1)] = cls
    c.meta["finite"] = {(0, 0): np.ones(len(cls), bool), (0, 1): np.ones(len(cls), bool)}
    c.meta["exact"] = len(recs)
    off, wit = witness_csr([[1], [0]])
    c.entries = dict(ids=[0, 1], poses=[np.eye(4), np.eye(4)], wit_off=off, wit=wit)
    c.expect["votes"][0] = c.expect["votes"][1] = ((cls == 2).astype(np.uint8), (cls == 4).astype(np.uint8))
    c.expect["kept"][0] = c.expect["kept"][1] = np.ones(len(cls), bool)
    return c


def _inward(v):
    """the record with its largest coordinate one f32 ulp nearer to zero"""
    v = np.array(v, np.float32)
    k = int(np.argmax(np.abs(v)))
    v[k] = np.nextafter(v[k], np.float32(0.0))
    return v


def min_range_edge(scale=1.0, p=EDGE):
    """min_range = 5 * scale (a power of two): the twelve in-plane records with r = min_range exactly - kept, r >= min_range - and each moved one f32 ulp
    inward - dropped.  z = 0 lies on edge n_rows / 2 (t = tan(0) = 0, 0 >= rho * 0 holds): row n_rows / 2, by the definition."""
    pm = with_(p, min_range=5.0 * scale)
    on = [(sx * a, sy * b, 0.0) for a, b in ((3.0, 4.0), (4.0, 3.0)) for sx in (1, -1) for sy in (1, -1)] + [(5.0, 0.0, 0.0), (-5.0, 0.0, 0.0), (0.0, 5.0, 0.0), (0.0, -5.0, 0.0)]
    on = np.array(on, np.float32) * np.float32(scale)
    on[1, 2] = -0.0; on[8, 1] = -0.0; on[9, 1] = -0.0; on[9, 2] = -0.0            # a negative zero is a zero: the half-plane test and the row edge see 0
    cloud = np.concatenate([on, np.array([_inward(v) for v in on])])
    kept = np.r_[np.ones(len(on), bool), np.zeros(len(on), bool)]
    far = checkerboard(pm, 40.0 * scale)                                          # the other keyframe of the pair
    c = Case("min-range-%g" % (5.0 * scale), pm, [cloud, far], pairs=[(0, 1, np.eye(4))])
    c.expect["kept"][0] = kept
    c.meta["dropped"] = {(0, 0): ~kept}
    off, wit = witness_csr([[1], [0]])
    c.entries = dict(ids=[0, 1], poses=[np.eye(4), np.eye(4)], wit_off=off, wit=wit)
    return c


def beyond_f32(p=EDGE):
    """a record whose r exceeds the f32 maximum: float32(r) = +inf, so near stays +inf and far becomes +inf; a second record in the same pixel at 30 m sees an
    unobserved pixel there; -0.0 coordinates beside it"""
    big = np.array([[3.0e38, 2.0e38, 0.5e38]], np.float32)
    pix = _pixel_of(p, *big[0].astype(np.float64).tolist())
    probe = centres(p, [pix[0]], [pix[1]], 30.0)
    zeros = np.array([[6.0, -0.0, 1.0], [-6.0, -0.0, 1.0], [-0.0, 6.0, -1.0], [-0.0, -6.0, -1.0], [-0.0, -0.0, 3.0], [7.0, 0.0, -0.0]], np.float32)
    c = Case("beyond-f32", p, [np.concatenate([big, zeros]), np.concatenate([probe, zeros])], pairs=[(1, 0, np.eye(4))])
    c.meta["inf_pixel"] = pix
    c.expect["cls"][(0, 0)] = np.array([1, 4, 4, 4, 4, 0, 4], np.uint8)            # the probe meets the +inf pixel; (-0, -0, 3) is on the z axis
    c.meta["finite"] = {(0, 0): np.ones(7, bool)}
    off, wit = witness_csr([[1], [0]])
    c.entries = dict(ids=[0, 1], poses=[np.eye(4), np.eye(4)], wit_off=off, wit=wit)
    return c


def subnormals(p=EDGE):
    """min_range = 0: f32 subnormal coordinates (r ~ 1e-40, float32(r) subnormal too), exact zeros beside them; tol_abs = 0 so that 1e-40 is not inside it"""
    ps = with_(p, min_range=0.0, tol_abs=0.0, tol_rel=0.25)
    rows, cols = even_pixels(ps)
    a = (centres(ps, rows, cols, 1.0).astype(np.float64) * weyl(len(rows), 1e-41, 9e-39)[:, None]).astype(np.float32)
    b = (a.astype(np.float64) * np.where(np.arange(len(a)) % 3 == 0, 1.0, np.where(np.arange(len(a)) % 3 == 1, 3.0, 0.25))[:, None]).astype(np.float32)
    extra = np.array([[0.0, 0.0, 0.0], [-0.0, 1e-45, 0.0], [1e-45, 0.0, 0.0]], np.float32)
    c = Case("subnormals", ps, [np.concatenate([a, extra]), np.concatenate([b, extra])], pairs=[(0, 1, np.eye(4))])
    off, wit = witness_csr([[1], [0]])
    c.entries = dict(ids=[0, 1], poses=[np.eye(4), np.eye(4)], wit_off=off, wit=wit)
    return c


def thresholds():
    return [zero_tolerance(), min_range_edge(1.0), min_range_edge(0.25), min_range_edge(8.0), beyond_f32(), subnormals()]


# ---- the twin on a case (shared by the CPU and the GPU module)
def twin_images(case):
    tabs = fs.tables(case.params)
    with np.errstate(over="ignore"):                     # (a range beyond the f32 maximum becomes +inf, on purpose)
        return [fs.range_images(c, case.params, tabs) for c in case.clouds]


def twin_pairs(case, images=None):
    """-> per pair (direction 0 record with classes, direction 1 record with classes)"""
    im = twin_images(case) if images is None else images
    out = []
    for q, c, T in case.pairs:
        r = fs.freespace(case.clouds[q], case.clouds[c], T, case.params, points=True, q_images=im[q], c_images=im[c])
        out.append((r["q_in_c"], r["c_in_q"]))
    return out


def twin_votes(case, images=None):
    """-> per entry (seen_through, agree): staticmap.votes evaluated once per distinct (keyframe, pose, witnesses' keyframes and poses) - it is a function of
    exactly those"""
    e = case.entries
    im = twin_images(case) if images is None else images
    ids = [int(i) for i in e["ids"]]
    P = [np.asarray(x, np.float64) for x in e["poses"]]
    pk = [x.tobytes() for x in P]
    off, wit = e["wit_off"], e["wit"]
    memo, out = {}, []
    for k in range(len(ids)):
        ws = [int(w) for w in wit[off[k]:off[k + 1]]]
        key = (ids[k], pk[k], tuple((ids[w], pk[w]) for w in ws))
        if key not in memo:
            sub_ids = [ids[k]] + [ids[w] for w in ws]
            so, sw = witness_csr([list(range(1, len(ws) + 1))] + [[]] * len(ws))
            memo[key] = sm.votes(dict(enumerate(case.clouds)), dict(enumerate(im)), sub_ids, [P[k]] + [P[w] for w in ws], so, sw, case.params)[0]
        out.append(memo[key])
    return out


# ---- the table
import functools

CASES = {"seams": seams, "seams-wide": lambda: seams(WIDE, [65, FS_TILE + 1], "seams-wide"), "scan-tiles": scan_tiles, "many-entries": many_entries,
         "reduce-tiles": reduce_tiles, "full-counters": full_counters, "knife-32x720": lambda: knife(KNIFE, "knife-32x720"),
         "knife-2x4608": lambda: knife(WIDE, "knife-2x4608")}
CASES.update({c: (lambda k: lambda: thresholds()[k])(k) for k, c in enumerate(["zero-tolerance", "min-range-5", "min-range-1.25", "min-range-40", "beyond-f32", "subnormals"])})
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def get(name):
    c = CASES[name]()
    assert c.name == name, (c.name, name)
    return c
