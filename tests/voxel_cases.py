"""The case table of the voxel-grid pipeline (voxel_submaps, csrc/qn_cloud.hip): deterministic inputs, each built to reach one branch of the
pipeline, and the branch asserted FROM THE INPUTS - with the numpy guard (voxel_guard, tests/test_kf_map_api.py) and the small restatements of
the engine's host logic below (bits_for, sort_groups, radix_items, tiles_of) - never from engine output.  Whoever changes those functions in
qn_cloud.hip changes them here, and sees which cases stop reaching their branch.

A case: keyframes (xyz, optional intensity), one pose per keyframe, submap lists (keyframe indices; one list = a single-submap case, which also
runs through the map), the leaf, and `expect`: the properties check() asserts.  tests/test_voxel_reference_cpu.py holds the two references (C++
oracle, numpy restatement) to each other on every case; tests/test_gpu_voxel_edges.py holds the engine to them.  No random draws: points come
from a Weyl sequence (fractional parts of multiples of fixed irrationals)."""
import functools
import numpy as np

from test_kf_map_api import voxel_guard

MAP_TILE = 4096                  # QN_MAP_TILE
MAP_ITEMS = 16                   # QN_MAP_ITEMS = QN_MAP_TILE / QN_BLOCK
INT32_MAX = 2 ** 31 - 1
RADIX_SWITCH = 256 * MAP_TILE    # 2^20 keys of one sort group: radix_items switches to MAP_TILE-key tiles


# ---- the engine's host logic, restated
def bits_for(v):
    """smallest b with v < 2^b"""
    b = 0
    while (1 << b) <= v:
        b += 1
    return b


def tiles_of(n):
    return (n + MAP_TILE - 1) // MAP_TILE


def radix_items(n):
    return 1 if n < RADIX_SWITCH else MAP_ITEMS


def sort_groups(lbits):
    """-> [(s0, s1, L, sb)]: consecutive submaps whose (submap, leaf) fields fit 32 key bits"""
    groups, g0, L = [], 0, 0
    for t in range(len(lbits)):
        L2 = max(L, lbits[t])
        if t > g0 and L2 + bits_for(t - g0) > 32:
            groups.append((g0, t, L, bits_for(t - 1 - g0))); g0 = t; L = lbits[t]
        else:
            L = L2
    groups.append((g0, len(lbits), L, bits_for(len(lbits) - 1 - g0)))
    return groups


# ---- cases
class Case:
    def __init__(self, name, kfs, lists, leaf, expect, poses=None, inten=None):
        self.name = name
        self.kfs = [np.ascontiguousarray(k, np.float32).reshape(-1, 3) for k in kfs]
        self.poses = [np.eye(4) for _ in kfs] if poses is None else [np.asarray(p, np.float64) for p in poses]
        # intensity on every other keyframe unless given: a keyframe without one carries 0 into the map
        self.inten = [intensity(len(k), i) if i % 2 else None for i, k in enumerate(self.kfs)] if inten is None else inten
        self.lists = [list(l) for l in lists]
        self.leaf = leaf
        self.expect = expect

    def pose_lists(self, lists=None):
        return [[self.poses[i] for i in l] for l in (self.lists if lists is None else lists)]

    def concat(self, l):
        """the transformed concatenation of one list -> (n, 4) f32, w = the intensity (0 for a keyframe without)"""
        parts = [np.zeros((0, 4), np.float32)]
        for i in l:
            p = np.zeros((len(self.kfs[i]), 4), np.float32)
            p[:, :3] = transform(self.kfs[i], self.poses[i])
            if self.inten[i] is not None:
                p[:, 3] = self.inten[i]
            parts.append(p)
        return np.concatenate(parts)


def transform(xyz, T):
    """transformPcd in the engine's f64 arithmetic and order (tests/test_kf_map_api.py transform_xyzi); 0 * inf = NaN is a value here, not an error"""
    x, y, z = (xyz[:, d].astype(np.float64) for d in range(3))
    out = np.empty((len(xyz), 3), np.float32)
    with np.errstate(invalid="ignore"):
        for r in range(3):
            out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def derive(case, lists=None):
    """what the pipeline's host logic does with these inputs -> dict(sub=[per submap: n, nfin, nonfinite, tripped, cells, lbits],
    groups=[per sort group: s0, s1, L, sb, passes, npts, items])"""
    sub = []
    for l in (case.lists if lists is None else lists):
        cat = case.concat(l)
        fin = cat[np.isfinite(cat[:, :3]).all(1)]
        d = dict(n=len(cat), nfin=len(fin), nonfinite=len(cat) - len(fin), tripped=None, cells=None)
        sentinel = 1
        if len(fin):
            d["tripped"], _, div = voxel_guard(fin[:, :3].min(0), fin[:, :3].max(0), case.leaf)
            if not d["tripped"]:
                d["cells"] = sentinel = div[0] * div[1] * div[2]
        d["lbits"] = bits_for(sentinel if d["nonfinite"] else sentinel - 1)
        sub.append(d)
    p0 = np.r_[0, np.cumsum([d["n"] for d in sub])]
    groups = []
    for s0, s1, L, sb in sort_groups([d["lbits"] for d in sub]):
        npts = int(p0[s1] - p0[s0])
        groups.append(dict(s0=s0, s1=s1, L=L, sb=sb, passes=(L + sb + 7) // 8, npts=npts, items=radix_items(npts)))
    return dict(sub=sub, groups=groups)


def check(case):
    """assert the branch the case exists to hit, from its inputs; returns derive(case)"""
    d = derive(case); e = case.expect; name = case.name
    per_sub = lambda key: [s[key] for s in d["sub"]]
    per_group = lambda key: [g[key] for g in d["groups"]]
    live = [g for g in d["groups"] if g["npts"]]
    got = dict(tripped=per_sub("tripped"), cells=per_sub("cells"), lbits=per_sub("lbits"), nfin=per_sub("nfin"), nonfinite=per_sub("nonfinite"),
               groups=len(d["groups"]), L=per_group("L"), sb=per_group("sb"), key_bits=[g["L"] + g["sb"] for g in d["groups"]],
               passes=per_group("passes"), items=per_group("items"), group_points=per_group("npts"),
               copy=any(g["passes"] % 2 != live[0]["passes"] % 2 for g in live) if live else False,      # a group ends in the other ping-pong buffer
               sizes=[len(k) for k in case.kfs], tiles=[tiles_of(len(k)) for k in case.kfs])
    for key, want in e.items():
        if key in got:
            assert got[key] == want, (name, key, got[key], want)
    if "min_abs_scaled" in e:                # some |coordinate * inv| of the concatenation reaches this (f32 integers are no longer all representable past 2^24)
        inv = np.float32(1) / np.float32(case.leaf)
        assert max(float(np.abs(case.concat(l)[:, :3] * inv).max()) for l in case.lists if l) >= e["min_abs_scaled"], name
    if "borders" in e:                       # at least this many listed values sit in another leaf than their lower f32 neighbour
        inv = np.float32(1) / np.float32(case.leaf)
        v = np.unique(np.concatenate([k.reshape(-1) for k in case.kfs]))
        assert int((np.floor(v * inv) != np.floor(np.nextafter(v, np.float32(-np.inf)) * inv)).sum()) >= e["borders"], name
    return d


_ALPHA = np.array([0.8191725133961645, 0.6710436067037893, 0.5497004779019703])     # 1/g, 1/g^2, 1/g^3 of g^4 = g + 1: a 3-D Weyl sequence


def fill(n, lo, hi, salt=0):
    """n points of the Weyl sequence in the box [lo, hi) (scalars or 3-vectors)"""
    u = ((np.arange(1, n + 1, dtype=np.float64)[:, None] + salt) * _ALPHA) % 1.0
    lo = np.broadcast_to(np.asarray(lo, np.float64), (3,)); hi = np.broadcast_to(np.asarray(hi, np.float64), (3,))
    return (lo + u * (hi - lo)).astype(np.float32)


def intensity(n, k):
    return ((np.arange(n) * 37 + 11 * k) % 256).astype(np.float32)


def boxed(n, lo, hi, salt=0):
    """the two corners lo, hi of a box and n Weyl points strictly inside it: the cloud's bounding box is exactly [lo, hi]"""
    lo = np.broadcast_to(np.asarray(lo, np.float64), (3,)); hi = np.broadcast_to(np.asarray(hi, np.float64), (3,))
    m = (hi - lo) * 1e-3
    return np.concatenate([np.float32(lo)[None], fill(n, lo + m, hi - m, salt), np.float32(hi)[None]])


def with_nan(k, at=None):
    """the keyframe with one NaN point inserted (in the middle unless told)"""
    at = len(k) // 2 if at is None else at
    return np.insert(np.asarray(k, np.float32), at, [np.nan, 0.0, 1.0], axis=0)


def yaw_pose(a, t):
    T = np.eye(4); T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; T[:3, 3] = t
    return T


CASES = {}


def case(fn):
    CASES[fn.__name__.replace("_", "-")] = fn
    return fn


def variants(names):
    def deco(fn):
        for tag, arg in names:
            CASES[fn.__name__.replace("_", "-") + ("-" + tag if tag else "")] = functools.partial(fn, arg)
        return fn
    return deco


@functools.lru_cache(maxsize=2)
def get(name):
    fn = CASES[name]
    c = fn()
    c.name = name
    return c


# ---- sizes: keyframes around the 256-point block and the 4096-point tile (tile_pos, tiles_of, the per-tile boxes)
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8193]


def _size_keyframes():
    kfs = [fill(n, -20.0, 20.0, salt=1000 * i) for i, n in enumerate(SIZES)]
    poses = [yaw_pose(0.1 * i, [0.5 * i, -0.3 * i, 0.02 * i]) for i in range(len(SIZES))]
    return kfs, poses


@case
def sizes_one_submap():
    kfs, poses = _size_keyframes()
    return Case("", kfs, [[3, 1, 8, 0, 4, 6, 2, 5, 7]], 0.3, dict(sizes=SIZES, tiles=[0, 1, 1, 1, 1, 1, 1, 2, 3], tripped=[False], groups=1), poses)


@case
def sizes_batch():
    kfs, poses = _size_keyframes()
    lists = [[i] for i in range(len(SIZES))] + [[6, 0, 7], [5, 6], [8, 2], [1, 0, 0, 1], [7, 7]]
    return Case("", kfs, lists, 0.3, dict(sizes=SIZES, tripped=[None] + [False] * 13, groups=1, nfin=SIZES + [8193, 8191, 8448, 2, 8194]), poses)


# ---- the radix switch: one sort group's keys at 2^20 - 1, 2^20, 2^20 + 1 (radix_items: one key per thread below, MAP_TILE-key tiles from there on)
def _million(total):
    """8 keyframes of `total` points together in a 200 m x 200 m x 50 m box: ~7e7 leaves at 0.3, a few points per leaf"""
    each = [131072] * 7 + [total - 7 * 131072]
    return [fill(n, [-100.0, -100.0, -25.0], [100.0, 100.0, 25.0], salt=131072 * i) for i, n in enumerate(each)]


@variants([("below", RADIX_SWITCH - 1), ("at", RADIX_SWITCH), ("above", RADIX_SWITCH + 1)])
def radix_switch(total):
    return Case("", _million(total), [list(range(8))], 0.3,
                dict(group_points=[total], items=[1 if total < RADIX_SWITCH else MAP_ITEMS], groups=1, tripped=[False], passes=[4]))


@case
def radix_switch_two_groups():
    """{A, B} sort in tiles, {C} one key per thread: A's 31 leaf bits close the group at the third submap"""
    a = np.concatenate([boxed(131070, 0.5, 1289.5, salt=131072 * i) for i in range(8)])           # 2^20 points, 1290^3 cells
    return Case("", [a, fill(300, 0.0, 30.0, 7), fill(5000, -30.0, 30.0, 9)], [[0], [1], [2]], 1.0,
                dict(groups=2, items=[MAP_ITEMS, 1], group_points=[RADIX_SWITCH + 300, 5000], L=[31, 18], sb=[1, 0], tripped=[False] * 3))


# ---- leaf bits: cells at and around the digit borders, with and without the sentinel leaf's bit
LEAF_BITS = [(1, (1, 1, 1)), (2, (2, 1, 1)), (255, (15, 17, 1)), (256, (16, 4, 4)), (257, (257, 1, 1)), (2 ** 16 - 1, (255, 257, 1)),
             (2 ** 16, (64, 32, 32)), (2 ** 16 + 1, (65537, 1, 1)), (2 ** 24, (256, 256, 256)), (2 ** 24 + 1, (97, 257, 673)),
             (1290 ** 3, (1290, 1290, 1290))]


@variants([("%d%s" % (cells, "-nan" if nan else ""), (cells, dims, nan)) for cells, dims in LEAF_BITS for nan in (False, True)])
def leaf_bits(arg):
    cells, dims, nan = arg
    a = boxed(1500, 0.5, np.array(dims) - 0.5, salt=1); b = fill(700, 0.25, np.array(dims) - 0.25, salt=5000)
    if nan:
        a = with_nan(a)
    L = bits_for(cells) if nan else bits_for(cells - 1)
    return Case("", [a, b], [[0, 1]], 1.0, dict(cells=[cells], lbits=[L], passes=[(L + 7) // 8], tripped=[False], nonfinite=[int(nan)], groups=1))


@variants([("", False), ("nan", True)])
def leaf_bits_long_axis(nan):
    """2147483521 cells on one axis: the largest f32 below 2^31 as a coordinate at leaf 1"""
    top = float(np.nextafter(np.float32(2.0 ** 31), np.float32(0)))
    a = boxed(1500, [0.5, 0.1, 0.1], [top, 0.9, 0.9], salt=3)
    if nan:
        a = with_nan(a)
    return Case("", [a], [[0]], 1.0, dict(cells=[2147483521], lbits=[31], passes=[4], tripped=[False], nonfinite=[int(nan)]))


@variants([("", False), ("nan", True)])
def single_point(nan):
    a = np.array([[3.25, -7.5, 0.125]], np.float32)
    if nan:
        a = with_nan(a, 0)
    return Case("", [a], [[0]], 0.3, dict(cells=[1], lbits=[int(nan)], passes=[int(nan)], nfin=[1]))


# ---- sort groups: L + bits_for(S - 1) at 32 and 33, three groups of different ping-pong parity, dead submaps inside a grouped batch
def _big30(i):
    return boxed(3000, 0.5, 999.5, salt=4000 * i)                     # 1000^3 cells: 30 leaf bits


@case
def groups_32_bits_one_group():
    return Case("", [_big30(i) for i in range(4)], [[0], [1], [2], [3]], 1.0, dict(groups=1, L=[30], sb=[2], key_bits=[32], passes=[4], cells=[10 ** 9] * 4))


@case
def groups_33_bits_two_groups():
    return Case("", [_big30(i) for i in range(5)], [[0], [1], [2], [3], [4]], 1.0,
                dict(groups=2, L=[30, 30], sb=[2, 0], key_bits=[32, 30], passes=[4, 4], copy=False))


@case
def groups_three_parities():
    """{a, tripped, [], all non-finite, b} 8 key bits, 1 pass; {31-bit, c} 32 bits, 4 passes: the other buffer, copied; {d} 20 bits, 3 passes"""
    small = lambda s: boxed(400, 0.5, 2.5, salt=s)                     # 27 cells
    allbad = np.full((300, 3), np.nan, np.float32); allbad[::2, 1] = np.inf; allbad[1::3, 2] = -np.inf
    kfs = [small(1), with_nan(boxed(500, 0.9, 1290.1, salt=2)), allbad, small(3), boxed(2500, 0.5, 1289.5, salt=4), fill(900, 0.0, 40.0, 5),
           boxed(2000, 0.5, 99.5, salt=6), np.zeros((0, 3), np.float32)]
    lists = [[0, 7], [1], [], [2, 7], [7, 3], [4], [5], [6]]
    return Case("", kfs, lists, 1.0,
                dict(groups=3, L=[5, 31, 20], sb=[3, 1, 0], passes=[1, 4, 3], copy=True, tripped=[False, True, None, None, False, False, False, False],
                     nfin=[402, 502, 0, 0, 402, 2502, 900, 2002], nonfinite=[0, 1, 0, 300, 0, 0, 0, 0]))


# ---- leaf borders: exact f32 multiples of the leaf, one ulp to either side, negative coordinates, -0.0
def _border_values(leaf, ks):
    lf = np.float32(leaf)
    v = np.array([np.float32(k) * lf for k in ks], np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf)), np.array([-0.0, 0.0], np.float32)])


@variants([(str(l), l) for l in (0.1, 0.3, 0.25, 1.0, 1e-3, 50.0)])
def leaf_borders(leaf):
    near = list(range(-12, 13)) + [-100, 100]
    vx = _border_values(leaf, near + [-4097, 4097]); vy = _border_values(leaf, near)
    i = np.arange(4 * len(vx))
    a = np.c_[vx[i % len(vx)], vy[(7 * i + 3) % len(vy)], vy[(13 * i + 5) % len(vy)]]
    return Case("", [a[:len(a) // 2], a[len(a) // 2:]], [[0, 1]], leaf, dict(tripped=[False], borders=20, groups=1))


# ---- far from the origin: the offset comes from the pose, in f64, and is rounded once
@variants([("8km-0.3", ((8000.0, -8000.0, 10.0), 0.3, 0.0)), ("utm-0.1", ((5e5, 4e6, 100.0), 0.1, 2.0 ** 24)), ("utm-0.3", ((5e5, 4e6, 100.0), 0.3, 0.0)),
           ("1e8-0.1", ((1e8, -1e8, 0.0), 0.1, 2.0 ** 24)), ("1e8-1.0", ((1e8, -1e8, 0.0), 1.0, 2.0 ** 24))])
def far(arg):
    t, leaf, scaled = arg
    kfs = [fill(3000, -15.0, 15.0, salt=1), fill(3000, -15.0, 15.0, salt=9000)]
    return Case("", kfs, [[0, 1]], leaf, dict(tripped=[False], min_abs_scaled=scaled, groups=1), [yaw_pose(0.3, t), yaw_pose(-1.1, np.array(t) + [2.5, 1.5, 0.1])])


# ---- the guard: each condition of the rule from one side and the other, each once more with a NaN point
def _outliers(*pts):
    return np.concatenate([fill(1000, -10.0, 10.0, salt=2), np.array(pts, np.float32).reshape(-1, 3)])


GUARD = [("pd-ok-cells-over", lambda: boxed(2000, 0.9, 1290.1), 1.0, True),          # pd = 1290^3 <= INT32_MAX < cells = 1291^3
         ("cells-just-under", lambda: boxed(2000, 0.9, 1289.1), 1.0, False),         # cells = 1290^3
         ("pd-just-over", lambda: boxed(2000, 0.0, 1290.0), 1.0, True),              # pd = cells = 1291^3
         ("pd-just-under", lambda: boxed(2000, 0.0, 1289.5), 1.0, False),            # pd = cells = 1290^3
         ("floor-out-of-int", lambda: np.c_[np.float32(1e9) + 64.0 * (np.arange(500) % 7), fill(500, -5.0, 5.0)[:, 1:]], 0.3, True),
         ("outlier-1e19", lambda: _outliers([1e19, 0.0, 0.0]), 0.3, True),
         ("outlier-1e30", lambda: _outliers([0.0, 1e30, 0.0]), 0.3, True),
         ("outliers-3e38", lambda: _outliers([3e38, 0.0, 0.0], [-3e38, 1.0, 0.0]), 0.3, True)]


@variants([(tag + ("-nan" if nan else ""), (make, leaf, trip, nan)) for tag, make, leaf, trip in GUARD for nan in (False, True)])
def guard(arg):
    make, leaf, trip, nan = arg
    a = np.asarray(make(), np.float32)
    n = len(a)
    if nan:
        a = with_nan(a)
    return Case("", [a], [[0]], leaf, dict(tripped=[trip], nfin=[n], nonfinite=[int(nan)], cells=[None if trip else 1290 ** 3]), inten=[intensity(len(a), 3)])


NAMES = sorted(CASES)
