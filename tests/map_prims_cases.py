"""The inputs and the references for the direct tests of the map units' shared device primitives (csrc/qn_map_compact.cuh, csrc/qn_union_find.cuh and the
geometry of csrc/qn_dense_grid.cuh through qn_kf_debug_map_prims; the records are those of include/qn_engine.h).  Pure numpy: every reference is a serial loop over Python ints or a numpy reduction in
int64, and nothing here comes from engine output.  tests/test_gpu_map_prims.py runs the device on these, tests/test_map_prims_cpu.py checks that the table is
what it says it is.

The inputs are the ones the units cannot produce and such primitives go wrong on: an extreme in lane 0, 31, 32 or 63 only; uint32_t values with the top bit set
beside small ones (a signed compare); int values around 0, INT_MIN and INT_MAX; unsigned long long values that differ only in the high or only in the low
word (a 32-bit shuffle); sums that wrap; floats with infinities, denormals, zeros of both signs and NaN; a key carried by a lane whose predicate is false;
star graphs whose centre is the highest index."""
import functools
import numpy as np

BLOCK, WAVE, WAVES, SCAN_BLOCK = 256, 64, 4, 1024
NONE = 0xffffffff
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1

LANE = np.dtype([("i", "<i4"), ("u", "<u4"), ("f", "<f4"), ("zero", "<u4"), ("q", "<u8"), ("s", "<i8")])
WAVE_OUT = np.dtype([("imin", "<i4"), ("imax", "<i4"), ("usum", "<u4"), ("umin", "<u4"), ("umax", "<u4"), ("fmin", "<f4"), ("fmax", "<f4"), ("zero", "<u4"),
                     ("qsum", "<u8"), ("qmin", "<u8"), ("ssum", "<i8"), ("zero2", "<u8")])
KEY_IN = np.dtype([("has", "<u4"), ("key", "<u4")])
KEY_OUT = np.dtype([("trip", "<u4"), ("lead", "<u4"), ("key", "<u4"), ("served", "<u4"), ("same", "<u8")])
BLOCK_IN = np.dtype([("pred", "<u4"), ("a", "<u4", (3,)), ("b", "<u8", (3,))])
BLOCK_OUT = np.dtype([("count", "<u4", (15,)), ("sum32", "<u4", (6,)), ("max32", "<u4", (6,)), ("again32", "<u4"), ("sum64", "<u8", (6,)),
                      ("max64", "<u8", (6,)), ("again64", "<u8"), ("wide", "<u8", (2,))])
EDGE_LANES = (1, 13)                                                             # the edges a lane takes: one, and k_mf_merge's up to 13
FOLD_K32, FOLD_K64 = (1, 2, 3, 5, 10), (1, 2, 3)                                 # the K of k_slot_fold the units launch, by grep over csrc/
NBS = (1, 63, 64, 1023, 1024, 1025, 2049, 4097)
TILE, RIM = 8, 10                                                                # DG_T and DG_H of csrc/qn_dense_grid.cuh: a tile's side, and with its one-voxel rim
VOXEL = np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("index", "<u4"), ("tile", "<u4"), ("place", "<u4"), ("pos", "<u4"), ("zero", "<u4")])
# (W, H, D): one side below, at and above the tile side on each axis, a one-voxel axis in each position, more than one 256-lane block, a partial last block
GRID_SHAPES = ((1, 1, 1), (8, 8, 8), (7, 9, 8), (9, 17, 1), (16, 8, 9), (300, 1, 1), (1, 1, 300))


def _rng(*seed):
    return np.random.default_rng([7, 31] + [int(s) for s in seed])


# ---------------------------------------------------------------------------------------------------------------- 0: the wave folds
def _wave(i=0, u=0, f=0.0, q=0, s=0):
    w = np.zeros(WAVE, LANE)
    w["i"], w["u"], w["f"], w["q"], w["s"] = i, u, f, q, s
    return w


def _at(lane, there, elsewhere, dtype):
    a = np.full(WAVE, elsewhere, dtype)
    a[lane] = there
    return a


@functools.lru_cache(None)
def wave_cases():
    """-> (names, (waves, 64) LANE): one wave per named case"""
    r = _rng(0)
    lanes = np.arange(WAVE)
    cases = {}
    for lane in (0, 31, 32, 63):
        # the smallest in one lane only, every other lane the neutral element of min (and, for the sums, the one non-zero term)
        cases["low@%d" % lane] = _wave(_at(lane, -3, INT_MAX, "i4"), _at(lane, 5, M32, "u4"), _at(lane, -1.5, np.inf, "f4"), _at(lane, (1 << 40) + 3, M64, "u8"),
                                       _at(lane, -(1 << 40) - 1, 0, "i8"))
        # the largest in one lane only, every other lane the neutral element of max
        cases["high@%d" % lane] = _wave(_at(lane, 3, INT_MIN, "i4"), _at(lane, 0x80000001, 0, "u4"), _at(lane, 2.5, -np.inf, "f4"), _at(lane, (1 << 63) + 9, 0, "u8"),
                                        _at(lane, 1 << 41, 0, "i8"))
    cases["all equal"] = _wave(-7, 0x90000000, 1.25, (5 << 32) | 1, -3)
    cases["top bit beside small"] = _wave(np.tile(np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX, 2], "i4"), 8)[r.permutation(WAVE)],
                                          np.where(lanes % 3 == 0, 0x80000000 + r.integers(0, 1 << 31, WAVE), r.integers(1, 100, WAVE)).astype("u4"),
                                          r.normal(size=WAVE), r.integers(0, 1 << 63, WAVE, dtype=np.uint64) | np.uint64(1 << 63) * (lanes % 2 == 0).astype("u8"),
                                          r.integers(-(1 << 62), 1 << 62, WAVE))
    # the smallest u32 has the top bit set too: every value >= 2^31; ints all negative but one INT_MAX
    cases["all top bit"] = _wave(_at(17, INT_MAX, -5, "i4") - lanes.astype("i4"), (0x80000000 + r.permutation(WAVE) * 1000).astype("u4"), -0.0,
                                 np.uint64(1 << 63) + r.permutation(WAVE).astype("u8"), -1)
    perm, perm2 = r.permutation(WAVE).astype("u8"), r.permutation(WAVE).astype("u8")
    cases["u64 high word only"] = _wave(q=((perm + np.uint64(3)) << np.uint64(32)) | np.uint64(0x12345678), s=((perm2.astype("i8") - 32) << 32) | 0x0abcdef0)
    cases["u64 low word only"] = _wave(q=(np.uint64(7) << np.uint64(32)) | (perm + np.uint64(0x80000000)), s=(-9 << 32) | (perm2.astype("i8") + 5))
    cases["sums wrap"] = _wave(u=0xf0000000 + lanes, q=(1 << 62) + (lanes.astype("u8") << np.uint64(33)), s=np.where(lanes % 2 == 0, 1 << 61, (1 << 61) + 1))
    cases["u64 sum above 2^40"] = _wave(u=(1 << 26) - 1, q=(1 << 40) + lanes.astype("u8"), s=-(1 << 40) - lanes)
    f = r.normal(size=WAVE).astype("f4")
    cases["inf"] = _wave(f=np.where(lanes == 9, np.inf, np.where(lanes == 40, -np.inf, f)))
    cases["denormals"] = _wave(f=(np.where(lanes % 2 == 0, 1, -1) * (r.permutation(WAVE) + 1)).astype("i4").astype("f4") * np.float32(1.401298464324817e-45))
    cases["positive denormals"] = _wave(f=(r.permutation(WAVE) + 2).astype("f4") * np.float32(1.401298464324817e-45))
    cases["zeros of both signs"] = _wave(f=np.where(lanes % 2 == 0, 0.0, -0.0))
    for lane in (0, 32, 63):
        cases["NaN@%d" % lane] = _wave(f=np.where(lanes == lane, np.nan, f))
    cases["NaN but lane 5"] = _wave(f=np.where(lanes == 5, 4.5, np.nan))
    cases["NaN everywhere"] = _wave(f=np.nan)
    for k in range(5):
        rr = _rng(1, k)
        cases["random %d" % k] = _wave(rr.integers(INT_MIN, INT_MAX, WAVE, endpoint=True), rr.integers(0, M32, WAVE, endpoint=True, dtype=np.uint64).astype("u4"),
                                       (rr.normal(size=WAVE) * 10.0 ** rr.integers(-30, 30, WAVE)).astype("f4"), rr.integers(0, M64, WAVE, endpoint=True, dtype=np.uint64),
                                       rr.integers(-(1 << 63), (1 << 63) - 1, WAVE, endpoint=True))
    names = list(cases)
    while len(names) % WAVES:
        cases["pad %d" % len(names)] = _wave()
        names.append("pad %d" % len(names))
    return names, np.stack([cases[k] for k in names])


def _fold_f32(vals, pick):
    """fminf / fmaxf over the lanes: a NaN lane is ignored unless every lane is NaN"""
    vals = [np.float32(v) for v in vals if not np.isnan(v)]
    return pick(vals) if vals else np.float32(np.nan)


def wave_reference(waves):
    """(W, 64) LANE -> (W,) WAVE_OUT by serial loops over Python ints; the sums are modular"""
    out = np.zeros(len(waves), WAVE_OUT)
    for k, w in enumerate(waves):
        i, u, q, s = ([int(v) for v in w[c]] for c in "iuqs")
        ssum = sum(s) & M64
        out[k] = (min(i), max(i), sum(u) & M32, min(u), max(u), _fold_f32(w["f"], min), _fold_f32(w["f"], max), 0, sum(q) & M64, min(q),
                  ssum - (1 << 64) if ssum >> 63 else ssum, 0)
    return out


def same_floats(got, want):
    """equal by value: +0 and -0 equal (the sign of a zero extreme is fminf's / fmaxf's own business), NaN only where NaN is wanted"""
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]))


# ---------------------------------------------------------------------------------------------------------------- 1: the key walk
def _keys(has, key):
    w = np.zeros(WAVE, KEY_IN)
    w["has"], w["key"] = has, key
    return w


@functools.lru_cache(None)
def key_cases():
    """-> (names, (waves, 64) KEY_IN): every named wave in each of the four wave positions of a block"""
    r = _rng(2)
    lanes = np.arange(WAVE)
    cases = {
        "none": _keys(0, 5),
        "one key": _keys(1, 12345),
        "64 distinct": _keys(1, 1000 + r.permutation(WAVE)),
        "two alternating": _keys(1, np.where(lanes % 2 == 0, 77, 3)),
        "only lane 63": _keys(lanes == 63, 9),
        "lanes 0 and 63": _keys((lanes == 0) | (lanes == 63), 4),
        "twenty random": _keys(r.random(WAVE) < 0.8, r.integers(0, M32, 20, endpoint=True)[r.integers(0, 20, WAVE)]),
        # the lanes without a key carry a live one: every odd lane key 7 like the even ones, and lane 0 - the would-be lead - without
        "dead carriers": _keys((lanes % 2 == 0) & (lanes > 0), np.where(lanes % 4 < 2, 7, 8)),
        "dead lane holds the only copy": _keys(lanes != 20, np.where(lanes == 20, 99, lanes // 16)),
        "0 and ffffffff": _keys(lanes % 5 != 0, np.where(lanes % 2 == 0, 0, M32)),
        "negative": _keys(lanes % 7 != 3, np.array([M32, M32 - 1, 0x80000000, 0x7fffffff], np.uint64)[r.integers(0, 4, WAVE)]),
        "low 16 bits equal": _keys(1, (r.integers(0, 6, WAVE) << 16) | 0xbeef),
        "high 16 bits equal": _keys(lanes % 9 != 0, 0xbeef0000 | r.integers(0, 6, WAVE)),
        "runs": _keys(1, lanes // 5),
        "random has, few keys": _keys(r.random(WAVE) < 0.5, r.integers(0, 3, WAVE)),
        "sparse": _keys(r.random(WAVE) < 0.1, r.integers(0, 1 << 31, WAVE) * 2),
    }
    names = list(cases)
    assert len(names) % WAVES == 0
    rolled = []
    for shift in range(WAVES):                                                   # block b of pass `shift` holds names[4 b + shift ..]: every case in every wave position
        rolled += names[shift:] + names[:shift]
    return rolled, np.stack([cases[k] for k in rolled])


def key_reference(waves):
    """(W, 64) KEY_IN -> ((W, 64) KEY_OUT, (W,) trips): a trip per distinct key among the lanes with has, in ascending order of first lane"""
    out = np.zeros(waves.shape, KEY_OUT)
    out["trip"] = NONE; out["lead"] = NONE
    trips = np.zeros(len(waves), np.uint32)
    for w, wave in enumerate(waves):
        first = {}
        for lane in range(WAVE):
            if wave["has"][lane]:
                first.setdefault(int(wave["key"][lane]), []).append(lane)
        for trip, (key, members) in enumerate(sorted(first.items(), key=lambda kv: kv[1][0])):
            same = sum(1 << lane for lane in members)
            for lane in members:
                out[w, lane] = (trip, members[0], key, 1, same)
        trips[w] = len(first)
    return out, trips


# ---------------------------------------------------------------------------------------------------------------- 2: the block folds
def _block(pred=0, a=(0, 0, 0), b=(0, 0, 0)):
    blk = np.zeros(BLOCK, BLOCK_IN)
    blk["pred"] = pred
    for j in range(3):
        blk["a"][:, j] = a[j]
        blk["b"][:, j] = b[j]
    return blk


@functools.lru_cache(None)
def block_cases():
    """-> (names, (blocks, 256) BLOCK_IN)"""
    r = _rng(3)
    t = np.arange(BLOCK)
    cases = {}
    for wave in range(WAVES):                                                    # a value in one lane of one wave only
        for lane in (0, 31, 32, 63):
            one = t == 64 * wave + lane
            cases["one lane %d.%d" % (wave, lane)] = _block(np.where(one, 31, 0), [np.where(one, v, 0) for v in (0x80000001, 5, M32)],
                                                            [np.where(one, np.uint64(v), np.uint64(0)) for v in ((1 << 63) + 9, (1 << 40) + 3, 1)])
    cases["all equal"] = _block(0b10101, (0x90000000, 1, 0x01000000), ((5 << 32) | 1, 1 << 56, 3))
    cases["all set"] = _block(31, (M32, 0, 1), (M64, 1 << 63, 0))
    cases["none"] = _block()
    # per wave another pattern: the extreme of wave w in lane (0, 31, 32, 63)[w], top-bit values beside small ones, u64 that differ in one word only
    lane_of = np.array([0, 31, 32, 63])[t // 64]
    edge = (t % 64) == lane_of
    perm = r.permutation(BLOCK).astype("u8")
    cases["per wave extremes"] = _block(np.where(edge, 0b01010, 0b00101), (np.where(edge, 0x80000000 + t // 64, t), np.where(edge, 0, 0xfffffff0), r.integers(0, 100, BLOCK)),
                                        (np.where(edge, np.uint64(1 << 63) + (t // 64).astype("u8"), t.astype("u8")), ((perm + np.uint64(1)) << np.uint64(32)) | np.uint64(0x55aa55aa),
                                         (np.uint64(9) << np.uint64(32)) | (perm + np.uint64(0x80000000))))
    cases["top bit beside small"] = _block(r.integers(0, 32, BLOCK), [np.where(r.random(BLOCK) < 0.3, 0x80000000 + r.integers(0, 1 << 31, BLOCK), r.integers(0, 100, BLOCK)) for _ in range(3)],
                                           [r.integers(0, 1 << 63, BLOCK, dtype=np.uint64) | (np.uint64(1 << 63) * (r.random(BLOCK) < 0.3).astype("u8")) for _ in range(3)])
    cases["sums wrap"] = _block(np.where(t % 3 == 0, 0b11011, 0b00100), (0xff000000 + t, 0x01000001, (1 << 31) + (t % 2)), ((1 << 60) + t.astype("u8"), 1 << 56, M64))
    cases["u64 sums above 2^40"] = _block(1, (1 << 24, (1 << 24) - 1, t), ((1 << 40) + t.astype("u8"), (1 << 41), (t.astype("u8") << np.uint64(33))))
    for k, dens in enumerate((0.02, 0.5, 0.98)):
        rr = _rng(4, k)
        pred = sum(((rr.random(BLOCK) < d).astype("u4") << j) for j, d in enumerate((dens, 0.5, 1 - dens, 0.1, 0.9)))
        cases["random %d" % k] = _block(pred, [rr.integers(0, M32, BLOCK, endpoint=True, dtype=np.uint64) for _ in range(3)],
                                        [rr.integers(0, M64, BLOCK, endpoint=True, dtype=np.uint64) for _ in range(3)])
    names = list(cases)
    return names, np.stack([cases[k] for k in names])


def block_reference(blocks):
    """(B, 256) BLOCK_IN -> (B,) BLOCK_OUT by serial sums over Python ints"""
    out = np.zeros(len(blocks), BLOCK_OUT)
    for k, blk in enumerate(blocks):
        pred = [int(p) for p in blk["pred"]]
        cnt = [sum((p >> j) & 1 for p in pred) for j in range(5)]
        a = [[int(v) for v in blk["a"][:, j]] for j in range(3)]
        b = [[int(v) for v in blk["b"][:, j]] for j in range(3)]
        first = lambda v, top: [v[j] for K in range(1, top + 1) for j in range(K)]         # the results of K = 1, 2, .. one after the other
        out[k]["count"] = first(cnt, 5)
        out[k]["sum32"] = first([sum(v) & M32 for v in a], 3); out[k]["max32"] = first([max(v) for v in a], 3); out[k]["again32"] = sum(a[1]) & M32
        out[k]["sum64"] = first([sum(v) & M64 for v in b], 3); out[k]["max64"] = first([max(v) for v in b], 3); out[k]["again64"] = sum(b[1]) & M64
        out[k]["wide"] = [sum(a[0]), sum(a[1])]
    return out


# ---------------------------------------------------------------------------------------------------------------- 3, 4: the slot folds and the scan
SLOT_PATTERNS = ("last slot only", "second trip only", "zeros", "large, the total wraps", "small counts")


def slots(pattern, nb, k, wide=False):
    """-> (nb, k) u32 (u64 with wide) slot words, a pattern of SLOT_PATTERNS.  `second trip only`: values in the slots 1024 .. 2047 alone, what a thread of
    the 1024 reads in its second trip of the stride loop (all zeros for nb <= 1024); `large`: values up to 2^31 (2^63) whose column totals wrap"""
    r = _rng(5, SLOT_PATTERNS.index(pattern), nb, k, wide)
    top = (1 << 63) if wide else (1 << 31)
    full = r.integers(0, top, (nb, k), endpoint=True, dtype=np.uint64)
    a = np.zeros((nb, k), np.uint64)
    if pattern == "last slot only":
        a[-1] = full[-1] | np.uint64(top)
    elif pattern == "second trip only":
        a[SCAN_BLOCK:2 * SCAN_BLOCK] = full[SCAN_BLOCK:2 * SCAN_BLOCK]
    elif pattern == "large, the total wraps":
        a = full
    elif pattern == "small counts":
        a = r.integers(0, BLOCK, (nb, k), endpoint=True, dtype=np.uint64)
    return a if wide else a.astype(np.uint32)


def fold_reference(a):
    """(nb, k) -> (k,) column sums over Python ints, modular in the words' width"""
    mask = M64 if a.dtype == np.uint64 else M32
    return np.array([sum(int(v) for v in a[:, j]) & mask for j in range(a.shape[1])], a.dtype)


def scan_reference(cnt):
    """(rows, nb) u32 -> ((rows, nb) exclusive offsets, (rows,) totals), modular: numpy sums in int64 (nb 2^31 < 2^63)"""
    c = np.cumsum(cnt.astype(np.int64), axis=1)
    return ((c - cnt) & M32).astype(np.uint32), (c[:, -1] & M32).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 5: the block rank
SEAM_SIZES = (63, 64, 65, 255, 256, 257)                                         # the record counts and kept patterns of tests/test_gpu_compact_seams.py
SEAM_PATTERNS = ("none", "all", "alternating", "lane63", "lane0_later_waves")


def seam_pattern(name, n):
    i = np.arange(n)
    return {"none": i < 0, "all": i >= 0, "alternating": i % 2 == 0, "lane63": i % 64 == 63, "lane0_later_waves": (i % 64 == 0) & (i >= 64)}[name]


@functools.lru_cache(None)
def rank_cases():
    """-> (keep (256 B,) u8, bases (B,) u32): the seams' patterns over n records (the lanes past n keep nothing), then seeded random densities; the bases
    non-zero, some within a block of 2^32 so that base + rank wraps"""
    keep = []
    for n in SEAM_SIZES:
        for name in SEAM_PATTERNS:
            k = np.zeros(-(-n // BLOCK) * BLOCK, bool)
            k[:n] = seam_pattern(name, n)
            keep.append(k)
    r = _rng(6)
    for dens in (0.01, 0.1, 0.5, 0.9, 0.99):
        keep.append(r.random(4 * BLOCK) < dens)
    keep = np.concatenate(keep).astype(np.uint8)
    nb = len(keep) // BLOCK
    bases = r.integers(1, 1 << 31, nb, dtype=np.uint64)
    bases[::3] = M32 - r.integers(0, BLOCK, len(bases[::3]), dtype=np.uint64)
    bases[1] = M32; bases[2] = 1 << 31
    return keep, bases.astype(np.uint32)


def rank_reference(keep, bases):
    """base + the kept lanes of the block before the lane, modulo 2^32, for every lane"""
    k = keep.reshape(-1, BLOCK).astype(np.int64)
    return ((bases.astype(np.int64)[:, None] + np.cumsum(k, axis=1) - k) & M32).astype(np.uint32).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- 6, 7: the union-find
N = 1 << 16
UF_FAMILIES = ("path ascending", "path descending", "path bit-reversed", "star high", "star low", "comb", "bipartite", "same edge", "random sparse", "random dense",
               "cliques", "tiny 1", "tiny 2", "tiny 257", "forest of runs", "forest of scattered groups", "deep forest")


def _hang_on_minimum(group):
    """group[x] = a group number per node -> parent0 with every node on the smallest node of its group"""
    order = np.argsort(group, kind="stable")
    g = group[order]
    start = np.r_[True, g[1:] != g[:-1]]
    parent = np.empty(len(group), np.uint32)
    parent[order] = order[np.flatnonzero(start)][np.cumsum(start) - 1]
    return parent


@functools.lru_cache(None)
def uf_family(name):
    """-> (n, edges (m, 2) u32, forest (n,) u32 or None); n = 65 536 and m <= 2^18 unless the family says otherwise"""
    r = _rng(8, UF_FAMILIES.index(name))
    n, forest = N, None
    i = np.arange(N - 1)
    if name.startswith("path"):
        order = {"ascending": i, "descending": i[::-1]}.get(name.split()[1])
        if order is None:                                                        # bit-reversed: neighbouring lanes unite far ends of the path
            rev = np.zeros(N, np.int64)
            for bit in range(16):
                rev |= ((np.arange(N) >> bit) & 1) << (15 - bit)
            order = rev[rev < N - 1]
        e = np.stack([order, order + 1], axis=1)
    elif name == "star high":                                                    # every union has the same high end: the most contended root word
        e = np.stack([i, np.full(N - 1, N - 1)], axis=1)
    elif name == "star low":
        e = np.stack([np.zeros(N - 1, np.int64), i + 1], axis=1)
    elif name == "comb":                                                         # 256 teeth of 255 nodes, tooth j hung on spine node n - 256 + j; the spine a path
        tooth = np.arange(256 * 255).reshape(256, 255)
        spine = N - 256 + np.arange(256)
        e = np.concatenate([np.stack([tooth[:, :-1].ravel(), tooth[:, 1:].ravel()], axis=1), np.stack([tooth[:, -1], spine], axis=1),
                            np.stack([spine[:-1], spine[1:]], axis=1)])
        e = e[r.permutation(len(e))]
    elif name == "bipartite":                                                    # complete K(64, 64) on 128 nodes
        n = 128
        a, b = np.meshgrid(np.arange(64), 64 + np.arange(64), indexing="ij")
        e = np.stack([a.ravel(), b.ravel()], axis=1)
    elif name == "same edge":                                                    # 2^16 lanes on one pair, every eighth a self-loop
        e = np.tile(np.array([[54321, 12345]]), (N, 1))
        e[::8] = 54321; e[4::16] = 12345; e[1::2] = e[1::2, ::-1]
    elif name == "random sparse":
        e = r.integers(0, N, (N // 2, 2))
    elif name == "random dense":
        e = r.integers(0, N, (4 * N, 2))
    elif name == "cliques":                                                      # 1024 disjoint groups of 64 scattered nodes: a spanning path and 193 random pairs each
        member = r.permutation(N).reshape(1024, 64)
        pairs = r.integers(0, 64, (1024, 193, 2))
        e = np.concatenate([np.stack([member[:, :-1].ravel(), member[:, 1:].ravel()], axis=1),
                            np.stack([np.take_along_axis(member, pairs[:, :, 0], 1).ravel(), np.take_along_axis(member, pairs[:, :, 1], 1).ravel()], axis=1)])
        e = e[r.permutation(len(e))]
    elif name == "tiny 1":
        n, e = 1, np.zeros((3, 2), np.int64)
    elif name == "tiny 2":
        n, e = 2, np.array([[0, 1], [1, 0], [1, 1], [0, 0]])
    elif name == "tiny 257":
        n = 257
        e = np.concatenate([np.stack([np.arange(0, 256, 2), np.arange(1, 257, 2)], axis=1), r.integers(0, 257, (40, 2)), [[256, 0]]])
    elif name == "forest of runs":                                               # contiguous runs of 1 .. 512 nodes hung on their first, as k_mf_tile leaves a tile
        ends = np.cumsum(r.integers(1, 512, N, endpoint=True))
        ends = ends[ends < N]
        group = np.searchsorted(ends, np.arange(N), side="right")
        forest = _hang_on_minimum(group)
        e = r.integers(0, N, (2048, 2))
    elif name == "forest of scattered groups":
        forest = _hang_on_minimum(r.integers(0, 2048, N))
        e = r.integers(0, N, (1024, 2))
    else:                                                                        # trees of depth > 1 inside every 64 nodes: parent0[x] anywhere in [64 (x / 64), x]
        x = np.arange(N)
        lo = x & ~63
        forest = (lo + (r.random(N) * (x - lo + 1)).astype(np.int64)).astype(np.uint32)
        e = r.integers(0, N, (N // 128, 2))
    e = np.ascontiguousarray(e, dtype=np.uint32)
    assert len(e) <= 1 << 18 and int(e.max()) < n and (forest is None or (forest <= np.arange(n)).all())
    return n, e, forest


@functools.lru_cache(None)
def uf_reference(name):
    """-> (n,) u32: the smallest node of every node's component in the family's edges plus its starting forest, by a plain serial union-find"""
    n, edges, forest = uf_family(name)
    return components(n, edges, forest)


def components(n, edges, forest=None):
    parent = list(range(n))
    pairs = edges.tolist() + ([] if forest is None else [[x, p] for x, p in enumerate(forest.tolist()) if p != x])
    for a, b in pairs:
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]; b = parent[b]
        if a != b:
            parent[max(a, b)] = min(a, b)
    for x in range(n):                                                           # ascending: parent[x] < x is final already
        parent[x] = parent[parent[x]]
    return np.array(parent, np.uint32)


def check_forest(parent, want, what):
    """the raw parent array after the unite launch against the reference roots: parent[x] <= x, parent[x] in x's component, every walk ends within n steps
    (pointer doubling: after ceil(log2 n) + 1 rounds a chain of up to n links has reached its end) at the component's smallest node, and the roots are
    exactly the component minima"""
    n = len(parent)
    x = np.arange(n)
    p = parent.astype(np.int64)
    assert (p <= x).all(), "%s: parent[x] > x at %s" % (what, np.flatnonzero(p > x)[:8])
    assert np.array_equal(want[p], want), "%s: parent[x] outside x's component at %s" % (what, np.flatnonzero(want[p] != want)[:8])
    for _ in range(max(n - 1, 1).bit_length() + 1):
        p = p[p]
    assert np.array_equal(p[p], p), "%s: a walk does not end within n steps" % what
    assert np.array_equal(p, want), "%s: a walk ends elsewhere than at the smallest node of the component, at %s" % (what, np.flatnonzero(p != want)[:8])
    assert np.array_equal(np.flatnonzero(parent == x), np.unique(want)), "%s: the roots are not the component minima" % what


# ---------------------------------------------------------------------------------------------------------------- 8: the grid geometry
def grid_reference(W, H, D):
    """-> ((W H D,) VOXEL, (tiles, 4) i32 tile origins, (26, 3) i32 walk offsets) by numpy's own index arithmetic: x fastest, tiles numbered like voxels"""
    tiles = tuple(-(-s // TILE) for s in (D, H, W))
    z, y, x = np.unravel_index(np.arange(W * H * D), (D, H, W))
    out = np.zeros(W * H * D, VOXEL)
    out["x"], out["y"], out["z"] = x, y, z
    out["index"] = np.ravel_multi_index((z, y, x), (D, H, W))
    out["tile"] = np.ravel_multi_index((z // TILE, y // TILE, x // TILE), tiles)
    out["place"] = np.ravel_multi_index((z % TILE, y % TILE, x % TILE), (TILE,) * 3)
    out["pos"] = np.ravel_multi_index((z % TILE + 1, y % TILE + 1, x % TILE + 1), (RIM,) * 3)
    bz, by, bx = np.unravel_index(np.arange(int(np.prod(tiles))), tiles)
    origin = np.stack([bx * TILE, by * TILE, bz * TILE, 0 * bx], axis=1).astype(np.int32)
    walk = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)], np.int32)
    return out, origin, walk


def grid_reference_divmod(W, H, D):
    """the same by a serial loop of divmod over Python ints, the way the device splits an index"""
    tx, ty = -(-W // TILE), -(-H // TILE)
    out = np.zeros(W * H * D, VOXEL)
    for i in range(W * H * D):
        row, x = divmod(i, W)
        z, y = divmod(row, H)
        (bx, lx), (by, ly), (bz, lz) = divmod(x, TILE), divmod(y, TILE), divmod(z, TILE)
        out[i] = (x, y, z, (z * H + y) * W + x, (bz * ty + by) * tx + bx, (lz * TILE + ly) * TILE + lx, ((lz + 1) * RIM + ly + 1) * RIM + lx + 1, 0)
    origin = np.array([(TILE * (t % tx), TILE * (t // tx % ty), TILE * (t // (tx * ty)), 0) for t in range(tx * ty * -(-D // TILE))], np.int32)
    walk = np.array([(k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1) for k in range(27) if k != 13], np.int32)
    return out, origin, walk
