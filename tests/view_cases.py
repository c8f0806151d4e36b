"""The case table of the occupancy map's view gain (csrc/qn_mapview.inc: k_mv_origin, k_mv_cast<PEEK>, k_mv_stats, with block_count, block_sum, k_slot_fold and
k_slot_max of csrc/qn_map_compact.cuh and dg_block_stats / dg_fold_stats of csrc/qn_dense_grid.cuh): deterministic three-class layouts, viewpoints and ray tables,
with what the construction itself determines stated in `expect` - never taken from the twin and never from engine output.
tests/test_map_view_twin.py holds the twin (qn_amd/mapview.py) to the definition (its brute()) and to these expectations; tests/test_gpu_map_view.py holds the
engine to the twin and to them.  Pure numpy, no GPU.

Classes on chosen voxels, by the construction of tests/frontier_cases.py (TWO_HITS, POSE, voxel 1): a voxel given one record is FREE, a voxel given two records
is OCCUPIED, every other voxel is UNKNOWN; the grid is the bounding box of voxel (0, 0, 0) and the records, so the far corner of a layout is never UNKNOWN and
world coordinates are grid coordinates.  Where a row must end in an UNKNOWN voxel (the column) it is row y = 0 of a layout two rows high whose far corner
(W - 1, 1, 0) is OCCUPIED; no ray of the case leaves row 0.

A Case: name, layout (D, H, W) uint8, viewpoints (Q, 3) f64, offsets (R, 3) int32, params (an mv.ViewParams) and `expect` (every key optional): rows, one
dict {field: value} per viewpoint (fields of mv.VIEW_DTYPE); cover {voxel (ix, iy, iz): count}, every other voxel 0; stats {field: value}.

Seams and the constant each belongs to (restated from the source; whoever changes one there changes it here):
  WAVE 64                   the rays of a wave start in one voxel: R = 63, 64, 65
  MO_BLOCK 256              rays per block of k_mv_cast, viewpoints per block of k_mv_origin, voxels per block of k_mv_stats: R = 255, 256, 257
  32                        bits of a word of a viewpoint's bitset: gain voxels at bit positions 31, 32 and 33
  QN_VIEW_PASS              viewpoints per pass: the five viewpoints of seam/passes under 1, 2 and unset (tests/test_gpu_map_view.py)"""
import functools
import numpy as np
import frontier_cases as fc
from qn_amd import mapoccupancy as mo, mapview as mv

UNK, FREE, OCC = mo.UNKNOWN, mo.FREE, mo.OCCUPIED
POSE, TWO_HITS = fc.POSE, fc.TWO_HITS
ONE = 1024
RAY_SEAMS = (63, 64, 65, 255, 256, 257)
LINE_LENGTHS = (8, 9, 65)
ENDS = ("blocked", "escaped", "spent", "reached")


def centre(x, y, z):
    return [x + 0.5, y + 0.5, z + 0.5]


class Case:
    def __init__(self, name, layout, viewpoints, offsets, params=(), expect=None):
        layout = np.asarray(layout, np.uint8)
        D, H, W = layout.shape
        self.name, self.layout, self.sides = name, layout, (W, H, D)
        free = np.argwhere(layout == FREE)[:, ::-1]; occ = np.argwhere(layout == OCC)[:, ::-1]      # (x, y, z)
        rec = np.concatenate([free, occ, occ])
        assert len(rec) and tuple(rec.max(axis=0) + 1) == (W, H, D), name      # the records span the grid
        self.records = np.ascontiguousarray(rec, np.float32).reshape(-1, 3)
        self.occ = TWO_HITS
        self.viewpoints = np.ascontiguousarray(viewpoints, np.float64).reshape(-1, 3)
        self.offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1, 3)
        self.params = mv.ViewParams(**dict(params))
        self.expect = {} if expect is None else expect


def row(gain=0, blocked=0, escaped=0, spent=0, reached=0, steps=0, status=mv.OK, **kw):
    return dict(status=status, gain=gain, blocked=blocked, escaped=escaped, spent=spent, reached=reached, steps=steps, **kw)


OUT = dict(status=mv.OUTSIDE, gain=0, blocked=0, escaped=0, spent=0, reached=0, steps=0, ijk=(0, 0, 0))


# ---- the column: the row [FREE, UNK, UNK, OCC, UNK] along x (row 0 of a 5 x 2 x 1 layout), viewpoint at the centre of voxel 0 unless said otherwise
def column_layout():
    lay = np.full((1, 2, 5), UNK, np.uint8)
    lay[0, 0] = [FREE, UNK, UNK, OCC, UNK]; lay[0, 1, 4] = OCC
    return lay


def column():
    lay = column_layout()
    v0 = [centre(0, 0, 0)]
    x = lambda k: [[k, 0, 0]]
    both = {(1, 0, 0): 1, (2, 0, 0): 1}
    return [
        Case("column/blocked", lay, v0, x(6 * ONE), (), dict(rows=[row(gain=2, blocked=1, steps=4, ijk=(0, 0, 0))], cover=both, stats=dict(covered=2, max_cover=1, total_gain=2, steps=4))),
        Case("column/spent", lay, v0, x(6 * ONE), dict(max_through=1), dict(rows=[row(gain=1, spent=1, steps=2)], cover={(1, 0, 0): 1})),
        Case("column/reached", lay, v0, x(2 * ONE), (), dict(rows=[row(gain=2, reached=1, steps=3)], cover=both)),
        Case("column/escaped", lay, v0, x(-ONE), (), dict(rows=[row(escaped=1, steps=1)], cover={})),
        Case("column/zero-offset", lay, v0, x(0), (), dict(rows=[row(reached=1, steps=1)], cover={})),
        # the viewpoint inside an UNKNOWN voxel: v_0 is marked
        Case("column/zero-offset-in-unknown", lay, [centre(1, 0, 0)], x(0), (), dict(rows=[row(gain=1, reached=1, steps=1, ijk=(1, 0, 0))], cover={(1, 0, 0): 1})),
        # the ray ends exactly in the stop voxel: blocked, not reached
        Case("column/ends-in-stop", lay, v0, x(3 * ONE), (), dict(rows=[row(gain=2, blocked=1, steps=4)], cover=both)),
        # through reaches max_through exactly at v_n: spent, not reached
        Case("column/spent-at-the-end", lay, v0, x(2 * ONE), dict(max_through=2), dict(rows=[row(gain=2, spent=1, steps=3)], cover=both)),
        # the viewpoint inside an OCCUPIED voxel: every ray blocked at v_0
        Case("column/inside-occupied", lay, [centre(3, 0, 0)], [[6 * ONE, 0, 0], [-6 * ONE, 0, 0], [0, 0, 0], [ONE, 0, 0], [-ONE, 3, 0]], (),
             dict(rows=[row(blocked=5, steps=5, ijk=(3, 0, 0))], cover={}, stats=dict(covered=0, max_cover=0, total_gain=0, steps=5, rays=5))),
        # nothing stops: voxels 0 .. 4 are examined, then the ray leaves through the +x face
        Case("column/stop-mask-0", lay, v0, x(6 * ONE), dict(stop_mask=0), dict(rows=[row(gain=3, escaped=1, steps=5)], cover={(1, 0, 0): 1, (2, 0, 0): 1, (4, 0, 0): 1})),
        Case("column/gain-free", lay, v0, x(6 * ONE), dict(gain_mask=1 << FREE), dict(rows=[row(gain=1, blocked=1, steps=4)], cover={(0, 0, 0): 1})),
    ]


# ---- the tie: viewpoint at a voxel centre, offset (1024, 1024, 0): the tie goes to the lowest axis, the ray visits (0, 0), (1, 0), (1, 1)
def tie():
    out = []
    for name, wall, want in (("x-first-blocks", (1, 0), row(blocked=1, steps=2)), ("y-first-does-not", (0, 1), row(gain=2, reached=1, steps=3))):
        lay = np.full((1, 3, 3), UNK, np.uint8); lay[0, 0, 0] = FREE; lay[0, 2, 2] = FREE; lay[0, wall[1], wall[0]] = OCC
        cover = {} if want["blocked"] else {(1, 0, 0): 1, (1, 1, 0): 1}
        out.append(Case("tie/" + name, lay, [centre(0, 0, 0)], [[ONE, ONE, 0]], (), dict(rows=[want], cover=cover)))
    return out


# ---- the face: A_x = 1024 exactly, the row [UNK, FREE, UNK, OCC]: heading down the ray is in voxel 1 and steps to voxel 0 at once, heading up it goes to voxel 2
def face():
    lay = np.array([[[UNK, FREE, UNK, OCC]]], np.uint8)
    v = [[1.0, 0.5, 0.5]]
    return [Case("face/down", lay, v, [[-512, 0, 0]], (), dict(rows=[row(gain=1, reached=1, steps=2, ijk=(1, 0, 0))], cover={(0, 0, 0): 1})),
            Case("face/up", lay, v, [[ONE, 0, 0]], (), dict(rows=[row(gain=1, reached=1, steps=2, ijk=(1, 0, 0))], cover={(2, 0, 0): 1}))]


# ---- the six faces: a 3 x 3 x 3 block of FREE voxels, viewpoint in the middle, a ray of two voxels along each axis both ways: the middle, a neighbour, then out
SIX = [[2 * ONE, 0, 0], [-2 * ONE, 0, 0], [0, 2 * ONE, 0], [0, -2 * ONE, 0], [0, 0, 2 * ONE], [0, 0, -2 * ONE]]


def faces():
    lay = np.full((3, 3, 3), FREE, np.uint8)
    mid = [centre(1, 1, 1)]
    seven = {(1, 1, 1): 1, (0, 1, 1): 1, (2, 1, 1): 1, (1, 0, 1): 1, (1, 2, 1): 1, (1, 1, 0): 1, (1, 1, 2): 1}
    out = [Case("faces/six-escapes", lay, mid, SIX, (), dict(rows=[row(escaped=6, steps=12, ijk=(1, 1, 1))], cover={})),
           # the middle voxel is crossed by all six rays and counted once
           Case("faces/six-escapes-gain-free", lay, mid, SIX, dict(gain_mask=1 << FREE, stop_mask=0), dict(rows=[row(gain=7, escaped=6, steps=12)], cover=seven))]
    for k, o in enumerate(SIX):
        out.append(Case("faces/escape-%d" % k, lay, mid, [o], (), dict(rows=[row(escaped=1, steps=2)], cover={})))
    # viewpoints that are OUTSIDE: not finite, 2^20 voxels from the origin, one voxel outside each face; the one in the middle is not
    bad = [[np.nan, 1.5, 1.5], [1.5, np.inf, 1.5], [1.5, 1.5, -np.inf], [1048576.0, 1.5, 1.5], [1.5, -1048576.0, 1.5], [-0.5, 1.5, 1.5], [3.5, 1.5, 1.5], [1.5, -0.5, 1.5],
           [1.5, 3.5, 1.5], [1.5, 1.5, -0.5], [1.5, 1.5, 3.5]]
    out.append(Case("faces/outside", lay, bad + mid, SIX, dict(gain_mask=1 << FREE, stop_mask=0),
                    dict(rows=[OUT] * len(bad) + [row(gain=7, escaped=6, steps=12, ijk=(1, 1, 1))], cover=seven,
                         stats=dict(viewpoints=12, outside=11, rays=6, covered=7, max_cover=1, total_gain=7, steps=12))))
    out.append(Case("faces/all-outside", lay, bad, SIX, (), dict(rows=[OUT] * len(bad), cover={}, stats=dict(viewpoints=11, outside=11, covered=0, total_gain=0, steps=0))))
    return out


# ---- the band: the column [FREE, UNK, UNK, UNK, OCC] along z, a ray up from layer 0: blocked at layer 4 after five voxels, through = 3
def band():
    lay = np.array([FREE, UNK, UNK, UNK, OCC], np.uint8).reshape(5, 1, 1)
    out = []
    for name, lo, hi, layers in (("above", 2, 9, (2, 3)), ("below", 0, 1, (1,)), ("clipped", -7, 1, (1,)), ("missing-the-grid", 5, 9, ()), ("all", 0, mv.INT32_MAX, (1, 2, 3))):
        out.append(Case("band/" + name, lay, [centre(0, 0, 0)], [[0, 0, 4 * ONE]], dict(iz_lo=lo, iz_hi=hi),
                        dict(rows=[row(gain=len(layers), blocked=1, steps=5)], cover={(0, 0, z): 1 for z in layers})))
    # the gain voxels of layers 1 and 2 lie outside the band and still count towards max_through: spent at layer 2, nothing marked
    out.append(Case("band/outside-counts-through", lay, [centre(0, 0, 0)], [[0, 0, 4 * ONE]], dict(iz_lo=3, iz_hi=3, max_through=2), dict(rows=[row(spent=1, steps=3)], cover={})))
    return out


# ---- distinctness: R rays that all cross voxel 0 (FREE) and end in voxel 1 (UNKNOWN) of [FREE, UNK, OCC]: reached R, the voxel counted once
def fan(R):
    return [[512 + (j * 7) % 1000, 0, 0] for j in range(R)]          # c(512 + offset) = 1 for an offset of 512 .. 1535


def distinct():
    lay = np.array([[[FREE, UNK, OCC]]], np.uint8)
    out = [Case("distinct/rays-%d" % R, lay, [centre(0, 0, 0)], fan(R), (), dict(rows=[row(gain=1, reached=R, steps=2 * R)], cover={(1, 0, 0): 1},
                                                                          stats=dict(rays=R, covered=1, max_cover=1, total_gain=1, steps=2 * R)))
           for R in RAY_SEAMS + (300,)]
    # two viewpoints that see the same voxel from both sides: the ray away from it leaves the grid at once
    lay = np.array([[[FREE, UNK, FREE]]], np.uint8)
    out.append(Case("distinct/two-viewpoints", lay, [centre(0, 0, 0), centre(2, 0, 0)], [[ONE, 0, 0], [-ONE, 0, 0]], (),
                    dict(rows=[row(gain=1, reached=1, escaped=1, steps=3, ijk=(0, 0, 0)), row(gain=1, reached=1, escaped=1, steps=3, ijk=(2, 0, 0))], cover={(1, 0, 0): 2},
                         stats=dict(viewpoints=2, outside=0, rays=2, covered=1, max_cover=2, total_gain=2, steps=6))))
    return out


# ---- seams
def seams():
    out = []
    # a viewpoint's bitset starts at its reach box's corner, here voxel 0: the gain voxels 31, 32, 33 are the last bit of a word and the first two of the next
    lay = np.full((1, 1, 40), FREE, np.uint8); lay[0, 0, 31:34] = UNK
    out.append(Case("seam/bits-31-32-33", lay, [centre(0, 0, 0)], [[39 * ONE, 0, 0]] * 3, (), dict(rows=[row(gain=3, reached=3, steps=120)], cover={(x, 0, 0): 1 for x in (31, 32, 33)})))
    # five viewpoints on [FREE, UNK, FREE, UNK, FREE, UNK, FREE, UNK, FREE], each looking two voxels both ways: a pass seam can fall between any two
    lay = np.array([FREE, UNK] * 4 + [FREE], np.uint8).reshape(1, 1, 9)
    rows = [row(gain=1 if x in (0, 8) else 2, reached=1 if x in (0, 8) else 2, escaped=1 if x in (0, 8) else 0, steps=4 if x in (0, 8) else 6, ijk=(x, 0, 0)) for x in (0, 2, 4, 6, 8)]
    out.append(Case("seam/passes", lay, [centre(x, 0, 0) for x in (0, 2, 4, 6, 8)], [[2 * ONE, 0, 0], [-2 * ONE, 0, 0]], (),
                    dict(rows=rows, cover={(x, 0, 0): 2 for x in (1, 3, 5, 7)}, stats=dict(viewpoints=5, outside=0, rays=2, covered=4, max_cover=2, total_gain=8, steps=26))))
    # lines of n voxels along each axis, UNKNOWN but for the FREE far end, walked from end to end
    for axis in range(3):
        for n in LINE_LENGTHS:
            sides = [1, 1, 1]; sides[axis] = n
            lay = np.full(sides[::-1], UNK, np.uint8); lay[-1, -1, -1] = FREE
            o = [0, 0, 0]; o[axis] = (n - 1) * ONE
            cover = {}
            for k in range(n - 1):
                v = [0, 0, 0]; v[axis] = k
                cover[tuple(v)] = 1
            out.append(Case("seam/line-%s-%d" % ("xyz"[axis], n), lay, [centre(0, 0, 0)], [o], (), dict(rows=[row(gain=n - 1, reached=1, steps=n)], cover=cover)))
    # an offset of exactly the limit on a line of 65 FREE voxels: the ray walks the line and leaves it
    lay = np.full((1, 1, 65), FREE, np.uint8)
    out.append(Case("seam/offset-limit", lay, [centre(0, 0, 0)], [[mv.MAX_OFFSET, 0, 0]], (), dict(rows=[row(escaped=1, steps=65)], cover={})))
    out.append(Case("seam/offset-limit-gain-free", lay, [centre(0, 0, 0)], [[mv.MAX_OFFSET, 0, 0], [-mv.MAX_OFFSET, 0, 0]], dict(gain_mask=1 << FREE, stop_mask=0),
                    dict(rows=[row(gain=65, escaped=2, steps=66)], cover={(x, 0, 0): 1 for x in range(65)})))
    return out


# ---- a seeded random three-class volume, no expect: held to the twin, and in the twin test to brute()
def random_volume():
    rng = np.random.default_rng(43)
    lay = rng.choice(np.array([UNK, FREE, OCC], np.uint8), size=(6, 12, 14), p=(0.5, 0.42, 0.08))
    lay[-1, -1, -1] = OCC
    off = rng.integers(-9 * ONE, 9 * ONE, size=(300, 3)).astype(np.int32)
    off[:8] = [[0, 0, 0], [ONE, ONE, ONE], [-ONE, -ONE, -ONE], [512, 512, 0], [3 * ONE, 0, -3 * ONE], [0, 2 * ONE, 2 * ONE], [-512, 1536, 0], [5 * ONE, 5 * ONE, 5 * ONE]]
    vps = np.concatenate([rng.uniform([0, 0, 0], [14, 12, 6], size=(3, 3)), [[7.0, 6.0, 3.0]]])      # the last one on three faces at once
    return [Case("random/14x12x6", lay, vps, off), Case("random/14x12x6-band-through", lay, vps, off, dict(iz_lo=1, iz_hi=3, max_through=4)),
            Case("random/14x12x6-free", lay, vps, off, dict(gain_mask=(1 << FREE) | (1 << UNK), stop_mask=0))]


GROUPS = {"column": column, "tie": tie, "face": face, "faces": faces, "band": band, "distinct": distinct, "seam": seams, "random": random_volume}
NAMES = list(GROUPS)


@functools.lru_cache(maxsize=None)
def group(name):
    return GROUPS[name]()


def all_cases():
    return [c for g in NAMES for c in group(g)]


def case(name):
    return next(c for c in group(name.split("/")[0]) if c.name == name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the occupancy twin's result of a case -> (classes, grid), computed once and shared (treat them as read-only)"""
    c = case(name)
    occ = mo.classify([c.records], [POSE], c.occ)
    assert occ["classes"].shape == c.layout.shape and np.array_equal(occ["classes"], c.layout), name
    return occ["classes"], occ["grid"]


@functools.lru_cache(maxsize=None)
def twin(name):
    """the twin's view gain of a case, computed once and shared (treat it as read-only)"""
    c = case(name)
    return mv.gain(*inputs(name), c.viewpoints, c.offsets, c.params)


def holds(c, info, cover, stats):
    """`expect` and what holds of every result against one (the twin's or the engine's): info of mv.VIEW_DTYPE, cover (D, H, W) uint32, stats a dict"""
    e = c.expect
    Q, R = len(c.viewpoints), len(c.offsets)
    assert info.dtype == mv.VIEW_DTYPE and info.shape == (Q,) and cover.dtype == np.uint32 and cover.shape == c.layout.shape, c.name
    ok = info["status"] == mv.OK
    assert ((info["status"] == mv.OUTSIDE) | ok).all() and not info["reserved"].any(), c.name
    ends = sum(info[f].astype(np.int64) for f in ENDS)
    assert np.array_equal(ends, np.where(ok, R, 0)), (c.name, ends)  # every ray of an OK viewpoint ends in exactly one way
    for f in ("gain", "steps", "ijk"):
        assert not info[f][~ok].any(), (c.name, f)
    assert int(cover.sum(dtype=np.uint64)) == int(info["gain"].sum(dtype=np.uint64)) == stats["total_gain"], c.name
    assert stats["viewpoints"] == Q and stats["rays"] == R and stats["outside"] == int((~ok).sum()) and stats["steps"] == int(info["steps"].sum(dtype=np.uint64)), (c.name, stats)
    assert stats["covered"] == int((cover > 0).sum()) and stats["max_cover"] == int(cover.max(initial=0)) <= int(ok.sum()), (c.name, stats)
    gainful = ((c.params.gain_mask >> c.layout.astype(np.int64)) & 1) == 1
    assert gainful[cover > 0].all(), c.name                          # a covered voxel is a gain voxel
    for f, v in e.get("stats", {}).items():
        assert stats[f] == v, (c.name, f, stats[f], v)
    if "rows" in e:
        assert len(e["rows"]) == Q, c.name
        for k, want in enumerate(e["rows"]):
            for f, v in want.items():
                assert np.array_equal(info[k][f], np.asarray(v, info.dtype[f].base)), (c.name, k, f, info[k][f], v)
    if "cover" in e:
        want = np.zeros(c.layout.shape, np.uint32)
        for (x, y, z), v in e["cover"].items():
            want[z, y, x] = v
        assert np.array_equal(cover, want), (c.name, np.argwhere(cover != want).tolist())
