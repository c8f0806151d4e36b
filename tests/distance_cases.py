"""The case table of the occupancy map's distance field (csrc/qn_mapdistance.inc: k_md_x, k_md_axis<false / true>, k_md_query, with k_dg_slice and dg_block_stats of csrc/qn_dense_grid.cuh,
block_count, block_max, block_sum, k_slot_fold and k_slot_max of csrc/qn_map_compact.cuh and oc_voxel of csrc/qn_dense_grid.cuh): deterministic inputs that
put sites on chosen voxels, with what the construction itself determines stated in `expect` - never taken from the twin and never from engine output.  tests/test_map_distance_twin.py holds the twin (qn_amd/mapdistance.py) to the definition (its
brute()) and to these expectations; tests/test_gpu_map_distance.py holds the engine to the twin and to them.  Pure numpy, no GPU.

Sites on chosen voxels: voxel 1.0, min_range 0, max_range 1e4 and shell 0xffffffff (no ray leaves a miss, so a voxel is OCCUPIED where a ray ends and UNKNOWN
elsewhere), one keyframe under the pose with translation (0.5, 0.5, 0.5) and no rotation: record (i, j, k) ends in voxel (i, j, k).  The grid is the bounding
box of the origin voxel (0, 0, 0) and the ends.  Both runners take the classes the occupancy call itself produced, so nothing depends on guessing them.

A Case: name, records (n, 3) f32, occ (an mo.OccupancyParams), params (an md.DistanceParams), sides (W, H, D) as the construction gives them, and `expect`
(every key optional): d2 {voxel (ix, iy, iz): value}, some voxels; full: the whole (D, H, W) field; stats {field: value}.

Seams and the constant each belongs to (restated from the source; whoever changes one there changes it here):
  MD_BLOCK = MO_BLOCK 256   voxels per block of k_md_x and k_md_axis, columns of k_dg_slice, points of k_md_query; the halo of k_md_x is one block either side
  WAVE 64                   one ballot word of k_md_x: the line lengths 63 .. 65, 127 .. 129, 255 .. 257 are its word and block seams, 1025 is four blocks
  MAX_RADIUS 255            the largest max_dist: 255^2 = 65025 is the largest d2, one below FAR's neighbourhood
  MO_WAVES 4, MO_SCAN_BLOCK 1024   the words of block_max and block_sum, the stride of k_slot_fold and k_slot_max: fold_seams() below"""
import functools
import numpy as np
from qn_amd import mapdistance as md, mapoccupancy as mo

F = np.float32
FAR = md.FAR
MD_BLOCK, WAVE = 256, 64
SITES = mo.OccupancyParams(1.0, 0.0, 1.0e4, 0xffffffff, 1, 2)        # a voxel is OCCUPIED where a ray ends, UNKNOWN elsewhere
POSE = np.eye(4); POSE[:3, 3] = 0.5
OCC, FREE, UNK = 1 << mo.OCCUPIED, 1 << mo.FREE, 1 << mo.UNKNOWN
LINE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
LINE_RADII = (1, 16, 255)
SLICE_CAP = 200000                                                   # voxels up to which the twin test runs brute(); a larger case states its whole field


class Case:
    def __init__(self, name, records, params, sides, expect=None, occ=SITES):
        self.name = name
        self.records = np.ascontiguousarray(records, F).reshape(-1, 3)
        self.params = md.DistanceParams(*params)
        self.sides = tuple(int(v) for v in sides)
        self.expect = {} if expect is None else expect
        self.occ = mo.OccupancyParams(*occ)

    @property
    def voxels(self):
        return self.sides[0] * self.sides[1] * self.sides[2]


def wi(i, m, salt=0):
    """the i-th value of the Weyl sequence of 1/golden ratio, as an integer in [0, m)"""
    return int((((i + 1 + 7919 * salt) * 0.6180339887498949) % 1.0) * m)


def box_of(records):
    """(W, H, D) of the bounding box of voxel (0, 0, 0) and the (non-negative integer) records"""
    r = np.asarray(records, np.int64).reshape(-1, 3)
    return tuple(int(v) + 1 for v in r.max(axis=0))


# ---- lines: a site at the far end only, along each axis
def lines(axis):
    out = []
    for n in LINE_LENGTHS:
        rec = [0, 0, 0]; rec[axis] = n - 1
        sides = [1, 1, 1]; sides[axis] = n
        for r in LINE_RADII:
            d = (n - 1 - np.arange(n)).astype(np.int64)
            full = np.where(d <= r, d * d, FAR).astype(np.uint16).reshape(sides[::-1])
            reached = (d >= 1) & (d <= r)
            expect = dict(full=full, stats=dict(sites=1, reached=int(reached.sum()), far=int((d > r).sum()), max_d2=int((d[reached] ** 2).max()) if reached.any() else 0,
                                                sum_d2=int((d[reached] ** 2).sum())))
            if n == 1025 and r == 255:                               # the voxel 255 away reads 65025 and the one 256 away reads FAR
                at = lambda p: tuple(p if k == axis else 0 for k in range(3))
                expect["d2"] = {at(n - 1 - 255): 65025, at(n - 1 - 256): FAR, at(n - 1): 0, at(0): FAR}
            out.append(Case("lines-%s/%d-r%d" % ("xyz"[axis], n, r), [rec], (OCC, r), sides, expect))
    return out


# ---- the 3-D knife edge: max_dist 5, a site at the origin and one at (7, 7, 2) for the extent
def knife_edge():
    # from the origin: (3, 4, 0) and (5, 0, 0) are at 25 = max_dist^2, still reached; (3, 4, 1) is at 26 from the origin and 16 + 9 + 1 = 26 from the far site:
    # FAR; (0, 5, 1) is at 26 and 49 + 4 + 1: FAR; (4, 4, 0) is at 32 from the origin, beyond its reach, and 9 + 9 + 4 = 22 from the far site
    expect = dict(d2={(0, 0, 0): 0, (7, 7, 2): 0, (3, 4, 0): 25, (5, 0, 0): 25, (0, 5, 0): 25, (0, 0, 2): 4, (3, 4, 1): FAR, (0, 5, 1): FAR, (4, 4, 0): 22, (4, 3, 0): 25,
                      (5, 1, 0): FAR, (7, 2, 2): 25, (7, 1, 2): FAR, (2, 7, 2): 25, (4, 3, 2): 25},
                  stats=dict(sites=2))
    return [Case("knife-edge", [[0, 0, 0], [7, 7, 2]], (OCC, 5), (8, 8, 3), expect)]


# ---- a window wider than every axis, and rows much shorter than the window beside rows wider than a block
def wide_window():
    small = Case("wide-window/5x4x3-r255", [[0, 0, 0], [4, 3, 2]], (OCC, 255), (5, 4, 3),
                 dict(d2={(4, 3, 0): 4, (0, 0, 2): 4, (2, 1, 1): 6, (2, 2, 1): 6, (4, 0, 0): 13, (0, 3, 2): 13}, stats=dict(sites=2, reached=58, far=0)))
    rec = [[(37 * i) % 300, wi(i, 3, 1), wi(i, 2, 2)] for i in range(9)] + [[299, 2, 1]]
    rows = Case("wide-window/300x3x2-r255", rec, (OCC, 255), (300, 3, 2), dict(stats=dict(far=0)))
    return [small, rows]


# ---- no site and all sites
FEW = [[0, 0, 0], [5, 2, 1], [3, 6, 2], [9, 0, 0]]


def no_site():
    return [Case("no-site", FEW, (FREE, 16), (10, 7, 3), dict(full=np.full((3, 7, 10), FAR, np.uint16), stats=dict(sites=0, reached=0, far=210, max_d2=0, sum_d2=0)))]


def all_sites():
    return [Case("all-sites", FEW, (7, 16), (10, 7, 3), dict(full=np.zeros((3, 7, 10), np.uint16), stats=dict(sites=210, reached=0, far=0, max_d2=0, sum_d2=0)))]


# ---- a fan of rays with shell 1: free, occupied and unknown voxels, every mask that means something
FAN_OCC = mo.OccupancyParams(1.0, 0.0, 1.0e4, 1, 1, 2)


def fan():
    rec = []
    for i in range(48):
        a = 0.5 * np.pi * (i + 0.5) / 48.0
        for k, rad in enumerate((14.0, 9.0)):
            rec.append([np.floor(rad * np.cos(a)), np.floor(rad * np.sin(a)), float((i + k) % 4)])
    sides = box_of(rec)
    return [Case("fan/%s" % name, rec, (mask, 4), sides, occ=FAN_OCC) for name, mask in (("occupied", OCC), ("occupied-unknown", OCC | UNK), ("free", FREE))]


# ---- random boxes
def random_boxes():
    out = []
    for name, n, sides, r, seed in (("70x40x9-r6", 200, (70, 40, 9), 6, 11), ("20x20x20-r3", 2000, (20, 20, 20), 3, 12)):
        rng = np.random.default_rng(seed)
        rec = np.stack([rng.integers(0, s, n) for s in sides], axis=1)
        rec[0] = [s - 1 for s in sides]                              # the box is the grid
        out.append(Case("random/" + name, rec, (OCC, r), sides))
    return out


# ---- the seams of block_max, block_sum and k_slot_max: the largest d2 in exactly one lane of one block
def fold_seams():
    """site_mask = UNKNOWN, D = 1: a 3 x 3 square of occupied voxels centred at p, one voxel or more inside the grid - the centre reads 4, its ring 1 - and the
    occupied far corner, which reads 1; every other voxel is a site.  p is lane 1 or 62 of the first or of the last wave of block 3, or lane 62 of block 1024
    of 1027 (262 905 voxels), the second trip of the stride loop of k_slot_fold and k_slot_max (MO_SCAN_BLOCK 1024).  W = 255, not 256: with block b = row b, lane 1 would put the
    square's side on the grid's edge, where nothing outside is a site and a second voxel reads 4; at 255 block b starts b voxels into row b.  Block 1026 of the
    large case is ragged but holds only sites and the corner, so the ragged last block that holds p is a case of its own, 20 x 30: block 2 has the last 88
    voxels, p = (10, 27) is its lane 38."""
    out = []
    for name, (W, H), lin in [("first-wave-lane-1", (255, 9), 3 * MD_BLOCK + 1), ("first-wave-lane-62", (255, 9), 3 * MD_BLOCK + 62),
                              ("last-wave-lane-1", (255, 9), 3 * MD_BLOCK + 193), ("last-wave-lane-62", (255, 9), 3 * MD_BLOCK + 254),
                              ("ragged-last-block", (20, 30), 2 * MD_BLOCK + 38), ("block-1024", (255, 1031), 1024 * MD_BLOCK + 62)]:
        px, py = lin % W, lin // W
        ring = [(px + dx, py + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
        assert all(1 <= x < W - 1 and 1 <= y < H - 1 for x, y in ring) and max(W - 1 - px, H - 1 - py) > 3      # unknown voxels all round the square, the corner apart
        rec = [[px, py, 0]] + [[x, y, 0] for x, y in ring] + [[W - 1, H - 1, 0]]
        full = np.zeros((1, H, W), np.uint16)
        for x, y in ring + [(W - 1, H - 1)]:
            full[0, y, x] = 1
        full[0, py, px] = 4
        out.append(Case("fold-seams/" + name, rec, (UNK, 4), (W, H, 1), dict(full=full, stats=dict(max_d2=4, sum_d2=13, reached=10, sites=W * H - 10, far=0))))
    return out


GROUPS = {"lines-x": lambda: lines(0), "lines-y": lambda: lines(1), "lines-z": lambda: lines(2), "knife-edge": knife_edge, "wide-window": wide_window,
          "no-site": no_site, "all-sites": all_sites, "fan": fan, "random": random_boxes, "fold-seams": fold_seams}
NAMES = list(GROUPS)


@functools.lru_cache(maxsize=None)
def group(name):
    return GROUPS[name]()


def all_cases():
    return [c for g in NAMES for c in group(g)]


@functools.lru_cache(maxsize=None)
def occupancy(name):
    """the occupancy twin's result of a case (classes, grid, stats), computed once and shared (treat it as read-only)"""
    c = next(c for c in group(name.split("/")[0]) if c.name == name)
    return mo.classify([c.records], [POSE], c.occ)


def holds(case, d2, stats):
    """`expect` and what holds of every field against one result (the twin's or the engine's): d2 (D, H, W) uint16, stats a dict"""
    e = case.expect
    assert d2.dtype == np.uint16 and d2.shape == case.sides[::-1], (case.name, d2.shape, case.sides)
    assert stats["sites"] + stats["reached"] + stats["far"] == case.voxels, (case.name, stats)
    r2 = case.params.max_dist ** 2
    reached = (d2 != 0) & (d2 != FAR)
    assert stats["sites"] == int((d2 == 0).sum()) and stats["reached"] == int(reached.sum()) and stats["far"] == int((d2 == FAR).sum()), (case.name, stats)
    assert stats["max_d2"] == (int(d2[reached].max()) if reached.any() else 0) <= r2 and stats["sum_d2"] == int(d2[reached].sum(dtype=np.uint64)), (case.name, stats)
    for f, v in e.get("stats", {}).items():
        assert stats[f] == v, (case.name, f, stats[f], v)
    if "full" in e:
        assert np.array_equal(d2, e["full"]), (case.name, "full", int((d2 != e["full"]).sum()))
    for (x, y, z), v in e.get("d2", {}).items():
        assert int(d2[z, y, x]) == v, (case.name, (x, y, z), int(d2[z, y, x]), v)


def slice_ranges(D):
    """the six (lo, hi) shapes the occupancy test uses: all layers, clipped below, one layer, clipped above, and the two bands that miss the grid"""
    return ((0, max(D - 1, 0)), (-5, 0), (D // 2, D // 2), (D - 1, D + 7), (D, D + 1), (-3, -1))


def query_points(grid, limit=400):
    """world points for a grid (an mo.OccupancyGrid): voxel centres (all, or `limit` of them spread over the grid), points on faces, edges and corners of voxels
    (the lower face belongs to the voxel), points just outside every side, and the points no grid holds: non-finite ones and one 2^20 voxels out
    -> (xyz (n, 3) f64, the index of the first point that must read OUTSIDE)"""
    g = mo.OccupancyGrid(*grid)
    n = g.width * g.height * g.depth
    k = np.arange(n, dtype=np.int64) if n <= limit else (np.arange(limit, dtype=np.int64) * (n - 1)) // (limit - 1)
    ijk = np.stack([k % g.width, (k // g.width) % g.height, k // (g.width * g.height)], axis=1).astype(np.float64)
    lo = np.asarray(g.minc, np.float64); v = float(g.voxel)
    side = np.array([g.width, g.height, g.depth], np.float64)
    centres = (lo + ijk + 0.5) * v
    faces = (lo + ijk[::3]) * v                                      # the lower corner of a voxel: still that voxel
    mixed = (lo + ijk[1::3] + np.array([0.0, 0.5, 0.999])) * v
    outside = []
    for a in range(3):
        for off in (-0.001, -1.5):
            p = lo + 0.5; p[a] = lo[a] + off; outside.append(p * v)
        for off in (0.0, 0.5, 300.0):
            p = lo + 0.5; p[a] = lo[a] + side[a] + off; outside.append(p * v)
    c = (lo + 0.5) * v
    never = [[np.nan, c[1], c[2]], [c[0], np.inf, c[2]], [c[0], c[1], -np.inf], [2.0 ** 20 * v, c[1], c[2]], [c[0], -(2.0 ** 20) * v, c[2]], [c[0], c[1], 1e300]]
    xyz = np.concatenate([centres, faces, mixed, np.array(outside), np.array(never)])
    return xyz, len(centres) + len(faces) + len(mixed)
