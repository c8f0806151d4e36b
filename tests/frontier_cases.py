"""The case table of the occupancy map's frontier regions (csrc/qn_mapfrontier.inc: k_mf_mark, k_mf_tile, k_mf_merge, k_mf_flatten, k_mf_roots, k_mf_pick,
k_mf_rows_init, k_mf_relabel, k_mf_rows, k_mf_costs, with k_dg_list_flag / _pick and the tile of csrc/qn_dense_grid.cuh and block_count, block_sum, block_max, wave_each_key, k_slot_fold, k_slot_max, block_rank and k_scan_rows of
csrc/qn_map_compact.cuh and uf_unite_min of csrc/qn_union_find.cuh): deterministic three-class layouts, with what the construction itself determines
stated in `expect` - never taken from the twin and never from engine output.
tests/test_map_frontier_twin.py holds the twin (qn_amd/mapfrontier.py) to the definition (its brute()) and to these expectations;
tests/test_gpu_map_frontier.py holds the engine to the twin and to them.  Pure numpy, no GPU.

Classes on chosen voxels, by the construction of tests/route_cases.py (TWO_HITS, POSE, voxel 1, shell 0xffffffff): a voxel given one record is FREE, a voxel
given two records is OCCUPIED, every other voxel is UNKNOWN; the grid is the bounding box of voxel (0, 0, 0) and the records.  Both runners take the classes
the occupancy call itself produced; inputs() checks that they are the layout.

A Case: name, layout (D, H, W) uint8 of classes, records, occ, params (an mf.FrontierParams), sides (W, H, D), route (an mr.RouteParams), dist (an
md.DistanceParams), goal (1, 3) f64 - for the cost call - and `expect` (every key optional): stats {field: value}; regions [{field: value}], one dict per
region in region order (fields of mf.INFO_DTYPE, some or all); labels {voxel (ix, iy, iz): value}; frontier: the (D, H, W) bool mask of the frontier voxels;
costs [(cost, (ix, iy, iz))] per region.

Seams and the constant each belongs to (restated from the source; whoever changes one there changes it here):
  DG_T 8                    the side of a tile of k_mf_tile and of the rims k_mf_merge joins: lines of 8, 9, 10, 17 and 65 voxels end on, one past and two past a seam
  MF_BLOCK = MO_BLOCK 256   voxels per block of the flat kernels (mark, merge, flatten, roots, pick, relabel, list, costs)
  MO_SCAN_BLOCK 1024        threads of k_scan_rows over the blocks' kept roots; the numbering case has 1728 regions in 134 blocks
  WAVE 64                   k_mf_flatten, k_mf_relabel and k_mf_costs fold the voxels of a wave that share a root or region (wave_each_key), one trip per region: the numbering case
                            has some twenty regions in a wave, the lines one
  MF_COPIES 32              copies of the regions' partial rows, a block adding into copy block % copies: the numbering case has 134 blocks, the lines one"""
import functools
import numpy as np
import route_cases as rc
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, maproute as mr

T, BLOCK, SCAN_BLOCK, WAVE = 8, 256, 1024, 64
UNK, FREE, OCC = mo.UNKNOWN, mo.FREE, mo.OCCUPIED
POSE, TWO_HITS = rc.POSE, rc.TWO_HITS
LINE_LENGTHS = (2, 8, 9, 10, 17, 65)
U, B = mr.UNREACHED, mr.BLOCKED


class Case:
    def __init__(self, name, layout, params=(), expect=None, route=(), goal=(0, 0, 0)):
        layout = np.asarray(layout, np.uint8)
        D, H, W = layout.shape
        self.name, self.layout, self.sides = name, layout, (W, H, D)
        free = np.argwhere(layout == FREE)[:, ::-1]; occ = np.argwhere(layout == OCC)[:, ::-1]      # (x, y, z)
        rec = np.concatenate([free, occ, occ])
        assert len(rec) and tuple(rec.max(axis=0) + 1) == (W, H, D), name      # the records span the grid
        self.records = np.ascontiguousarray(rec, np.float32).reshape(-1, 3)
        self.occ = TWO_HITS
        self.params = mf.FrontierParams(**dict(params))
        r = dict(pass_mask=1 << FREE, min_d2=0); r.update(route)
        self.route = mr.RouteParams(**r)
        self.dist = md.DistanceParams(1 << OCC, 2)
        self.goal = np.array([rc.centre(*goal)], np.float64)
        self.expect = {} if expect is None else expect

    @property
    def cells(self):
        return self.layout.size


def lin(sides, x, y, z):
    return (z * sides[1] + y) * sides[0] + x


# ---- lines: all FREE, n x 1 x 1 along each axis: with edge_unknown 1 one component of n voxels, root 0, every voxel with its 4 side faces and the ends one more
def lines(axis):
    out = []
    for n in LINE_LENGTHS:
        sides = [1, 1, 1]; sides[axis] = n
        lay = np.full(sides[::-1], FREE, np.uint8)
        hi = [0, 0, 0]; hi[axis] = n - 1
        region = dict(root=0, size=n, faces=4 * n + 2, lo=(0, 0, 0), hi=tuple(hi), sum=tuple(n * (n - 1) // 2 if k == axis else 0 for k in range(3)))
        stats = dict(candidates=n, frontier=n, components=1, regions=1, too_small=0, region_voxels=n, rejected_voxels=0, largest=n, unknown_faces=4 * n + 2)
        out.append(Case("lines-%s/%d" % ("xyz"[axis], n), lay, dict(min_size=1), dict(stats=stats, regions=[region], frontier=np.ones(lay.shape, bool))))
        none = dict(candidates=n, frontier=0, components=0, regions=0, too_small=0, region_voxels=0, rejected_voxels=0, largest=0, unknown_faces=0)
        out.append(Case("lines-%s/%d-closed" % ("xyz"[axis], n), lay, dict(min_size=1, edge_unknown=0), dict(stats=none, regions=[], frontier=np.zeros(lay.shape, bool))))
    return out


# ---- slab: a FREE layer under an UNKNOWN one, an OCCUPIED far corner on layer 1 for the extent, edge_unknown 0: the voxel under the corner has no unknown neighbour
def slab():
    out = []
    for W, H in ((9, 9), (17, 9), (10, 10)):
        lay = np.full((2, H, W), UNK, np.uint8); lay[0] = FREE; lay[1, -1, -1] = OCC
        n = W * H - 1
        front = np.zeros(lay.shape, bool); front[0] = True; front[0, -1, -1] = False
        sx = H * (W * (W - 1) // 2) - (W - 1); sy = W * (H * (H - 1) // 2) - (H - 1)
        region = dict(root=0, size=n, faces=n, lo=(0, 0, 0), hi=(W - 1, H - 1, 0), sum=(sx, sy, 0))
        stats = dict(candidates=W * H, frontier=n, components=1, regions=1, too_small=0, region_voxels=n, rejected_voxels=0, largest=n, unknown_faces=n)
        out.append(Case("slab/%dx%d" % (W, H), lay, dict(edge_unknown=0), dict(stats=stats, regions=[region], frontier=front, labels={(W - 1, H - 1, 0): mf.NONE, (0, 0, 0): 0})))
    return out


# ---- adjacency knife edges (edge_unknown 0, min_size 1: only the UNKNOWN voxels of the layout open a face)
def knife_edges():
    out = []
    lay = np.full((4, 4, 4), UNK, np.uint8); lay[1, 1, 1] = lay[2, 2, 2] = FREE; lay[3, 3, 3] = OCC
    s = (4, 4, 4)
    out.append(Case("knife/corner-touch", lay, dict(edge_unknown=0, min_size=1),
                    dict(stats=dict(candidates=2, frontier=2, components=1, regions=1, largest=2, unknown_faces=12),
                         regions=[dict(root=lin(s, 1, 1, 1), size=2, faces=12, lo=(1, 1, 1), hi=(2, 2, 2), sum=(3, 3, 3))], labels={(1, 1, 1): 0, (2, 2, 2): 0, (0, 0, 0): mf.NONE})))
    lay = np.full((4, 4, 5), UNK, np.uint8); lay[1, 1, 1] = lay[1, 1, 3] = FREE; lay[3, 3, 4] = OCC
    s = (5, 4, 4)
    out.append(Case("knife/two-apart", lay, dict(edge_unknown=0, min_size=1),
                    dict(stats=dict(candidates=2, frontier=2, components=2, regions=2, largest=1, unknown_faces=12),
                         regions=[dict(root=lin(s, 1, 1, 1), size=1, faces=6), dict(root=lin(s, 3, 1, 1), size=1, faces=6)], labels={(1, 1, 1): 0, (3, 1, 1): 1, (2, 1, 1): mf.NONE})))
    lay = np.array([[[OCC, FREE, OCC]]], np.uint8)
    out.append(Case("knife/walled-in", lay, dict(edge_unknown=0, min_size=1),
                    dict(stats=dict(candidates=1, frontier=0, components=0, regions=0, unknown_faces=0), regions=[], frontier=np.zeros(lay.shape, bool))))
    # a column in z: FREE, UNKNOWN, FREE, OCCUPIED.  Band 2 .. 3: the candidate z = 0 lies outside it and is no frontier voxel, though the unknown voxel z = 1 -
    # itself outside the band - still counts for z = 2.  Band 0 .. 0: the other way round.
    col = np.array([FREE, UNK, FREE, OCC], np.uint8).reshape(4, 1, 1)
    for name, lo, hi, at, other in (("band-above", 2, 3, 2, 0), ("band-below", 0, 0, 0, 2), ("band-clipped", -7, 0, 0, 2)):
        out.append(Case("knife/" + name, col, dict(edge_unknown=0, min_size=1, iz_lo=lo, iz_hi=hi),
                        dict(stats=dict(candidates=1, frontier=1, components=1, regions=1, unknown_faces=1),
                             regions=[dict(root=at, size=1, faces=1, lo=(0, 0, at), hi=(0, 0, at), sum=(0, 0, at))], labels={(0, 0, at): 0, (0, 0, other): mf.NONE})))
    out.append(Case("knife/band-both", col, dict(edge_unknown=0, min_size=1), dict(stats=dict(candidates=2, frontier=2, components=2, regions=2, unknown_faces=2))))
    out.append(Case("knife/band-miss", col, dict(edge_unknown=0, min_size=1, iz_lo=4, iz_hi=9), dict(stats=dict(candidates=0, frontier=0, components=0, regions=0), regions=[])))
    return out


# ---- min_size: a row of exactly min_size voxels and one of min_size - 1, two rows apart, side by side: one kept, one rejected
def min_size():
    out = []
    for k in (5, 8):
        W = k + 2
        lay = np.full((1, 3, W), UNK, np.uint8); lay[0, 0, :k] = FREE; lay[0, 2, :k - 1] = FREE; lay[0, 2, W - 1] = OCC
        s = (W, 3, 1)
        out.append(Case("min-size/%d" % k, lay, dict(edge_unknown=0, min_size=k),
                        dict(stats=dict(candidates=2 * k - 1, frontier=2 * k - 1, components=2, regions=1, too_small=1, region_voxels=k, rejected_voxels=k - 1, largest=k),
                             regions=[dict(root=0, size=k, lo=(0, 0, 0), hi=(k - 1, 0, 0), sum=(k * (k - 1) // 2, 0, 0))],
                             labels={(0, 0, 0): 0, (k - 1, 0, 0): 0, (0, 2, 0): mf.REJECTED, (k - 2, 2, 0): mf.REJECTED, (k - 1, 2, 0): mf.NONE})))
        out.append(Case("min-size/%d-kept-both" % k, lay, dict(edge_unknown=0, min_size=k - 1),
                        dict(stats=dict(components=2, regions=2, too_small=0, region_voxels=2 * k - 1, rejected_voxels=0, largest=k),
                             regions=[dict(root=0, size=k), dict(root=lin(s, 0, 2, 0), size=k - 1)])))
    return out


# ---- late joins: one voxel thick, the smallest index far from where the parts meet
def loop_path():
    """along the edges of a 25^3 cube: +x, +y, +z, -x, -y, -z down to z = 2 - every axis' three tile seams (7|8, 15|16, 23|24) crossed twice, six crossings an
    axis; the ends (0, 0, 0) and (0, 0, 2) do not touch"""
    n = 24
    p = [(x, 0, 0) for x in range(n + 1)] + [(n, y, 0) for y in range(1, n + 1)] + [(n, n, z) for z in range(1, n + 1)]
    p += [(x, n, n) for x in range(n - 1, -1, -1)] + [(0, y, n) for y in range(n - 1, -1, -1)] + [(0, 0, z) for z in range(n - 1, 1, -1)]
    return p


def late_joins():
    out = []
    p = loop_path()
    assert len(set(p)) == len(p) == 6 * 24 - 1
    lay = np.full((25, 25, 25), UNK, np.uint8)
    for x, y, z in p:
        lay[z, y, x] = FREE
    front = lay == FREE
    one = lambda n: dict(candidates=n, frontier=n, components=1, regions=1, too_small=0, region_voxels=n, rejected_voxels=0, largest=n)
    out.append(Case("late/serpentine", lay, (), dict(stats=one(len(p)), regions=[dict(root=0, size=len(p), lo=(0, 0, 0), hi=(24, 24, 24))], frontier=front,
                                                     labels={(0, 0, 2): 0, (0, 0, 0): 0, (0, 0, 1): mf.NONE})))
    # a U: arms along x at y = 0 and y = 3 that join only at x = 20
    L = 20
    lay = np.full((1, 4, L + 1), UNK, np.uint8); lay[0, 0, :] = FREE; lay[0, 3, :] = FREE; lay[0, :, L] = FREE
    n = 2 * (L + 1) + 2
    out.append(Case("late/u", lay, (), dict(stats=one(n), regions=[dict(root=0, size=n, lo=(0, 0, 0), hi=(L, 3, 0))], frontier=lay == FREE, labels={(0, 3, 0): 0})))
    # a comb: 9 teeth along y at x = 0, 2, .. 16, joined by a spine at y = 17, the highest indices
    lay = np.full((1, 18, 17), UNK, np.uint8); lay[0, :, ::2] = FREE; lay[0, 17, :] = FREE
    n = 9 * 17 + 17
    out.append(Case("late/comb", lay, (), dict(stats=one(n), regions=[dict(root=0, size=n, lo=(0, 0, 0), hi=(16, 17, 0))], frontier=lay == FREE,
                                               labels={(16, 0, 0): 0, (1, 0, 0): mf.NONE})))
    return out


# ---- numbering: isolated FREE voxels on a stride-3 lattice in 70 x 70 x 7, min_size 1, edge_unknown 0: 24 x 24 x 3 = 1728 regions of one voxel each, region k
#      the k-th lattice voxel in linear order, its faces the neighbours its place in the grid leaves it
def numbering():
    W, H, D = 70, 70, 7
    lay = np.full((D, H, W), UNK, np.uint8); lay[::3, ::3, ::3] = FREE
    regions = []
    for z in range(0, D, 3):
        for y in range(0, H, 3):
            for x in range(0, W, 3):
                f = (x > 0) + (x < W - 1) + (y > 0) + (y < H - 1) + (z > 0) + (z < D - 1)
                regions.append(dict(root=lin((W, H, D), x, y, z), size=1, faces=f, lo=(x, y, z), hi=(x, y, z), sum=(x, y, z)))
    assert len(regions) == 1728 > SCAN_BLOCK
    stats = dict(candidates=1728, frontier=1728, components=1728, regions=1728, too_small=0, region_voxels=1728, rejected_voxels=0, largest=1,
                 unknown_faces=sum(r["faces"] for r in regions))
    return [Case("numbering", lay, dict(min_size=1, edge_unknown=0), dict(stats=stats, regions=regions, frontier=lay == FREE)),
            Case("numbering/all-rejected", lay, dict(min_size=2, edge_unknown=0), dict(stats=dict(components=1728, regions=0, too_small=1728, rejected_voxels=1728), regions=[]))]


# ---- costs: a FREE floor 20 x 5 with edge_unknown 0, so that only the UNKNOWN voxels of the layout open a face, route over FREE without a clearance, goal (0, 2):
#   U1 = (10, 0): the region {(9, 0), (11, 0), (10, 1)}, root (9, 0); (9, 0) is two corner moves and seven face moves from the goal, 29, the straight line's bound
#   U2 = (4, 2) behind the OCCUPIED (3, 2): the region {(4, 1), (5, 2), (4, 3)}, root (4, 1); (4, 1) and (4, 3) mirror each other about the goal's row, one
#        corner move and three face moves, 13 each (no diagonal may pass the wall's block): the smaller index (4, 1) wins
#   U3 = (18, 2) behind a wall of OCCUPIED voxels at x = 15: the region {(18, 1), (17, 2), (19, 2), (18, 3)}, root (18, 1), cut off: UNREACHED and (0, 0, 0)
# in ascending root the regions are those of U1, U2, U3.  With a second layer that repeats the first and a planar route over both, a column passes where the
# floor does: the same costs, attained on layer 0.
def cost_floor(layers):
    lay = np.full((layers, 5, 20), FREE, np.uint8)
    lay[:, 0, 10] = UNK; lay[:, 2, 4] = UNK; lay[:, 2, 3] = OCC; lay[:, :, 15] = OCC; lay[:, 2, 18] = UNK
    return lay


def costs():
    want = [(29, (9, 0, 0)), (13, (4, 1, 0)), (U, (0, 0, 0))]
    roots = [dict(root=9, size=3), dict(root=24, size=3), dict(root=38, size=4)]
    flat = Case("costs/3d", cost_floor(1), dict(edge_unknown=0, min_size=1), dict(stats=dict(components=3, regions=3, frontier=10), regions=roots, costs=want), goal=(0, 2, 0))
    two = [dict(root=r["root"], size=2 * r["size"]) for r in roots]
    planar = Case("costs/planar", cost_floor(2), dict(edge_unknown=0, min_size=1), dict(stats=dict(components=3, regions=3, frontier=20), regions=two, costs=want),
                  route=dict(planar=1, iz_lo=0, iz_hi=1), goal=(0, 2, 1))
    return [flat, planar]


# ---- a seeded random three-class volume, no expect: held to the twin, and in the twin test to brute()
def random_volume():
    rng = np.random.default_rng(41)
    lay = rng.choice(np.array([UNK, FREE, OCC], np.uint8), size=(19, 33, 40), p=(0.45, 0.45, 0.10))
    lay[-1, -1, -1] = OCC
    sparse = np.where(rng.random(lay.shape) < 0.75, UNK, lay).astype(np.uint8); sparse[-1, -1, -1] = OCC      # few FREE voxels: many small components
    half = np.where(rng.random(lay.shape) < 0.55, UNK, lay).astype(np.uint8); half[-1, -1, -1] = OCC
    return [Case("random/40x33x19", lay), Case("random/40x33x19-closed", half, dict(edge_unknown=0, min_size=1)),
            Case("random/40x33x19-band", half, dict(min_size=3, iz_lo=5, iz_hi=11)), Case("random/40x33x19-sparse", sparse, dict(min_size=4)),
            Case("random/40x33x19-occupied-unknown", lay, dict(unknown_mask=(1 << UNK) | (1 << OCC), min_size=2))]


GROUPS = {"lines-x": lambda: lines(0), "lines-y": lambda: lines(1), "lines-z": lambda: lines(2), "slab": slab, "knife": knife_edges, "min-size": min_size,
          "late": late_joins, "numbering": numbering, "costs": costs, "random": random_volume}
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
    """the twin's frontier regions of a case, computed once and shared (treat them as read-only)"""
    return mf.frontier(inputs(name)[0], case(name).params)


def holds(c, labels, info, stats):
    """`expect` and what holds of every result against one (the twin's or the engine's): labels (D, H, W) int32, info of mf.INFO_DTYPE, stats a dict"""
    e = c.expect
    assert labels.dtype == np.int32 and labels.shape == c.layout.shape and info.dtype == mf.INFO_DTYPE, (c.name, labels.shape)
    R = len(info)
    assert stats["regions"] == R and stats["components"] == R + stats["too_small"] and stats["frontier"] == stats["region_voxels"] + stats["rejected_voxels"], (c.name, stats)
    assert stats["frontier"] == int((labels != mf.NONE).sum()) and stats["rejected_voxels"] == int((labels == mf.REJECTED).sum()), (c.name, stats)
    assert stats["candidates"] >= stats["frontier"] and stats["unknown_faces"] >= stats["frontier"] and labels.min(initial=mf.NONE) >= mf.NONE and labels.max(initial=-1) == R - 1, c.name
    free = ((c.params.free_mask >> c.layout.astype(np.int64)) & 1) == 1
    assert free[labels != mf.NONE].all(), c.name                     # a frontier voxel is a candidate
    assert (np.diff(info["root"].astype(np.int64)) > 0).all() and (info["size"] >= c.params.min_size).all() and not info["reserved"].any(), c.name
    assert np.array_equal(np.bincount(labels[labels >= 0], minlength=R), info["size"]), c.name
    if R:
        assert np.array_equal(labels.ravel()[info["root"]], np.arange(R)) and stats["largest"] >= int(info["size"].max()), c.name
    for f, v in e.get("stats", {}).items():
        assert stats[f] == v, (c.name, f, stats[f], v)
    if "regions" in e:
        assert R == len(e["regions"]), (c.name, R, len(e["regions"]))
        for k, want in enumerate(e["regions"]):
            for f, v in want.items():
                assert np.array_equal(info[k][f], np.asarray(v, info.dtype[f].base)), (c.name, k, f, info[k][f], v)
    if "frontier" in e:
        assert np.array_equal(labels != mf.NONE, e["frontier"]), c.name
    for (x, y, z), v in e.get("labels", {}).items():
        assert int(labels[z, y, x]) == v, (c.name, (x, y, z), int(labels[z, y, x]), v)


def costs_hold(c, cost, ijk):
    """the `costs` of expect against one result of the cost call under c.route and c.goal"""
    if "costs" in c.expect:
        got = [(int(a), tuple(int(v) for v in b)) for a, b in zip(cost, ijk)]
        assert got == c.expect["costs"], (c.name, got)
