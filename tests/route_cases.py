"""The case table of the occupancy map's route field (csrc/qn_maproute.inc: k_mr_init, k_mr_goals, k_mr_relax, k_mr_stats, k_mr_path, k_mr_query, with k_slot_fold
and k_slot_max of csrc/qn_map_compact.cuh and the tile, dg_block_stats and oc_voxel of csrc/qn_dense_grid.cuh): deterministic wall layouts, with what the construction itself determines stated in
`expect` - never taken from the twin and never from engine output.  tests/test_map_route_twin.py holds the twin (qn_amd/maproute.py) to the definition (its
dijkstra()) and to these expectations; tests/test_gpu_map_route.py holds the engine to the twin and to them.  Pure numpy, no GPU.

Walls on chosen voxels, by the construction of tests/distance_cases.py (SITES, POSE, voxel 1, shell 0xffffffff: record (i, j, k) makes voxel (i, j, k) OCCUPIED
and everything else UNKNOWN; the grid is the bounding box of voxel (0, 0, 0) and the records): pass_mask = UNK gives arbitrary wall layouts whose far corner is
a wall.  Where a layout needs an open far corner (the 2 x 2 x 2 corner rule, the serpentine's end), min_hits is 2 instead: a wall is a record given twice, the far
corner a record given once - FREE - and pass_mask = UNK | FREE.  Both runners take the classes and the d2 of the calls themselves, (OCC, r) for the distance.

A Case: name, records, occ, dist (an md.DistanceParams), params (an mr.RouteParams), goals (n, 3) f64 world points, sides (W, H, D), walls (D, H, W) bool, and
`expect` (every key optional): cost {voxel (ix, iy, iz): value} (in planar mode iz = 0), full: the whole field, stats {field: value}, reached / unreached: bool
masks of cells that must be reached / must read UNREACHED, min_of: the names of two cases whose fields' minimum this field is, same_as: the name of a case
with the same field.

Seams and the constant each belongs to (restated from the source; whoever changes one there changes it here):
  DG_T 8                    the side of a tile of k_mr_relax: lines of 8, 9, 10, 17 and 65 voxels end on, one past and two past a tile seam
  MR_BLOCK = MO_BLOCK 256   cells per block of k_mr_init and k_mr_stats, points of k_mr_goals, k_mr_path and k_mr_query"""
import functools
import numpy as np
import distance_cases as dc
from qn_amd import mapdistance as md, mapoccupancy as mo, maproute as mr

T = 8
B, U = mr.BLOCKED, mr.UNREACHED
OCC, FREE, UNK = dc.OCC, dc.FREE, dc.UNK
POSE = dc.POSE
TWO_HITS = mo.OccupancyParams(1.0, 0.0, 1.0e4, 0xffffffff, 2, 2)     # a voxel is OCCUPIED where two rays end, FREE where one does, UNKNOWN elsewhere
LINE_LENGTHS = (2, 8, 9, 10, 17, 65)


class Case:
    def __init__(self, name, walls, goals, params=(), r=2, expect=None):
        walls = np.asarray(walls, bool)
        D, H, W = walls.shape
        self.name, self.walls, self.sides = name, walls, (W, H, D)
        rec = np.argwhere(walls)[:, ::-1]                            # (x, y, z)
        if walls[-1, -1, -1]:
            self.occ, mask = dc.SITES, UNK
        else:                                                        # an open far corner: walls twice, the corner once
            self.occ, mask = TWO_HITS, UNK | FREE
            rec = np.concatenate([rec, rec, [[W - 1, H - 1, D - 1]]])
        self.records = np.ascontiguousarray(rec, np.float32).reshape(-1, 3)
        self.dist = md.DistanceParams(OCC, r)
        p = dict(pass_mask=mask, min_d2=0); p.update(params)
        self.params = mr.RouteParams(**p)
        self.goals = np.asarray(goals, np.float64).reshape(-1, 3)
        self.expect = {} if expect is None else expect

    @property
    def field_sides(self):
        W, H, D = self.sides
        return (W, H, 1) if self.params.planar else (W, H, D)

    @property
    def cells(self):
        W, H, D = self.field_sides
        return W * H * D

    def starts(self):
        """8 to 16 world points for the path call: voxels spread over the field (reached, blocked or unreached as the layout has them), the first goal, a wall,
        a voxel the construction cuts off where there is one, and a point outside the grid"""
        W, H, D = self.sides
        pts = [centre(dc.wi(i, W, 1), dc.wi(i, H, 2), dc.wi(i, D, 3)) for i in range(12)]
        pts.append(self.goals[0])
        if self.walls.any():
            z, y, x = np.argwhere(self.walls)[0]
            pts.append(centre(x, y, z))
        cut_off = [v for v, c in self.expect.get("cost", {}).items() if c == U]
        if cut_off:
            pts.append(centre(*cut_off[0]))                          # a start that is passable but reaches no goal
        pts.append(centre(W, 0, 0))
        return np.array(pts, np.float64)


def centre(x, y, z):
    """the world centre of voxel (x, y, z): the grid starts at voxel (0, 0, 0) and the voxel is 1"""
    return [x + 0.5, y + 0.5, z + 0.5]


def open_with_corner(sides):
    W, H, D = sides
    w = np.zeros((D, H, W), bool); w[-1, -1, -1] = True
    return w


# ---- lines: the far-end record is a wall, so n - 1 voxels pass; goal at 0; cost = 3 index
def lines(axis):
    out = []
    for n in LINE_LENGTHS:
        sides = [1, 1, 1]; sides[axis] = n
        full = np.where(np.arange(n) == n - 1, B, 3 * np.arange(n)).astype(np.uint32).reshape(sides[::-1])
        k = np.arange(n - 1)
        expect = dict(full=full, stats=dict(passable=n - 1, blocked=1, reached=n - 1, unreached=0, goals_used=1, goals_blocked=0, max_cost=3 * (n - 2), sum_cost=int(3 * k.sum())))
        out.append(Case("lines-%s/%d" % ("xyz"[axis], n), open_with_corner(sides), [centre(0, 0, 0)], expect=expect))
    return out


# ---- open boxes: every passable voxel costs 3 a + b + c, a >= b >= c its sorted coordinates (a corner moves, then edge moves, then face moves)
def open_box():
    out = []
    for sides in ((9, 9, 9), (17, 9, 2), (10, 10, 10)):
        W, H, D = sides
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        s = np.sort(np.stack([x, y, z]), axis=0)                     # c <= b <= a
        full = (3 * s[2] + s[1] + s[0]).astype(np.uint32); full[-1, -1, -1] = B
        out.append(Case("open-box/%dx%dx%d" % sides, open_with_corner(sides), [centre(0, 0, 0)], expect=dict(full=full, stats=dict(blocked=1, unreached=0, goals_used=1))))
    return out


# ---- the corner rule
def staircase(door):
    """9 x 9 x 1: a wall at x = 4 for y < 4 and x = 5 for y >= 4, which leaves only a diagonal gap between (4, 4) and (5, 3) -> (walls, the mask right of it)"""
    w = np.zeros((1, 9, 9), bool)
    w[0, :4, 4] = True; w[0, 4:, 5] = True
    right = np.zeros((1, 9, 9), bool)
    right[0, :4, 5:] = True; right[0, 4:, 6:] = True
    if door:
        w[0, 7, 5] = False
    return w, right


def corner_rule():
    w = np.zeros((2, 2, 2), bool); w[0, 0, 1] = True
    # in z, y, x order; the edge move to (1, 1, 0) is forbidden - its block holds the wall - so it costs 6 over (0, 1, 0), not 4
    cube = Case("corner-rule/2x2x2", w, [centre(0, 0, 0)], expect=dict(full=np.array([0, B, 3, 6, 3, 6, 4, 7], np.uint32).reshape(2, 2, 2), cost={(1, 1, 0): 6}))
    w, right = staircase(False)
    closed = Case("corner-rule/staircase", w, [centre(0, 0, 0)], expect=dict(unreached=right, reached=~right & ~w, cost={(3, 3, 0): 12, (4, 4, 0): 18, (5, 3, 0): U}))
    w, right = staircase(True)
    # through the door at (5, 7): (0, 0) to (4, 7) is 4 corner and 3 face moves, then two face moves through the door, which no diagonal may enter
    door = Case("corner-rule/staircase-door", w, [centre(0, 0, 0)], expect=dict(reached=~w, cost={(4, 7, 0): 25, (5, 7, 0): 28, (6, 7, 0): 31, (6, 3, 0): 43, (5, 3, 0): 46}))
    return [cube, closed, door]


# ---- the min_d2 knife edge: max_dist 2, one wall at the far corner (7, 2, 2) of an 8 x 3 x 3 box, min_d2 4 = max_dist^2
def clearance():
    # (5, 2, 2) is at d2 4: passes.  (6, 1, 1) is at 3, (6, 2, 2) at 1, (6, 2, 1) at 2: blocked.  (5, 1, 1) is at 6 > max_dist^2 and (2, 2, 2) five voxels away:
    # both FAR, which passes any min_d2.  With min_d2 0 everything but the wall passes.
    w = open_with_corner((8, 3, 3))
    blocked = {(6, 1, 1): B, (6, 2, 2): B, (6, 2, 1): B, (6, 1, 2): B, (7, 1, 2): B, (7, 2, 2): B}
    knife = Case("clearance/min_d2-4", w, [centre(0, 0, 0)], dict(min_d2=4), 2,
                 dict(cost={**blocked, (5, 2, 2): 3 * 5 + 4, (5, 1, 1): 3 * 5 + 2, (2, 2, 2): 10, (0, 0, 0): 0, (7, 0, 0): 21, (6, 0, 0): 18},
                      stats=dict(blocked=8, unreached=0)))
    off = Case("clearance/min_d2-0", w, [centre(0, 0, 0)], dict(min_d2=0), 2, dict(cost={(6, 1, 1): 3 * 6 + 2, (6, 2, 2): 3 * 6 + 4}, stats=dict(blocked=1)))
    return [knife, off]


# ---- bands of layers, and the planar mode
def band_walls():
    rng = np.random.default_rng(21)
    w = rng.random((6, 5, 7)) < 0.2
    w[:, 0, 0] = False; w[-1, -1, -1] = True
    return w


def band():
    w = band_walls()
    g = [centre(0, 0, 2), centre(0, 0, 0), centre(0, 0, 5)]
    out = []
    for name, lo, hi, used in (("inside", 2, 3, 1), ("below", -5, 1, 1), ("above", 4, 100, 1), ("all", -(2 ** 31), 2 ** 31 - 1, 3)):
        out.append(Case("band/" + name, w, g, dict(iz_lo=lo, iz_hi=hi), expect=dict(stats=dict(goals_used=used, goals_blocked=3 - used))))
    for name, lo, hi in (("over", 6, 20), ("under", -9, -1)):        # a band that misses the grid: all BLOCKED, every goal ignored, status OK
        out.append(Case("band/" + name, w, g, dict(iz_lo=lo, iz_hi=hi),
                        expect=dict(full=np.full(w.shape, B, np.uint32), stats=dict(passable=0, blocked=w.size, reached=0, unreached=0, goals_used=0, goals_blocked=3, max_cost=0,
                                                                                    sum_cost=0))))
    # planar over a band = the 3-D run on a one-layer grid holding the AND pattern (a wall where any layer of the band has one)
    for name, lo, hi in (("planar-2-4", 2, 4), ("planar-clipped", -3, 1), ("planar-5", 5, 5)):
        a, b = max(lo, 0), min(hi, 5)
        flat = w[a:b + 1].any(axis=0)[None]
        out.append(Case("band/%s-flat" % name, flat, [centre(0, 0, 0)]))
        out.append(Case("band/" + name, w, [centre(0, 0, 3)], dict(iz_lo=lo, iz_hi=hi, planar=1), expect=dict(same_as="band/%s-flat" % name)))
    out.append(Case("band/planar-miss", w, [centre(0, 0, 3)], dict(iz_lo=6, iz_hi=9, planar=1),
                    expect=dict(full=np.full((1, 5, 7), B, np.uint32), stats=dict(passable=0, blocked=35, goals_blocked=1))))
    return out


# ---- goals
def goal_walls():
    rng = np.random.default_rng(22)
    w = rng.random((3, 10, 12)) < 0.2
    w[0, 0, 0] = w[2, 9, 0] = False; w[1, 4, 6] = True; w[-1, -1, -1] = True
    return w


def goals():
    w = goal_walls()
    a, b = centre(0, 0, 0), centre(0, 9, 2)
    never = [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, 2.0 ** 20], centre(-1, 0, 0), centre(12, 0, 0), centre(0, -1, 0), centre(0, 10, 0), centre(0, 0, -1),
             centre(0, 0, 3), centre(6, 4, 1)]                       # not finite, 2^20 voxels out, outside every side, in a wall
    out = [Case("goals/a", w, [a]), Case("goals/b", w, [b]),
           Case("goals/two", w, [a, b], expect=dict(min_of=("goals/a", "goals/b"), stats=dict(goals_used=2, goals_blocked=0), cost={(0, 0, 0): 0, (0, 9, 2): 0})),
           Case("goals/duplicates", w, [a, a, a], expect=dict(same_as="goals/a", stats=dict(goals_used=3, goals_blocked=0))),
           Case("goals/one-of-many", w, never + [a], expect=dict(same_as="goals/a", stats=dict(goals_used=1, goals_blocked=len(never)))),
           Case("goals/all-blocked", w, never, expect=dict(stats=dict(goals_used=0, goals_blocked=len(never), reached=0, max_cost=0, sum_cost=0)))]
    # an enclosed pocket: (3, 3) inside a ring of walls stays UNREACHED
    p = np.zeros((1, 7, 7), bool); p[0, 2:5, 2:5] = True; p[0, 3, 3] = False
    out.append(Case("goals/pocket", p, [centre(0, 0, 0)], expect=dict(cost={(3, 3, 0): U, (1, 1, 0): 4, (2, 2, 0): B}, stats=dict(unreached=1, blocked=8, reached=40))))
    return out


# ---- serpentine: 33 x 17 x 1, a wall every 4 columns with its door alternately at y = 16 and y = 0
def serpentine():
    w = np.zeros((1, 17, 33), bool)
    for k in range(1, 8):
        w[0, :, 4 * k] = True
        w[0, 16 if k % 2 else 0, 4 * k] = False
    # no diagonal enters a door, so the cells before, in and behind it are crossed by face moves.  (0, 0) to (3, 16): 3 corner + 13 face moves, 51; through the
    # door to (5, 16): 6.  Each later chamber: across, 2 corner + 14 face moves, 50, and through its door, 6 - six times.  Then (29, 16) to (32, 16): 9.
    far = 51 + 6 + 6 * (50 + 6) + 9
    return [Case("serpentine", w, [centre(0, 0, 0)], expect=dict(cost={(32, 16, 0): far, (5, 16, 0): 57, (3, 16, 0): 51}, reached=~w, min_rounds=3))]


# ---- corridor: 129 x 9 x 1 open, 17 x 2 tiles, goal at one end: a round visits only the tiles near the front
def corridor():
    w = np.zeros((1, 9, 129), bool)
    return [Case("corridor", w, [centre(0, 4, 0)], expect=dict(cost={(128, 4, 0): 384, (128, 0, 0): 3 * 124 + 4 * 4}, stats=dict(blocked=0, unreached=0), dirty_rule=True))]


# ---- late improvement: a voxel holds two different finite costs in successive rounds, so a tile is revisited after it first settled
LATE_SEED = 7


def late_walls(seed):
    w = np.random.default_rng(seed).random((1, 24, 24)) < 0.35
    w[0, 0, 0] = False
    return w


def _relax2d(cost, free, own):
    """cost (h, w) int64 relaxed in place to the fixed point of the 8 moves with the block rule, only the cells of `own` changing"""
    INF = np.int64(1) << 40
    h, w = cost.shape
    while True:
        new = cost.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                ys, yd = slice(max(0, -dy), h - max(0, dy)), slice(max(0, dy), h - max(0, -dy))      # from, to
                xs, xd = slice(max(0, -dx), w - max(0, dx)), slice(max(0, dx), w - max(0, -dx))
                ok = free[ys, xs] & free[yd, xd] & free[ys, xd] & free[yd, xs]
                cand = np.where(ok & (cost[ys, xs] < INF), cost[ys, xs] + 2 + abs(dx) + abs(dy), INF)
                new[yd, xd] = np.minimum(new[yd, xd], cand)
        new = np.where(own, new, cost)
        if (new == cost).all():
            return cost
        cost = new


def tile_rounds(walls2d, goal=(0, 0)):
    """the rounds of the tiled relaxation, every tile of a round taken to its fixed point under the halo the previous round left (T = 8)
    -> (the number of voxels that held two different finite costs in successive rounds, the rounds until nothing changed)"""
    INF = np.int64(1) << 40
    free = ~walls2d
    h, w = free.shape
    cost = np.full((h, w), INF); cost[goal[1], goal[0]] = 0
    late = np.zeros((h, w), bool)
    rounds = 0
    while True:
        rounds += 1
        new = cost.copy()
        for ty in range(0, h, T):
            for tx in range(0, w, T):
                y0, y1, x0, x1 = max(ty - 1, 0), min(ty + T + 1, h), max(tx - 1, 0), min(tx + T + 1, w)
                own = np.zeros((y1 - y0, x1 - x0), bool); own[ty - y0:ty - y0 + T, tx - x0:tx - x0 + T] = True
                sub = _relax2d(cost[y0:y1, x0:x1].copy(), free[y0:y1, x0:x1], own)
                new[ty:ty + T, tx:tx + T] = sub[own].reshape(new[ty:ty + T, tx:tx + T].shape)
        late |= (cost < INF) & (new < cost)
        if (new == cost).all():
            return int(late.sum()), rounds
        cost = new


def late_improvement():
    w = late_walls(LATE_SEED)
    n_late, rounds = tile_rounds(w[0])
    assert n_late >= 1 and rounds >= 3, (n_late, rounds)             # the property the seed was chosen for
    return [Case("late-improvement", w, [centre(0, 0, 0)], expect=dict(cost={(0, 0, 0): 0}, min_rounds=3))]


# ---- random boxes
def random_boxes():
    out = []
    for name, sides, frac, seed in (("40x30x9", (40, 30, 9), 0.25, 31), ("20x20x20", (20, 20, 20), 0.30, 32)):
        W, H, D = sides
        w = np.random.default_rng(seed).random((D, H, W)) < frac
        w[0, 0, 0] = False; w[-1, -1, -1] = True
        for d in (0, 2):
            out.append(Case("random/%s-d%d" % (name, d), w, [centre(0, 0, 0), centre(W // 2, H // 2, D // 2)], dict(min_d2=d), 2, dict(stats=dict(goals_blocked=0) if d == 0 and not w[D // 2, H // 2, W // 2] else {})))
    # the same boxes with few walls, where a clearance of 2 leaves most of the space connected
    for name, sides, seed in (("40x30x9", (40, 30, 9), 33), ("20x20x20", (20, 20, 20), 34)):
        W, H, D = sides
        w = np.random.default_rng(seed).random((D, H, W)) < 0.02
        w[:3, :3, :3] = False; w[-1, -1, -1] = True
        out.append(Case("random/%s-sparse-d2" % name, w, [centre(0, 0, 0), centre(W // 2, H // 2, D // 2)], dict(min_d2=2), 2, dict(cost={(0, 0, 0): 0})))
    return out


GROUPS = {"lines-x": lambda: lines(0), "lines-y": lambda: lines(1), "lines-z": lambda: lines(2), "open-box": open_box, "corner-rule": corner_rule, "clearance": clearance,
          "band": band, "goals": goals, "serpentine": serpentine, "corridor": corridor, "late-improvement": late_improvement, "random": random_boxes}
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
    """the occupancy and distance twins' results of a case -> (classes, d2, grid), computed once and shared (treat them as read-only)"""
    c = case(name)
    occ = mo.classify([c.records], [POSE], c.occ)
    assert occ["classes"].shape == c.sides[::-1] and ((occ["classes"] == mo.OCCUPIED) == c.walls).all(), name
    return occ["classes"], md.transform(occ["classes"], c.dist)["d2"], occ["grid"]


@functools.lru_cache(maxsize=None)
def twin_field(name):
    """the twin's field of a case, computed once and shared (treat it as read-only)"""
    c = case(name)
    cls, d2, grid = inputs(name)
    return mr.field(cls, d2, grid, c.goals, c.params)


def holds(c, cost, stats, other=twin_field):
    """`expect` and what holds of every field against one result (the twin's or the engine's): cost (Df, H, W) uint32, stats a dict; other(name) -> the result
    dict(cost=...) of another case for min_of and same_as"""
    e = c.expect
    assert cost.dtype == np.uint32 and cost.shape == c.field_sides[::-1], (c.name, cost.shape, c.field_sides)
    reached = cost < B
    assert stats["passable"] == stats["reached"] + stats["unreached"] and stats["passable"] + stats["blocked"] == c.cells, (c.name, stats)
    assert stats["reached"] == int(reached.sum()) and stats["unreached"] == int((cost == U).sum()) and stats["blocked"] == int((cost == B).sum()), (c.name, stats)
    assert stats["max_cost"] == (int(cost[reached].max()) if reached.any() else 0) and stats["sum_cost"] == int(cost[reached].sum(dtype=np.uint64)), (c.name, stats)
    assert stats["goals_used"] + stats["goals_blocked"] == len(c.goals), (c.name, stats)
    if not c.params.planar and c.params.min_d2 == 0 and c.params.iz_lo <= 0 and c.params.iz_hi >= c.sides[2] - 1:
        assert ((cost == B) == c.walls).all(), c.name                # without a clearance and a band the walls are what is blocked
    for f, v in e.get("stats", {}).items():
        assert stats[f] == v, (c.name, f, stats[f], v)
    if "full" in e:
        assert np.array_equal(cost, e["full"]), (c.name, "full", int((cost != e["full"]).sum()))
    for (x, y, z), v in e.get("cost", {}).items():
        assert int(cost[z, y, x]) == v, (c.name, (x, y, z), int(cost[z, y, x]), v)
    if "reached" in e:
        assert reached[e["reached"]].all(), c.name
    if "unreached" in e:
        assert (cost[e["unreached"]] == U).all(), c.name
    if "min_of" in e:
        a, b = (other(n)["cost"] for n in e["min_of"])
        assert np.array_equal(cost, np.minimum(a, b)), c.name
    if "same_as" in e:
        assert np.array_equal(cost, other(e["same_as"])["cost"]), c.name
