"""The numpy twin of the occupancy map's route field (qn_amd/maproute.py) against the definition: its bucketed field() equals its dijkstra() - the explicit edge
list of every allowed move handed to a shortest-path routine - byte for byte on the case table of tests/route_cases.py, and both meet what the construction of
each case determines.  Then the paths (every step the first allowed move in the stated order whose cost drop is its weight), the queries, the refusals of
check_params, metres and centres, and the street scene of tests/test_gpu_map_distance.py with its numbers.  Integers throughout: no tolerance.  No GPU."""
import numpy as np
import pytest
import distance_cases as dc
import route_cases as rc
from qn_amd import mapdistance as md, mapoccupancy as mo, maproute as mr, synth

SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
# (params, passable, reached, max_cost, the costs at the voxels of POSES[0 .. 3]): scipy's Dijkstra under the definition on the occupancy and distance twins
STREET = (((1 << mo.FREE, 4, 0, mr.INT32_MAX, 0), 161688, 160901, 1118, (0, mr.BLOCKED, 458, 486)),
          ((1 << mo.FREE, 0, 0, mr.INT32_MAX, 0), 181038, 181013, 901, (0, 63, 128, 188)),
          ((1 << mo.FREE, 4, 6, 6, 1), 13626, 5946, 254, (0, mr.BLOCKED, mr.UNREACHED, mr.UNREACHED)))


def path_holds(cost, grid, params, starts, lens, ijk, max_len, what):
    """every path of one paths() result (the twin's or the engine's) against the definition, without the walk of the twin: cost the (Df, H, W) field"""
    inside, c = mr.voxels_of(grid, starts, params)
    Df, H, W = cost.shape
    for i in range(len(starts)):
        v = tuple(int(a) for a in c[i])
        at = int(cost[v[2], v[1], v[0]]) if inside[i] else mr.BLOCKED
        if at >= mr.BLOCKED:
            assert lens[i] == 0 and not ijk[i].any(), (what, i)      # outside, blocked or unreached
            continue
        n = int(lens[i])
        assert 1 <= n <= at // 3 + 1 and tuple(ijk[i, 0]) == v, (what, i, n, at)
        assert not ijk[i, min(n, max_len):].any(), (what, i)
        for k in range(min(n, max_len)):
            x, y, z = (int(a) for a in ijk[i, k])
            cur = int(cost[z, y, x])
            if k == n - 1:
                assert cur == 0, (what, i, k)                        # the path ends at a goal
                break
            if k + 1 == max_len:
                break                                                # truncated: the next voxel is not returned
            step = tuple(int(a) for a in ijk[i, k + 1] - ijk[i, k])
            first = next(o for o in mr.MOVES if mr.allowed(cost, (x, y, z), o) and int(cost[z + o[2], y + o[1], x + o[0]]) + mr.weight(o) == cur)
            assert step == first, (what, i, k, step, first)          # an allowed move whose cost drop is its weight, and the first such in the stated order
        if n <= max_len:
            assert int(cost[tuple(ijk[i, n - 1][::-1])]) == 0, (what, i)


@pytest.mark.parametrize("g", rc.NAMES)
def test_field_is_the_definition_on_the_table(g):
    for c in rc.group(g):
        cls, d2, grid = rc.inputs(c.name)
        got = rc.twin_field(c.name)
        rc.holds(c, got["cost"], got["stats"]._asdict())
        want = mr.dijkstra(cls, d2, grid, c.goals, c.params)
        assert got["cost"].tobytes() == want["cost"].tobytes() and got["stats"] == want["stats"], (c.name, int((got["cost"] != want["cost"]).sum()))
        free = mr.passable(cls, d2, c.params)
        assert np.array_equal(got["cost"] != mr.BLOCKED, free) and got["stats"] == mr.stats_of(got["cost"], got["stats"].goals_used, got["stats"].goals_blocked), c.name


@pytest.mark.parametrize("g", rc.NAMES)
def test_paths_walk_down_the_field(g):
    for c in rc.group(g):
        _, _, grid = rc.inputs(c.name)
        cost = rc.twin_field(c.name)["cost"]
        starts = c.starts()
        assert 8 <= len(starts) <= 16
        full = int(cost[cost < mr.BLOCKED].max()) // 3 + 1 if (cost < mr.BLOCKED).any() else 1
        for max_len in (full, 3):
            lens, ijk = mr.paths(cost, grid, starts, max_len, c.params)
            assert lens.dtype == np.uint32 and ijk.dtype == np.int32 and ijk.shape == (len(starts), max_len, 3)
            path_holds(cost, grid, c.params, starts, lens, ijk, max_len, (c.name, max_len))
        lens, _ = mr.paths(cost, grid, starts, full, c.params)
        q = mr.query(cost, grid, starts, c.params)
        assert lens[-1] == 0 and q[12] in (0, mr.BLOCKED) and lens[12] == (1 if q[12] == 0 else 0), c.name      # the point outside; the goal itself, used or ignored
        if c.walls.any() and not c.params.planar:
            assert lens[13] == 0, c.name                             # the wall
        assert ((q < mr.BLOCKED) == (lens > 0)).all() and (lens[q < mr.BLOCKED] <= q[q < mr.BLOCKED] // 3 + 1).all(), c.name


def test_a_path_longer_than_max_len_is_truncated_and_an_unreached_start_has_none():
    c = rc.case("serpentine")
    _, _, grid = rc.inputs(c.name)
    cost = rc.twin_field(c.name)["cost"]
    lens, ijk = mr.paths(cost, grid, [rc.centre(32, 16, 0)], 5, c.params)
    assert lens[0] > 100 and ijk[0].tolist()[:2] == [[32, 16, 0], [31, 16, 0]] and ijk.shape == (1, 5, 3)
    c = rc.case("goals/pocket")
    _, _, grid = rc.inputs(c.name)
    lens, ijk = mr.paths(rc.twin_field(c.name)["cost"], grid, [rc.centre(3, 3, 0), rc.centre(2, 2, 0), rc.centre(1, 1, 0)], 4, c.params)
    assert lens.tolist() == [0, 0, 2] and ijk[2].tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("name", ["band/inside", "band/planar-5", "goals/two", "random/20x20x20-d0"])
def test_queries_are_direct_indexing(name):
    c = rc.case(name)
    _, _, grid = rc.inputs(name)
    cost = rc.twin_field(name)["cost"]
    xyz, first_outside = dc.query_points(grid)
    q = mr.query(cost, grid, xyz, c.params)
    out = xyz[first_outside:]
    with np.errstate(invalid="ignore"):                              # in planar mode a point above or below the grid still reads its column
        column = (np.abs(out) < 2.0 ** 20).all(axis=1) & (out[:, 0] >= 0) & (out[:, 0] < grid.width) & (out[:, 1] >= 0) & (out[:, 1] < grid.height) & bool(c.params.planar)
    assert q.dtype == np.uint32 and (q[first_outside:][~column] == mr.BLOCKED).all()
    assert np.array_equal(q[first_outside:][column], cost[0, np.floor(out[column, 1]).astype(int), np.floor(out[column, 0]).astype(int)])
    inside = np.floor(xyz[:first_outside]).astype(np.int64)          # (voxel 1, the grid starts at voxel 0: exact)
    if c.params.planar:
        inside[:, 2] = 0
    assert np.array_equal(q[:first_outside], cost[inside[:, 2], inside[:, 1], inside[:, 0]])
    if c.params.planar:                                              # z does not choose the column, but must be finite and below the limit
        p = mr.query(cost, grid, [[0.5, 0.5, 1e5], [0.5, 0.5, -77.0], [0.5, 0.5, np.nan], [0.5, 0.5, 2.0 ** 20]], c.params)
        assert p.tolist() == [int(cost[0, 0, 0])] * 2 + [mr.BLOCKED] * 2


def test_check_params_refusals_and_defaults():
    assert mr.RouteParams() == (1 << mo.FREE, 4, 0, 0x7fffffff, 0) and mr.BLOCKED == 0xfffffffe and mr.UNREACHED == 0xffffffff
    bad = ((0, 4, 0, 1, 0), (8, 4, 0, 1, 0), (9, 0, 0, 1, 0), (1.5, 0, 0, 1, 0), (2, -1, 0, 1, 0), (2, 2 ** 32, 0, 1, 0), (2, 0.5, 0, 1, 0), (2, 4, 2, 1, 0),
           (2, 4, 0, 2 ** 31, 0), (2, 4, -2 ** 31 - 1, 0, 0), (2, 4, 0.5, 1, 0), (2, 4, 0, 1, 2), (2, 4, 0, 1, 0.5), (-1, 4, 0, 1, 0))
    for p in bad:
        with pytest.raises(ValueError):
            mr.check_params(mr.RouteParams(*p))
        with pytest.raises(ValueError):
            mr.field(np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint16), mo.OccupancyGrid((0.0, 0.0, 0.0), 1.0, 1, 1, 1, (0, 0, 0)), [[0.5, 0.5, 0.5]], p)
    for ok in ((1, 0, 0, 0, 0), (7, 65025, -2 ** 31, 2 ** 31 - 1, 1), (2, 4, 3, 3, 0)):
        mr.check_params(mr.RouteParams(*ok))
    mr.check_params(mr.RouteParams(2, 4), max_dist=2)                # min_d2 = max_dist^2 is accepted, one more is refused
    with pytest.raises(ValueError):
        mr.check_params(mr.RouteParams(2, 5), max_dist=2)
    grid = mo.OccupancyGrid((0.0, 0.0, 0.0), 1.0, 1, 1, 1, (0, 0, 0))
    one = (np.zeros((1, 1, 1), np.uint8), np.full((1, 1, 1), md.FAR, np.uint16), grid)
    for goals in (np.zeros((0, 3)), np.zeros(((1 << 20) + 1, 3))):
        with pytest.raises(ValueError):
            mr.field(*one, goals, (1, 0))
    with pytest.raises(ValueError):
        mr.paths(np.zeros((1, 1, 1), np.uint32), grid, [[0.5, 0.5, 0.5]], 0)
    with pytest.raises(ValueError):
        mr.passable(np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint16))


def test_the_empty_grid():
    grid = mo.OccupancyGrid((0.0, 0.0, 0.0), 0.3, 0, 0, 0, (0, 0, 0))
    for planar in (0, 1):
        p = mr.RouteParams(planar=planar)
        r = mr.field(np.zeros((0, 0, 0), np.uint8), np.zeros((0, 0, 0), np.uint16), grid, [[0.0, 0.0, 0.0]], p)
        assert r["cost"].size == 0 and r["cost"].dtype == np.uint32 and r["stats"] == (0, 0, 0, 0, 0, 1, 0, 0)
        assert mr.query(r["cost"], grid, np.zeros((2, 3)), p).tolist() == [mr.BLOCKED] * 2
        assert mr.paths(r["cost"], grid, np.zeros((2, 3)), 3, p)[0].tolist() == [0, 0]


def test_metres_and_centres():
    m = mr.metres(np.array([0, 3, 4, 5, 300, mr.BLOCKED, mr.UNREACHED], np.uint32), 0.5)
    assert m.dtype == np.float64 and m[:5].tolist() == [0.0, 0.5, 4.0 / 3.0 * 0.5, 5.0 / 3.0 * 0.5, 50.0] and np.isinf(m[5:]).all()
    # the chamfer metric against the straight line: 4 / (3 sqrt 2) along a face diagonal, the lowest ratio, sqrt(11) / 3 in the direction (3, 1, 1), the highest
    for v in ((9, 9, 9), (9, 9, 0), (9, 4, 0), (9, 3, 3), (9, 3, 0), (9, 0, 0)):
        s = sorted(v)
        assert 0.9428 <= (3 * s[2] + s[1] + s[0]) / 3.0 / np.sqrt(float(np.dot(v, v))) <= 1.1056, v
    grid = mo.OccupancyGrid((-0.6, 0.3, 0.9), 0.3, 4, 5, 6, (-2, 1, 3))
    ijk = np.array([[0, 0, 0], [3, 4, 5]])
    assert np.allclose(mr.centres(grid, ijk), [[-0.45, 0.45, 1.05], [0.45, 1.65, 2.55]], atol=1e-12)
    flat = mr.centres(grid, np.array([[0, 0, 0], [3, 4, 0]]), mr.RouteParams(iz_lo=2, iz_hi=9, planar=1))
    assert np.allclose(flat, [[-0.45, 0.45, (3 + 4.0) * 0.3], [0.45, 1.65, (3 + 4.0) * 0.3]], atol=1e-12)      # the middle of the layers 2 .. 5
    assert np.isnan(mr.centres(grid, [[0, 0, 0]], mr.RouteParams(iz_lo=6, iz_hi=9, planar=1))[0, 2])


def test_late_improvement_really_revisits_a_settled_tile():
    """the property the seed of the late-improvement case was chosen for, and that other seeds lack"""
    assert rc.T == 8
    n_late, rounds = rc.tile_rounds(rc.late_walls(rc.LATE_SEED)[0])
    assert n_late >= 1 and rounds >= 3
    assert any(rc.tile_rounds(rc.late_walls(s)[0])[0] == 0 for s in (1, 2, 5))


@pytest.fixture(scope="module")
def street():
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    scans = [synth.lidar_scan(prims, SEN, T, sd) for T, sd in zip(POSES, [11, 12, 13, 14])]
    occ = mo.classify(scans, POSES)
    assert occ["classes"].shape == (14, 334, 344)
    return occ["classes"], md.transform(occ["classes"], (1 << mo.OCCUPIED, 16))["d2"], occ["grid"]


@pytest.mark.parametrize("params, passable, reached, max_cost, at_poses", STREET)
def test_street_scene(street, params, passable, reached, max_cost, at_poses):
    cls, d2, grid = street
    goal = [POSES[0][:3, 3]]
    assert mr.voxels_of(grid, goal, params)[1].tolist() == [[151, 164, 0 if params[4] else 6]]
    got = mr.field(cls, d2, grid, goal, params)
    want = mr.dijkstra(cls, d2, grid, goal, params)
    assert got["cost"].tobytes() == want["cost"].tobytes() and got["stats"] == want["stats"]
    s = got["stats"]
    print(params, s)
    assert (s.passable, s.reached, s.max_cost, s.goals_used) == (passable, reached, max_cost, 1)
    assert mr.query(got["cost"], grid, np.array([P[:3, 3] for P in POSES]), params).tolist() == list(at_poses)
    lens, ijk = mr.paths(got["cost"], grid, [P[:3, 3] for P in POSES], 400, params)
    path_holds(got["cost"], grid, mr.RouteParams(*params), np.array([P[:3, 3] for P in POSES]), lens, ijk, 400, "street")
