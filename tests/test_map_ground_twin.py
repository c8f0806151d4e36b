"""The numpy twin of the map's ground stage (qn_amd/mapground.py, the specification of qn_kf_map_ground): its relaxed envelope against the closed form, the
hand cases whose answers follow from the geometry, and what it does to the ray-cast street scene.  No GPU."""
import numpy as np
import pytest
from qn_amd import mapground as mg, synth

F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]


@pytest.mark.parametrize("step_s", [1, 2, 7, 300])
def test_relaxed_envelope_is_the_closed_form(step_s):
    rng = np.random.default_rng(step_s)
    step_d = (step_s * 181) >> 7
    assert step_s <= step_d <= 2 * step_s
    shapes = [(1, 1), (1, 40), (40, 1), (40, 40), (33, 17)] + [tuple(rng.integers(1, 41, 2)) for _ in range(12)]
    for H, W in shapes:
        for share in (0.0, None, 0.05, 0.5, 1.0):                   # no seed, one seed, a few, half, all
            seed = np.full((H, W), mg.INF, np.int32)
            if share is None:
                seed[rng.integers(H), rng.integers(W)] = rng.integers(-4000, 4000)
            else:
                m = rng.random((H, W)) < share
                seed[m] = rng.integers(-4000, 4000, int(m.sum()))
            g = mg.envelope(seed, step_s, step_d)
            assert g.dtype == np.int32 and np.array_equal(g, mg.envelope_closed_form(seed, step_s, step_d)), (H, W, share)
            assert (g <= seed).all() and ((g == mg.INF).all() if (seed == mg.INF).all() else (g < mg.INF).all())


def test_envelope_saturates_instead_of_wrapping():
    seed = np.full((1, 9), mg.INF, np.int32); seed[0, 0] = 2 ** 30 - 1
    g = mg.envelope(seed, 2 ** 29, (2 ** 29 * 181) >> 7)
    assert g.tolist() == [[2 ** 30 - 1, 2 ** 30 - 1 + 2 ** 29] + [mg.INF] * 7] and np.array_equal(g, mg.envelope_closed_form(seed, 2 ** 29, (2 ** 29 * 181) >> 7))


def test_units():
    assert mg.units(mg.GroundParams()) == (11, 307, 434, 410, 4096)                      # 0.3 * 0.5 * 2^11 = 307.2; 0.2 * 2^11 = 409.6
    assert [mg.quant_exponent(c) for c in (0.5, 0.51, 1.0, 1024.0, 1025.0, 2 ** -20, 1e300, 1e-300)] == [11, 10, 10, 0, -1, 30, -126, 127]
    assert mg.units((1.0, 1e-9, 0.0, 1.0, 1))[1:3] == (1, 1)
    assert mg.units((0.5, 2.5 / 1024, 0.5 / 2048, 1.5 / 2048, 1))[1:] == (2, 2, 0, 2)     # ties at .5 go to even: 2.5 -> 2, 0.5 -> 0, 1.5 -> 2
    for bad in [(0.0, 0.3, 0.2, 2.0, 1), (0.5, 0.0, 0.2, 2.0, 1), (0.5, 0.3, -0.1, 2.0, 1), (0.5, 0.3, 0.2, 0.2, 1), (0.5, 0.3, 0.2, 2.0, 0), (0.5, 0.3, 0.2, 2.0, 1.5),
                (float("nan"), 0.3, 0.2, 2.0, 1), (0.5, float("inf"), 0.2, 2.0, 1), (0.5, 1e7, 0.2, 2.0, 1), (0.5, 0.3, 0.2, 1e6, 1)]:
        with pytest.raises(ValueError):
            mg.units(bad)


def _floor(nx, ny, cell=0.5, z=0.0):
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([(ix.ravel() + 0.5) * cell, (iy.ravel() + 0.5) * cell, np.full(nx * ny, z)], axis=1).astype(np.float32)


def test_flat_floor_with_a_box_on_it():
    """a 12 x 12 m floor and a 2 x 2 x 3 m box: the floor is GROUND, the box's sides are OBSTACLE up to the clearance and OVERHEAD above it, like its top"""
    floor = _floor(24, 24)
    floor = floor[~((floor[:, 0] > 5) & (floor[:, 0] < 7) & (floor[:, 1] > 5) & (floor[:, 1] < 7))]          # nothing is seen under the box
    zs = np.arange(0.5, 3.0, 0.25)                                  # (a return 0.25 m up a wall is within ground_tol of the envelope one step off the floor)
    side = np.array([[x, y, z] for z in zs for x in (5.05, 6.95) for y in np.arange(5.25, 7.0, 0.5)] +
                    [[x, y, z] for z in zs for y in (5.05, 6.95) for x in np.arange(5.25, 7.0, 0.5)], np.float32)
    top = _floor(4, 4, 0.5, 3.0) + F([5.0, 5.0, 0.0])
    r = mg.classify(np.concatenate([floor, side, top]))
    c = r["classes"]; nf, ns = len(floor), len(side)
    assert (c[:nf] == mg.GROUND).all()
    assert np.array_equal(c[nf:nf + ns], np.where(side[:, 2] <= 2.0, mg.OBSTACLE, mg.OVERHEAD))
    inner = (top[:, 0] > 5.5) & (top[:, 0] < 6.5) & (top[:, 1] > 5.5) & (top[:, 1] < 6.5)
    assert (c[nf + ns:] == mg.OVERHEAD).all() and inner.sum() == 4
    occ = r["occupancy"]
    assert occ.shape == (24, 24) and (occ[10:14, 10:14] == [[2, 2, 2, 2], [2, 1, 1, 2], [2, 1, 1, 2], [2, 2, 2, 2]]).all()      # the rim occupies, the roof alone does not
    assert (np.delete(occ.ravel(), [y * 24 + x for y in range(10, 14) for x in range(10, 14)]) == 1).all()
    assert r["ground_q"][10, 11] == 307 and r["ground_q"][11, 11] == 614 and r["ground_q"][12, 12] == 614      # under the box: straight steps off the floor around it
    s = r["stats"]
    assert (s.width, s.height, s.seeded, s.occupied, s.free, s.unknown) == (24, 24, 576, 12, 564, 0) and s.n_ground == nf and s.n_below == 0


def test_a_slab_above_an_empty_span_leaves_it_free():
    """two strips of floor 6 m apart and a slab 4 m above the gap between them: the columns under the slab hold OVERHEAD points only and stay free"""
    a = _floor(4, 6); b = _floor(4, 6) + F([8.0, 0.0, 0.0])
    slab = _floor(12, 6, 0.5, 4.0) + F([2.0, 0.0, 0.0])
    r = mg.classify(np.concatenate([a, b, slab]))
    assert (r["classes"][:48] == mg.GROUND).all() and (r["classes"][48:] == mg.OVERHEAD).all()
    assert (r["occupancy"] == 1).all() and r["stats"].occupied == 0
    g = r["ground_q"][0]
    assert g[:4].tolist() == [0] * 4 and g[4:16].tolist() == [307 * min(k + 1, 12 - k) for k in range(12)] and g[16:].tolist() == [0] * 4
    assert r["seed"][0, 4] == 4 * 2048                               # the slab seeds its columns, the floor beside it lowers them


def test_a_lone_point_below_the_floor_and_min_points():
    floor = _floor(9, 9)
    pit = np.array([[2.25, 2.25, -1.5]], np.float32)
    r = mg.classify(np.concatenate([floor, pit]))
    # min_points = 1: the lone point seeds its column and drags the ground down around it - it is GROUND, its column's floor point an OBSTACLE
    assert r["classes"][-1] == mg.GROUND and r["classes"][4 * 9 + 4] == mg.OBSTACLE and r["stats"].n_below == 0
    assert r["ground_q"][4, 4] == -3072 and r["ground_q"][4, 5] == -3072 + 307
    # min_points = 3 with three floor points everywhere but in the columns of a 3 x 3 patch, which hold one floor point and at most one more: those nine are
    # not seeded, their ground comes from around them (one step up at the rim, two in the middle), and class BELOW appears there and only there
    rest = floor[[i for i in range(81) if not (3 <= i % 9 <= 5 and 3 <= i // 9 <= 5)]]
    both = np.concatenate([floor, rest, rest, pit, [[2.75, 2.25, -0.05], [1.75, 2.75, -0.3]]]).astype(np.float32)
    r = mg.classify(both, (0.5, 0.3, 0.2, 2.0, 3))
    assert r["stats"].seeded == 72 and (r["seed"][3:6, 3:6] == mg.INF).all()
    assert r["ground_q"][4, 4] == 2 * 307 and r["ground_q"][4, 5] == 307 and r["ground_q"][5, 3] == 307
    assert r["classes"][-3:].tolist() == [mg.BELOW, mg.GROUND, mg.BELOW] and r["height_q"][-3:].tolist() == [-3072 - 614, -102 - 307, -614 - 307]
    below = np.flatnonzero(r["classes"] == mg.BELOW)
    assert below.tolist() == [4 * 9 + 4, len(both) - 3, len(both) - 1]               # the middle column's own floor point lies 614 > tol_q under its envelope
    assert (np.delete(r["classes"], below) == mg.GROUND).all() and r["stats"].n_below == 3


def test_ties_of_the_quantisation_and_cell_borders():
    # cell 0.5: 2^-11 m units; z = (k + 0.5) 2^-11 is a tie and goes to the even neighbour
    z = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5], np.float64) / 2048
    pts = np.stack([np.full(6, 0.25), np.full(6, 0.25), z], axis=1).astype(np.float32)
    r = mg.classify(pts, (0.5, 0.3, 0.0, 1.0, 1))
    assert r["height_q"].tolist() == [0 + 2, 2 + 2, 2 + 2, 0 + 2, 0, 4 + 2]              # zq = 0 2 2 0 -2 4, seed = rint(-1.5) = -2
    assert r["classes"].tolist() == [mg.OBSTACLE] * 4 + [mg.GROUND, mg.OBSTACLE]
    # x and y on cell borders, negative too: the border belongs to the cell above it
    xs = np.array([-1.0, -0.5, -1e-30, 0.0, 0.5, 0.75, 1.0], np.float32)
    pts = np.stack([xs, -xs, np.zeros(7)], axis=1).astype(np.float32)
    r = mg.classify(pts)
    assert (r["info"].origin_x, r["info"].origin_y, r["info"].width, r["info"].height) == (-1.0, -1.0, 5, 5)
    occ = r["occupancy"]
    want = np.zeros((5, 5), np.uint8)
    for cx, cy in [(0, 4), (1, 3), (1, 2), (2, 2), (3, 1), (3, 0), (4, 0)]:               # floor(2 x) + 2, floor(-2 x) + 2
        want[cy, cx] = 1
    assert np.array_equal(occ, want) and r["stats"].unknown == 18


def test_non_finite_records_and_an_all_non_finite_map():
    pts = np.array([[0.1, 0.1, 0.0], [np.nan, 0.1, 0.0], [0.1, np.inf, 0.0], [0.1, 0.1, -np.inf], [0.2, 0.2, 1.0]], np.float32)
    r = mg.classify(pts)
    assert r["classes"].tolist() == [1, 0, 0, 0, 2] and r["height_q"].tolist() == [0, mg.NO_HEIGHT, mg.NO_HEIGHT, mg.NO_HEIGHT, 2048]
    assert (r["stats"].n, r["stats"].n_finite, r["stats"].n_none, r["stats"].width, r["stats"].height) == (5, 2, 3, 1, 1)
    r = mg.classify(pts[1:4])
    assert r["classes"].tolist() == [0, 0, 0] and r["ground_q"].shape == (0, 0) and r["occupancy"].shape == (0, 0)
    assert r["info"] == (0.0, 0.0, 0.5, 0, 0, 11) and r["stats"].n_none == 3 and r["stats"].unknown == 0
    assert mg.to_pgm(r["occupancy"]) == b"P5\n0 0\n255\n"
    with pytest.raises(mg.CapacityError):
        mg.classify(np.array([[0, 0, 0], [40000, 40000, 0]], np.float32), (0.5, 0.3, 0.2, 2.0, 1))      # 80001^2 columns
    with pytest.raises(mg.CapacityError):
        mg.classify(np.array([[0, 0, 2.0 ** 19]], np.float32))                                         # 2^19 * 2^11 = 2^30
    assert mg.classify(np.array([[0, 0, 2.0 ** 19 - 1]], np.float32))["stats"].n_ground == 1


def test_to_pgm_and_map_yaml():
    occ = np.array([[2, 1, 0], [1, 1, 2]], np.uint8)                 # row 0 is the smallest y
    pgm = mg.to_pgm(occ)
    assert pgm == b"P5\n3 2\n255\n" + bytes([254, 254, 0, 0, 254, 205])           # the image's first row is the largest y
    y = mg.map_yaml(mg.GridInfo(-12.5, 3.0, 0.5, 3, 2, 11))
    assert y.splitlines()[:3] == ["image: map.pgm", "resolution: 0.5", "origin: [-12.5, 3.0, 0]"] and "negate: 0" in y and "occupied_thresh" in y and "free_thresh" in y
    assert mg.keep(np.arange(10).reshape(5, 2), [0, 1, 2, 3, 4], 0b10010).tolist() == [[2, 3], [8, 9]]
    for bad in (0, 32, 33, -1):
        with pytest.raises(ValueError):
            mg.keep(np.zeros((1, 3)), [0], bad)


def street_scene_by_kind():
    """the four ray-cast scans of the street scene in the world frame, and for every record whether its ray hit the ground primitive: a ray that hits
    something else returns the same bytes when the scene is cast without its ground, a ray that hit the ground does not"""
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    rest = prims[prims["kind"] != synth.PRIM_GROUND]
    pts = []; ground = []
    for pose, seed in zip(POSES, [11, 12, 13, 14]):
        full = synth.lidar_scan(prims, SEN, pose, seed)
        other = {r.tobytes() for r in synth.lidar_scan(rest, SEN, pose, seed)}
        ground.append(np.array([r.tobytes() not in other for r in full]))
        T = np.asarray(pose, np.float64)
        pts.append((full[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    return np.concatenate(pts), np.concatenate(ground)


def test_street_scene_ground_and_what_stands_on_it():
    """MEASURED with the twin on the CPU, default parameters, the four scans of tests/test_gpu_map_outliers.py (16 beams x 300 columns) in the world frame,
    15 497 records: 10 308 were hit on QN_SIM_GROUND and every one of them (share 1.0000) comes out GROUND; of the 5 189 wall, pole and box records 87.26 % do
    not come out GROUND (the others are the returns off the foot of a wall, a pole or a box, within ground_tol of the envelope).  Classes: 10 969 GROUND,
    3 930 OBSTACLE, 598 OVERHEAD; grid 240 x 218 with 518 occupied columns.  The bounds below are what the twin alone was seen to satisfy."""
    pts, on_ground = street_scene_by_kind()
    r = mg.classify(pts)
    c = r["classes"]
    g_share = float((c[on_ground] == mg.GROUND).mean()); o_share = float((c[~on_ground] != mg.GROUND).mean())
    print("street scene: %d records, %d on the ground of which %.4f GROUND; %d on walls, poles and boxes of which %.4f not GROUND; classes %s; grid %d x %d, occupied %d"
          % (len(pts), on_ground.sum(), g_share, (~on_ground).sum(), o_share, np.bincount(c, minlength=5).tolist(), r["stats"].width, r["stats"].height,
             r["stats"].occupied))
    assert len(pts) > 8000 and on_ground.sum() > 2000 and (~on_ground).sum() > 2000
    assert g_share >= G_BOUND and o_share >= O_BOUND


G_BOUND, O_BOUND = 0.99, 0.85
