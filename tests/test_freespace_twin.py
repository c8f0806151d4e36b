"""The free-space (see-through) check's specification, qn_amd/freespace.py, on the CPU: the bisection against the plain count, the bins against an arctan2
projection, a scan against itself, the dropped points, the window's wrap and clip, and what the figure is for.

The scenario (test_true_pose_is_seen_through_less_than_wrong_ones): three synth street scenes, a 32 x 720 sensor, two poses 5, 12 and 20 m apart with the second
turned by 0.7 rad, window 1 x 1, tolerance 0.3 m + 2 % of range.  Share of the observed points seen through (q in c, c in q), by the exact rule of the twin:
  scene, separation   true pose        2 m along        3 m across       10 degrees       180 degrees
  0,  5 m             0.0000 0.0000    0.0569 0.1152    0.0807 0.1056    0.0964 0.1068    0.0678 0.1198
  1, 12 m             0.0000 0.0013    0.0550 0.0622    0.0460 0.0552    0.0740 0.0561    0.0322 0.0673
  2, 20 m             0.0000 0.0000    0.2780 0.0337    0.0004 0.0015    0.0036 0.0001    0.1318 0.0002
(18 500 .. 22 800 observed points per direction.  The 20 m scene's sideways and 10 degree cases stay small: its far scan sees little of what the near one sees.
These replace the approximate figures of the CPU probe that used an arctan projection.)
Only the ordering is asserted: each wrong transform's larger direction exceeds both directions of the true pose."""
import math
import numpy as np
import pytest
from qn_amd import freespace as fs, synth


def _params(**kw):
    d = dict(n_rows=16, n_cols=90, el_lo=math.radians(-20.0), el_hi=math.radians(12.0), min_range=1.0)
    d.update(kw)
    return fs.Params(**d)


def _plain_rows(z, rho, t):
    return sum((fs.row_predicate(z, rho, t, np.full(len(z), i)).astype(np.int64) for i in range(len(t))), np.zeros(len(z), np.int64))


def _plain_cols(x, y, c, s):
    return sum((fs.col_predicate(x, y, c, s, np.full(len(x), j)).astype(np.int64) for j in range(1, len(c))), np.zeros(len(x), np.int64))


def test_bisection_equals_the_plain_count():
    rng = np.random.default_rng(1)
    for p in (_params(), _params(n_rows=1, n_cols=1, window_rows=0, window_cols=0), _params(n_rows=37, n_cols=721), fs.Params()):
        t, c, s = fs.tables(p)
        a = rng.normal(0, 20, (4000, 3)); a[:, 2] *= 0.2
        a = a.astype(np.float32).astype(np.float64)
        # points exactly on the column boundaries (as far as f32 allows) and on the row edges, and the axes
        rad = rng.uniform(1, 50, len(c))
        on_col = np.stack([rad * c, rad * s, rng.normal(0, 1, len(c))], 1).astype(np.float32).astype(np.float64)
        rho = rng.uniform(1, 50, len(t))
        on_row = np.stack([rho, np.zeros(len(t)), rho * t], 1)
        on_row32 = on_row.astype(np.float32).astype(np.float64)
        axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [3, 0, 0.0], [-3, 0, 0.5]], np.float64)
        pts = np.concatenate([a, on_col, on_row, on_row32, axes])
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        rho = np.sqrt(x * x + y * y)
        assert np.array_equal(fs.count_rows(z, rho, t), _plain_rows(z, rho, t))
        assert np.array_equal(fs.count_cols(x, y, c, s), _plain_cols(x, y, c, s))
        # a point built exactly on edge i (z = rho t[i] in f64) has that edge at or below it
        rows = fs.count_rows(on_row[:, 2], on_row[:, 0], t) - 1
        assert np.array_equal(rows, np.arange(len(t)))


def test_bins_equal_an_arctan2_projection_away_from_the_edges():
    rng = np.random.default_rng(2)
    for p in (_params(), _params(n_rows=37, n_cols=721), fs.Params()):
        nr, nc = p.n_rows, p.n_cols
        a = rng.normal(0, 25, (20000, 3)); a[:, 2] *= 0.25
        a = a.astype(np.float32).astype(np.float64)
        x, y, z = a[:, 0], a[:, 1], a[:, 2]
        el = np.arctan2(z, np.hypot(x, y)); az = np.mod(np.arctan2(y, x), 2 * np.pi)
        fr = (el - p.el_lo) / (p.el_hi - p.el_lo) * nr; fc = az / (2 * np.pi) * nc
        clear = (np.abs(fr - np.round(fr)) * (p.el_hi - p.el_lo) / nr > 1e-6) & (np.abs(fc - np.round(fc)) * 2 * np.pi / nc > 1e-6)
        row, col, r, fin, keep = fs.project(a, p)
        want_row = np.floor(fr).astype(np.int64); want_col = np.floor(fc).astype(np.int64)
        inside = (want_row >= 0) & (want_row < nr)
        assert clear.sum() > 19000 and inside.sum() > 2000
        assert np.array_equal(keep[clear], (inside & (r >= p.min_range))[clear])
        k = clear & keep
        assert np.array_equal(row[k], want_row[k]) and np.array_equal(col[k], want_col[k])
        assert np.allclose(r, np.sqrt((a * a).sum(1)), rtol=1e-15)


def _street(seed, separation, sensor):
    rng = np.random.Generator(np.random.PCG64(synth.BASE_SEED + 700000 + seed))
    scene = synth.Scene(rng, 120.0)
    for _ in range(500):
        x, y = rng.uniform(-25.0, 25.0, 2); yaw = rng.uniform(-np.pi, np.pi)
        xb, yb = x + separation * np.cos(yaw), y + separation * np.sin(yaw)
        if synth._free_spot(scene, x, y) and synth._free_spot(scene, xb, yb):
            break
    else:
        raise RuntimeError("no free sensor spot")
    Pa, Pb = synth.sensor_pose(x, y, yaw), synth.sensor_pose(xb, yb, yaw + 0.7)
    prims = scene.primitives()
    return synth.lidar_scan(prims, sensor, Pa, 11 + seed), synth.lidar_scan(prims, sensor, Pb, 977 + seed), np.linalg.inv(Pb) @ Pa


def test_a_scan_against_itself_agrees_everywhere():
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    p = fs.Params.for_sensor(sen)
    a, b, _ = _street(0, 5.0, sen)
    assert len(a) > 5000 and len(b) > 5000
    rec = fs.freespace(a, b, np.eye(4), p)
    for scan, key, other in ((a, "q_in_c", b), (b, "c_in_q", a)):
        own = fs.direction(scan, np.eye(4), *fs.range_images(scan, p), p, points=True)
        assert own["n"] == len(scan) == own["n_finite"] and own["seen_through"] == 0 and own["occluded"] == 0
        assert own["agree"] == own["observed"] == own["in_fov"] > 0.99 * len(scan)
        assert set(np.unique(own["classes"])) <= {fs.DROPPED, fs.AGREE}
        assert rec[key]["n"] == len(scan)


def test_every_simulated_beam_sits_at_a_row_centre():
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    p = fs.Params.for_sensor(sen)
    t, _, _ = fs.tables(p)
    el = sen.elevations()
    centres = p.el_lo + (np.arange(32) + 0.5) * (p.el_hi - p.el_lo) / 32
    assert np.allclose(centres, el, atol=1e-12) and t[0] < math.tan(el[0]) and t[-1] > math.tan(el[-1])
    a, _, _ = _street(0, 5.0, sen)
    row, col, r, fin, keep = fs.project(a[:, :3].astype(np.float64), p)
    assert keep.sum() > 0.99 * len(a)


def test_dropped_points_are_class_0_and_counted_as_specified():
    p = _params(min_range=2.0)
    near = np.full((p.n_rows, p.n_cols), 10.0, np.float32); far = near.copy()
    pts = np.array([[10, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 0, 0],          # agree, three non-finite, inside min_range
                    [5, 0, 5], [5, 0, -5], [0, 0, 3], [0, 0, 0], [0, -10, 0.1]], np.float32)         # above, below the field of view, the axis, the origin, agree
    rec = fs.direction(pts, np.eye(4), near, far, p, points=True)
    assert rec["classes"].tolist() == [4, 0, 0, 0, 0, 0, 0, 0, 0, 4]
    assert (rec["n"], rec["n_finite"], rec["in_fov"], rec["observed"], rec["seen_through"], rec["occluded"], rec["agree"]) == (10, 7, 2, 2, 0, 0, 2)
    im = fs.range_images(pts, p)
    assert np.isfinite(im[0]).sum() == 2 and (im[1] > 0).sum() == 2
    # a transform that overflows makes the point non-finite: dropped, not counted as finite
    T = np.eye(4); T[0, 3] = 1e308; T[0, 0] = 1e308
    rec = fs.direction(np.array([[1e30, 0, 0]], np.float32), T, near, far, p)
    assert (rec["n"], rec["n_finite"], rec["in_fov"]) == (1, 0, 0)
    assert fs.see_through_fraction(rec) == 0.0
    for bad in (dict(el_lo=0.5, el_hi=0.4), dict(el_hi=2.0), dict(n_rows=0), dict(n_cols=8193), dict(n_rows=1025), dict(tol_abs=-1.0), dict(tol_rel=float("nan")),
                dict(window_rows=16), dict(window_cols=45), dict(min_range=-1.0)):
        with pytest.raises(ValueError):
            fs.tables(_params(**bad))


def test_the_classes_and_the_window():
    p = _params(window_rows=1, window_cols=1)
    nr, nc = p.n_rows, p.n_cols
    t, c, s = fs.tables(p)

    def at(row, col, r):
        el = p.el_lo + (row + 0.5) * (p.el_hi - p.el_lo) / nr; az = 2 * math.pi * (col + 0.5) / nc
        return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]

    near = np.full((nr, nc), np.inf, np.float32); far = np.zeros((nr, nc), np.float32)
    near[5, 0] = far[5, 0] = 20.0                                     # one return, in column 0
    pts = np.array([at(5, 0, 20.0), at(5, 0, 10.0), at(5, 0, 30.0), at(5, 0, 20.5), at(5, 0, 19.4),
                    at(5, nc - 1, 10.0), at(5, 1, 10.0), at(5, 2, 10.0), at(5, nc - 2, 10.0),         # the window wraps in columns
                    at(4, 0, 10.0), at(6, 0, 10.0), at(3, 0, 10.0), at(7, 0, 10.0)], np.float32)
    cls, _ = fs.classify(pts.astype(np.float64), near, far, p)
    assert cls.tolist() == [4, 2, 3, 4, 4, 2, 2, 1, 1, 2, 2, 1, 1]
    # tolerances: 0.3 + 0.02 r
    for r, want in ((19.33, 4), (19.30, 2), (20.70, 4), (20.73, 3)):          # 1.02 r + 0.3 < 20 below 19.3137; 0.98 r - 0.3 > 20 above 20.7143
        assert fs.classify(np.array([at(5, 0, r)], np.float32).astype(np.float64), near, far, p)[0][0] == want, r
    # the window is clipped in rows: a return in the top row is not seen from the bottom row
    near[:] = np.inf; far[:] = 0.0
    near[nr - 1, 7] = far[nr - 1, 7] = 20.0
    pts = np.array([at(0, 7, 10.0), at(nr - 1, 7, 10.0), at(nr - 2, 7, 10.0)], np.float32)
    assert fs.classify(pts.astype(np.float64), near, far, p)[0].tolist() == [1, 2, 2]
    # a wider window, and none
    near[:] = np.inf; far[:] = 0.0
    near[5, 0] = far[5, 0] = 20.0
    pts = np.array([at(5, nc - 3, 10.0), at(5, 3, 10.0), at(5, 4, 10.0), at(8, 0, 10.0)], np.float32).astype(np.float64)
    assert fs.classify(pts, near, far, _params(window_rows=1, window_cols=3))[0].tolist() == [2, 2, 1, 1]
    assert fs.classify(pts, near, far, _params(window_rows=3, window_cols=0))[0].tolist() == [1, 1, 1, 2]
    assert fs.classify(np.array([at(5, 0, 10.0), at(5, 1, 10.0)]), near, far, _params(window_rows=0, window_cols=0))[0].tolist() == [2, 1]
    # near and far of one pixel are the min and the max
    im = fs.range_images(np.array([at(2, 3, 7.0), at(2, 3, 9.0), at(2, 3, 8.0)], np.float32), p)
    assert im[0][2, 3] == np.float32(np.sqrt((np.array(at(2, 3, 7.0), np.float32).astype(np.float64) ** 2).sum())) and im[0][2, 3] < im[1][2, 3]
    assert np.isinf(im[0]).sum() == nr * nc - 1 and (im[1] == 0).sum() == nr * nc - 1


def _delta(dx=0.0, dy=0.0, yaw=0.0):
    D = np.eye(4); c, s = math.cos(yaw), math.sin(yaw)
    D[:2, :2] = [[c, -s], [s, c]]; D[0, 3] = dx; D[1, 3] = dy
    return D


WRONG = (("2 m along", _delta(dx=2.0)), ("3 m across", _delta(dy=3.0)), ("10 degrees", _delta(yaw=math.radians(10.0))), ("180 degrees", _delta(yaw=math.pi)))


def test_inverse_is_the_engines():
    from qn_amd import scancontext as sc
    T = synth.sensor_pose(3.0, -4.0, 0.9) @ _delta(0.2, 0.1, 0.05)
    assert np.array_equal(fs.inverse(T), sc.relative_pose(T, np.eye(4)))
    assert np.allclose(fs.inverse(T) @ T, np.eye(4), atol=1e-14)


def test_true_pose_is_seen_through_less_than_wrong_ones():
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    p = fs.Params.for_sensor(sen)
    for seed, sep in ((0, 5.0), (1, 12.0), (2, 20.0)):
        a, b, T = _street(seed, sep, sen)
        qi, ci = fs.range_images(a, p), fs.range_images(b, p)
        true = fs.freespace(a, b, T, p, q_images=qi, c_images=ci)
        ft = (fs.see_through_fraction(true["q_in_c"]), fs.see_through_fraction(true["c_in_q"]))
        print("scene %d, %2.0f m: true pose          %.4f %.4f  (observed %d / %d of %d / %d)" % (seed, sep, ft[0], ft[1], true["q_in_c"]["observed"],
                                                                                                true["c_in_q"]["observed"], len(a), len(b)))
        assert true["q_in_c"]["observed"] > 1000 and true["c_in_q"]["observed"] > 1000
        for name, D in WRONG:
            w = fs.freespace(a, b, D @ T, p, q_images=qi, c_images=ci)
            fw = (fs.see_through_fraction(w["q_in_c"]), fs.see_through_fraction(w["c_in_q"]))
            print("scene %d, %2.0f m: %-18s %.4f %.4f" % (seed, sep, name, fw[0], fw[1]))
            assert max(fw) > ft[0] and max(fw) > ft[1], (seed, name, fw, ft)
