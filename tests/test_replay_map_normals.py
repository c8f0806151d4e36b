"""tools/replay.py --save-map-normals: the option checks (no GPU needed), and under -m gpu a short spinning-LiDAR replay whose map.pcd carries the seven
fields x y z intensity normal_x normal_y normal_z curvature with finite unit normals on at least 90 % of its points.  The replay's sensor has 32 rings and its
twelve keyframes stand about 15 m apart, so far ground rings are sparse: within 0.9 m 97.7 % of the map's points have five neighbours (within the default 0.6 m:
90.6 %, a coin toss against the bound; a host k-d tree on the twin's scans under the odometry poses), hence --normal-radius 0.9 here."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(save_map_normals=True),                                                  # no save_dir, no leaf
               dict(save_map_normals=True, save_dir=d),                                      # --save-map-normals without --save-map-leaf
               dict(save_map_normals=True, save_map_leaf=0.3),                               # no save_dir
               dict(save_map_normals=True, save_dir=d, save_map_leaf=0.3, backend="oracle"),  # the oracle backend writes no map
               dict(save_map_normals=True, save_dir=d, save_map_leaf=0.3, normal_radius=0.0),
               dict(save_map_normals=True, save_dir=d, save_map_leaf=0.3, normal_radius=float("nan")),
               dict(save_map_normals=True, save_dir=d, save_map_leaf=0.3, normal_min_neighbors=2),
               dict(save_map_normals=True, save_dir=d, save_map_leaf=0.3, normal_min_neighbors=5.5)):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, **kw)
    assert not os.listdir(d)


def test_the_command_line_refuses_normals_without_a_map(tmp_path):
    for args in (["--save-map-normals"], ["--save-map-normals", "--save-dir", str(tmp_path)], ["--save-map-normals", "--save-map-leaf", "0.3"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "--save-map-normals needs --save-dir and --save-map-leaf" in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(str(tmp_path))


def test_the_pcd_writer_names_the_seven_fields(tmp_path):
    import replay
    p = os.path.join(str(tmp_path), "m.pcd")
    replay.write_pcd_xyzi_normal(p, np.float32([[1, 2, 3, 4], [5, 6, 7, 8]]), np.float32([[0, 0, 1], [np.nan] * 3]), np.float32([0.25, np.nan]))
    lines = open(p).read().splitlines()
    assert "FIELDS x y z intensity normal_x normal_y normal_z curvature" in lines and "POINTS 2" in lines and "COUNT 1 1 1 1 1 1 1 1" in lines
    assert lines[-2].split() == ["1", "2", "3", "4", "0", "0", "1", "0.25"] and lines[-1].split()[4:] == ["nan"] * 4


@pytest.mark.gpu
def test_replay_writes_a_map_with_unit_normals(tmp_path):
    import replay
    out = replay.run(n_kf=12, seed=7, verbose=False, sensor="spinning", save_dir=str(tmp_path), save_map_leaf=0.3, save_map_normals=True, normal_radius=0.9)
    lines = open(os.path.join(str(tmp_path), "map.pcd")).read().splitlines()
    assert "FIELDS x y z intensity normal_x normal_y normal_z curvature" in lines
    m = np.array([[float(v) for v in l.split()] for l in lines[lines.index("DATA ascii") + 1:]], np.float64)
    assert m.shape == (out["map_points"], 8) and m.shape[0] > 1000
    ok = np.isfinite(m[:, 4:]).all(axis=1)
    print("map.pcd: %d points, %d with a normal (%.1f %%)" % (len(m), ok.sum(), 100.0 * ok.mean()))
    assert ok.sum() == out["map_normals_valid"] and ok.mean() >= 0.90
    assert np.abs(np.linalg.norm(m[ok, 4:7], axis=1) - 1.0).max() < 1e-6 and (m[ok, 7] >= 0).all() and (m[ok, 7] <= 1.0 / 3.0 + 1e-6).all()
    corrected = np.array([T[:3, 3] for T in out["poses"]])
    d = corrected[np.argmin(((m[ok, None, :3] - corrected[None]) ** 2).sum(axis=2), axis=1)] - m[ok, :3]
    assert ((m[ok, 4:7] * d).sum(axis=1) > -1e-5 * np.linalg.norm(d, axis=1)).all()                  # every normal faces the nearest keyframe position
