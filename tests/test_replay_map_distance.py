"""tools/replay.py --occ-distance: the option checks, the command line, the run on the oracle backend (no GPU: out["distance"] carries the twin's statistics,
occupancy_inflated.pgm is mapground.to_pgm of mapdistance.inflate of the twin's two slices) and, under -m gpu, on the GPU backend, which writes the same files
byte for byte.  Without the option a run writes what it wrote."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapdistance as md, mapground as mg, mapoccupancy as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
Z = (0.3, 1.8)
RADIUS = 0.7


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    occ = dict(occupancy_3d=True, save_dir=d)
    for kw in (dict(occ_distance=True), dict(occ_distance=True, save_dir=d), dict(occ, occ_unknown_obstacle=True), dict(occ, robot_radius=0.5),
               dict(occ, occ_distance=True, occ_dist_max=0), dict(occ, occ_distance=True, occ_dist_max=256), dict(occ, occ_distance=True, occ_dist_max=2.5),
               dict(occ, occ_distance=True, robot_radius=-1.0), dict(occ, occ_distance=True, robot_radius=float("nan"))):
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_parses_its_options(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(o in h.stdout for o in ("--occ-distance", "--occ-dist-max", "--occ-unknown-obstacle", "--robot-radius M"))
    d = str(tmp_path)
    for args, msg in ((["--occ-distance", "--save-dir", d], "--occ-distance needs --occupancy-3d"),
                      (["--occupancy-3d", "--save-dir", d, "--robot-radius", "0.5"], "need --occ-distance"),
                      (["--occupancy-3d", "--save-dir", d, "--occ-unknown-obstacle"], "need --occ-distance"),
                      (["--occupancy-3d", "--save-dir", d, "--occ-distance", "--occ-dist-max", "1.5"], "invalid int value")):
        r = subprocess.run(exe + ["--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(d)
    import inspect, replay
    p = inspect.signature(replay.run).parameters
    assert {"occ_distance", "occ_dist_max", "occ_unknown_obstacle", "robot_radius"} <= set(p)
    assert (p["occ_distance"].default, p["occ_dist_max"].default, p["occ_unknown_obstacle"].default, p["robot_radius"].default) == (False, 16, False, None)


def _run(tmp_path, backend, n_kf, name, **kw):
    import replay
    d = str(tmp_path / name); os.makedirs(d)
    out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, occ_slice=Z, **kw)
    return d, out


def _want(n_kf, poses):
    """the occupancy twin's volume of the run's scans under its corrected poses"""
    import replay
    from qn_amd import synth
    prims, lidar, seeds, gt, odom, stamps = replay.make_lidar_stream(n_kf, 7, yaw_bias=0.006)
    scans = [synth.lidar_scan(prims, lidar, T, int(sd)) for T, sd in zip(gt, seeds)]
    return mo.classify(scans, poses)


def _run_and_check(tmp_path, backend, n_kf):
    plain, out0 = _run(tmp_path, backend, n_kf, "plain")
    assert "distance" not in out0 and "occupancy_inflated.pgm" not in os.listdir(plain)
    want = _want(n_kf, out0["poses"])
    g = want["grid"]
    lo, hi = mo.layer_of(Z[0], g), mo.layer_of(Z[1], g)
    occ = mo.slice2d(want["classes"], lo, hi)
    files = {}
    for name, kw, mask, r in (("occupied", dict(occ_distance=True, robot_radius=RADIUS), 1 << mo.OCCUPIED, 16),
                              ("unknown", dict(occ_distance=True, robot_radius=RADIUS, occ_unknown_obstacle=True, occ_dist_max=5), (1 << mo.OCCUPIED) | (1 << mo.UNKNOWN), 5)):
        d, out = _run(tmp_path, backend, n_kf, name, **kw)
        field = md.transform(want["classes"], (mask, r))
        s = field["stats"]
        print("%s backend, %s: %d x %d x %d, sites %d reached %d far %d max_d2 %d sum_d2 %d" % (backend, name, g.width, g.height, g.depth, *s))
        assert out["distance"] == dict(s._asdict(), site_mask=mask, max_dist=r) and out["occupancy"] == out0["occupancy"]
        assert sorted(os.listdir(d)) == sorted(os.listdir(plain) + ["occupancy_inflated.pgm", "occupancy_inflated.yaml"])
        for f in os.listdir(plain):                                  # what a run wrote without the option, it writes with it
            assert open(os.path.join(d, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        r2 = int(np.floor((RADIUS / g.voxel) ** 2))
        inflated = md.inflate(occ, md.slice2d(field["d2"], lo, hi), r2)
        assert r2 == 5 and (inflated == 2).sum() > (occ == 2).sum() > 0 and ((inflated == 2) | (inflated == occ)).all()
        assert open(os.path.join(d, "occupancy_inflated.pgm"), "rb").read() == mg.to_pgm(inflated)
        assert open(os.path.join(d, "occupancy_inflated.yaml")).read() == mg.map_yaml(mg.GridInfo(g.origin[0], g.origin[1], g.voxel, g.width, g.height, 0),
                                                                                     "occupancy_inflated.pgm")
        files[name] = open(os.path.join(d, "occupancy_inflated.pgm"), "rb").read()
    assert files["occupied"] != files["unknown"]                     # unknown space as an obstacle closes more of the slice
    # occ_distance without a slice or a radius: the statistics alone
    import replay
    d = str(tmp_path / "stats"); os.makedirs(d)
    out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, occ_distance=True)
    assert out["distance"]["max_dist"] == 16 and sorted(os.listdir(d)) == ["occupied.pcd", "poses_kitti.txt", "poses_tum.txt"]
    return files


def test_oracle_backend_writes_the_twins_field(tmp_path):
    _run_and_check(tmp_path, "oracle", 5)


@pytest.mark.gpu
def test_gpu_backend_writes_the_oracles_bytes(tmp_path):
    gpu = _run_and_check(tmp_path / "gpu", "gpu", 5)
    oracle = {}
    for name, kw in (("occupied", {}), ("unknown", dict(occ_unknown_obstacle=True, occ_dist_max=5))):
        d, _ = _run(tmp_path / "oracle", "oracle", 5, name, occ_distance=True, robot_radius=RADIUS, **kw)
        oracle[name] = open(os.path.join(d, "occupancy_inflated.pgm"), "rb").read()
    assert gpu == oracle
