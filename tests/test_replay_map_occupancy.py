"""tools/replay.py --occupancy-3d: the option checks, the command line, the writers on the numpy twin's output (no GPU: occupied.pcd has a valid header and one
row per occupied voxel, occupancy_slice.pgm is mapground.to_pgm of the twin's slice), the run on the oracle backend and, under -m gpu, on the GPU backend,
which writes the same files byte for byte."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapground as mg, mapoccupancy as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(occupancy_3d=True), dict(occ_slice=(0.0, 1.0), save_dir=d), dict(occupancy_3d=True, save_dir=d, occ_voxel=0.0),
               dict(occupancy_3d=True, save_dir=d, occ_voxel=float("nan")), dict(occupancy_3d=True, save_dir=d, occ_min_range=-1.0),
               dict(occupancy_3d=True, save_dir=d, occ_max_range=0.5), dict(occupancy_3d=True, save_dir=d, occ_shell=-1),
               dict(occupancy_3d=True, save_dir=d, occ_slice=(2.0, 1.0)), dict(occupancy_3d=True, save_dir=d, occ_slice=(0.0, float("inf")))):
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_parses_its_options(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(o in h.stdout for o in ("--occupancy-3d", "--occ-voxel", "--occ-min-range", "--occ-max-range", "--occ-shell", "--occ-slice ZLO ZHI"))
    for args, msg in ((["--occupancy-3d"], "--occupancy-3d needs --save-dir"), (["--occ-slice", "0", "1", "--save-dir", str(tmp_path)], "--occ-slice needs --occupancy-3d"),
                      (["--occupancy-3d", "--save-dir", str(tmp_path), "--occ-slice", "0"], "expected 2 arguments"),
                      (["--occupancy-3d", "--save-dir", str(tmp_path), "--occ-shell", "1.5"], "invalid int value")):
        r = subprocess.run(exe + ["--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(str(tmp_path))
    import inspect, replay
    assert {"occupancy_3d", "occ_voxel", "occ_min_range", "occ_max_range", "occ_shell", "occ_slice"} <= set(inspect.signature(replay.run).parameters)


def _read_pcd(path):
    lines = open(path).read().splitlines()
    i = lines.index("DATA ascii")
    head = dict(l.split(None, 1) for l in lines[1:i])
    return head, np.array([[float(v) for v in l.split()] for l in lines[i + 1:]], np.float64).reshape(-1, 5)


def _check_files(d, want, z):
    """occupied.pcd and occupancy_slice.pgm / .yaml in d are those of the twin's result `want` and the heights z"""
    g = want["grid"]
    head, rows = _read_pcd(os.path.join(d, "occupied.pcd"))
    ijk, hits, misses = mo.voxel_list(want, 1 << mo.OCCUPIED)
    assert head["VERSION"] == "0.7" and head["FIELDS"] == "x y z hits misses" and head["SIZE"] == "4 4 4 4 4" and head["TYPE"] == "F F F U U"
    assert head["COUNT"] == "1 1 1 1 1" and head["WIDTH"] == head["POINTS"] == str(len(ijk)) and head["HEIGHT"] == "1" and len(rows) == len(ijk) == want["stats"].occupied
    assert np.array_equal(rows[:, :3].astype(F), mo.centres(ijk, g).astype(F)) and np.array_equal(rows[:, 3], hits) and np.array_equal(rows[:, 4], misses)
    lo, hi = mo.layer_of(z[0], g), mo.layer_of(z[1], g)
    occ = mo.slice2d(want["classes"], lo, hi)
    assert open(os.path.join(d, "occupancy_slice.pgm"), "rb").read() == mg.to_pgm(occ)
    y = open(os.path.join(d, "occupancy_slice.yaml")).read()
    assert y == mg.map_yaml(mg.GridInfo(g.origin[0], g.origin[1], g.voxel, g.width, g.height, 0), "occupancy_slice.pgm")
    assert y.splitlines()[:3] == ["image: occupancy_slice.pgm", "resolution: %r" % g.voxel, "origin: [%r, %r, 0]" % (g.origin[0], g.origin[1])]
    return lo, hi, occ


def test_writers_on_the_twins_output(tmp_path):
    import replay
    rng = np.random.default_rng(5)
    d = rng.normal(size=(400, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    clouds = [(d * rng.uniform(1.0, 6.0, (400, 1))).astype(F), (d[::-1] * 4.0).astype(F)]
    poses = [np.eye(4), np.eye(4)]; poses[1][:3, 3] = [2.0, -1.0, 0.5]
    want = mo.classify(clouds, poses)
    assert replay.write_occupancy(str(tmp_path), want) is None and sorted(os.listdir(str(tmp_path))) == ["occupied.pcd"]
    layers = replay.write_occupancy(str(tmp_path), want, (-0.5, 1.0))
    lo, hi, occ = _check_files(str(tmp_path), want, (-0.5, 1.0))
    assert layers == (lo, hi) and lo < hi and (occ == 2).any() and (occ == 1).any() and (occ == 0).any()
    pgm = open(os.path.join(str(tmp_path), "occupancy_slice.pgm"), "rb").read()
    assert pgm.startswith(b"P5\n%d %d\n255\n" % (want["grid"].width, want["grid"].height)) and len(pgm) == len(b"P5\n%d %d\n255\n" % occ.shape[::-1]) + occ.size


def _run_and_check(tmp_path, backend, n_kf):
    import replay
    from qn_amd import synth
    d = str(tmp_path / "occ"); os.makedirs(d)
    z = (0.3, 1.8)
    out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, occ_slice=z)
    prims, lidar, seeds, gt, odom, stamps = replay.make_lidar_stream(n_kf, 7, yaw_bias=0.006)
    scans = [synth.lidar_scan(prims, lidar, T, int(sd)) for T, sd in zip(gt, seeds)]
    want = mo.classify(scans, out["poses"])
    lo, hi, occ = _check_files(d, want, z)
    s = want["stats"]
    print("%s backend: %d rays, %d misses, grid %d x %d x %d, occupied %d free %d unknown %d, slice layers %d .. %d"
          % (backend, s.n_rays, s.total_misses, s.width, s.height, s.depth, s.occupied, s.free, s.unknown, lo, hi))
    assert out["occupancy"] == dict(n_rays=s.n_rays, total_misses=s.total_misses, width=s.width, height=s.height, depth=s.depth, occupied=s.occupied, free=s.free,
                                    unknown=s.unknown, slice_layers=[lo, hi])
    assert s.occupied > 1000 and s.free > s.occupied and (occ == 1).sum() > (occ == 2).sum() > 0
    assert sorted(os.listdir(d)) == ["occupancy_slice.pgm", "occupancy_slice.yaml", "occupied.pcd", "poses_kitti.txt", "poses_tum.txt"]
    # without the option the directory holds what it held
    d2 = d + "_plain"; os.makedirs(d2)
    replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d2)
    assert sorted(os.listdir(d2)) == ["poses_kitti.txt", "poses_tum.txt"]
    for f in os.listdir(d2):
        assert open(os.path.join(d2, f), "rb").read() == open(os.path.join(d, f), "rb").read(), f


def test_oracle_backend_writes_the_twins_volume(tmp_path):
    _run_and_check(tmp_path, "oracle", 5)


@pytest.mark.gpu
def test_gpu_backend_writes_the_twins_volume(tmp_path):
    _run_and_check(tmp_path, "gpu", 8)
