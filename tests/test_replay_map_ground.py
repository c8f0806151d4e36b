"""tools/replay.py --occupancy-grid: the option checks, the run on the oracle backend (no GPU: the oracle's voxel grid as the map, the numpy twin's grid) and,
under -m gpu, on the GPU backend: map.pgm is, byte for byte, qn_amd/mapground.to_pgm of the twin's classification of the points of the written map.pcd,
map.yaml names it with its resolution and origin, --drop-ground writes the map without its ground, and without the option the directory holds what it held."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapground as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARAMS = (0.5, 0.3, 0.2, 2.0, 1)


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(occupancy_grid=True), dict(occupancy_grid=True, save_dir=d), dict(occupancy_grid=True, save_map_leaf=0.3),
               dict(drop_ground=True, save_dir=d, save_map_leaf=0.3),
               dict(occupancy_grid=True, save_dir=d, save_map_leaf=0.3, grid_cell=0.0), dict(occupancy_grid=True, save_dir=d, save_map_leaf=0.3, grid_cell=float("nan")),
               dict(occupancy_grid=True, save_dir=d, save_map_leaf=0.3, max_slope=0.0), dict(occupancy_grid=True, save_dir=d, save_map_leaf=0.3, ground_tol=-0.1),
               dict(occupancy_grid=True, save_dir=d, save_map_leaf=0.3, clearance=0.2)):
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_refuses_the_grid_without_a_map(tmp_path):
    for args, msg in ((["--occupancy-grid"], "--occupancy-grid needs"), (["--occupancy-grid", "--save-dir", str(tmp_path)], "--occupancy-grid needs"),
                      (["--drop-ground", "--save-dir", str(tmp_path), "--save-map-leaf", "0.3"], "--drop-ground needs --occupancy-grid")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(str(tmp_path))


def _read_pcd(path):
    lines = open(path).read().splitlines()
    fields = [l for l in lines if l.startswith("FIELDS")][0].split()[1:]
    return fields, np.array([[float(v) for v in l.split()] for l in lines[lines.index("DATA ascii") + 1:]], np.float64).astype(np.float32)


def _check_dir(d, out, sensor_kw):
    import replay
    fields, m = _read_pcd(os.path.join(d, "map.pcd"))
    want = mg.classify(m, PARAMS)
    s = want["stats"]
    print("map.pcd: %d points; grid %d x %d, %d occupied, %d free, %d unknown" % (len(m), s.width, s.height, s.occupied, s.free, s.unknown))
    assert fields[:4] == ["x", "y", "z", "intensity"] and len(m) > 500 and s.occupied > 0 and s.free > s.occupied
    assert open(os.path.join(d, "map.pgm"), "rb").read() == mg.to_pgm(want["occupancy"])
    y = open(os.path.join(d, "map.yaml")).read()
    assert y == mg.map_yaml(want["info"], "map.pgm")
    assert y.splitlines()[:3] == ["image: map.pgm", "resolution: 0.5", "origin: [%r, %r, 0]" % (want["info"].origin_x, want["info"].origin_y)]
    assert out["grid"] == dict(width=s.width, height=s.height, occupied=s.occupied, free=s.free, unknown=s.unknown, n_ground=s.n_ground)
    # --drop-ground: the same grid, the map without its GROUND class
    d2 = d + "_dropped"; os.makedirs(d2)
    replay.run(verbose=False, save_dir=d2, save_map_leaf=0.3, occupancy_grid=True, drop_ground=True, **sensor_kw)
    _, m2 = _read_pcd(os.path.join(d2, "map.pcd"))
    assert np.array_equal(m2.view(np.uint32), mg.keep(m, want["classes"], 0b11101).view(np.uint32)) and 0 < len(m2) < len(m)
    assert open(os.path.join(d2, "map.pgm"), "rb").read() == open(os.path.join(d, "map.pgm"), "rb").read()
    # without the option the directory holds what it held, byte for byte
    d3 = d + "_plain"; os.makedirs(d3)
    replay.run(verbose=False, save_dir=d3, save_map_leaf=0.3, **sensor_kw)
    assert sorted(os.listdir(d3)) == sorted(f for f in os.listdir(d) if f not in ("map.pgm", "map.yaml") and (sensor_kw["backend"] == "gpu" or f != "map.pcd"))
    for f in os.listdir(d3):
        assert open(os.path.join(d3, f), "rb").read() == open(os.path.join(d, f), "rb").read(), f


def test_oracle_backend_writes_the_twins_grid(tmp_path):
    import replay
    d = str(tmp_path / "grid"); os.makedirs(d)
    kw = dict(n_kf=6, seed=7, sensor="spinning", backend="oracle")
    out = replay.run(verbose=False, save_dir=d, save_map_leaf=0.3, occupancy_grid=True, **kw)
    _check_dir(d, out, kw)


@pytest.mark.gpu
def test_gpu_backend_writes_the_twins_grid(tmp_path):
    import replay
    d = str(tmp_path / "grid"); os.makedirs(d)
    kw = dict(n_kf=8, seed=7, sensor="spinning", backend="gpu")
    out = replay.run(verbose=False, save_dir=d, save_map_leaf=0.3, occupancy_grid=True, **kw)
    _check_dir(d, out, kw)
