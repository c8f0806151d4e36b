"""tools/replay.py --occ-frontiers: the option checks, the command line, the run on the oracle backend (no GPU: out["frontiers"] carries the twin's statistics,
frontiers.csv the twin's regions of the replayed map) and, under -m gpu, on the GPU backend, which writes the same file byte for byte.  Without the option a
run writes what it wrote."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, maproute as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
Z = (0.3, 1.8)
HEAD = "region size faces cx cy cz lo_x lo_y lo_z hi_x hi_y hi_z"


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    occ = dict(occupancy_3d=True, save_dir=d)
    for kw in (dict(occ_frontiers=True), dict(occ_frontiers=True, save_dir=d), dict(occ, frontier_min_size=3), dict(occ, occ_frontiers=True, frontier_min_size=0),
               dict(occ, occ_frontiers=True, frontier_min_size=2.5), dict(occ, occ_frontiers=True, frontier_min_size=-4)):
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_parses_its_options(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(o in h.stdout for o in ("--occ-frontiers", "--frontier-min-size", "frontiers.csv"))
    d = str(tmp_path)
    for args, msg in ((["--occ-frontiers", "--save-dir", d], "--occ-frontiers needs --occupancy-3d"),
                      (["--occupancy-3d", "--save-dir", d, "--frontier-min-size", "3"], "--frontier-min-size needs --occ-frontiers"),
                      (["--occupancy-3d", "--occ-frontiers"], "--occupancy-3d needs --save-dir"),
                      (["--occupancy-3d", "--occ-frontiers", "--save-dir", d, "--frontier-min-size", "1.5"], "invalid int value")):
        r = subprocess.run(exe + ["--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(d)
    import inspect, replay
    p = inspect.signature(replay.run).parameters
    assert (p["occ_frontiers"].default, p["frontier_min_size"].default) == (False, 8)


def _run(tmp_path, backend, n_kf, name, **kw):
    import replay
    d = str(tmp_path / name); os.makedirs(d)
    out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, **kw)
    return d, out


def _want(n_kf, poses):
    """the occupancy twin's volume of the run's scans under its corrected poses"""
    import replay
    from qn_amd import synth
    prims, lidar, seeds, gt, odom, stamps = replay.make_lidar_stream(n_kf, 7, yaw_bias=0.006)
    scans = [synth.lidar_scan(prims, lidar, T, int(sd)) for T, sd in zip(gt, seeds)]
    return mo.classify(scans, poses)


def _read(path, cols):
    rows = open(path).read().splitlines()
    assert rows[0] == HEAD + (" reach ex ey ez" if cols == 16 else "")
    return np.array([[float(v) for v in r.split()] for r in rows[1:]], np.float64).reshape(-1, cols)


def _run_and_check(tmp_path, backend, n_kf):
    plain, out0 = _run(tmp_path, backend, n_kf, "plain", occ_slice=Z, occ_distance=True)
    assert "frontiers" not in out0 and "frontiers.csv" not in os.listdir(plain)
    occ = _want(n_kf, out0["poses"])
    g = occ["grid"]
    layers = (mo.layer_of(Z[0], g), mo.layer_of(Z[1], g))
    goal = tuple(float(x) for x in np.asarray(out0["poses"][0])[:3, 3])
    files = {}
    # every layer with the defaults and no distance field at all; the slice's band with a smaller min_size and the reach costs of a route field
    for name, kw, fp, rp in (("all", dict(occ_frontiers=True), mf.FrontierParams(), None),
                             ("reach", dict(occ_frontiers=True, frontier_min_size=5, occ_slice=Z, occ_distance=True, occ_route=goal, route_min_d2=0),
                              mf.FrontierParams(min_size=5, iz_lo=layers[0], iz_hi=layers[1]), mr.RouteParams(min_d2=0))):
        d, out = _run(tmp_path, backend, n_kf, name, **kw)
        want = mf.frontier(occ["classes"], fp)
        print("%s backend, %s: %s" % (backend, name, want["stats"]))
        assert out["frontiers"] == dict(want["stats"]._asdict(), **fp._asdict())
        assert want["stats"].regions >= 1
        base = [f for f in os.listdir(plain) if name != "all" or not f.startswith("occupancy_slice")]
        assert sorted(os.listdir(d)) == sorted(base + ["frontiers.csv"] + (["route.csv"] if rp is not None else []))
        for f in base:                                               # what a run wrote without the option, it writes with it
            assert open(os.path.join(d, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        rows = _read(os.path.join(d, "frontiers.csv"), 16 if rp is not None else 12)
        info = want["info"]
        assert len(rows) == len(info) and rows[:, 0].tolist() == list(range(len(info)))
        assert rows[:, 1].tolist() == info["size"].tolist() and rows[:, 2].tolist() == info["faces"].tolist()
        assert np.allclose(rows[:, 3:6], mo.centres(mf.centroid(info), g), atol=1e-6)
        assert np.array_equal(rows[:, 6:9], info["lo"]) and np.array_equal(rows[:, 9:12], info["hi"])
        if rp is not None:
            d2 = md.transform(occ["classes"], md.DistanceParams())["d2"]
            cost = mr.field(occ["classes"], d2, g, [goal], rp)["cost"]
            k, at = mf.costs(want["labels"], len(info), cost)
            ok = k < mr.BLOCKED
            assert ok.any() and np.allclose(rows[ok, 12], mr.metres(k, g.voxel)[ok], atol=1e-6) and np.isinf(rows[~ok, 12]).all()
            assert np.allclose(rows[ok, 13:16], mo.centres(at[ok], g), atol=1e-6) and np.isnan(rows[~ok, 13:16]).all()
        files[name] = open(os.path.join(d, "frontiers.csv"), "rb").read()
    return files


def test_oracle_backend_writes_the_twins_regions(tmp_path):
    files = _run_and_check(tmp_path, "oracle", 5)
    assert all(len(f.splitlines()) >= 2 for f in files.values())


@pytest.mark.gpu
def test_gpu_backend_writes_the_oracles_bytes(tmp_path):
    gpu = _run_and_check(tmp_path / "gpu", "gpu", 5)
    oracle = {}
    goal = None
    for name, kw in (("all", dict(occ_frontiers=True)), ("reach", dict(occ_frontiers=True, frontier_min_size=5, occ_slice=Z, occ_distance=True, route_min_d2=0))):
        if name == "reach":
            kw["occ_route"] = goal
        d, out = _run(tmp_path / "oracle", "oracle", 5, name, **kw)
        goal = tuple(float(x) for x in np.asarray(out["poses"][0])[:3, 3])
        oracle[name] = open(os.path.join(d, "frontiers.csv"), "rb").read()
    assert gpu == oracle
