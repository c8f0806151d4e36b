"""tools/replay.py --occ-view-gain: the option checks, the command line, the run on the oracle backend (no GPU: out["view_gain"] carries the twin's statistics,
view_gain.csv one row per frontier region of the replayed map) and, under -m gpu, on the GPU backend, which writes the same file byte for byte.  Without the
option a run writes what it wrote, and frontiers.csv stays as it is with it."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapdistance as md, mapfrontier as mf, mapoccupancy as mo, maproute as mr, mapview as mv
from test_replay_map_frontier import _run, _want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEAD = "region x y z gain blocked escaped spent reached"
SENSOR = dict(view_range=12.0, view_beams=8, view_azimuth=90)


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    occ = dict(occupancy_3d=True, save_dir=d)
    fr = dict(occ, occ_frontiers=True)
    for kw in (dict(occ_view_gain=True), dict(occ, occ_view_gain=True), dict(fr, view_range=30.0), dict(fr, view_beams=8), dict(fr, view_azimuth=90),
               dict(fr, occ_view_gain=True, view_range=0.0), dict(fr, occ_view_gain=True, view_range=float("nan")), dict(fr, occ_view_gain=True, view_beams=0),
               dict(fr, occ_view_gain=True, view_azimuth=2.5), dict(fr, occ_view_gain=True, view_beams=2048, view_azimuth=1024),
               dict(fr, occ_view_gain=True, view_range=1.0e4)):                    # 2^20 rays at most; 1e4 m at 0.3 m a voxel is beyond the offset limit
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_parses_its_options(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(o in h.stdout for o in ("--occ-view-gain", "--view-range", "--view-beams", "--view-azimuth", "view_gain.csv"))
    d = str(tmp_path)
    for args, msg in ((["--occupancy-3d", "--occ-view-gain", "--save-dir", d], "--occ-view-gain needs --occupancy-3d and --occ-frontiers"),
                      (["--occupancy-3d", "--occ-frontiers", "--save-dir", d, "--view-range", "30"], "--view-range, --view-beams and --view-azimuth need --occ-view-gain"),
                      (["--occupancy-3d", "--occ-frontiers", "--save-dir", d, "--view-beams", "8"], "need --occ-view-gain"),
                      (["--occupancy-3d", "--occ-frontiers", "--occ-view-gain", "--save-dir", d, "--view-azimuth", "1.5"], "invalid int value")):
        r = subprocess.run(exe + ["--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(d)
    import inspect, replay
    p = inspect.signature(replay.run).parameters
    assert (p["occ_view_gain"].default, p["view_range"].default, p["view_beams"].default, p["view_azimuth"].default) == (False, 20.0, 16, 300)


def _read(path):
    rows = open(path).read().splitlines()
    assert rows[0] == HEAD
    return np.array([[float(v) for v in r.split()] for r in rows[1:]], np.float64).reshape(-1, 9)


def _run_and_check(tmp_path, backend, n_kf):
    Z = (0.3, 1.8)
    plain, out0 = _run(tmp_path, backend, n_kf, "plain", occ_frontiers=True)
    assert "view_gain" not in out0 and "view_gain.csv" not in os.listdir(plain)
    occ = _want(n_kf, out0["poses"])
    g = occ["grid"]
    goal = tuple(float(x) for x in np.asarray(out0["poses"][0])[:3, 3])
    off = mv.sensor_offsets(0.3, SENSOR["view_range"], SENSOR["view_beams"], SENSOR["view_azimuth"], -15.0, 15.0)
    layers = (mo.layer_of(Z[0], g), mo.layer_of(Z[1], g))
    files = {}
    # from the regions' root voxels; from where the route field enters them
    for name, kw, fp, rp in (("roots", dict(occ_frontiers=True), mf.FrontierParams(), None),
                             ("entries", dict(occ_frontiers=True, frontier_min_size=5, occ_slice=Z, occ_distance=True, occ_route=goal, route_min_d2=0),
                              mf.FrontierParams(min_size=5, iz_lo=layers[0], iz_hi=layers[1]), mr.RouteParams(min_d2=0))):
        d, out = _run(tmp_path, backend, n_kf, name, occ_view_gain=True, **SENSOR, **kw)
        fr = mf.frontier(occ["classes"], fp)
        info = fr["info"]
        assert len(info) >= 1
        root = info["root"].astype(np.int64)
        at = np.stack([root % g.width, (root // g.width) % g.height, root // (g.width * g.height)], axis=1)
        if rp is not None:
            cost = mr.field(occ["classes"], md.transform(occ["classes"], md.DistanceParams())["d2"], g, [goal], rp)["cost"]
            k, entry = mf.costs(fr["labels"], len(info), cost)
            assert (k < mr.BLOCKED).any()
            at = np.where((k < mr.BLOCKED)[:, None], entry, at)
        vps = mo.centres(at, g)
        want = mv.gain(occ["classes"], g, vps, off)
        print("%s backend, %s: %s" % (backend, name, want["stats"]))
        assert out["view_gain"] == dict(want["stats"]._asdict(), range=12.0, beams=8, azimuth=90)
        assert want["stats"].outside == 0 and want["stats"].total_gain > 0
        if name == "roots":                                              # what a run wrote without the option, it writes with it - frontiers.csv too
            assert sorted(os.listdir(d)) == sorted(os.listdir(plain) + ["view_gain.csv"])
            for f in os.listdir(plain):
                assert open(os.path.join(d, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        rows = _read(os.path.join(d, "view_gain.csv"))
        assert len(rows) == len(info) and rows[:, 0].tolist() == list(range(len(info)))
        assert np.allclose(rows[:, 1:4], vps, atol=1e-6)
        for j, f in enumerate(("gain", "blocked", "escaped", "spent", "reached")):
            assert rows[:, 4 + j].tolist() == want["info"][f].tolist(), f
        assert (rows[:, 5:9].sum(axis=1) == len(off)).all()
        files[name] = open(os.path.join(d, "view_gain.csv"), "rb").read()
    return files


def test_oracle_backend_writes_the_twins_gains(tmp_path):
    files = _run_and_check(tmp_path, "oracle", 5)
    assert all(len(f.splitlines()) >= 2 for f in files.values())


@pytest.mark.gpu
def test_gpu_backend_writes_the_oracles_bytes(tmp_path):
    gpu = _run_and_check(tmp_path / "gpu", "gpu", 5)
    oracle = {}
    goal = None
    for name, kw in (("roots", dict(occ_frontiers=True)), ("entries", dict(occ_frontiers=True, frontier_min_size=5, occ_slice=(0.3, 1.8), occ_distance=True, route_min_d2=0))):
        if name == "entries":
            kw["occ_route"] = goal
        d, out = _run(tmp_path / "oracle", "oracle", 5, name, occ_view_gain=True, **SENSOR, **kw)
        goal = tuple(float(x) for x in np.asarray(out["poses"][0])[:3, 3])
        oracle[name] = open(os.path.join(d, "view_gain.csv"), "rb").read()
    assert gpu == oracle
