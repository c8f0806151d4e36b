"""tools/replay.py --occ-route: the option checks, the command line, the run on the oracle backend (no GPU: out["route"] carries the twin's statistics, route.csv
the path down the twin's field) and, under -m gpu, on the GPU backend, which writes the same file byte for byte.  Without the options a run writes what it
wrote."""
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import mapdistance as md, mapoccupancy as mo, maproute as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
Z = (0.3, 1.8)


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    occ = dict(occupancy_3d=True, save_dir=d)
    dist = dict(occ, occ_distance=True)
    G = (1.0, 2.0, 0.5)
    for kw in (dict(occ_route=G), dict(occ_route=G, save_dir=d), dict(occ, occ_route=G), dict(dist, route_from=G), dict(dist, route_planar=True), dict(dist, route_min_d2=0),
               dict(dist, occ_route=(1.0, 2.0)), dict(dist, occ_route=(1.0, 2.0, float("nan"))), dict(dist, occ_route=G, route_from=(0.0, float("inf"), 0.0)),
               dict(dist, occ_route=G, route_min_d2=-1), dict(dist, occ_route=G, route_min_d2=2.5), dict(dist, occ_route=G, route_min_d2=257),
               dict(dist, occ_dist_max=3, occ_route=G, route_min_d2=10)):
        for backend in ("oracle", "gpu"):
            with pytest.raises(ValueError):
                replay.run(n_kf=4, verbose=False, backend=backend, **kw)
    assert not os.listdir(d)


def test_the_command_line_parses_its_options(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(o in h.stdout for o in ("--occ-route GX GY GZ", "--route-from X Y Z", "--route-min-d2", "--route-planar"))
    d = str(tmp_path)
    for args, msg in ((["--occupancy-3d", "--save-dir", d, "--occ-route", "1", "2", "3"], "--occ-route needs --occupancy-3d and --occ-distance"),      # a missing --occ-distance
                      (["--occ-distance", "--save-dir", d, "--occ-route", "1", "2", "3"], "needs --occupancy-3d"),
                      (["--occupancy-3d", "--occ-distance", "--save-dir", d, "--route-planar"], "need --occ-route"),
                      (["--occupancy-3d", "--occ-distance", "--save-dir", d, "--route-from", "1", "2", "3"], "need --occ-route"),
                      (["--occupancy-3d", "--occ-distance", "--save-dir", d, "--occ-route", "1", "2"], "expected 3 arguments"),
                      (["--occupancy-3d", "--occ-distance", "--save-dir", d, "--occ-route", "1", "2", "3", "--route-min-d2", "1.5"], "invalid int value")):
        r = subprocess.run(exe + ["--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(d)
    import inspect, replay
    p = inspect.signature(replay.run).parameters
    assert (p["occ_route"].default, p["route_from"].default, p["route_min_d2"].default, p["route_planar"].default) == (None, None, 4, False)


def _run(tmp_path, backend, n_kf, name, **kw):
    import replay
    d = str(tmp_path / name); os.makedirs(d)
    out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, occ_slice=Z, occ_distance=True, **kw)
    return d, out


def _want(n_kf, poses):
    """the occupancy and distance twins' volume of the run's scans under its corrected poses"""
    import replay
    from qn_amd import synth
    prims, lidar, seeds, gt, odom, stamps = replay.make_lidar_stream(n_kf, 7, yaw_bias=0.006)
    scans = [synth.lidar_scan(prims, lidar, T, int(sd)) for T, sd in zip(gt, seeds)]
    occ = mo.classify(scans, poses)
    return occ, md.transform(occ["classes"], md.DistanceParams())["d2"]


def _read(path):
    rows = open(path).read().splitlines()
    assert rows[0] == "x y z cost"
    return np.array([[float(v) for v in r.split()] for r in rows[1:]], np.float64).reshape(-1, 4)


def _nearest(occ, d2, rp, xyz):
    """the centre of the passable cell nearest to the world point xyz: an input the run can use as a goal or a start"""
    g = occ["grid"]
    v = np.argwhere(mr.passable(occ["classes"], d2, rp))[:, ::-1]
    c = mr.centres(g, v, rp)
    k = 2 if rp.planar else 3
    return tuple(float(x) for x in c[np.argmin(((c[:, :k] - np.asarray(xyz)[:k]) ** 2).sum(axis=1))])


def _cases(occ, d2, poses, layers):
    """(name, the options, the twin's parameters, the start): the defaults between the passable voxels nearest the first and the last keyframe, the clearance
    off from a given start, and the plane of columns over the slice's layers"""
    first, last = np.asarray(poses[0])[:3, 3], np.asarray(poses[-1])[:3, 3]
    out = []
    rp = mr.RouteParams()
    goal, start = _nearest(occ, d2, rp, first), _nearest(occ, d2, rp, last)
    out.append(("default", dict(occ_route=goal, route_from=start), rp, start))
    rp = mr.RouteParams(min_d2=0)
    out.append(("wide", dict(occ_route=tuple(float(x) for x in first), route_min_d2=0), rp, last))      # the start defaults to the last keyframe's position
    rp = mr.RouteParams(2, 1, layers[0], layers[1], 1)
    goal, start = _nearest(occ, d2, rp, first), _nearest(occ, d2, rp, last)
    out.append(("planar", dict(occ_route=goal, route_from=start, route_planar=True, route_min_d2=1), rp, start))
    return out


def _run_and_check(tmp_path, backend, n_kf):
    plain, out0 = _run(tmp_path, backend, n_kf, "plain")
    assert "route" not in out0 and "route.csv" not in os.listdir(plain)
    occ, d2 = _want(n_kf, out0["poses"])
    g = occ["grid"]
    layers = (mo.layer_of(Z[0], g), mo.layer_of(Z[1], g))
    files = {}
    for name, kw, rp, start in _cases(occ, d2, out0["poses"], layers):
        goal = kw["occ_route"]
        d, out = _run(tmp_path, backend, n_kf, name, **kw)
        want = mr.field(occ["classes"], d2, g, [goal], rp)
        at = int(mr.query(want["cost"], g, [start], rp)[0])
        lens, ijk = mr.paths(want["cost"], g, [start], at // 3 + 1 if at < mr.BLOCKED else 1, rp)
        n = int(lens[0])
        print("%s backend, %s: %s, path of %d voxels, cost %d" % (backend, name, want["stats"], n, at))
        assert out["route"] == dict(want["stats"]._asdict(), **rp._asdict(), path_len=n, path_cost=at if at < mr.BLOCKED else None)
        assert out["occupancy"] == out0["occupancy"] and out["distance"] == out0["distance"]
        assert sorted(os.listdir(d)) == sorted(os.listdir(plain) + ["route.csv"])
        for f in os.listdir(plain):                                  # what a run wrote without the option, it writes with it
            assert open(os.path.join(d, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        rows = _read(os.path.join(d, "route.csv"))
        assert len(rows) == n
        if n:                                                        # the rows are a valid path: the start's voxel first, a goal last, every step an allowed move
            v = ijk[0, :n]
            assert np.allclose(rows[:, :3], mr.centres(g, v, rp), atol=1e-6) and rows[:, 3].tolist() == want["cost"][v[:, 2], v[:, 1], v[:, 0]].tolist()
            assert rows[0, 3] == at and rows[-1, 3] == 0 and (np.diff(rows[:, 3]) < 0).all()
            for a, b in zip(v[:-1], v[1:]):
                o = tuple(int(x) for x in b - a)
                assert mr.allowed(want["cost"], tuple(int(x) for x in a), o) and int(want["cost"][a[2], a[1], a[0]]) - int(want["cost"][b[2], b[1], b[0]]) == mr.weight(o)
        files[name] = open(os.path.join(d, "route.csv"), "rb").read()
    assert out0["occupancy"]["slice_layers"] == list(layers)
    return files


def test_oracle_backend_writes_the_twins_path(tmp_path):
    files = _run_and_check(tmp_path, "oracle", 5)
    assert len(files["default"].splitlines()) > 3 and len(files["wide"].splitlines()) > 3      # both 3-D runs have a path; a start that is cut off writes the header alone


@pytest.mark.gpu
def test_gpu_backend_writes_the_oracles_bytes(tmp_path):
    gpu = _run_and_check(tmp_path / "gpu", "gpu", 5)
    _, probe = _run(tmp_path / "oracle", "oracle", 5, "probe")
    occ, d2 = _want(5, probe["poses"])
    oracle = {}
    for name, kw, _, _ in _cases(occ, d2, probe["poses"], (mo.layer_of(Z[0], occ["grid"]), mo.layer_of(Z[1], occ["grid"]))):
        d, _ = _run(tmp_path / "oracle", "oracle", 5, name, **kw)
        oracle[name] = open(os.path.join(d, "route.csv"), "rb").read()
    assert gpu == oracle
