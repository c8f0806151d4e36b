"""tools/replay.py --map-outliers: the option checks (no GPU needed), and under -m gpu the short spinning-LiDAR replay of tests/test_replay_map_normals.py with
the filter on: the saved map.pcd is, byte for byte, the twin's filtered map (qn_amd/mapoutliers.remove of the unfiltered map, which the test rebuilds from the
same ray-cast keyframes and the run's corrected poses), and with --save-map-normals the normals in it are those of the FILTERED map."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARAMS = (1.0, 2.0, 8)                                                # radius, std_mul, k: the defaults
NORMALS = (0.9, 5)                                                    # the radius test_replay_map_normals.py argues for


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(map_outliers=True),                                                      # no save_dir, no leaf
               dict(map_outliers=True, save_dir=d),                                          # --map-outliers without --save-map-leaf
               dict(map_outliers=True, save_map_leaf=0.3),                                   # no save_dir
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, backend="oracle"),      # the oracle backend writes no map
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_radius=0.0),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_radius=float("nan")),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_std=-1.0),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_std=float("inf")),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_k=0),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_k=33),
               dict(map_outliers=True, save_dir=d, save_map_leaf=0.3, outlier_k=7.5)):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, **kw)
    assert not os.listdir(d)


def test_the_command_line_refuses_the_filter_without_a_map(tmp_path):
    for args in (["--map-outliers"], ["--map-outliers", "--save-dir", str(tmp_path)], ["--map-outliers", "--save-map-leaf", "0.3", "--outlier-k", "4"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "--map-outliers needs --save-dir and --save-map-leaf" in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(str(tmp_path))


def _read_pcd(path):
    lines = open(path).read().splitlines()
    fields = [l for l in lines if l.startswith("FIELDS")][0].split()[1:]
    return fields, np.array([[float(v) for v in l.split()] for l in lines[lines.index("DATA ascii") + 1:]], np.float64).astype(np.float32)


@pytest.fixture(scope="module")
def run_and_unfiltered(tmp_path_factory):
    """one replay with the filter and the normals on, and the unfiltered map of the same keyframes under its corrected poses"""
    import replay
    from qn_amd import engine
    d = str(tmp_path_factory.mktemp("filtered"))
    out = replay.run(n_kf=12, seed=7, verbose=False, sensor="spinning", save_dir=d, save_map_leaf=0.3, map_outliers=True, outlier_radius=PARAMS[0],
                     outlier_std=PARAMS[1], outlier_k=PARAMS[2], save_map_normals=True, normal_radius=NORMALS[0])
    prims, lidar, seeds, gt, _, _ = replay.make_lidar_stream(12, 7, yaw_bias=0.006)
    store = engine.KeyframeStore()
    try:
        ids = [int(i) for i in store.add_lidar_scans(prims, lidar, gt, seeds)]
        full = store.download_map(store.build_map(ids, out["poses"], 0.3))
    finally:
        store.close()
    return out, d, full


@pytest.mark.gpu
def test_the_saved_map_is_the_twins_filtered_map(run_and_unfiltered):
    from qn_amd import mapoutliers as mo
    out, d, full = run_and_unfiltered
    fields, m = _read_pcd(os.path.join(d, "map.pcd"))
    want = mo.remove(full, PARAMS)
    removed = len(full) - len(want)
    print("map.pcd: %d of %d points kept, %d removed" % (len(m), len(full), removed))
    assert fields[:4] == ["x", "y", "z", "intensity"] and len(full) > 1000 and 0 < removed < len(full)
    assert out["map_points"] == len(want) and out["map_outliers_removed"] == removed
    assert len(m) == len(want) and np.array_equal(np.ascontiguousarray(m[:, :4]).view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_the_saved_normals_are_those_of_the_filtered_map(run_and_unfiltered):
    """filter first, normals second: map.pcd holds what map_normals gives on the filtered map (which equals the twin's on such a map:
    tests/test_gpu_map_outliers.py), not the unfiltered map's normals with rows dropped"""
    from qn_amd import engine, mapoutliers as mo
    import replay
    out, d, full = run_and_unfiltered
    fields, m = _read_pcd(os.path.join(d, "map.pcd"))
    assert fields == ["x", "y", "z", "intensity", "normal_x", "normal_y", "normal_z", "curvature"]
    cls = mo.classify(full, PARAMS)
    kept = full[cls["removed"] == 0]
    assert m.shape == (len(kept), 8) and np.array_equal(np.ascontiguousarray(m[:, :4]).view(np.uint32), kept.view(np.uint32))
    views = np.array([T[:3, 3] for T in out["poses"]])
    prims, lidar, seeds, gt, _, _ = replay.make_lidar_stream(12, 7, yaw_bias=0.006)
    store = engine.KeyframeStore()
    try:
        ids = [int(i) for i in store.add_lidar_scans(prims, lidar, gt, seeds)]
        store.build_map(ids, out["poses"], 0.3)
        unfiltered = store.map_normals(engine.NormalParams(*NORMALS), views)
        store.map_outliers(engine.OutlierParams(*PARAMS))
        assert store.map_remove_outliers()[1] == len(kept)
        want = store.map_normals(engine.NormalParams(*NORMALS), views)
    finally:
        store.close()
    assert np.array_equal(np.ascontiguousarray(m[:, 4:7]).view(np.uint32), want["normals"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(m[:, 7]).view(np.uint32), want["curvature"].view(np.uint32))
    assert out["map_normals_valid"] == int(np.isfinite(want["curvature"]).sum()) and out["map_points"] == len(kept)
    assert (unfiltered["count"][cls["removed"] == 0] != want["count"]).any()          # a kept point that lost a neighbour to the filter
