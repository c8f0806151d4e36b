"""tools/replay.py --map-clusters: the option checks (no GPU needed), and under -m gpu the short spinning-LiDAR replay of tests/test_replay_map_outliers.py with
the clustering on: map.pcd gains an integer label field that is, value for value, the twin's label of the written map (qn_amd/mapclusters.classify of the
points map.pcd itself holds), and clusters.csv lists the twin's clusters of that map - id, size, box and centroid."""
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARAMS = (0.5, 10, 0xffffffff, 0)                                     # tolerance, min_size, max_size, class_mask: the defaults


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(map_clusters=True),                                                      # no save_dir, no leaf
               dict(map_clusters=True, save_dir=d),                                          # --map-clusters without --save-map-leaf
               dict(map_clusters=True, save_map_leaf=0.3),                                   # no save_dir
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, backend="oracle"),      # the oracle backend writes no map of its own
               dict(drop_small_clusters=True, save_dir=d, save_map_leaf=0.3),                # nothing to drop without the clustering
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_tol=0.0),
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_tol=float("nan")),
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_min=0),
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_min=7.5),
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_min=20, cluster_max=19),
               dict(map_clusters=True, save_dir=d, save_map_leaf=0.3, cluster_max=2 ** 32)):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, **kw)
    assert not os.listdir(d)


def test_the_command_line_refuses_the_clustering_without_a_map(tmp_path):
    for args in (["--map-clusters"], ["--map-clusters", "--save-dir", str(tmp_path)], ["--map-clusters", "--save-map-leaf", "0.3", "--cluster-min", "4"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--keyframes", "4"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "--map-clusters needs --save-dir and --save-map-leaf" in r.stderr, (args, r.stderr[-300:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), "--keyframes", "4", "--drop-small-clusters"], capture_output=True, text=True)
    assert r.returncode == 2 and "--drop-small-clusters needs --map-clusters" in r.stderr
    assert not os.listdir(str(tmp_path))


def test_the_writers_round_trip(tmp_path):
    import replay
    pts = np.array([[1.5, -2.25, 0.1, 7.0], [np.float32(0.3), 4.0, -0.0, 0.5]], np.float32)
    replay.write_pcd_labelled(str(tmp_path / "a.pcd"), pts, np.array([3, -2], np.int32))
    fields, types, m = _read_pcd(str(tmp_path / "a.pcd"))
    assert fields == ["x", "y", "z", "intensity", "label"] and types == ["F", "F", "F", "F", "I"]
    assert np.array_equal(m[:, :4].astype(np.float32), pts) and list(m[:, 4]) == [3, -2]
    cl = dict(size=np.array([12, 3], np.uint32), lo=np.array([[0.1, 0.2, 0.3], [1, 2, 3]], np.float32), hi=np.array([[0.4, 0.5, 0.6], [4, 5, 6]], np.float32),
              centroid=np.array([[0.1, 1 / 3, 0.5], [2.5, 3.5, 4.5]]))
    replay.write_clusters_csv(str(tmp_path / "c.csv"), cl)
    rows = _read_csv(str(tmp_path / "c.csv"))
    assert np.array_equal(rows[:, 0], [0, 1]) and np.array_equal(rows[:, 1], [12, 3]) and np.array_equal(rows[:, 2:5].astype(np.float32), cl["lo"])
    assert np.array_equal(rows[:, 5:8].astype(np.float32), cl["hi"]) and np.array_equal(rows[:, 8:11], cl["centroid"])


def _read_pcd(path):
    lines = open(path).read().splitlines()
    fields = [l for l in lines if l.startswith("FIELDS")][0].split()[1:]
    types = [l for l in lines if l.startswith("TYPE")][0].split()[1:]
    return fields, types, np.array([[float(v) for v in l.split()] for l in lines[lines.index("DATA ascii") + 1:]], np.float64)


def _read_csv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "id,size,min_x,min_y,min_z,max_x,max_y,max_z,centroid_x,centroid_y,centroid_z"
    return np.array([[float(v) for v in l.split(",")] for l in lines[1:]], np.float64).reshape(-1, 11)


@pytest.mark.gpu
def test_the_saved_labels_and_clusters_are_the_twins(tmp_path):
    import replay
    from qn_amd import mapclusters as mc
    d = str(tmp_path)
    out = replay.run(n_kf=12, seed=7, verbose=False, sensor="spinning", save_dir=d, save_map_leaf=0.3, map_clusters=True, cluster_tol=PARAMS[0],
                     cluster_min=PARAMS[1], cluster_max=PARAMS[2])
    fields, types, m = _read_pcd(os.path.join(d, "map.pcd"))
    assert fields == ["x", "y", "z", "intensity", "label"] and types[-1] == "I" and len(m) == out["map_points"] > 1000
    want = mc.classify(m[:, :4].astype(np.float32), PARAMS)
    s = want["stats"]
    print("map.pcd: %d points, %d clusters of %d components, %d points in rejected clumps" % (len(m), s.clusters, s.components, s.rejected_points))
    assert np.array_equal(m[:, 4].astype(np.int32), want["label"]) and s.clusters >= 1 and s.rejected_points > 0
    assert out["clusters"] == dict(clusters=s.clusters, components=s.components, too_small=s.too_small, too_large=s.too_large, clustered_points=s.clustered_points,
                                   rejected_points=s.rejected_points)
    rows = _read_csv(os.path.join(d, "clusters.csv"))
    c = want["clusters"]
    assert len(rows) == s.clusters and np.array_equal(rows[:, 0], np.arange(s.clusters)) and np.array_equal(rows[:, 1], c["size"])
    assert np.array_equal(rows[:, 2:5].astype(np.float32), c["lo"]) and np.array_equal(rows[:, 5:8].astype(np.float32), c["hi"])
    assert np.array_equal(rows[:, 8:11], want["centroid"])
