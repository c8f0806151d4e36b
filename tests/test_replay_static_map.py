"""tools/replay.py --static-map / --moving-boxes: the option checks (no GPU needed), the moving boxes of the spinning sensor's scene, and under -m gpu the
replay that writes map.pcd and map_static.pcd, the second with fewer points where the boxes drove."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(static_map=True),                                                       # no save_dir, no leaf
               dict(static_map=True, save_dir=d),                                           # no leaf
               dict(static_map=True, save_map_leaf=0.3),                                    # no save_dir
               dict(static_map=True, save_dir=d, save_map_leaf=0.0),
               dict(static_map=True, save_dir=d, save_map_leaf=float("nan")),
               dict(static_map=True, save_dir=d, save_map_leaf=0.3, backend="oracle"),      # the oracle backend writes no map
               dict(static_map=True, save_dir=d, save_map_leaf=0.3, static_max_k=256),
               dict(static_map=True, save_dir=d, save_map_leaf=0.3, static_radius=-1.0),
               dict(moving_boxes=2),                                                        # the uniform sensor has no scene to put them in
               dict(moving_boxes=2, sensor="uniform"),
               dict(moving_boxes=-1, sensor="spinning"),
               dict(moving_boxes=1.5, sensor="spinning")):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, **kw)
    assert not os.listdir(d)


def test_the_boxes_stand_elsewhere_in_every_keyframe():
    import replay
    from qn_amd import synth
    assert len(replay.moving_box_prims(0, 3)) == 0
    a, b = replay.moving_box_prims(2, 0), replay.moving_box_prims(2, 1)
    assert a.dtype == synth.PRIM_DTYPE and len(a) == 2 and (a["kind"] == synth.PRIM_BOX).all()
    assert a["p"][:, 1].tolist() == [replay.moving_box_lane(0), replay.moving_box_lane(1)] == [6.0, 15.0]
    assert np.allclose(b["p"][:, 0] - a["p"][:, 0], 2.5) and (a["p"][:, 2:5] == replay.MOVING_BOX_SIZE).all()
    xs = np.array([replay.moving_box_prims(2, k)["p"][:, 0] for k in range(70)])
    assert xs.min() >= -35.0 and xs.max() < 35.0 and len(set(xs[:, 0].tolist())) == 28      # 2.5 m steps over 70 m: 28 places, then again


def test_without_the_options_the_spinning_run_is_the_one_it_was():
    import replay
    kw = dict(n_kf=6, seed=3, verbose=False, backend="oracle", sensor="spinning")
    a = replay.run(**kw)
    b = replay.run(static_map=False, moving_boxes=0, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(a["poses"], b["poses"])) and sorted(a) == sorted(b)
    c = replay.run(moving_boxes=2, **kw)                           # the boxes change the scans, not the trajectory's ground truth
    assert all(np.array_equal(p, q) for p, q in zip(a["gt"], c["gt"]))


def _pcd(path):
    lines = open(path).read().splitlines()
    i = lines.index("DATA ascii")
    return np.array([[float(v) for v in l.split()] for l in lines[i + 1:]], np.float32).reshape(-1, 4)


@pytest.mark.gpu
def test_replay_writes_both_maps_and_the_static_one_has_fewer_points_where_the_boxes_drove(tmp_path):
    import replay
    out = replay.run(n_kf=40, seed=7, verbose=False, sensor="spinning", moving_boxes=2, static_map=True, save_dir=str(tmp_path), save_map_leaf=0.3)
    m = _pcd(os.path.join(str(tmp_path), "map.pcd")); s = _pcd(os.path.join(str(tmp_path), "map_static.pcd"))
    assert len(m) == out["map_points"] and len(s) == out["static_map_points"] and out["static_removed"] > 0

    def lanes(p):                                                  # above the ground, inside the two lanes
        return int(sum(((np.abs(p[:, 1] - replay.moving_box_lane(j)) < 1.0) & (np.abs(p[:, 0]) < 37.0) & (p[:, 2] > 0.3) & (p[:, 2] < 1.6)).sum() for j in range(2)))
    print("map", len(m), "static map", len(s), "records removed", out["static_removed"], "in the lanes", lanes(m), lanes(s))
    assert len(s) < len(m) and lanes(s) < lanes(m)
