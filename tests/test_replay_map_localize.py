"""tools/replay.py --localize-every: the option checks (no GPU needed), and under -m gpu a short spinning-LiDAR replay in which every fourth keyframe is
localised in the corrected map from its displaced corrected pose: out["localized"] has one entry per chosen keyframe, at least one is valid, and
localized_tum.txt has one row per entry.  The crop radius is beyond the sensor's reach, so a scan's far points have partners in the crop (with a smaller radius
the score counts them as misses).  In the GICP form, which starts from the guess - 0.5 m / 3 degrees from the pose the map was built with, the displacement the
CPU oracle converges from on the street scene (tests/test_gpu_map_localize.py) - every valid entry must also end nearer to that pose than it started.  The
coarse-to-fine form matches features against the whole neighbourhood and ignores the guess's heading: on this repetitive street it can accept a pose elsewhere
(keyframe 4 lands 56 m away with score 1.41 under the threshold 1.5), so no such claim is made of it."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_options_are_checked_before_anything_runs(tmp_path):
    import replay
    d = str(tmp_path)
    for kw in (dict(localize_every=2),                                                      # no save_dir
               dict(localize_every=2, save_dir=d, backend="oracle"),                        # the map is the store's
               dict(localize_every=-1, save_dir=d), dict(localize_every=1.5, save_dir=d),
               dict(localize_every=2, save_dir=d, localize_radius=0.0), dict(localize_every=2, save_dir=d, localize_radius=float("nan")),
               dict(localize_every=2, save_dir=d, localize_shift=float("inf")), dict(localize_every=2, save_dir=d, localize_yaw=float("nan"))):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, **kw)
    assert not os.listdir(d)


def _rows(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "#timestamp x y z qx qy qz qw"
    return np.array([[float(v) for v in l.split()] for l in lines[1:]], np.float64).reshape(-1, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("quatro", [False, True])
def test_every_fourth_keyframe_is_localised_in_the_map(tmp_path, quatro):
    import replay
    d = str(tmp_path)
    out = replay.run(n_kf=12, seed=7, verbose=False, sensor="spinning", save_dir=d, use_quatro=quatro, localize_every=4, localize_radius=150.0)
    loc = out["localized"]
    assert [r["id"] for r in loc] == [0, 4, 8] and out["localize_stats"]["n_pairs"] == 3 and out["localize_stats"]["n_crops"] == 3
    for r in loc:
        print("keyframe %d: valid %s, score %.4f, guess %.3f m / %.2f deg -> %.4f m / %.3f deg" %
              (r["id"], r["valid"], r["score"], r["guess_t_err"], np.degrees(r["guess_r_err"]), r["t_err"], np.degrees(r["r_err"])))
        assert abs(r["guess_t_err"] - 0.5) < 1e-9 and abs(np.degrees(r["guess_r_err"]) - 3.0) < 1e-6 and r["status"] == 0
        if r["valid"] and not quatro:
            assert r["t_err"] < r["guess_t_err"] and r["r_err"] < r["guess_r_err"]
    assert any(r["valid"] for r in loc)
    rows = _rows(os.path.join(d, "localized_tum.txt"))
    assert len(rows) == len(loc)
    for row, r in zip(rows, loc):
        assert np.allclose(row[1:4], r["T"][:3, 3], atol=1e-8) and abs(np.linalg.norm(row[4:]) - 1.0) < 1e-6
