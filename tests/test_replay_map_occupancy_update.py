"""tools/replay.py --occupancy-3d --occ-incremental: the option checks (no GPU) and, under -m gpu, the run on the GPU backend - the volume kept live through
the run by KeyframeStore.map_occupancy_update writes the files of the one-shot run byte for byte and reports the same out["occupancy"], with fewer entries
walked than listed."""
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FILES = ["occupancy_slice.pgm", "occupancy_slice.yaml", "occupied.pcd", "poses_kitti.txt", "poses_tum.txt"]


def test_the_option_needs_the_volume(tmp_path):
    import inspect, replay
    assert "occ_incremental" in inspect.signature(replay.run).parameters
    for backend in ("oracle", "gpu"):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, backend=backend, save_dir=str(tmp_path), occ_incremental=True)
    exe = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    h = subprocess.run(exe + ["--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--occ-incremental" in h.stdout
    r = subprocess.run(exe + ["--keyframes", "4", "--occ-incremental", "--save-dir", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "--occ-incremental needs --occupancy-3d" in r.stderr
    assert not os.listdir(str(tmp_path))


def run_both(tmp_path, backend, n_kf, **kw):
    """-> (the directory and out of the one-shot run, those of the incremental run); the files are compared here"""
    import replay
    runs = []
    for name, inc in (("once", False), ("live", True)):
        d = str(tmp_path / name); os.makedirs(d)
        out = replay.run(n_kf=n_kf, seed=7, sensor="spinning", backend=backend, verbose=False, save_dir=d, occupancy_3d=True, occ_slice=(0.3, 1.8), occ_incremental=inc, **kw)
        runs.append((d, out))
    (d0, once), (d1, live) = runs
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1)) == FILES
    for f in FILES:
        assert open(os.path.join(d0, f), "rb").read() == open(os.path.join(d1, f), "rb").read(), f
    extra = ("updates", "entries_listed", "entries_walked")
    assert {k: v for k, v in live["occupancy"].items() if k not in extra} == once["occupancy"] and not any(k in once["occupancy"] for k in extra)
    return once, live


@pytest.mark.gpu
def test_gpu_backend_writes_the_files_of_the_one_shot_run(tmp_path):
    n = 8
    once, live = run_both(tmp_path, "gpu", n)
    o = live["occupancy"]
    print("gpu backend: %d updates, %d entries listed, %d walked; occupied %d free %d unknown %d" % (o["updates"], o["entries_listed"], o["entries_walked"], o["occupied"],
                                                                                                  o["free"], o["unknown"]))
    assert o["updates"] == n and o["entries_listed"] == n * (n + 1) // 2 and n <= o["entries_walked"] < o["entries_listed"] and o["occupied"] > 1000
