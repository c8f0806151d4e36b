"""qn_map::mapGround / occupancyGrid / keepClasses (shim/qn_map/map_ground.hpp): tests/shim_map_ground.cpp compiles against the stand-ins and, without a device,
checks the layouts, the defaults and the refusal of a null store; under -m gpu it gives the bytes the Python wrappers give."""
import os
import subprocess
import numpy as np
import pytest
from qn_amd import synth
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3)]


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    txt = subprocess.check_output([build_shim("shim_map_ground.cpp", tmp_path)], text=True)
    assert txt.count("refused") == 3 and all(s in txt for s in ("qn_kf_map_ground:", "qn_kf_map_ground_grid:", "qn_kf_map_keep_classes:"))
    assert "params 40 bytes, stats 80 bytes, grid 40 bytes" in txt


def _fnv(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


@pytest.mark.gpu
def test_cpp_helper_gives_the_python_result(tmp_path):
    from qn_amd import engine
    exe = build_shim("shim_map_ground.cpp", tmp_path)
    store = engine.KeyframeStore()
    try:
        prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
        ids = [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12])]
        with open(tmp_path / "kf.bin", "wb") as f:
            for i in ids:
                c = store.keyframe(i)
                f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
        np.ascontiguousarray(np.array(POSES, np.float64)).tofile(str(tmp_path / "poses.bin"))
        txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "0.5", "0.3", "0.2", "2.0"], text=True)
        n = store.build_map(ids, POSES, 0.3)
        st, cls, hq = store.map_ground(engine.GroundParams(0.5, 0.3, 0.2, 2.0, 1))
        info, gq, occ = store.map_ground_grid()
        hp = _fnv(cls[i].tobytes() + hq[i].tobytes() for i in range(n))
        hg = _fnv(a.tobytes() + b.tobytes() for a, b in zip(gq.ravel(), occ.ravel()))
        _, m = store.map_keep_classes(0b11101)
        kept = store.download_map(m)
        hm = _fnv(kept[i].tobytes() for i in range(m))
        assert txt.splitlines() == ["ground %d %d %d %d %016x" % (n, st["n_ground"], st["n_obstacle"], st["n_overhead"], hp),
                                    "grid %d %d %d %d %d %016x" % (info["width"], info["height"], st["occupied"], st["free"], st["unknown"], hg),
                                    "kept %d %016x" % (m, hm)], txt
        assert m == n - st["n_ground"] and st["n_ground"] > 0 and st["occupied"] > 0
    finally:
        store.close()
