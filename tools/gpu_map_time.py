#!/usr/bin/env python
"""Time the corrected global map at map scale (about 3e7 points: 500 keyframes x 60k points along a 400 m path, leaf 0.3 =
save_voxel_resolution): qn_kf_build_map next to qn_kf_assemble on the same ids (xyz only), the map download, and the CPU oracle's
voxel grid on the same points (the oracle, not PCL).  Both GPU calls end in a stream synchronise, so a host clock around each call
is its time on the device plus the launch and read-back gaps; the median over --reps after --warmup calls is reported.
Prints one JSON line; needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))
import numpy as np


def scene(nkf, npts, seed=9):
    rng = np.random.default_rng(seed)
    xyz = [np.c_[rng.uniform(-30, 30, (npts, 2)), rng.uniform(-1.5, 3.5, npts)].astype(np.float32) for _ in range(nkf)]
    inten = [rng.uniform(0, 255, npts).astype(np.float32) for _ in range(nkf)]
    poses = []
    for k in range(nkf):
        a = 0.3 * np.sin(k / 60.0); T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; T[:3, 3] = [0.8 * k, 15.0 * np.sin(k / 50.0), 0.002 * k]
        poses.append(T)
    return xyz, inten, poses


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=500)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--oracle", action="store_true", help="also time the CPU oracle's voxel grid on the same points")
    a = ap.parse_args()
    from qn_amd import engine
    xyz, inten, poses = scene(a.keyframes, a.points)
    store = engine.KeyframeStore()
    ids = [store.add(x, i) for x, i in zip(xyz, inten)]
    res = dict(points=int(sum(len(x) for x in xyz)), keyframes=a.keyframes, leaf=a.leaf)
    box = {}
    box["n"] = store.build_map(ids, poses, a.leaf)
    res["map_points"] = box["n"]
    res["build_map_ms"] = timed(lambda: store.build_map(ids, poses, a.leaf), a.warmup, a.reps)
    res["assemble_ms"] = timed(lambda: store.assemble(ids, poses, a.leaf, 0), a.warmup, a.reps)
    store.build_map(ids, poses, a.leaf)
    res["download_map_ms"] = timed(lambda: store.download_map(box["n"]), a.warmup, a.reps)
    store.close()
    if a.oracle:
        from oracle import oracle as orc
        cat = np.concatenate([orc.transform_pcd(x, T) for x, T in zip(xyz, poses)])
        t0 = time.perf_counter(); m = orc.voxel_grid(cat, a.leaf); res["oracle_cpu_voxel_grid_ms"] = 1e3 * (time.perf_counter() - t0)
        res["oracle_map_points"] = int(len(m))
        res["oracle_note"] = "the single-threaded C++ oracle (not PCL), voxel grid only, xyz only, one run on the host CPU"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
