#!/usr/bin/env python
"""Time the ground stage of the corrected global map on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, leaf 0.3):
qn_kf_map_ground (extent, quantise and bin, the tiled envelope relaxation, classify, counts; 2 + ceil(rounds / 8) host synchronisations), the grid download
(qn_kf_map_ground_grid) and qn_kf_map_keep_classes without the ground, beside qn_kf_build_map of the same list - the build that fed it - and beside what the
host pays for the same result: the download of the map plus a numpy column minimum (np.minimum.at) and the twin's sweeps to the envelope's fixed point
(qn_amd/mapground.py: the specification, so the host result is the GPU's).  A keep changes the slot, so every repetition is build, classify, grid, keep, each
under its own host clock; every call ends in a stream synchronise.  The median (min, max) over --reps after --warmup rounds.  Prints rounds, grid size and
points in one JSON line per size; needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from gpu_map_time import scene


def stat(ts):
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="map sizes: keyframes of --points records each (500 x 60000 is gpu_map_time.py's map)")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--cell", type=float, default=0.5)
    ap.add_argument("--max-slope", type=float, default=0.3)
    ap.add_argument("--ground-tol", type=float, default=0.2)
    ap.add_argument("--clearance", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-cells", type=int, default=4000000, help="skip the host yardstick above this many grid columns")
    a = ap.parse_args()
    from qn_amd import engine, mapground
    C = engine.C
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        res = dict(points=int(sum(len(x) for x in xyz)), keyframes=nkf, leaf=a.leaf, cell=a.cell, max_slope=a.max_slope, ground_tol=a.ground_tol, clearance=a.clearance)
        params = engine.GroundParams(a.cell, a.max_slope, a.ground_tol, a.clearance, 1)
        st = engine.GroundStats(); ptr = C.c_void_p(); cnt = C.c_uint32()
        tb, tc, tg, tk = [], [], [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); n = store.build_map(ids, poses, a.leaf)
            t1 = time.perf_counter(); store._check(store._l.qn_kf_map_ground(store.h, C.byref(params), C.byref(st)))
            t2 = time.perf_counter(); store.map_ground_grid()
            t3 = time.perf_counter(); store._check(store._l.qn_kf_map_keep_classes(store.h, C.c_uint32(0b11101), C.byref(ptr), C.byref(cnt)))
            t4 = time.perf_counter()
            if rep >= a.warmup:
                tb.append(1e3 * (t1 - t0)); tc.append(1e3 * (t2 - t1)); tg.append(1e3 * (t3 - t2)); tk.append(1e3 * (t4 - t3))
        res.update(map_points=n, grid=[int(st.width), int(st.height)], columns=int(st.width) * int(st.height), seeded=int(st.seeded), rounds=int(st.rounds),
                   classes=[int(getattr(st, f)) for f in ("n_none", "n_ground", "n_obstacle", "n_overhead", "n_below")], occupied=int(st.occupied),
                   left_without_ground=int(cnt.value), build_map_ms=stat(tb), map_ground_ms=stat(tc), grid_download_ms=stat(tg), keep_classes_ms=stat(tk))
        if int(st.width) * int(st.height) > a.host_max_cells:
            res["host"] = "skipped above --host-max-cells"
        else:
            store.build_map(ids, poses, a.leaf)
            t0 = time.perf_counter(); pts = store.download_map(n); res["download_map_ms"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter(); want = mapground.classify(pts, params.twin()); res["host_twin_ms"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter(); mapground.envelope(want["seed"], int(st.step_s), int(st.step_d)); res["host_sweeps_ms"] = 1e3 * (time.perf_counter() - t0)
            got = store.map_ground(params)
            res["equals_twin"] = bool(np.array_equal(got[1], want["classes"]) and np.array_equal(store.map_ground_grid()[2], want["occupancy"]))
            res["host_note"] = "numpy: np.minimum.at column minimum + the twin's eight-direction sweeps to the fixed point, one thread, one run"
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
