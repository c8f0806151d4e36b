#!/usr/bin/env python
"""Time the occupancy map's distance field on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, voxel 0.3):
qn_kf_map_distance (three passes over the resident class bytes, the statistics; one host synchronisation) for both site masks - the occupied voxels, and the
occupied or unknown ones - at each --max-dist, beside qn_kf_map_occupancy on the same store, and beside what a user without it would do: the download of the
class bytes (qn_kf_map_occupancy_grid, classes only) plus scipy.ndimage.distance_transform_edt on the host (exact and uncapped; skipped when scipy is
missing).  Each call under its own host clock; every call ends in a stream synchronise.  The median (min, max) over --reps after --warmup rounds.  Every field
is compared with the numpy twin's (qn_amd/mapdistance.py: the specification) up to --twin-max-voxels.  One JSON line per size.  Needs a GPU (no fall-back)."""
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
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="list sizes: keyframes of --points records each (500 x 60000 is gpu_map_time.py's map)")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--max-dist", type=int, nargs="+", default=[16, 64], help="the field's reach in voxels")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-max-voxels", type=int, default=30000000, help="skip the comparison with the numpy twin above this many voxels")
    a = ap.parse_args()
    from qn_amd import engine, mapdistance
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    C = engine.C
    occupied = 1 << engine.QN_OCC_OCCUPIED
    masks = (("occupied", occupied), ("occupied_or_unknown", occupied | (1 << engine.QN_OCC_UNKNOWN)))
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = np.array([store.add(x, i) for x, i in zip(xyz, inten)], np.int32)
        P = np.ascontiguousarray(poses, np.float64).reshape(nkf, 16)
        oparams = engine.OccupancyParams(voxel=a.voxel)
        ost = engine.OccupancyStats(); dst = engine.DistanceStats()
        to = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); store._check(store._l.qn_kf_map_occupancy(store.h, engine._p(ids), engine._p(P), C.c_uint32(nkf), C.byref(oparams), C.byref(ost)))
            if rep >= a.warmup:
                to.append(1e3 * (time.perf_counter() - t0))
        W, H, D = int(ost.width), int(ost.height), int(ost.depth)
        n = W * H * D
        res = dict(records=int(sum(len(x) for x in xyz)), keyframes=nkf, voxel=a.voxel, grid=[W, H, D], voxels=n,
                   classes=[int(ost.occupied), int(ost.free), int(ost.unknown)], map_occupancy_ms=stat(to), field_bytes=2 * n)
        cls = np.zeros(max(n, 1), np.uint8); g = engine.OccupancyGrid()
        td = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); store._check(store._l.qn_kf_map_occupancy_grid(store.h, C.byref(g), None, None, engine._p(cls)))
            if rep >= a.warmup:
                td.append(1e3 * (time.perf_counter() - t0))
        res["class_download_ms"] = stat(td)
        cls = cls[:n].reshape(D, H, W)
        equal = True
        for name, mask in masks:
            for r in a.max_dist:
                p = engine.DistanceParams(mask, r)
                ts = []
                for rep in range(a.warmup + a.reps):
                    t0 = time.perf_counter(); store._check(store._l.qn_kf_map_distance(store.h, C.byref(p), C.byref(dst)))
                    if rep >= a.warmup:
                        ts.append(1e3 * (time.perf_counter() - t0))
                key = "%s_r%d" % (name, r)
                res[key + "_ms"] = stat(ts)
                res[key + "_voxels_per_s"] = n / (1e-3 * float(np.median(ts))) if n else 0.0
                res[key + "_stats"] = [int(dst.sites), int(dst.reached), int(dst.far), int(dst.max_d2), int(dst.sum_d2)]
                if n <= a.twin_max_voxels:
                    want = mapdistance.transform(cls, (mask, r))
                    equal = equal and bool(np.array_equal(store.map_distance_grid()[2], want["d2"]) and tuple(res[key + "_stats"]) == tuple(want["stats"]))
            if ndimage is not None and n:
                site = mapdistance.sites_of(cls, mask)
                if site.any() and not site.all():
                    t0 = time.perf_counter(); ndimage.distance_transform_edt(~site); res["host_edt_%s_ms" % name] = 1e3 * (time.perf_counter() - t0)
        res["equals_twin"] = equal if n <= a.twin_max_voxels else "skipped above --twin-max-voxels"
        res["host_note"] = "scipy.ndimage.distance_transform_edt of the downloaded classes, f64, uncapped, one thread, one run" if ndimage is not None else "scipy is not installed"
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
