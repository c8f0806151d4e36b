#!/usr/bin/env python
"""Time the outlier filter of the corrected global map on the scene of tools/gpu_map_normals_time.py (tools/gpu_map_time.py's: --keyframes x --points records
along a 400 m path, leaf 0.3): qn_kf_map_outliers (cell index, the k-nearest selection, the statistics, the flags; three host synchronisations) and
qn_kf_map_remove_outliers (compaction into the map slot) beside qn_kf_build_map of the same list, beside qn_kf_map_normals at the SAME radius on the same map -
the same traversal of the same index, so the natural yardstick - and, when scipy is importable, beside what the host pays for the same filter: the download of
the map plus scipy.spatial.cKDTree.query of the k nearest within the radius and numpy statistics (f64 distances: the host-side yardstick, not the twin).
A remove changes the slot, so every repetition is build, classify, remove, each under its own host clock; every call ends in a stream synchronise.  The median
(min, max) over --reps after --warmup rounds.  Prints one JSON line per size; needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from gpu_map_time import scene, timed


def host_filter(pts, radius, std_mul, k, workers):
    """cKDTree k-nearest within the radius + PCL's statistics -> (tree + query ms, statistics ms, removed points)"""
    from scipy.spatial import cKDTree
    p = pts[:, :3].astype(np.float64)
    t0 = time.perf_counter()
    d, _ = cKDTree(p).query(p, k + 1, distance_upper_bound=radius, workers=workers)         # the point itself comes first
    t1 = time.perf_counter()
    dense = np.isfinite(d[:, k])
    mean = d[dense, 1:].mean(axis=1)
    thr = mean.mean() + std_mul * mean.std(ddof=1) if len(mean) > 1 else np.inf
    removed = int((~dense).sum() + (mean > thr).sum())
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), removed


def stat(ts):
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="map sizes: keyframes of --points records each (500 x 60000 is gpu_map_time.py's map)")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--k", type=int, nargs="+", default=[8], help="one classify timing per k (8, 16 and 32 are the kernel's three list sizes)")
    ap.add_argument("--std-mul", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-points", type=int, default=3000000, help="skip the host yardstick above this many map points")
    ap.add_argument("--workers", type=int, default=16, help="threads of the host k-d tree query")
    a = ap.parse_args()
    from qn_amd import engine
    try:
        import scipy                                                 # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        views = np.array([T[:3, 3] for T in poses])
        res = dict(points=int(sum(len(x) for x in xyz)), keyframes=nkf, leaf=a.leaf, radius=a.radius, std_mul=a.std_mul)
        n = store.build_map(ids, poses, a.leaf)
        res["map_points"] = n
        nparams = engine.NormalParams(a.radius, 5)
        ptr = engine.C.c_void_p(); cnt = engine.C.c_uint32()
        vp = engine._p(views)
        res["map_normals_ms"] = timed(lambda: store._check(store._l.qn_kf_map_normals(store.h, engine.C.byref(nparams), vp, engine.C.c_uint32(len(views)),
                                                                                      engine.C.byref(ptr), engine.C.byref(cnt))), a.warmup, a.reps)
        st = engine.OutlierStats()
        for k in a.k:
            params = engine.OutlierParams(a.radius, a.std_mul, k)
            tb, tc, tr = [], [], []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter(); store.build_map(ids, poses, a.leaf)
                t1 = time.perf_counter(); store._check(store._l.qn_kf_map_outliers(store.h, engine.C.byref(params), engine.C.byref(st)))
                t2 = time.perf_counter(); store._check(store._l.qn_kf_map_remove_outliers(store.h, engine.C.byref(ptr), engine.C.byref(cnt)))
                t3 = time.perf_counter()
                if rep >= a.warmup:
                    tb.append(1e3 * (t1 - t0)); tc.append(1e3 * (t2 - t1)); tr.append(1e3 * (t3 - t2))
            res["build_map_ms"] = stat(tb)
            res["k%d" % k] = dict(map_outliers_ms=stat(tc), remove_ms=stat(tr), dense=int(st.dense), sparse=int(st.sparse), removed=int(st.removed), left=int(cnt.value),
                                  mean_m=st.mean_q * 2.0 ** -st.quant_exp, threshold_m=st.thr_q * 2.0 ** -st.quant_exp)
        if not have_scipy:
            res["host"] = "scipy is not importable: no host yardstick"
        elif n > a.host_max_points:
            res["host"] = "skipped above --host-max-points"
        else:
            store.build_map(ids, poses, a.leaf)
            t0 = time.perf_counter(); pts = store.download_map(n); res["download_map_ms"] = 1e3 * (time.perf_counter() - t0)
            res["host_kdtree_ms"], res["host_stats_ms"], res["host_removed"] = host_filter(pts, a.radius, a.std_mul, a.k[0], a.workers)
            res["host_note"] = "scipy cKDTree.query of the %d nearest within the radius (%d threads) + numpy statistics, f64, one run" % (a.k[0], a.workers)
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
