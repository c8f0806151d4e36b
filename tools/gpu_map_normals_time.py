#!/usr/bin/env python
"""Time the normals of the corrected global map at the map sizes tools/gpu_map_time.py uses (its scene: --keyframes x --points records along a 400 m path,
leaf 0.3): qn_kf_map_normals (cell index, one pass, two host synchronisations; the viewpoints are the keyframe positions) beside qn_kf_build_map of the same
list, the download of normals, counts and viewpoint indices, and - when scipy is importable - what the host pays for the same answer on the downloaded map:
scipy.spatial.cKDTree.query_ball_point at the radius plus a numpy covariance and eigh per point (f64 distances: the host-side yardstick, not the twin).
A host clock around each call, which ends in a stream synchronise; the median (min, max) over --reps after --warmup calls.  Prints one JSON line per size;
needs a GPU (no fall-back)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from gpu_map_time import scene, timed


def host_normals(pts, radius, min_neighbors, views, workers):
    """cKDTree + numpy PCA -> (tree + query ms, PCA ms, valid points)"""
    from scipy.spatial import cKDTree
    p = pts[:, :3].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(p)
    nb = tree.query_ball_point(p, radius, workers=workers)
    t1 = time.perf_counter()
    lens = np.fromiter((len(x) for x in nb), np.int64, len(nb))
    flat = np.concatenate([np.asarray(x, np.int64) for x in nb]) if len(nb) else np.zeros(0, np.int64)
    own = np.repeat(np.arange(len(p)), lens)
    d = p[flat] - p[own]
    k = lens.astype(np.float64)
    m = np.stack([np.bincount(own, d[:, a], len(p)) for a in range(3)], axis=1) / k[:, None]
    C = np.zeros((len(p), 3, 3))
    for i in range(3):
        for j in range(i, 3):
            C[:, i, j] = C[:, j, i] = np.bincount(own, d[:, i] * d[:, j], len(p)) / k - m[:, i] * m[:, j]
    ok = lens >= min_neighbors
    w, U = np.linalg.eigh(C[ok])
    n = U[:, :, 0]
    v = views[cKDTree(views).query(p[ok])[1]] - p[ok]
    n[(n * v).sum(axis=1) < 0] *= -1.0
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="map sizes: keyframes of --points records each (500 x 60000 is gpu_map_time.py's map)")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--radius", type=float, default=0.6)
    ap.add_argument("--min-neighbors", type=int, default=5)
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
        params = engine.NormalParams(a.radius, a.min_neighbors)
        res = dict(points=int(sum(len(x) for x in xyz)), keyframes=nkf, leaf=a.leaf, radius=a.radius, min_neighbors=a.min_neighbors, viewpoints=len(views))
        n = store.build_map(ids, poses, a.leaf)
        res["map_points"] = n
        res["build_map_ms"] = timed(lambda: store.build_map(ids, poses, a.leaf), a.warmup, a.reps)
        store.build_map(ids, poses, a.leaf)
        ptr = engine.C.c_void_p(); cnt = engine.C.c_uint32()
        vp = engine._p(views)

        def call():
            store._check(store._l.qn_kf_map_normals(store.h, engine.C.byref(params), vp, engine.C.c_uint32(len(views)), engine.C.byref(ptr), engine.C.byref(cnt)))
        res["map_normals_ms"] = timed(call, a.warmup, a.reps)
        out = np.zeros((n, 4), np.float32); k = np.zeros(n, np.uint32); vi = np.zeros(n, np.int32)
        res["download_normals_ms"] = timed(lambda: store._check(store._l.qn_kf_download_map_normals(store.h, engine._p(out), engine._p(k), engine._p(vi))), a.warmup, a.reps)
        res["valid_points"] = int(np.isfinite(out[:, 3]).sum()); res["mean_neighbors"] = float(k.mean())
        if not have_scipy:
            res["host"] = "scipy is not importable: no host yardstick"
        elif n > a.host_max_points:
            res["host"] = "skipped above --host-max-points"
        else:
            t0 = time.perf_counter(); pts = store.download_map(n); res["download_map_ms"] = 1e3 * (time.perf_counter() - t0)
            res["host_kdtree_ms"], res["host_pca_ms"], res["host_valid_points"] = host_normals(pts, a.radius, a.min_neighbors, views, a.workers)
            res["host_note"] = "scipy cKDTree.query_ball_point (%d threads) + numpy bincount covariance + numpy.linalg.eigh, f64, one run" % a.workers
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
