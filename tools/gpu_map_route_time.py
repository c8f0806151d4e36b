#!/usr/bin/env python
"""Time the occupancy map's route field on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, voxel 0.3), for each size in
3-D and in the plane of columns (the band: the goal's layer): qn_kf_map_route (the tiled relaxation to the shortest-path field; its rounds and tile visits are
printed), the extraction of 1 path and of 64 paths (qn_kf_map_route_path), qn_kf_map_distance on the same volume for scale, and what a user without the unit
would do: the download of the class bytes and the d2 field plus scipy's Dijkstra on the same graph (qn_amd/maproute.py dijkstra(): the edge list of every
allowed move, then scipy.sparse.csgraph.dijkstra; one run; skipped when scipy is missing or above --host-max-voxels).  The goal is the passable cell nearest
the first keyframe's position, the starts are passable cells spread over the field.  Each call under its own host clock; every call ends in a stream
synchronise.  The median (min, max) over --reps after --warmup rounds.  The field is compared with the numpy twin's (maproute.field: the specification) up to
--twin-max-voxels.  One JSON line per size.  Needs a GPU (no fall-back)."""
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
    ap.add_argument("--min-d2", type=int, default=4, help="the clearance a passable voxel has, as a squared distance in voxels")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-max-voxels", type=int, default=30000000, help="skip the comparison with the numpy twin above this many voxels")
    ap.add_argument("--host-max-voxels", type=int, default=30000000, help="skip the host route above this many voxels")
    a = ap.parse_args()
    from qn_amd import engine, mapoccupancy, maproute
    try:
        import scipy.sparse.csgraph                                  # noqa: F401 (maproute.dijkstra falls back to a heap, which is no host baseline)
        have_scipy = True
    except ImportError:
        have_scipy = False
    C = engine.C
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        ost = store.map_occupancy(ids, poses, engine.OccupancyParams(voxel=a.voxel))
        W, H, D = ost["width"], ost["height"], ost["depth"]
        n = W * H * D
        res = dict(records=int(sum(len(x) for x in xyz)), keyframes=nkf, voxel=a.voxel, grid=[W, H, D], voxels=n, min_d2=a.min_d2)
        dp = engine.DistanceParams(); dst = engine.DistanceStats()
        ts = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); store._check(store._l.qn_kf_map_distance(store.h, C.byref(dp), C.byref(dst)))
            if rep >= a.warmup:
                ts.append(1e3 * (time.perf_counter() - t0))
        res["map_distance_ms"] = stat(ts)
        t0 = time.perf_counter()
        info, _, _, cls = store.map_occupancy_grid()
        d2 = store.map_distance_grid()[2]
        res["download_ms"] = 1e3 * (time.perf_counter() - t0)       # (with the hit and miss counts the Python wrapper also fetches: an upper bound)
        grid = mapoccupancy.OccupancyGrid(*(info[f] for f in mapoccupancy.OccupancyGrid._fields))
        first = np.asarray(poses[0], np.float64)[:3, 3]
        equal = True
        for mode in ("3d", "planar"):
            k = mapoccupancy.layer_of(first[2], grid)
            tp = maproute.RouteParams(1 << mapoccupancy.FREE, a.min_d2, *((k, k, 1) if mode == "planar" else (0, maproute.INT32_MAX, 0)))
            free = np.argwhere(maproute.passable(cls, d2, tp))[:, ::-1]
            if not len(free):
                res[mode] = "no passable cell"
                continue
            centres = maproute.centres(grid, free, tp)
            goal = np.ascontiguousarray(centres[np.argmin(((centres[:, :2] - first[:2]) ** 2).sum(axis=1) + (0.0 if tp.planar else (centres[:, 2] - first[2]) ** 2))][None])
            p = engine.RouteParams(*tp); st = engine.RouteStats()
            ts = []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter(); store._check(store._l.qn_kf_map_route(store.h, engine._p(goal), C.c_uint32(1), C.byref(p), C.byref(st)))
                if rep >= a.warmup:
                    ts.append(1e3 * (time.perf_counter() - t0))
            r = dict(map_route_ms=stat(ts), stats=[int(v) for v in st.twin()], rounds=int(st.rounds), tile_visits=int(st.tile_visits),
                     tiles=int(np.prod([(s + 7) // 8 for s in (W, H, 1 if tp.planar else D)])))
            starts = np.ascontiguousarray(centres[(np.arange(64) * (len(centres) - 1)) // 63])
            at = store.map_route_query(starts)
            max_len = int(at[at < maproute.BLOCKED].max()) // 3 + 1 if (at < maproute.BLOCKED).any() else 1
            far = starts[[int(np.argmax(np.where(at < maproute.BLOCKED, at, 0)))]]
            for name, pts in (("path_1_ms", far), ("path_64_ms", starts)):
                lens = np.zeros(len(pts), np.uint32); ijk = np.zeros((len(pts), max_len, 3), np.int32)
                ts = []
                for rep in range(a.warmup + a.reps):
                    t0 = time.perf_counter(); store._check(store._l.qn_kf_map_route_path(store.h, engine._p(pts), C.c_uint32(len(pts)), C.c_uint32(max_len), engine._p(lens),
                                                                                         engine._p(ijk)))
                    if rep >= a.warmup:
                        ts.append(1e3 * (time.perf_counter() - t0))
                r[name] = stat(ts); r[name[:-3] + "_voxels"] = int(lens.sum())
            if n <= a.twin_max_voxels:
                t0 = time.perf_counter(); want = maproute.field(cls, d2, grid, goal, tp); r["twin_field_ms"] = 1e3 * (time.perf_counter() - t0)
                equal = equal and bool(np.array_equal(store.map_route_grid()[2], want["cost"]) and tuple(r["stats"]) == tuple(want["stats"]))
            if have_scipy and n <= a.host_max_voxels:
                t0 = time.perf_counter(); maproute.dijkstra(cls, d2, grid, goal, tp); r["host_dijkstra_ms"] = 1e3 * (time.perf_counter() - t0)
            res[mode] = r
        res["equals_twin"] = equal if n <= a.twin_max_voxels else "skipped above --twin-max-voxels"
        res["host_note"] = ("maproute.dijkstra of the downloaded classes and d2: numpy edge list plus scipy.sparse.csgraph.dijkstra, one thread, one run" if have_scipy
                            else "scipy is not installed")
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
