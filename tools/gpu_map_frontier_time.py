#!/usr/bin/env python
"""Time the occupancy map's frontier regions on the scene of tools/gpu_map_route_time.py (--keyframes x --points records along a 400 m path, voxel 0.3): for each
size qn_kf_map_occupancy for scale, qn_kf_map_frontiers (mark, the union-find labelling, the numbering; its statistics are printed), the list of every frontier
voxel (qn_kf_map_frontier_list), the regions' reach costs under a route field to the first keyframe's position (qn_kf_map_frontier_costs, after
qn_kf_map_distance and qn_kf_map_route, which are not timed here), and what a user without the unit would do after every map update: the download of the class
bytes, the marking of the frontier voxels in numpy (qn_amd/mapfrontier.py mark()) and scipy.ndimage.label with the 3 x 3 x 3 structure on the marked volume (one
run; skipped when scipy is missing or above --host-max-voxels).  Each call under its own host clock; every call ends in a stream synchronise.  The median
(min, max) over --reps after --warmup rounds.  The result is compared with the numpy twin's (mapfrontier.frontier: the specification) up to --twin-max-voxels.
One JSON line per size.  Needs a GPU (no fall-back)."""
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
    ap.add_argument("--min-size", type=int, default=8, help="the smallest component, in voxels, that is a region")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-max-voxels", type=int, default=30000000, help="skip the comparison with the numpy twin above this many voxels")
    ap.add_argument("--host-max-voxels", type=int, default=30000000, help="skip the host route above this many voxels")
    a = ap.parse_args()
    from qn_amd import engine, mapfrontier
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    C = engine.C

    def timed(call):
        ts = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); call()
            if rep >= a.warmup:
                ts.append(1e3 * (time.perf_counter() - t0))
        return stat(ts)

    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = np.ascontiguousarray([store.add(x, i) for x, i in zip(xyz, inten)], np.int32)
        P = np.ascontiguousarray(poses, np.float64).reshape(len(ids), 16)
        op = engine.OccupancyParams(voxel=a.voxel); ost = engine.OccupancyStats()
        res = dict(records=int(sum(len(x) for x in xyz)), keyframes=nkf, voxel=a.voxel, min_size=a.min_size)
        res["map_occupancy_ms"] = timed(lambda: store._check(store._l.qn_kf_map_occupancy(store.h, engine._p(ids), engine._p(P), C.c_uint32(len(ids)), C.byref(op), C.byref(ost))))
        W, H, D = int(ost.width), int(ost.height), int(ost.depth)
        n = W * H * D
        res.update(grid=[W, H, D], voxels=n)
        fp = engine.FrontierParams(min_size=a.min_size); fst = engine.FrontierStats()
        res["map_frontiers_ms"] = timed(lambda: store._check(store._l.qn_kf_map_frontiers(store.h, C.byref(fp), C.byref(fst))))
        res["stats"] = [int(v) for v in fst.twin()]; res["rounds"] = int(fst.rounds)
        m, R = int(fst.frontier), int(fst.regions)
        ijk = np.zeros((max(m, 1), 3), np.int32); lab = np.zeros(max(m, 1), np.int32); cnt = C.c_uint32()
        res["frontier_list_ms"] = timed(lambda: store._check(store._l.qn_kf_map_frontier_list(store.h, engine._p(ijk), engine._p(lab), C.c_uint32(len(lab)), C.byref(cnt))))
        store.map_distance()
        store.map_route([np.asarray(poses[0], np.float64)[:3, 3]], engine.RouteParams(min_d2=0))
        cost = np.zeros(max(R, 1), np.uint32); at = np.zeros((max(R, 1), 3), np.int32)
        res["frontier_costs_ms"] = timed(lambda: store._check(store._l.qn_kf_map_frontier_costs(store.h, engine._p(cost), engine._p(at))))
        res["regions_reached"] = int((cost[:R] < engine.QN_ROUTE_BLOCKED).sum())
        # ---- the host route: the class bytes alone come down, are marked and labelled
        g = engine.OccupancyGrid(); cls = np.zeros(max(n, 1), np.uint8)
        t0 = time.perf_counter(); store._check(store._l.qn_kf_map_occupancy_grid(store.h, C.byref(g), None, None, engine._p(cls)))
        res["host_download_ms"] = 1e3 * (time.perf_counter() - t0)
        cls = cls[:n].reshape(D, H, W)
        tp = fp.twin()
        if ndimage is not None and n <= a.host_max_voxels:
            t0 = time.perf_counter(); _, faces = mapfrontier.mark(cls, tp); res["host_mark_ms"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter(); _, comps = ndimage.label(faces > 0, structure=np.ones((3, 3, 3), bool)); res["host_label_ms"] = 1e3 * (time.perf_counter() - t0)
            res["host_components"] = int(comps)
        res["host_note"] = ("the class download, mapfrontier.mark in numpy and scipy.ndimage.label (3 x 3 x 3), one thread, one run; sizes, numbering and the regions' "
                            "rows would come on top" if ndimage is not None else "scipy is not installed")
        if n <= a.twin_max_voxels:
            t0 = time.perf_counter(); want = mapfrontier.frontier(cls, tp); res["twin_frontier_ms"] = 1e3 * (time.perf_counter() - t0)
            res["equals_twin"] = bool(np.array_equal(store.map_frontier_grid()[2], want["labels"]) and store.map_frontier_regions().tobytes() == want["info"].tobytes() and
                                      tuple(res["stats"]) == tuple(want["stats"]))
        else:
            res["equals_twin"] = "skipped above --twin-max-voxels"
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
