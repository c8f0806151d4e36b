#!/usr/bin/env python
"""Time the occupancy map's view gain on the volumes of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, voxel 0.3): for each size
qn_kf_map_occupancy and qn_kf_map_frontiers on the same store for scale, then qn_kf_map_view_gain with Q = 1, 16 and 256 viewpoints at the centres of the
frontier regions' root voxels (the regions taken round-robin when there are fewer than Q), the ray table of a 64-beam, 900-step sensor (R = 57600, elevations
-25 .. 15 degrees) of 20 m and of 60 m range.  Each call under its own host clock; every call ends in a stream synchronise.  The median (min, max) over --reps
after --warmup rounds, the steps per second (the statistics' steps over the median), the same call under QN_VIEW_NO_PEEK=1 (the returning atomicOr on every
visit of a gain voxel in the band: the yardstick of the plain read), and for Q = 1 the numpy twin (mapview.gain: the specification; one thread, one run) with
the comparison of rows, cover and statistics.  One JSON line per size.  Needs a GPU (no fall-back)."""
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
    ap.add_argument("--viewpoints", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--ranges", type=float, nargs="+", default=[20.0, 60.0])
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=900)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-max-voxels", type=int, default=30000000, help="skip the numpy twin above this many voxels")
    a = ap.parse_args()
    from qn_amd import engine, mapoccupancy, mapview
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
        res = dict(records=int(sum(len(x) for x in xyz)), keyframes=nkf, voxel=a.voxel, rays=a.beams * a.azimuth)
        res["map_occupancy_ms"] = timed(lambda: store._check(store._l.qn_kf_map_occupancy(store.h, engine._p(ids), engine._p(P), C.c_uint32(len(ids)), C.byref(op), C.byref(ost))))
        W, H, D = int(ost.width), int(ost.height), int(ost.depth)
        n = W * H * D
        res.update(grid=[W, H, D], voxels=n, carve_visits=int(ost.total_hits) + int(ost.total_misses))
        fp = engine.FrontierParams(); fst = engine.FrontierStats()
        res["map_frontiers_ms"] = timed(lambda: store._check(store._l.qn_kf_map_frontiers(store.h, C.byref(fp), C.byref(fst))))
        rows = store.map_frontier_regions()
        res["regions"] = len(rows)
        if not len(rows):
            store.close(); print(json.dumps(dict(res, note="no frontier region")), flush=True)
            continue
        oinfo, _, _, cls = store.map_occupancy_grid()
        grid = mapoccupancy.OccupancyGrid(**oinfo)
        root = rows["root"].astype(np.int64)
        centres = mapoccupancy.centres(np.stack([root % W, (root // W) % H, root // (W * H)], axis=1), grid)
        vp = engine.ViewParams(); vst = engine.ViewStats()
        res["calls"] = []
        for rng in a.ranges:
            off = mapview.sensor_offsets(a.voxel, rng, a.beams, a.azimuth, -25.0, 15.0)
            for Q in a.viewpoints:
                pts = np.ascontiguousarray(centres[np.arange(Q) % len(centres)])
                info = np.zeros(Q, mapview.VIEW_DTYPE)
                call = lambda: store._check(store._l.qn_kf_map_view_gain(store.h, engine._p(pts), C.c_uint32(Q), engine._p(off), C.c_uint32(len(off)), C.byref(vp), engine._p(info), C.byref(vst)))
                os.environ.pop("QN_VIEW_NO_PEEK", None)
                r = dict(range=rng, viewpoints=Q, view_gain_ms=timed(call), stats=[int(v) for v in vst.twin()], passes=int(vst.passes))
                r["steps_per_s"] = float(vst.steps) / (1e-3 * r["view_gain_ms"][0])
                got = (info.copy(), store.map_view_grid()[2])
                os.environ["QN_VIEW_NO_PEEK"] = "1"
                r["no_peek_ms"] = timed(call)
                os.environ.pop("QN_VIEW_NO_PEEK", None)
                r["no_peek_same_bytes"] = bool(info.tobytes() == got[0].tobytes() and np.array_equal(store.map_view_grid()[2], got[1]))
                if Q == 1 and n <= a.twin_max_voxels:
                    t0 = time.perf_counter(); want = mapview.gain(cls, grid, pts, off, vp.twin()); r["twin_ms"] = 1e3 * (time.perf_counter() - t0)
                    r["equals_twin"] = bool(got[0].tobytes() == want["info"].tobytes() and np.array_equal(got[1], want["cover"]) and tuple(r["stats"]) == tuple(want["stats"]))
                res["calls"].append(r)
        res["carve_visits_per_s"] = res["carve_visits"] / (1e-3 * res["map_occupancy_ms"][0])
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
