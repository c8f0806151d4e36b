#!/usr/bin/env python
"""Time the 3-D occupancy map on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, voxel 0.3): qn_kf_map_occupancy (the
extent pass, the ray walk with its integer scatter-adds, classify and counts; two host synchronisations), the list of occupied voxels
(qn_kf_map_occupancy_list: count, scan, compact and the download) and a slice (qn_kf_map_occupancy_slice), beside qn_kf_build_map of the same list, each under
its own host clock; every call ends in a stream synchronise.  The median (min, max) over --reps after --warmup rounds.  Prints the rays, total_misses and the
integer adds per second of the whole call (hits + misses over its median: the extent pass, the memsets and the classify pass are inside that time, so the walk
alone is faster than this figure) in one JSON line per size.  On the sizes up to --host-max-rays also one run of the host twin (qn_amd/mapoccupancy.py: the
specification, so the host result is the GPU's), numpy on one thread.  Needs a GPU (no fall-back)."""
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
    ap.add_argument("--leaf", type=float, default=0.3, help="the leaf of the qn_kf_build_map timed beside it")
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--min-range", type=float, default=0.5)
    ap.add_argument("--max-range", type=float, default=60.0)
    ap.add_argument("--shell", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-fold", action="store_true", help="the yardstick: every lane adds its own miss to the first voxel (QN_OCC_NO_FOLD; the same bytes)")
    ap.add_argument("--host-max-rays", type=int, default=4000000, help="skip the host twin above this many records")
    a = ap.parse_args()
    if a.no_fold:
        os.environ["QN_OCC_NO_FOLD"] = "1"                           # read by the library at every call
    from qn_amd import engine, mapoccupancy
    C = engine.C
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = np.array([store.add(x, i) for x, i in zip(xyz, inten)], np.int32)
        P = np.ascontiguousarray(poses, np.float64).reshape(nkf, 16)
        params = engine.OccupancyParams(a.voxel, a.min_range, a.max_range, a.shell, 1, 2)
        res = dict(records=int(sum(len(x) for x in xyz)), keyframes=nkf, voxel=a.voxel, min_range=a.min_range, max_range=a.max_range, shell=a.shell, fold=not a.no_fold)
        st = engine.OccupancyStats()
        tb, to, tl, ts = [], [], [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); store.build_map(ids, poses, a.leaf)
            t1 = time.perf_counter(); store._check(store._l.qn_kf_map_occupancy(store.h, engine._p(ids), engine._p(P), C.c_uint32(nkf), C.byref(params), C.byref(st)))
            t2 = time.perf_counter(); occ = store.map_occupancy_list(1 << engine.QN_OCC_OCCUPIED)
            t3 = time.perf_counter(); store.map_occupancy_slice(0, int(st.depth) - 1)
            t4 = time.perf_counter()
            if rep >= a.warmup:
                tb.append(1e3 * (t1 - t0)); to.append(1e3 * (t2 - t1)); tl.append(1e3 * (t3 - t2)); ts.append(1e3 * (t4 - t3))
        adds = int(st.total_hits) + int(st.total_misses)
        res.update(rays=int(st.n_rays), skipped=[int(st.n_nonfinite), int(st.n_near), int(st.n_far)], total_misses=int(st.total_misses),
                   grid=[int(st.width), int(st.height), int(st.depth)], voxels=int(st.width) * int(st.height) * int(st.depth),
                   classes=[int(st.occupied), int(st.free), int(st.unknown)], listed=int(len(occ[0])), build_map_ms=stat(tb), map_occupancy_ms=stat(to),
                   occupied_list_ms=stat(tl), slice_ms=stat(ts), adds_per_s=adds / (1e-3 * float(np.median(to))),
                   steps_per_ray=float(st.total_misses) / max(int(st.n_rays), 1))
        if res["records"] > a.host_max_rays:
            res["host"] = "skipped above --host-max-rays"
        else:
            t0 = time.perf_counter(); want = mapoccupancy.classify(xyz, poses, params.twin()); res["host_twin_ms"] = 1e3 * (time.perf_counter() - t0)
            _, hits, misses, cls = store.map_occupancy_grid()
            res["equals_twin"] = bool(np.array_equal(hits, want["hits"]) and np.array_equal(misses, want["misses"]) and np.array_equal(cls, want["classes"]))
            res["host_note"] = "numpy: all rays advance one walk step a round, one bincount per 2^22 visited voxels, one thread, one run"
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
