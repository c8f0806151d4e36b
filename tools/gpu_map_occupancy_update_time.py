#!/usr/bin/env python
"""Time qn_kf_map_occupancy_update on the stores of tools/gpu_map_occupancy_time.py (--keyframes x --points records along a 400 m path, voxel 0.3), beside the
full qn_kf_map_occupancy of the same list in the same run and beside qn_kf_map_frontiers on the same volume.  Per round, each call under its own host clock (every
call ends in a stream synchronise):
  full          qn_kf_map_occupancy of the whole list (it drops the ledger)
  from_nothing  the update of the list without its last keyframe, with no ledger to start from (rebuilt = 1): the full call's work plus the bookkeeping
  add_last      the update that adds the last keyframe to that volume
  unchanged     the update of the same list again: nothing walked, the classes formed again
  moved_tail    the update after the last 10 % of the poses moved (a loop closure): those entries walked out and in
  all_moved     the update after every pose moved: the worst case, everything walked twice
  frontiers     qn_kf_map_frontiers on the volume that leaves
The median (min, max) over --reps after --warmup rounds, one JSON line per size, with the counters of qn_occupancy_update for each update and, once, whether the
volume after the last update equals a full call of the same list byte for byte.  Needs a GPU (no fall-back)."""
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
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="list sizes: keyframes of --points records each")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from qn_amd import engine
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        P = np.ascontiguousarray(poses, np.float64).reshape(nkf, 4, 4)
        nudge = np.eye(4); c, s = np.cos(0.01), np.sin(0.01)
        nudge[:2, :2] = [[c, -s], [s, c]]; nudge[:3, 3] = (0.2, -0.1, 0.02)
        tail = max(1, nkf // 10)
        moved = P.copy(); moved[nkf - tail:] = nudge @ P[nkf - tail:]
        shifted = (nudge @ nudge) @ P
        params = engine.OccupancyParams(a.voxel)
        steps = (("from_nothing", ids[:-1], P[:-1]), ("add_last", ids, P), ("unchanged", ids, P), ("moved_tail", ids, moved), ("all_moved", ids, shifted))
        times = {k: [] for k in ("full", "frontiers") + tuple(s[0] for s in steps)}
        counters = {}
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); full = store.map_occupancy(ids, P, params); t = {"full": time.perf_counter() - t0}
            for name, l, p in steps:
                t0 = time.perf_counter(); st, up = store.map_occupancy_update(l, p, params); t[name] = time.perf_counter() - t0
                counters[name] = {k: up[k] for k in ("entries_kept", "entries_added", "entries_removed", "rebuilt", "regridded", "records_walked")}
                if name == "unchanged":
                    assert st == full, (st, full)
            t0 = time.perf_counter(); fr = store.map_frontiers(); t["frontiers"] = time.perf_counter() - t0
            if rep >= a.warmup:
                for k, v in t.items():
                    times[k].append(1e3 * v)
        got = store.map_occupancy_grid()
        store.map_occupancy(ids, shifted, params)
        want = store.map_occupancy_grid()
        equal = got[0] == want[0] and all(x.tobytes() == y.tobytes() for x, y in zip(got[1:], want[1:]))
        res = dict(keyframes=nkf, records=int(sum(len(x) for x in xyz)), voxel=a.voxel, rays=full["n_rays"], grid=[full["width"], full["height"], full["depth"]],
                   voxels=full["width"] * full["height"] * full["depth"], frontier_regions=fr["regions"], equals_rebuild=bool(equal),
                   ms={k: stat(v) for k, v in times.items()}, update=counters)
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
