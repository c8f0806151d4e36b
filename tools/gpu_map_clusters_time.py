#!/usr/bin/env python
"""Time the clustering of the corrected global map on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, leaf 0.3), the
maps tools/gpu_map_ground_time.py uses: qn_kf_map_clusters (cell index, lock-free union-find over the radius graph, flatten, numbering, the clusters' boxes and
sums; at most four host synchronisations) over every finite point (class_mask 0) and over what stands on the ground (OBSTACLE | OVERHEAD after
qn_kf_map_ground, which is outside the clock), beside qn_kf_build_map of the same list - the build that fed it - and beside what the host pays for the same
components: scipy.spatial.cKDTree.query_pairs plus scipy.sparse.csgraph.connected_components on the downloaded map (f64 distances; the component count is
printed beside the GPU's, they agree wherever no pair lies on the tolerance).  A classify does not change the slot, so the repetitions run on one build; every
call ends in a stream synchronise and is under a host clock of its own.  The median (min, max) over --reps after --warmup rounds, two JSON lines per size (the GPU's
figures as soon as they are known, then the whole record with the host's); needs a GPU (no fall-back)."""
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
    ap.add_argument("--tolerance", type=float, default=0.5)
    ap.add_argument("--min-size", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-points", type=int, default=8000000, help="skip the host yardstick above this many map points")
    a = ap.parse_args()
    from qn_amd import engine, mapground
    C = engine.C
    objects = (1 << mapground.OBSTACLE) | (1 << mapground.OVERHEAD)
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        res = dict(points=int(sum(len(x) for x in xyz)), keyframes=nkf, leaf=a.leaf, tolerance=a.tolerance, min_size=a.min_size)
        st = engine.ClusterStats()
        tb = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); n = store.build_map(ids, poses, a.leaf)
            if rep >= a.warmup:
                tb.append(1e3 * (time.perf_counter() - t0))
        res.update(map_points=n, build_map_ms=stat(tb))
        store.map_ground(engine.GroundParams())
        for name, mask in (("all_points", 0), ("objects", objects)):
            params = engine.ClusterParams(a.tolerance, a.min_size, 0xffffffff, mask)
            ts = []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter(); store._check(store._l.qn_kf_map_clusters(store.h, C.byref(params), C.byref(st)))
                if rep >= a.warmup:
                    ts.append(1e3 * (time.perf_counter() - t0))
            res[name] = dict(map_clusters_ms=stat(ts), members=int(st.members), edges=int(st.edges), components=int(st.components), clusters=int(st.clusters),
                             largest=int(st.largest))
        print(json.dumps(dict(res, stage="gpu")), flush=True)              # (the host yardstick below takes far longer than everything above)
        if n > a.host_max_points:
            res["host"] = "skipped above --host-max-points"
        else:
            from scipy.spatial import cKDTree
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            t0 = time.perf_counter(); pts = store.download_map(n); res["download_map_ms"] = 1e3 * (time.perf_counter() - t0)
            x = pts[np.isfinite(pts[:, :3]).all(axis=1), :3].astype(np.float64)
            t0 = time.perf_counter(); tree = cKDTree(x); t1 = time.perf_counter()
            pr = tree.query_pairs(a.tolerance, output_type="ndarray"); t2 = time.perf_counter()
            k, _ = connected_components(coo_matrix((np.ones(len(pr), np.int8), (pr[:, 0], pr[:, 1])), shape=(len(x), len(x))), directed=False)
            t3 = time.perf_counter()
            res.update(host_kdtree_ms=1e3 * (t1 - t0), host_query_pairs_ms=1e3 * (t2 - t1), host_components_ms=1e3 * (t3 - t2), host_total_ms=1e3 * (t3 - t0),
                       host_pairs=int(len(pr)), host_components=int(k),
                       host_note="scipy cKDTree.query_pairs + csgraph.connected_components over every finite point, f64, one thread, one run")
        store.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
