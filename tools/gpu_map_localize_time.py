#!/usr/bin/env python
"""Time the localisation of scans in the corrected global map on the scene of tools/gpu_map_time.py (--keyframes x --points records along a 400 m path, leaf
0.3), the maps the other map tools use.  For K = --pairs pose guesses (K keyframes spread over the path, each displaced by 0.5 m / 3 degrees):
  crop_ms        qn_kf_map_crop alone: the K neighbourhoods of --radius cut out of the map slot (count, scan, one host read, compaction; two synchronisations)
  localize_ms    qn_kf_map_localize: the crops, the K scans' voxel grids and ONE batched registration of the K device pairs
  host_route_ms  what a caller pays without it: download the map, crop it with numpy (the twin's arithmetic), voxel-filter the scans on the device
                 (assemble_batch) and download them, then gicp_align_batch of the host clouds (which uploads both sides again); its parts are listed
  loop_pairs_ms  qn_kf_verify_loop_pairs of K (keyframe, next keyframe) pairs with --submap-range, for scale: windows of a similar number of points
Every call ends in a stream synchronise and is under a host clock of its own.  The median (min, max) over --reps after --warmup rounds, two JSON lines per map
size and K (the GPU's figures as soon as they are known, then the whole record); needs a GPU (no fall-back)."""
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


def timed(fn, warmup, reps):
    ts = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter(); fn()
        if rep >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    return stat(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 500], help="map sizes: keyframes of --points records each (500 x 60000 is gpu_map_time.py's map)")
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--radius", type=float, default=20.0, help="the crop radius [m] (a crop must fit --max-points)")
    ap.add_argument("--max-points", type=int, default=400000, help="the registration context's capacity")
    ap.add_argument("--submap-range", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    a = ap.parse_args()
    from qn_amd import engine, maplocalize as ml
    C = engine.C
    D = np.eye(4); c, s = np.cos(np.radians(3.0)), np.sin(np.radians(3.0))
    D[:2, :2] = [[c, -s], [s, c]]; D[:3, 3] = (0.3, 0.4, 0.0)
    for nkf in a.keyframes:
        xyz, inten, poses = scene(nkf, a.points)
        store = engine.KeyframeStore()
        ids = [store.add(x, i) for x, i in zip(xyz, inten)]
        ctx = engine.Context(a.max_points)
        g = engine.NanoGICP(ctx)
        g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(1.5 * a.radius); g.setTransformationEpsilon(0.01); g.bind()
        n = store.build_map(ids, poses, a.leaf)
        params = engine.LocalizeParams(a.radius, a.leaf, 1.5, 0)
        for K in a.pairs:
            q = [int(i * nkf // K) for i in range(K)] if K <= nkf else [i % nkf for i in range(K)]
            G = [poses[k] @ D for k in q]
            if K > nkf:                                                 # more guesses than keyframes: further positions along the path for the same scans
                for j in range(nkf, K):
                    G[j] = G[j].copy(); G[j][0, 3] += 0.37 * (j // nkf)
            centres = np.array([ml.guess_f32(T)[:3, 3] for T in G], np.float64)
            counts = np.zeros(K, np.uint32)
            res = dict(keyframes=nkf, points=int(nkf * a.points), map_points=int(n), leaf=a.leaf, radius=a.radius, pairs=K)
            res["crop_ms"] = timed(lambda: store._check(store._l.qn_kf_map_crop(store.h, engine._p(centres), C.c_uint32(K), C.c_double(a.radius), C.c_uint32(0),
                                                                               engine._p(counts))), a.warmup, a.reps)
            res.update(crop_points=int(counts.sum()), crop_largest=int(counts.max()))
            out = {}
            def loc():
                out["r"] = store.map_localize(ctx, [ids[k] for k in q], G, params)
            res["localize_ms"] = timed(loc, a.warmup, a.reps)
            rs, st = out["r"]
            res.update(n_scans=st["n_scans"], n_crops=st["n_crops"], passes=st["passes"], ok=sum(r["status"] == 0 for r in rs), valid=sum(r["valid"] for r in rs),
                       iterations=[r["iterations"] for r in rs][:8])
            print(json.dumps(dict(res, stage="gpu")), flush=True)          # (the host route below takes far longer than everything above)
            if not a.no_host:
                parts = dict(download=[], crop=[], scans=[], register=[])
                def host():
                    t0 = time.perf_counter(); m = store.download_map(n); t1 = time.perf_counter()
                    crops = [ml.crop(m, cc, a.radius)[0] for cc in centres]; t2 = time.perf_counter()
                    uq = list(dict.fromkeys(q))
                    segs = store.assemble_batch([[ids[k]] for k in uq], [[np.eye(4)]] * len(uq), a.leaf)
                    scans = {k: store.download_batch(i, segs[i][1]) for i, k in enumerate(uq)}; t3 = time.perf_counter()
                    pairs = [(scans[k], len(scans[k]), np.ascontiguousarray(cr[:, :3]), len(cr), 12, 0) for k, cr in zip(q, crops)]      # (n, 3) packed, both sides
                    engine.gicp_align_batch(ctx, pairs, 1.5, guesses=G)
                    t4 = time.perf_counter()
                    for k, v in zip(("download", "crop", "scans", "register"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                        parts[k].append(1e3 * v)
                res["host_route_ms"] = timed(host, a.warmup, a.reps)
                res["host_parts_ms"] = {k: float(np.median(v[a.warmup:])) for k, v in parts.items()}
            if nkf >= 2:
                qq = list(dict.fromkeys(k if k + 1 < nkf else k - 1 for k in q))
                cc = [k + 1 for k in qq]
                def loop():
                    out["l"] = store.verify_loop_pairs(ctx, [ids[k] for k in qq], [ids[k] for k in cc], None, poses, a.submap_range, a.leaf)
                res["loop_pairs_ms"] = timed(loop, a.warmup, a.reps)
                res.update(loop_pairs=len(qq), loop_ok=sum(r["status"] == 0 for r in out["l"]), loop_iterations=[r["iterations"] for r in out["l"]][:8],
                           loop_window_points=int(np.mean(store._batch_n[len(qq):])) if len(store._batch_n) > len(qq) else 0)
            print(json.dumps(res), flush=True)
        ctx.close(); store.close()


if __name__ == "__main__":
    main()
