#!/usr/bin/env python
"""Time the drift-free verification of K loop candidates of one query (KeyframeStore.verify_loop_candidates: one assembly, one batched
registration from the Scan Context headings) against K separate assemble + qn_icp_alignment_device calls on the same pairs (the world-frame
path the replay takes per candidate, one candidate per call), for K = 1, 4, 8, 16.

Keyframes: ray-cast spinning-LiDAR scans (synth.SpinningLidar, 32 beams x 720 columns) of the street scene, three passes back and forth along
30 m, put into the store by add_lidar_scans; the query is the last keyframe, its candidates the K older keyframes nearest to it (the last 8
excluded), seeded with their true heading differences; submap_range 5, leaf 0.3, NanoGICP as
LoopClosure's ctor sets it (k 15, 32 iterations, max_corr_dist 18, epsilon 0.01).  Both sides register the same source and target clouds (the
separate path assembles them with the relative poses too, so only the way they are driven differs); the separate path starts from identity, as
qn_icp_alignment_device does (the headings here differ by at most 0.6 rad).  Every timed call returns after its own host synchronisation; a host clock around it, median of --reps after --warmup
runs.  Prints the GPU, the point counts and the number of runs with the times as one JSON line; needs a GPU (no fall-back)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))
import numpy as np


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=60)
    a = ap.parse_args()
    from qn_amd import engine, synth, scancontext as sc
    import torch
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    N = a.keyframes
    # back and forth along a 30 m stretch of street (three passes): the last keyframe revisits places many older keyframes have seen
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 20), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = list(store.add_lidar_scans(prims, sen, poses, np.arange(N) + 1))
    ctx = engine.Context(400000)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(18.0); g.setTransformationEpsilon(0.01); g.bind()
    q, R, leaf = ids[-1], 5, 0.3
    props = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
    out = dict(gpu="%s (%s)" % (props.name, props.gcnArchName) if props is not None else "unknown", keyframes=N,
               points_per_keyframe=int(np.mean([store._sizes[i] for i in ids])), submap_range=R, leaf=leaf, warmup=a.warmup, reps=a.reps, cases={})
    for K in (1, 4, 8, 16):
        near = sorted(range(N - 8), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))
        cand = sorted(near[:K])
        yaw = [math.atan2(poses[c][1, 0], poses[c][0, 0]) - math.atan2(poses[q][1, 0], poses[q][0, 0]) for c in cand]      # the headings Scan Context would give
        first = store.verify_loop_candidates(ctx, q, cand, yaw, poses, R, leaf)
        n_src, n_tgt = store._batch_n[0], store._batch_n[1:]
        batched = timed(lambda: store.verify_loop_candidates(ctx, q, cand, yaw, poses, R, leaf), a.warmup, a.reps)

        def separate():
            for c, y in zip(cand, yaw):
                sub = engine.loop_submap_ids(q, c, R, False, False, len(poses))[1]
                ps, ns = store.assemble([q], [np.eye(4)], leaf, 0)
                pd, nd = store.assemble(sub, [sc.relative_pose(poses[c], poses[i]) for i in sub], leaf, 1)
                res = engine.GicpResult(); v = C.c_int()
                ctx.check(ctx._l.qn_icp_alignment_device(ctx.h, C.c_void_p(ps), C.c_uint32(ns), C.c_void_p(pd), C.c_uint32(nd), C.c_uint32(16),
                                                         C.c_double(1.5), C.byref(res), C.byref(v)))
        sep = timed(separate, a.warmup, a.reps)
        out["cases"]["K%d" % K] = dict(verify_ms=round(batched, 3), separate_ms=round(sep, 3), speedup=round(sep / batched, 2),
                                       source_points=n_src, target_points_mean=int(np.mean(n_tgt)), valid=sum(r["valid"] for r in first))
    print(json.dumps(out))
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
