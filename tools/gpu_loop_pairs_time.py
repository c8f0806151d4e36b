#!/usr/bin/env python
"""Time one multi-query verification (KeyframeStore.verify_loop_pairs / verify_loop_pairs_c2f) against Q single-query calls
(verify_loop_candidates / verify_loop_candidates_c2f) over the same (query, candidate) pairs, for Q in {1, 4, 8, 16} queries x K in {1, 4, 8}
candidates per query.

Keyframes: ray-cast spinning-LiDAR scans (synth.SpinningLidar, 32 beams x 720 columns) of the street scene along a 30 m stretch, as
tools/gpu_sc_c2f_time.py, put into the store by add_lidar_scans and described once (quatro_describe, leaf 0.3).  Queries: the last Q keyframes;
each query's candidates: the K older keyframes nearest to it (the last 24 excluded), so that neighbouring queries share candidates the way the
keyframes of one timer tick do.  GICP path: poses = the ground truth, submap_range 5, seeds from yaw 0.  NanoGICP as LoopClosure's ctor sets it
(k 15, 32 iterations, max_corr_dist 18, epsilon 0.01), Quatro at the reference's parameters.  The records of both forms are checked equal before
timing.  Every timed call ends in a host synchronisation; a host clock around it, median of --reps after --warmup runs.  Prints one JSON line per
(path, Q, K); needs a GPU (no fall-back)."""
import argparse
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from qn_amd import engine, synth
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    N, leaf, rng_sub = 96, 0.3, 5
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 20), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(N) + 1)]
    ctx = engine.Context(200000)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(18.0); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    assert store.quatro_describe(ctx, ids, leaf) == [0] * N
    for Q in (1, 4, 8, 16):
        for K in (1, 4, 8):
            qs = ids[N - Q:]
            cands = {q: sorted(sorted(range(N - 24), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))[:K]) for q in qs}
            pq = [q for q in qs for _ in cands[q]]; pc = [c for q in qs for c in cands[q]]
            for path in ("gicp", "c2f"):
                if path == "gicp":
                    many = lambda: store.verify_loop_pairs(ctx, pq, pc, None, poses, rng_sub, leaf)
                    one = lambda: [r for q in qs for r in store.verify_loop_candidates(ctx, q, cands[q], None, poses, rng_sub, leaf)]
                else:
                    many = lambda: store.verify_loop_pairs_c2f(ctx, pq, pc)
                    one = lambda: [r for q in qs for r in store.verify_loop_candidates_c2f(ctx, q, cands[q])]
                rm, r1 = many(), one()
                assert [(r["status"], r["valid"], r["T"].tobytes()) for r in rm] == [(r["status"], r["valid"], r["T"].tobytes()) for r in r1], (path, Q, K)
                t_many, t_one = timed(many, a.warmup, a.reps), timed(one, a.warmup, a.reps)
                print(json.dumps(dict(path=path, Q=Q, K=K, pairs=len(pq), distinct_candidates=len(set(pc)), multi_ms=round(t_many, 3),
                                      single_calls_ms=round(t_one, 3), speedup=round(t_one / t_many, 2), valid=sum(r["valid"] for r in rm))), flush=True)
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
