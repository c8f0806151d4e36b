#!/usr/bin/env python
"""Time the range images (KeyframeStore.range_describe) and the free-space check of every pair of a verify call (KeyframeStore.freespace_batch) against
the verify call that produced the pairs.

Setup of tools/gpu_overlap_time.py with the full-size sensor: ray-cast spinning-LiDAR keyframes (64 beams x 1800 columns, ~100k records each) of the street
scene, leaf 0.3, the GICP path (verify_loop_pairs, poses = the ground truth, submap_range 5, NanoGICP as LoopClosure's ctor sets it with max_corr_dist 18).
  (a) range_describe of S = 64 and S = 512 keyframes (64 x 1800 images);
  (b) one query with K = 1 / 16 candidates, and a 64-pair call (16 queries x 4 candidates): the verify call - the yardstick - and freespace_batch on its
      pairs' transforms, both directions of every pair on the raw scans.
Every timed call ends in a host synchronisation; a host clock around it; --warmup runs, then the median of --reps with min .. max.  One JSON line per case;
needs a GPU (no fall-back)."""
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
    return dict(median_ms=round(1e3 * float(np.median(ts)), 3), min_ms=round(1e3 * min(ts), 3), max_ms=round(1e3 * max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=512)
    a = ap.parse_args()
    from qn_amd import engine, synth, freespace
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar()
    N, leaf, rng_sub = a.keyframes, 0.3, 5
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 20), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = []
    for s in range(0, N, 64):                                     # (the ray-caster's own scratch grows with the number of scans per call)
        ids += [int(i) for i in store.add_lidar_scans(prims, sen, poses[s:s + 64], np.arange(s, min(s + 64, N)) + 1)]
    sizes = [store._sizes[i] for i in ids]
    store.range_set_params(engine.RangeParams.for_sensor(sen))
    for S in (64, N):
        t = timed(lambda: store.range_describe(ids[:S]), a.warmup, a.reps)
        print(json.dumps(dict(case="describe", S=S, records=int(sum(sizes[:S])), image="%dx%d" % (sen.n_beams, sen.n_cols), describe=t,
                              us_per_keyframe=round(1e3 * t["median_ms"] / S, 2))), flush=True)
    ctx = engine.Context(400000)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(18.0); g.setTransformationEpsilon(0.01); g.bind()
    M = min(N, 96)                                                # the pairs come from the first 96 keyframes, as tools/gpu_overlap_time.py's
    for Q, K in ((1, 1), (1, 16), (16, 4)):
        qs = ids[M - Q:M]
        cands = {q: sorted(sorted(range(M - 24), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))[:K]) for q in qs}
        pq = [q for q in qs for _ in cands[q]]; pc = [c for q in qs for c in cands[q]]
        P = len(pq)
        verify = lambda: store.verify_loop_pairs(ctx, pq, pc, None, poses[:M], rng_sub, leaf)
        t_verify = timed(verify, a.warmup, a.reps)
        rs = verify()
        assert all(r["status"] == 0 for r in rs)
        T = [np.array(r["record"].T64).reshape(4, 4) for r in rs]
        recs = store.freespace_batch(pq, pc, T)
        assert all(o["status"] == 0 for o in recs)
        t = timed(lambda: store.freespace_batch(pq, pc, T), a.warmup, a.reps)
        fr = [[freespace.see_through_fraction(o[k]) for o in recs] for k in ("q_in_c", "c_in_q")]
        print(json.dumps(dict(case="check", Q=Q, K=K, pairs=P, valid=sum(r["valid"] for r in rs), records=sum(o["q_in_c"]["n"] + o["c_in_q"]["n"] for o in recs),
                              verify=t_verify, freespace=t, ratio=round(t["median_ms"] / t_verify["median_ms"], 4),
                              see_through_valid=[round(float(np.mean([f for f, r in zip(fr[d], rs) if r["valid"]] or [0.0])), 4) for d in (0, 1)],
                              see_through_invalid=[round(float(np.mean([f for f, r in zip(fr[d], rs) if not r["valid"]] or [0.0])), 4) for d in (0, 1)])), flush=True)
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
