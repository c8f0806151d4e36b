#!/usr/bin/env python
"""Time the two-way overlap of every pair of a verify call (KeyframeStore.verify_overlap) against the verify call that produced the pairs.

Setup of tools/gpu_loop_pairs_time.py: 96 ray-cast spinning-LiDAR keyframes (32 beams x 720 columns) of the street scene, leaf 0.3, the GICP path
(verify_loop_pairs, poses = the ground truth, submap_range 5, NanoGICP as LoopClosure's ctor sets it with max_corr_dist 18).  One query with K = 1 / 4 / 16
candidates, and a 64-pair call (16 queries x 4 candidates).  Per case:
  (a) verify_overlap for all pairs of the call, at r = 0.3 and r = 0.6;
  (b) the verify call itself - the yardstick;
  (c) for context: downloading the same clouds (verify_cloud FINAL / DST) and running the twin's cKDTree form on the host.
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
    ap.add_argument("--no-host", action="store_true", help="skip (c)")
    a = ap.parse_args()
    from qn_amd import engine, synth, overlap
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
    for Q, K in ((1, 1), (1, 4), (1, 16), (16, 4)):
        qs = ids[N - Q:]
        cands = {q: sorted(sorted(range(N - 24), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))[:K]) for q in qs}
        pq = [q for q in qs for _ in cands[q]]; pc = [c for q in qs for c in cands[q]]
        P = len(pq)
        verify = lambda: store.verify_loop_pairs(ctx, pq, pc, None, poses, rng_sub, leaf)
        t_verify = timed(verify, a.warmup, a.reps)
        rs = verify()
        assert all(r["status"] == 0 for r in rs)
        row = dict(Q=Q, K=K, pairs=P, valid=sum(r["valid"] for r in rs), verify=t_verify)
        for r in (0.3, 0.6):
            recs = store.verify_overlap(r, n_pairs=P)
            assert all(o["status"] == 0 for o in recs)
            t = timed(lambda: store.verify_overlap(r, n_pairs=P), a.warmup, a.reps)
            row["overlap_r%.1f" % r] = t
            row["ratio_r%.1f" % r] = round(t["median_ms"] / t_verify["median_ms"], 4)
            row["points"] = sum(o["a_to_b"]["n"] + o["b_to_a"]["n"] for o in recs)
            row["mean_overlap_r%.1f" % r] = [round(float(np.mean([overlap.overlap_fraction(o[k]) for o in recs])), 4) for k in ("a_to_b", "b_to_a")]
            if not a.no_host:
                def host():
                    out = []
                    for j in range(P):
                        fin, dst = store.verify_cloud(j, engine.QN_VERIFY_FINAL), store.verify_cloud(j, engine.QN_VERIFY_DST)
                        out.append((overlap.direction_kdtree(fin, dst, r), overlap.direction_kdtree(dst, fin, r)))
                    return out
                hs = host()                                  # (f64 distances: a count may differ by a point that sits on the radius in one precision only)
                assert all(abs(h[0]["inliers"] - o["a_to_b"]["inliers"]) <= 8 and abs(h[1]["inliers"] - o["b_to_a"]["inliers"]) <= 8 for h, o in zip(hs, recs))
                row["host_ckdtree_r%.1f" % r] = timed(host, 1, 3)
        print(json.dumps(row), flush=True)
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
