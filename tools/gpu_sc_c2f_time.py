#!/usr/bin/env python
"""Time the resident Quatro descriptors (KeyframeStore.quatro_describe) and the coarse-to-fine check that borrows them
(KeyframeStore.verify_loop_candidates_c2f) against the uncached path on the same clouds: qn_kf_assemble_batch of the query and the K candidates,
each alone with the identity pose, then qn_coarse_to_fine_align_batch on one context (grids, normals, SPFH and FPFH rebuilt for every pair, the
query's shared across its candidates).

Keyframes: ray-cast spinning-LiDAR scans (synth.SpinningLidar, 32 beams x 720 columns) of the street scene along a 30 m stretch, put into the
store by add_lidar_scans; leaf 0.3, Quatro at the reference's parameters, NanoGICP as LoopClosure's ctor sets it (k 15, 32 iterations,
max_corr_dist 18, epsilon 0.01).  describe: S = 64 and 512 keyframes in one call.  verify: the query is the last keyframe, its candidates the K
older keyframes nearest to it (the last 8 excluded), K = 1, 4, 8, 16.  target_share = 1 - verify / uncached: the part of an uncached call
that describing the clouds once removes.  Every timed call ends in a host synchronisation; a host clock around it, median of --reps after
--warmup runs.  Prints one JSON line; needs a GPU (no fall-back)."""
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


def _ctx(engine):
    ctx = engine.Context(100000)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(18.0); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from qn_amd import engine, synth
    import torch
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    N, leaf = 512, 0.3
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 20), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(N) + 1)]
    ctx = _ctx(engine)
    props = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
    out = dict(gpu="%s (%s)" % (props.name, props.gcnArchName) if props is not None else "unknown", leaf=leaf, warmup=a.warmup, reps=a.reps,
               points_per_keyframe=int(np.mean([store._sizes[i] for i in ids])), describe={}, verify={})
    for S in (64, 512):
        st = store.quatro_describe(ctx, ids[:S], leaf)
        ms = timed(lambda: store.quatro_describe(ctx, ids[:S], leaf), a.warmup, a.reps)
        out["describe"]["S%d" % S] = dict(ms=round(ms, 3), us_per_keyframe=round(1e3 * ms / S, 2), described=sum(x == 0 for x in st),
                                          voxel_points_mean=int(np.mean([store.quatro_cloud(i)[1] for i in ids[:S]])))
    q = ids[-1]
    for K in (1, 4, 8, 16):
        near = sorted(range(N - 8), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))
        cand = [ids[i] for i in sorted(near[:K])]
        first = store.verify_loop_candidates_c2f(ctx, q, cand)
        cached = timed(lambda: store.verify_loop_candidates_c2f(ctx, q, cand), a.warmup, a.reps)

        def uncached():
            got = store.assemble_batch([[q]] + [[c] for c in cand], [[np.eye(4)]] + [[np.eye(4)] for _ in cand], leaf)
            (sp, ns, _), rest = got[0], got[1:]
            return engine.coarse_to_fine_align_batch([ctx], [(sp, ns, dp, nt, 16, 1) for dp, nt, _ in rest])
        base = uncached()
        assert [(r["status"], r["valid"], r["T"].tobytes()) for r in base] == [(r["status"], r["valid"], r["T"].tobytes()) for r in first]
        unc = timed(uncached, a.warmup, a.reps)
        out["verify"]["K%d" % K] = dict(cached_ms=round(cached, 3), uncached_ms=round(unc, 3), speedup=round(unc / cached, 2),
                                        target_share=round(1.0 - cached / unc, 3), valid=sum(r["valid"] for r in first))
    print(json.dumps(out))
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
