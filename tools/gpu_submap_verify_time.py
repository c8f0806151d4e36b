#!/usr/bin/env python
"""Time the resident local submaps (KeyframeStore.submap_describe) and the submap-to-submap checks that borrow them (verify_loop_pairs_submap,
verify_loop_pairs_submap_c2f) against the only way to do the same thing without them: assemble_batch of the same windows (each distinct window once),
then gicp_align_batch(guesses=) / coarse_to_fine_align_batch on one context - the windows, and with Quatro every grid and FPFH row, rebuilt per call.
Both paths run from this script on the same store, so they see the same clouds; their records are compared bit for bit before anything is timed.

Keyframes: ray-cast spinning-LiDAR scans (32 beams x 720 columns) along a 30 m stretch of the street scene that is driven back and forth, submap_range 5,
leaf 0.3, NanoGICP as LoopClosure's ctor sets it (k 15, 32 iterations, max_corr_dist 18, epsilon 0.01), Quatro at the reference's parameters.
  verify:   the query is the last keyframe, its candidates the K older keyframes nearest to it (the last 16 excluded), K = 1, 4, 16; and a catch-up call of
            64 pairs (16 queries x 4 candidates).  (a) resident: the verify call alone, entries described beforehand; (c) baseline: assembly + batch.
  describe: (b) all distinct windows of the 64-pair call in one submap_describe, with and without rows, per keyframe.
Every timed call ends in a host synchronisation; a host clock around it; --warmup untimed runs, then --reps runs alternating (a) and (c); the median and
the min .. max spread of each are reported.  Prints one JSON line; needs a GPU (no fall-back)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))
import numpy as np


def timed_ab(fns, warmup, reps):
    """alternate the functions; -> per function (median ms, min ms, max ms)"""
    for _ in range(warmup):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t0 = time.perf_counter(); f(); t.append(1e3 * (time.perf_counter() - t0))
    return [(round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)) for t in ts]


def _ctx(engine, cap):
    ctx = engine.Context(cap)
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(18.0); g.setTransformationEpsilon(0.01); g.bind()
    engine.Quatro(ctx)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=160)
    ap.add_argument("--skip-c2f", action="store_true")
    a = ap.parse_args()
    from qn_amd import engine, synth, scancontext as sc
    import torch
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    N, leaf, R = a.keyframes, 0.3, 5
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 80), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = [int(i) for i in store.add_lidar_scans(prims, sen, poses, np.arange(N) + 1)]
    ctx = _ctx(engine, 200000)
    props = torch.cuda.get_device_properties(0) if torch.cuda.is_available() else None
    out = dict(gpu="%s (%s)" % (props.name, props.gcnArchName) if props is not None else "unknown", leaf=leaf, submap_range=R, warmup=a.warmup, reps=a.reps,
               keyframes=N, points_per_keyframe=int(np.mean([store._sizes[i] for i in ids])), verify={}, describe={})

    def nearest(q, K, taken=()):
        near = sorted((i for i in range(N - 16) if abs(i - q) > 2 * R and i not in taken), key=lambda i: (np.linalg.norm(poses[i][:2, 3] - poses[q][:2, 3]), i))
        return sorted(near[:K])
    cases = {"K%d" % K: ([N - 1] * K, nearest(N - 1, K)) for K in (1, 4, 16)}
    qs64 = list(range(N - 16, N))
    cases["catchup64"] = ([q for q in qs64 for _ in range(4)], [c for q in qs64 for c in nearest(q, 4)])
    for name, (qs, cs) in cases.items():
        yaws = [math.atan2(poses[c][1, 0], poses[c][0, 0]) - math.atan2(poses[q][1, 0], poses[q][0, 0]) for q, c in zip(qs, cs)]
        used = list(dict.fromkeys(qs + cs))
        lists = [engine.local_submap_ids(x, R, N) for x in used]
        rels = [[sc.relative_pose(poses[x], poses[i]) for i in l] for x, l in zip(used, lists)]
        for form in ("gicp",) if a.skip_c2f else ("gicp", "c2f"):
            st = store.submap_describe(ctx, used, poses, R, leaf, with_features=form == "c2f")
            assert st == [0] * len(used), st
            npts = [store.submap_cloud(x)[1] for x in used]

            def resident():
                if form == "gicp":
                    return store.verify_loop_pairs_submap(ctx, qs, cs, yaws)
                return store.verify_loop_pairs_submap_c2f(ctx, qs, cs)

            def baseline():
                got = store.assemble_batch(lists, rels, leaf)
                at = {x: g for x, g in zip(used, got)}
                descs = [(at[q][0], at[q][1], at[c][0], at[c][1], 16, 1) for q, c in sorted(zip(qs, cs), key=lambda p: used.index(p[0]))]
                if form == "gicp":
                    order = sorted(range(len(qs)), key=lambda j: used.index(qs[j]))
                    return engine.gicp_align_batch(ctx, descs, guesses=[sc.seed_from_yaw(yaws[j]) for j in order])
                return engine.coarse_to_fine_align_batch([ctx], descs)
            first, base = resident(), baseline()
            order = sorted(range(len(qs)), key=lambda j: used.index(qs[j]))
            if form == "gicp":
                same = all(np.array_equal(np.array(first[j]["record"].T64), np.array(base[0][k].T64)) and int(first[j]["valid"]) == base[1][k] for k, j in enumerate(order))
            else:
                same = all(first[j]["T"].tobytes() == base[k]["T"].tobytes() and first[j]["valid"] == base[k]["valid"] for k, j in enumerate(order))
            assert same, (name, form)
            (r_med, r_lo, r_hi), (b_med, b_lo, b_hi) = timed_ab([resident, baseline], a.warmup, a.reps)
            out["verify"]["%s_%s" % (name, form)] = dict(pairs=len(qs), windows=len(used), points_per_window=int(np.mean(npts)), resident_ms=r_med, resident_range=[r_lo, r_hi],
                                                         baseline_ms=b_med, baseline_range=[b_lo, b_hi], speedup=round(b_med / r_med, 2), valid=sum(bool(r["valid"]) for r in first))
    qs, cs = cases["catchup64"]
    used = list(dict.fromkeys(qs + cs))
    for feat in (False,) if a.skip_c2f else (False, True):
        (med, lo, hi), = timed_ab([lambda: store.submap_describe(ctx, used, poses, R, leaf, with_features=feat)], a.warmup, a.reps)
        npts = [store.submap_cloud(x)[1] for x in used]
        out["describe"]["rows" if feat else "cloud_only"] = dict(windows=len(used), ms=med, range=[lo, hi], us_per_keyframe=round(1e3 * med / len(used), 1),
                                                                  points_per_window=int(np.mean(npts)), resident_bytes_per_keyframe=int(np.mean(npts) * (24 + (144 if feat else 0))))
    print(json.dumps(out))
    ctx.close(); store.close()


if __name__ == "__main__":
    main()
