#!/usr/bin/env python
"""Time the static map (KeyframeStore.static_classify, build_map_static) against the plain map (build_map) and against the only route to the same votes
without it: freespace_batch over the count x W (entry, witness) pairs, freespace_points downloads of the entries' class bytes and host sums.

Setup of tools/gpu_freespace_time.py: ray-cast spinning-LiDAR keyframes (64 beams x 1800 columns, ~100k records each) of the street scene, poses = the ground
truth, leaf 0.3.  Sizes: S = 64 / --keyframes (512) keyframes, W = 4 / 10 witnesses per entry (the +-W/2 neighbours in the list).  The old route is cut into
calls of at most 32767 pairs (its cap) and its votes are checked against static_points on the first entries.  It does twice the projections (both directions
of every pair) plus count x W downloads, so the ratio is reported, not promised.
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=512)
    ap.add_argument("--old-reps", type=int, default=3, help="repetitions of the freespace_batch route (it is slow)")
    a = ap.parse_args()
    from qn_amd import engine, synth, staticmap, scancontext
    rng = np.random.Generator(np.random.PCG64(31))
    prims = synth.Scene(rng, 120.0).primitives()
    sen = synth.SpinningLidar()
    N, leaf = a.keyframes, 0.3
    poses = [synth.sensor_pose(30.0 + 15.0 * math.sin(2 * math.pi * i / 20), -24.0 + 0.4 * math.cos(0.3 * i), 0.3 * math.sin(0.7 * i)) for i in range(N)]
    store = engine.KeyframeStore()
    ids = []
    for s in range(0, N, 64):
        ids += [int(i) for i in store.add_lidar_scans(prims, sen, poses[s:s + 64], np.arange(s, min(s + 64, N)) + 1)]
    sizes = [store._sizes[i] for i in ids]
    store.range_set_params(engine.RangeParams.for_sensor(sen))
    store.range_describe(ids)
    for S in sorted({min(64, N), N}):
        for W in (4, 10):
            l_ids, l_poses = ids[:S], poses[:S]
            wit = staticmap.window_witnesses(l_ids, W // 2)
            t_cls = timed(lambda: store.static_classify(l_ids, l_poses, witnesses=wit), a.warmup, a.reps)
            res = store.static_classify(l_ids, l_poses, witnesses=wit)
            t_static = timed(lambda: store.build_map_static(leaf), a.warmup, a.reps)
            n_static = store.build_map_static(leaf)
            t_plain = timed(lambda: store.build_map(l_ids, l_poses, leaf), a.warmup, a.reps)
            n_plain = store.build_map(l_ids, l_poses, leaf)
            # the old route: entry e as the query, its witness as the candidate, T = inv(P_w) P_e; direction 0 of each pair is the vote
            off, w = wit
            pe = [e for e in range(S) for _ in range(int(off[e + 1] - off[e]))]; pw = [int(x) for x in w]
            T = [scancontext.relative_pose(l_poses[x], l_poses[e]) for e, x in zip(pe, pw)]

            def old(check=False):
                st = [np.zeros(sizes[e], np.uint8) for e in range(S)]; ag = [np.zeros(sizes[e], np.uint8) for e in range(S)]
                for c0 in range(0, len(pe), 32767):
                    c1 = min(c0 + 32767, len(pe))
                    store.freespace_batch([l_ids[e] for e in pe[c0:c1]], [l_ids[x] for x in pw[c0:c1]], T[c0:c1])
                    for j in range(c0, c1):
                        cls = store.freespace_points(j - c0, 0)
                        st[pe[j]] += cls == 2; ag[pe[j]] += cls == 4
                return st, ag
            t_old = timed(old, 0, a.old_reps)
            st, ag = old()
            store.static_classify(l_ids, l_poses, witnesses=wit)
            same = all(np.array_equal(store.static_points(e)[0], st[e]) and np.array_equal(store.static_points(e)[1], ag[e]) for e in range(min(S, 8)))
            print(json.dumps(dict(case="static_map", S=S, W=W, pairs=len(pe), records=int(sum(sizes[:S])), removed=int(res["removed"].sum()), classify=t_cls,
                                  build_map_static=t_static, build_map=t_plain, map_points=n_plain, static_map_points=n_static, freespace_route=t_old,
                                  route_over_classify=round(t_old["median_ms"] / t_cls["median_ms"], 2), same_votes=bool(same))), flush=True)
    store.close()


if __name__ == "__main__":
    main()
