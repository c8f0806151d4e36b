#!/usr/bin/env python
"""Time the loop-closure submaps of one query and K candidates (setSrcAndDstCloud, loop_closure.cpp:58-108): qn_kf_assemble_batch (all
1 + K submaps in one call) next to a loop of 1 + K qn_kf_assemble calls over the same lists.  Every submap is 21 keyframes (submap_range 10)
of 20k points, leaf 0.3.  Both sides end in a stream synchronise (the batch call twice, each qn_kf_assemble twice), so a host clock around a
whole call / loop is its device time plus the launch and read-back gaps; the median over --reps after --warmup repetitions is reported, with
the C entry points called directly (argument arrays built once).  Prints one JSON line; needs a GPU (no fall-back)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))
import numpy as np


def scene(nkf, npts, seed=11):
    rng = np.random.default_rng(seed)
    xyz = [np.c_[rng.uniform(-30, 30, (npts, 2)), rng.uniform(-1.5, 3.5, npts)].astype(np.float32) for _ in range(nkf)]
    poses = []
    for k in range(nkf):
        a = 0.3 * np.sin(k / 60.0); T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; T[:3, 3] = [0.8 * k, 15.0 * np.sin(k / 50.0), 0.002 * k]
        poses.append(T)
    return xyz, poses


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--nkf", type=int, default=120)
    ap.add_argument("--npts", type=int, default=20000)
    ap.add_argument("--range", type=int, default=10)
    ap.add_argument("--leaf", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from qn_amd import engine
    xyz, poses = scene(a.nkf, a.npts)
    store = engine.KeyframeStore()
    for x in xyz:
        store.add(x)
    l = store._l; p = lambda v: v.ctypes.data_as(C.c_void_p)
    query = a.nkf - 1
    out = dict(metric="submap_batch_ms", nkf=a.nkf, npts=a.npts, submap_keyframes=2 * a.range + 1, leaf=a.leaf, timing="host clock around calls that end in a stream synchronise; median of %d" % a.reps, rows=[])
    for K in [int(k) for k in a.ks.split(",")]:
        centres = [query - a.range] + [a.range + (c * 7) % (a.nkf - 3 * a.range - 1) for c in range(K)]
        lists = [list(range(c - a.range, c + a.range + 1)) for c in centres]
        seg = np.zeros(len(lists) + 1, np.uint32); seg[1:] = np.cumsum([len(x) for x in lists])
        ids = np.ascontiguousarray(np.concatenate(lists), np.int32)
        T = np.ascontiguousarray([poses[i].reshape(16) for i in ids], np.float64)
        S = len(lists)
        ptrs = (C.c_void_p * S)(); n = np.zeros(S, np.uint32); st = np.zeros(S, np.int32)
        ptr1 = C.c_void_p(); n1 = C.c_uint32()

        def batch():
            assert l.qn_kf_assemble_batch(store.h, p(ids), p(T), p(seg), C.c_uint32(S), C.c_double(a.leaf), ptrs, p(n), p(st)) == 0

        loop_n = np.zeros(S, np.uint32)

        def loop():
            for s in range(S):
                a0 = int(seg[s])
                assert l.qn_kf_assemble(store.h, C.c_void_p(ids.ctypes.data + 4 * a0), C.c_void_p(T.ctypes.data + 128 * a0), C.c_uint32(len(lists[s])), C.c_double(a.leaf),
                                        C.c_int(s & 1), C.byref(ptr1), C.byref(n1)) == 0
                loop_n[s] = n1.value

        tb = timed(batch, a.warmup, a.reps)
        tl = timed(loop, a.warmup, a.reps)
        assert (st == 0).all() and np.array_equal(n, loop_n), "the batch and the loop disagree on the submap sizes"
        out["rows"].append(dict(K=K, submaps=S, input_points=int(S * (2 * a.range + 1) * a.npts), out_points=int(n.sum()),
                                batch_ms=round(tb[0], 3), batch_min_ms=round(tb[1], 3), loop_ms=round(tl[0], 3), loop_min_ms=round(tl[1], 3), speedup=round(tl[0] / tb[0], 2)))
    store.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
