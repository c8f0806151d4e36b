#!/usr/bin/env python
"""Time the Scan Context loop-candidate calls (qn_kf_sc_describe / qn_kf_sc_query) on one GPU.

  * describe: 64 keyframes of 20k and of 100k points (uniform in a 160 m square, 8 m tall) per call -> ms per keyframe;
  * query: against 1k / 10k / 50k described keyframes (small ray-cast scans: 16 x 128 rays of the street scene), exhaustive and with the
    ring-key prefilter (P = 50): one query per call, and 64 queries in one call (ms per query), top_k = 10.
Every timed call returns after its own host synchronisation; a host clock around it, median of --reps after --warmup runs.  Prints one JSON
line; needs a GPU (no fall-back)."""
import argparse
import json
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


def describe_times(engine, warmup, reps):
    out = {}
    rng = np.random.default_rng(1)
    for n in (20000, 100000):
        st = engine.KeyframeStore()
        ids = [st.add(np.c_[rng.uniform(-80, 80, (n, 2)), rng.uniform(-2, 6, n)].astype(np.float32)) for _ in range(64)]
        flip = [0]

        def run():                                             # a parameter change discards the descriptors: every run describes all 64
            flip[0] ^= 1
            st.sc_set_params(lidar_height=2.0 + 0.5 * flip[0])
            st.sc_describe(ids)
        ms = timed(run, warmup, reps)
        out["n%d" % n] = dict(ms_per_call=round(ms, 3), ms_per_keyframe=round(ms / 64, 4), points_per_s=64 * n / (ms * 1e-3))
        st.close()
    return out


def query_times(engine, synth, warmup, reps):
    out = {}
    prims = synth.Scene(np.random.Generator(np.random.PCG64(5))).primitives()
    sen = synth.SpinningLidar(n_beams=16, n_cols=128)
    rng = np.random.default_rng(2)
    for N in (1000, 10000, 50000):
        st = engine.KeyframeStore()
        poses = [synth.sensor_pose(*rng.uniform(-40, 40, 2), rng.uniform(-np.pi, np.pi)) for _ in range(N)]
        ids = st.add_lidar_scans(prims, sen, poses, np.arange(N, dtype=np.uint32))
        t0 = time.perf_counter(); st.sc_describe(ids); t_desc = time.perf_counter() - t0
        stamps = np.arange(N) * 1.0
        row = dict(describe_all_ms=round(1e3 * t_desc, 2))
        for P in (0, 50):
            st.sc_set_params(ringkey_prefilter=P)
            one = timed(lambda: st.sc_query([N - 1], stamps, 10.0, 10), warmup, reps)
            many = timed(lambda: st.sc_query(list(range(N - 64, N)), stamps, 10.0, 10), warmup, reps)
            row["P%d" % P] = dict(one_query_ms=round(one, 3), q64_ms=round(many, 3), q64_ms_per_query=round(many / 64, 4))
        out["N%d" % N] = row
        st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from qn_amd import engine, synth
    res = dict(describe=describe_times(engine, a.warmup, a.reps), query=query_times(engine, synth, a.warmup, a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
