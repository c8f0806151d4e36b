#!/usr/bin/env python
"""Time the spinning-LiDAR ray-caster (qn_sim_lidar_to_store) and the registration paths on sensor-shaped clouds.

  * simulator: S = 1, 64, 512 default scans (64 x 1800 rays, the 81-primitive street scene) cast into a fresh keyframe store;
  * density: raw points per scan, points after the 0.3 m voxel grid, points per m^2 of ground-plane area in range annuli;
  * registration on make_lidar_pair pairs against make_pair (uniform) pairs of the same N: lone icp_alignment at the reference operating
    point (LM, k = 15), qn_icp_alignment_batch pairs/s (3 contexts x 8 lanes), Quatro align, qn_coarse_to_fine_align_batch pairs/s, and the
    qn_prof kernel-family ms per registration plus the k-NN search counters of the source covariances.
Every timed call ends in a stream synchronise; a host clock around it, median of --reps after --warmup runs.  Prints one JSON line; needs a
GPU (no fall-back)."""
import argparse
import ctypes as C
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


def poses_along(S, seed):
    from qn_amd import synth
    rng = np.random.default_rng(seed)
    return [synth.sensor_pose(*rng.uniform(-40, 40, 2), rng.uniform(-np.pi, np.pi)) for _ in range(S)]


def sim_times(engine, synth, prims, sen, warmup, reps):
    out = {}
    for S in (1, 64, 512):
        poses = poses_along(S, S); seeds = np.arange(S, dtype=np.uint32)
        stores = []

        def run():
            st = engine.KeyframeStore(); stores.append(st)
            t0 = time.perf_counter(); st.add_lidar_scans(prims, sen, poses, seeds); run.dt.append(time.perf_counter() - t0)
        run.dt = []
        for _ in range(warmup + reps):
            run()
            stores.pop().close()
        ms = 1e3 * float(np.median(run.dt[warmup:]))
        out["S%d" % S] = dict(ms=round(ms, 3), rays_per_s=S * sen.rays / (ms * 1e-3))
    return out


def density(synth, prims, sen, n_scans=8):
    raw, vox = [], []
    ann = [(2, 10), (10, 20), (20, 40), (40, 100)]
    cnt = np.zeros(len(ann))
    for P in poses_along(n_scans, 99):
        s = synth.lidar_scan(prims, sen, P, 3)
        raw.append(len(s)); vox.append(len(synth.voxel_centroids(s[:, :3].astype(np.float64), 0.3)))
        d = np.linalg.norm(s[:, :2].astype(np.float64), axis=1)
        cnt += [((d >= a) & (d < b)).sum() for a, b in ann]
    per_m2 = {"%d-%dm" % ab: float(c / n_scans / (np.pi * (ab[1] ** 2 - ab[0] ** 2))) for ab, c in zip(ann, cnt)}
    return dict(raw_points=float(np.mean(raw)), voxel_points=float(np.mean(vox)), points_per_m2=per_m2)


def make_ctx(engine, cap, lanes=1, k=15, optimizer="lm"):
    ctx = engine.Context(cap)
    if lanes > 1:
        ctx.debug_set("batch_lanes", lanes)
    p = engine.GicpParams(); engine.lib().qn_gicp_default_params(C.byref(p))
    p.k_correspondences = k; p.max_iterations = 32; p.max_corr_dist = 52.5; p.transformation_epsilon = 0.01; p.optimizer = 1 if optimizer == "gn" else 0
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(p)))
    engine.Quatro(ctx)
    return ctx


def registration(engine, synth, pairs, qpairs, warmup, reps):
    cap = max(max(len(s), len(t)) for s, t in pairs + qpairs) + 1024
    out = {}
    ctx = make_ctx(engine, cap)
    s, t = pairs[0]
    out["icp_alignment_ms"] = timed(lambda: engine.icp_alignment(ctx, s, t), warmup, reps)
    ctx.prof_enable(True); ctx.prof_reset()
    for s, t in pairs:
        engine.icp_alignment(ctx, s, t)
    ctx.synchronize()
    out["prof_ms_per_registration"] = {k: round(v[0] / len(pairs), 4) for k, v in ctx.prof_stats().items() if v[1]}
    ctx.prof_enable(False)
    g = engine.NanoGICP(ctx); g.setCorrespondenceRandomness(15)
    cnt = []
    for s, _ in pairs:
        g.setInputSource(s); ctx.debug_set("dbg_counters", 1); g.calculateSourceCovariances(); ctx.synchronize()
        c = (C.c_uint32 * 16)(); ctx.check(ctx._l.qn_debug_get_counters(ctx.h, c)); ctx.debug_set("dbg_counters", 0)
        cnt.append(list(c))
    c = np.sum(cnt, 0)
    out["knn_counters_per_cloud"] = dict(cluster_rounds=float(c[0]) / len(pairs), candidates=float(c[1]) / len(pairs),
                                         retried_lanes=float(c[3]) / len(pairs), list_pass_entries=float(c[4]) / len(pairs))
    q = engine.Quatro(ctx)
    s, t = qpairs[0]
    out["quatro_align_ms"] = timed(lambda: q.align(s, t), warmup, reps)
    ctx.close()
    ctxs = [make_ctx(engine, cap, lanes=8) for _ in range(3)]
    hp = [(s, len(s), t, len(t), 12, 0) for s, t in pairs]
    ms = timed(lambda: engine.icp_alignment_batch(ctxs, hp), warmup, reps)
    out["icp_alignment_batch_pairs_per_s"] = len(hp) / (ms * 1e-3)
    hq = [(s, len(s), t, len(t), 12, 0) for s, t in qpairs]
    ms = timed(lambda: engine.coarse_to_fine_align_batch(ctxs, hq), warmup, reps)
    out["coarse_to_fine_batch_pairs_per_s"] = len(hq) / (ms * 1e-3)
    for c in ctxs:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--skip-registration", action="store_true")
    a = ap.parse_args()
    from qn_amd import engine, synth
    prims = synth.Scene(np.random.Generator(np.random.PCG64(synth.BASE_SEED))).primitives()
    sen = synth.SpinningLidar()
    res = dict(n_prims=len(prims), rays_per_scan=sen.rays, sim=sim_times(engine, synth, prims, sen, a.warmup, a.reps), density=density(synth, prims, sen))
    if not a.skip_registration:
        lp = [synth.make_lidar_pair(i)[:2] for i in range(a.pairs)]
        lq = [synth.make_lidar_pair(100 + i, mode="quatro")[:2] for i in range(max(2, a.pairs // 3))]
        up = [synth.make_pair(i, len(s), len(t))[:2] for i, (s, t) in enumerate(lp)]
        uq = [synth.make_pair(100 + i, len(s), len(t), mode="quatro")[:2] for i, (s, t) in enumerate(lq)]
        res["n_src_tgt"] = [[len(s), len(t)] for s, t in lp]
        res["lidar"] = registration(engine, synth, lp, lq, a.warmup, a.reps)
        res["uniform"] = registration(engine, synth, up, uq, a.warmup, a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
