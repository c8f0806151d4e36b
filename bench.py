#!/usr/bin/env python
"""bench.py - scan-pair registrations/s on synthetic 100k-point clouds (BASELINE.json metric).

A "step" is ONE full Nano-GICP scan-pair registration = LoopClosure::icpAlignment
(fast_lio_sam_qn/src/loop_closure.cpp:110-136): setInputSource + calculateSourceCovariances +
setInputTarget + calculateTargetCovariances + align + getFitnessScore, on BASELINE.json
configs[1]: 100k x 100k points, k = 20 covariances, 20 forced Gauss-Newton iterations.
The raw clouds are resident in HBM when the timed region starts (device-pointer entry points).

`--gpus N`: one process per GPU.  Launched by torchrun (RANK / WORLD_SIZE in the environment) the script is one rank; launched
plainly with N > 1 it starts the N ranks itself (and refuses when fewer than N GPUs are visible - there is no GPU sharing and no
CPU fallback).  Candidate pairs are sharded pair i -> rank i mod N with no data-path collective (independent registrations); one
RCCL all_gather of the fixed-size best-result records at the end lets rank 0 pick the winning loop.  Weak
scaling: every rank runs K steps.  The same line also carries BASELINE configs[3] literally (`batch64`: 64 distinct pairs sharded
over the ranks through qn_multi_align_best + the gather), the reference's operating point (configs[0], `reference_operating_point`)
and the Quatro stage (configs[2], `quatro`).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))

import numpy as np
import torch

N_PTS, K_COV, GN_ITERS = 100000, 20, 20
C2F_TRUE_LOOP_SCENES = (402, 403, 404, 409, 410, 412, 419, 420)      # synth.make_pair(id, 30000, mode="quatro") ids on which the coarse-to-fine ORACLE registers the pair (clique 11-33, 2 LM iterations)
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md); 6290 GB/s measured-achievable
FP32_VALU_PEAK_TF = 157.3    # f32 vector peak with FMA (MI355X_MICROARCH.md); 78.6 without FMA contraction
MFMA_F16_PEAK_TF = 2500.0    # dense f16 / bf16 matrix-core peak (MI355X_MICROARCH.md)


def algorithmic_bytes(n=N_PTS, k=K_COV, it=GN_ITERS):
    """SURVEY.md 8(d) accounting, compact fp32 layouts (point 16 B, covariance 24 B)."""
    return {
        "grid_build": 36 * n,                       # per cloud
        "knn_cov": n * (16 + 16 * k + 24),          # per cloud
        "gn_iteration": 80 * n,                     # NN search + accumulate of one iteration
        "lm_error_pass": 56 * n,
        "fitness": 32 * n,
        "transform": 32 * n,
        "align": 80 * it * n + 32 * n,
        "full": 36 * 2 * n + (40 + 16 * k) * 2 * n + 80 * it * n + 64 * n,
    }


def profile_stale(stored_sha):
    """True when a stored profile (profiles/pmc_latest.json, profiles/valu_budget_latest.json) was NOT collected on the kernel sources of this tree (or carries no tag)"""
    try:
        from qn_amd.build import csrc_sha1
        return not (stored_sha and stored_sha == csrc_sha1())
    except Exception:
        return True


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, prefix=""):
    """--dump-outputs: write what the timed block returned, one row per timed step (row -1 = the last step), as <out_dir>/<prefix><name>.npy in
    float32 / float64.  Past DUMP_MAX_BYTES in all, a fixed, seeded sample of the rows is kept (the last step always among them); `step_index` names the rows."""
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    n = len(next(iter(arrays.values())))
    row_bytes = sum(v.nbytes // max(n, 1) for v in arrays.values()) + 8
    keep = np.arange(n)
    if n * row_bytes > DUMP_MAX_BYTES:
        m = max(1, DUMP_MAX_BYTES // row_bytes)
        keep = np.union1d(np.random.default_rng(0).choice(n - 1, size=m - 1, replace=False), [n - 1])
    arrays = {k: v[keep] for k, v in arrays.items()}
    arrays["step_index"] = keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
        np.save(os.path.join(out_dir, prefix + k + ".npy"), v)


def gicp_result_arrays(results, valid, status):
    """the GicpResult records of engine.icp_alignment_batch as arrays (integers as float64)"""
    return {"T": np.array([list(r.T) for r in results], dtype=np.float32).reshape(-1, 4, 4),
            "T64": np.array([list(r.T64) for r in results], dtype=np.float64).reshape(-1, 4, 4),
            "H": np.array([list(r.H) for r in results], dtype=np.float64).reshape(-1, 6, 6),
            "fitness": np.array([r.fitness for r in results], dtype=np.float64),
            "iterations": np.array([r.iterations for r in results], dtype=np.float64),
            "converged": np.array([r.converged for r in results], dtype=np.float64),
            "lm_failed": np.array([r.lm_failed for r in results], dtype=np.float64),
            "valid": np.array(valid, dtype=np.float64), "status": np.array(status, dtype=np.float64)}


def pct(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    return {"median": round(float(np.median(xs)), 4), "p10": round(float(np.percentile(xs, 10)), 4), "p90": round(float(np.percentile(xs, 90)), 4), "n": int(len(xs))}


def whole_registration(ms_step):
    ab = algorithmic_bytes()
    if not ms_step:
        return None
    return {"algorithmic_bytes": ab["full"], "achieved": round(ab["full"] / (ms_step * 1e-3) / 1e9, 2), "frac": round(ab["full"] / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
            "note": "amortised over the registrations in flight"}


def roofline_leg(ctx, register, ms_step, align_ms, nprof=4):
    """per-kernel-family device time from hipEvents on the engine's own stream (qn_prof_*), the `roofline` object of the dominant single-kernel family"""
    ctx.prof_reset(); ctx.prof_enable(True)
    for j in range(nprof):
        register(j)
    ctx.synchronize(); ctx.prof_enable(False)
    stats = ctx.prof_stats()
    fam_ms = {k: v[0] / nprof for k, v in stats.items() if v[1] > 0}             # ms per registration
    fam_avg = {k: v[0] / v[1] for k, v in stats.items() if v[1] > 0}             # ms per profiled span (= one launch for the single-kernel families)
    ab = algorithmic_bytes()
    # kernel families timed as ONE kernel per span, with the rocprofv3 name of that kernel and its algorithmic bytes per launch
    single_k = {"knn_select": ("k_knn_hist<false, 32>", N_PTS * (16 + 16 * K_COV)),          # k-NN selection of one cloud: point + k neighbour points
                "gn_tick_fused": ("k_tick<512, 4, 0, false>", ab["gn_iteration"]),                # one whole GN / LM tick (controller + tracked NN + accumulate)
                "nn_search": ("k_nn_search<0, false, 256>", ab["gn_iteration"]),                # first (unseeded) NN passes of an align
                "nn_fallback": ("k_nn_search<0, true, 256>", ab["gn_iteration"]),
                "accumulate": ("k_accumulate", ab["gn_iteration"]), "solve": ("k_solve<512>", 28 * 8 * 512)}
    dom = max((k for k in fam_ms if k in single_k), key=fam_ms.get)
    dom_kernel, per_launch_bytes = single_k[dom]
    dom_ms = fam_avg[dom]
    achieved = per_launch_bytes / (dom_ms * 1e-3) / 1e9
    pmc, pmc_all = None, None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    if os.path.exists(pmc_path):
        try:
            pmc_all = json.load(open(pmc_path)); pmc = pmc_all.get(dom)
        except Exception:
            pmc = None
    traffic = pmc.get("hbm_bytes_per_launch") if isinstance(pmc, dict) else None
    kernels = {k: {"kernel": single_k[k][0], "avg_launch_ms": round(fam_avg[k], 5), "launches_per_registration": round(stats[k][1] / nprof, 2),
                   "algorithmic_bytes_per_launch": single_k[k][1], "achieved_GBs": round(single_k[k][1] / (fam_avg[k] * 1e-3) / 1e9, 2),
                   "frac": round(single_k[k][1] / (fam_avg[k] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                   "traffic": (pmc_all or {}).get(k, {}).get("hbm_bytes_per_launch") if isinstance(pmc_all, dict) else None} for k in single_k if k in fam_avg}
    roofline = {"bound": "hbm", "kernel": dom_kernel, "family": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                "traffic_source": "NOT measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same workload (tools/gpu_round.sh <tag> pmc), stored in profiles/pmc_latest.json",
                "stale_from": (pmc_all or {}).get("_meta", {}).get("tag", "profiles/pmc_latest.json") if isinstance(pmc_all, dict) else None,
                "traffic_detail": pmc, "avg_launch_ms": round(dom_ms, 5), "algorithmic_bytes_per_launch": per_launch_bytes,
                "whole_registration": whole_registration(ms_step),
                "align_only": {"algorithmic_bytes": ab["align"], "ms": round(align_ms, 4),
                               "frac": round(ab["align"] / (align_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)},
                "family_ms_per_registration": {k: round(v, 4) for k, v in fam_ms.items()}, "kernels": kernels,
                "note": "working set (<=20 MB) is L2/MALL resident: nominal HBM yardstick (SURVEY 8d)"}
    return roofline


def batched_roofline_leg(engine, ctx, pairs, lanes, rounds=3):
    """The path `value` runs: qn_gicp_align_batch on ONE context, `lanes` registrations per kernel launch (k_lanes<F>, the pair as a grid dimension).  hipEvents around every
    batched launch on the context's own stream (qn_prof_*; a family's `launches` count the registrations a launch carried, so total / launches = the per-registration share of a launch);
    measured with nothing else on the GPU, so the durations are the kernels' own."""
    descs = [(pairs[j % len(pairs)][0].data_ptr(), N_PTS, pairs[j % len(pairs)][1].data_ptr(), N_PTS, 12, 1) for j in range(lanes)]
    engine.gicp_align_batch(ctx, descs)
    ctx.prof_reset(); ctx.prof_enable(True)
    for _ in range(rounds):
        _, _, st = engine.gicp_align_batch(ctx, descs)
        assert all(x == 0 for x in st), st
    ctx.synchronize(); ctx.prof_enable(False)
    stats = ctx.prof_stats(); nreg = rounds * lanes
    fam_ms = {k: v[0] / nreg for k, v in stats.items() if v[1] > 0}             # ms per registration (amortised over the lanes)
    fam_avg = {k: v[0] / v[1] for k, v in stats.items() if v[1] > 0}            # ms per registration-launch = batched launch duration / lanes
    ab = algorithmic_bytes()
    single_k = {"knn_select": ("k_lanes<KnnHistK<false, 32, true>>", N_PTS * (16 + 16 * K_COV)),
                "gn_tick_fused": ("k_lanes<TickK<512, 4, 0, false>>", ab["gn_iteration"]),
                "nn_search": ("k_lanes<NnLaneK<0>>", ab["gn_iteration"]),
                "nn_fallback": ("k_lanes<NnSearchK<0, true, 256, true>>", ab["gn_iteration"]),
                "accumulate": ("k_lanes<AccumulateK>", ab["gn_iteration"])}
    dom = max((k for k in fam_ms if k in single_k), key=fam_ms.get)
    dom_kernel, per_launch_bytes = single_k[dom]
    pmc_all = None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    if os.path.exists(pmc_path):
        try:
            pmc_all = json.load(open(pmc_path))
        except Exception:
            pmc_all = None
    def traffic_of(k):
        e = (pmc_all or {}).get("batched", {}).get(k) if isinstance(pmc_all, dict) else None
        return e.get("hbm_bytes_per_registration_launch") if isinstance(e, dict) else None
    per_lane = {"knn_select": 2}                                                 # table entries a lane contributes to one launch: the k-NN selection carries the source AND the target cloud of every lane
    kernels = {k: {"kernel": single_k[k][0], "avg_launch_ms_per_entry": round(fam_avg[k], 6), "entries_per_launch": per_lane.get(k, 1) * lanes,
                   "entry": "one cloud" if per_lane.get(k, 1) == 2 else "one registration", "avg_batched_launch_ms": round(fam_avg[k] * lanes * per_lane.get(k, 1), 5),
                   "launches_per_registration": round(stats[k][1] / nreg, 2), "algorithmic_bytes_per_registration_launch": single_k[k][1],
                   "achieved_GBs": round(single_k[k][1] / (fam_avg[k] * 1e-3) / 1e9, 2), "frac": round(single_k[k][1] / (fam_avg[k] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                   "traffic": traffic_of(k)} for k in single_k if k in fam_avg}
    achieved = per_launch_bytes / (fam_avg[dom] * 1e-3) / 1e9
    total_ms = sum(fam_ms.values())
    return {"bound": "hbm", "kernel": dom_kernel, "family": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
            "traffic": traffic_of(dom),
            "traffic_source": "NOT measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same batched workload (tools/gpu_round4.sh <tag> pmc -> profiles/pmc_latest.json, build named in stale_from); null = not collected",
            "stale_from": (pmc_all or {}).get("_meta", {}).get("tag") if isinstance(pmc_all, dict) else None,
            "traffic_stale": profile_stale((pmc_all or {}).get("_meta", {}).get("csrc_sha1") if isinstance(pmc_all, dict) else None),      # the stored PMC passes were collected on other kernel sources than this tree's
            "lanes": lanes, "registrations_profiled": nreg,
            "avg_batched_launch_ms": round(fam_avg[dom] * lanes * per_lane.get(dom, 1), 5), "avg_launch_ms_per_entry": round(fam_avg[dom], 6), "algorithmic_bytes_per_launch": per_launch_bytes * lanes * per_lane.get(dom, 1),
            "family_ms_per_registration": {k: round(v, 4) for k, v in fam_ms.items()}, "kernel_ms_per_registration_one_context": round(total_ms, 4),
            "kernels": kernels,
            "path": "qn_gicp_align_batch on one context alone on the GPU: hipEvents around every k_lanes launch on the context's stream; every feature of the measured path is on "
                    "(the batched path has no second stream and no persistent kernel to switch off)",
            "note": "working set of a batch (lanes x ~30 MB) is MALL/L2 resident: nominal HBM yardstick (SURVEY 8d); the engine is VALU-issue / latency bound - see valu_issue"}


def shim_latency(synth, reps=12):
    """ms per icpAlignment / coarseToFineAlignment call of the compiled shim programs (their own process, their own contexts), 30k and 100k points"""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_shim
    if not (os.path.exists(test_shim.BIN) and os.path.exists(test_shim.BIN2)):
        test_shim.build_shim_program()
    out = {"note": "wall time inside the C++ process around the reference's call sequence, median of %d calls after one warm-up call; host buffers of pcl::PointXYZI (32 B / point)" % reps}
    with tempfile.TemporaryDirectory() as td:
        for npts in (30000, N_PTS):
            e = {}
            s_, t_, _ = synth.make_pair(700 + npts // 1000, npts)
            a, b = os.path.join(td, "s.bin"), os.path.join(td, "t.bin"); s_.tofile(a); t_.tofile(b)
            o = subprocess.check_output([test_shim.BIN, a, b, "s", str(reps)], stderr=subprocess.DEVNULL).decode().split("BENCH")
            e["icpAlignment_ms"] = float(o[1].split()[1]); e["icpAlignment_min_ms"] = float(o[1].split()[2]); e["icpAlignment_valid"] = bool(int(o[0].split()[0]))
            qs, qt, _ = synth.make_pair(C2F_TRUE_LOOP_SCENES[0], npts, mode="quatro")
            qs.tofile(a); qt.tofile(b)
            o = subprocess.check_output([test_shim.BIN2, a, b, str(max(3, reps // 2))], stderr=subprocess.DEVNULL).decode().split("BENCH")
            e["coarseToFine_ms"] = float(o[1].split()[1]); e["coarseToFine_min_ms"] = float(o[1].split()[2]); e["coarseToFine_valid"] = bool(int(o[0].split()[0]))
            out["%dk" % (npts // 1000)] = e
    return out


def spawn_ranks(args):
    """plain `python bench.py --gpus N`: start the N ranks (one process per GPU) and relay rank 0's JSON line."""
    n = args.gpus
    backend = os.environ.get("QN_BENCH_BACKEND", "nccl")
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if backend == "nccl" and have < n:
        raise SystemExit("bench.py --gpus %d needs %d GPUs, %d visible: refusing to run fewer ranks or to share a GPU (QN_BENCH_BACKEND=gloo is the 1-GPU plumbing test)" % (n, n, have))
    if have < 1:
        raise SystemExit("bench.py needs a GPU: the engine has no CPU fallback")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out.decode()); sys.stdout.flush()
    if any(rcs):
        raise SystemExit("bench.py: rank exit codes %s" % rcs)


def latency_legs(engine, synth, pairs, args, world, ctx=None, p80=None):
    """One registration at a time (the reference's deployment: ONE candidate pair per 2 Hz timer tick, fast_lio_sam_qn.cpp:213-219): single-stream latency,
    PCIe-inclusive latency, align()-only, the per-kernel roofline leg, the CPU baseline, the parity spot check, the 80 %-overlap pairs, the reference's
    operating point and the Quatro stage - on the first of the in-flight contexts, after the throughput legs.  (The latency depends on the PAIR far more than
    on anything else: a 10-degree initial yaw error costs 0.3 ms more than a 1-degree one, tools/gpu_probe_pairs.py; medians are over 8 distinct pairs.)"""
    own = ctx is None
    if own:
        ctx = engine.Context(N_PTS + 1024, device=torch.cuda.current_device())
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(K_COV); g.setMaximumIterations(GN_ITERS); g.setMaxCorrespondenceDistance(52.5)
    g.setOptimizer("gn"); g.setForceIterations(GN_ITERS)

    def register(j):
        s, t, _ = pairs[j % len(pairs)]
        g.setInputSourceDevice(s.data_ptr(), N_PTS, 12); g.calculateSourceCovariances()
        g.setInputTargetDevice(t.data_ptr(), N_PTS, 12); g.calculateTargetCovariances()
        return g.align()

    # ---- one registration at a time on one stream (latency view): median / p10 / p90 over distinct pairs
    for j in range(2):
        register(j)
    lat = []
    for j in range(30):
        tl = time.perf_counter(); register(j); lat.append(1e3 * (time.perf_counter() - tl))
    single = pct(lat)
    # ---- PCIe-inclusive view: the same registration with the clouds handed over as HOST buffers (never `value`)
    s_host, t_host = pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy()
    def register_host():
        g.setInputSource(s_host); g.calculateSourceCovariances()
        g.setInputTarget(t_host); g.calculateTargetCovariances()
        return g.align()
    register_host()
    lat = []
    for _ in range(10):
        th = time.perf_counter(); register_host(); lat.append(1e3 * (time.perf_counter() - th))
    host = pct(lat)
    # ---- align-only timing (clouds + covariances resident): BASELINE's "ms/align"
    register(0); ctx.synchronize(); torch.cuda.synchronize()
    lat = []
    for _ in range(max(30, args.steps // 4)):
        ta = time.perf_counter(); g.align(); lat.append(1e3 * (time.perf_counter() - ta))
    align = pct(lat); align_ms = align["median"]

    roofline = roofline_leg(ctx, register, None, align_ms)
    # ---- the persistent align kernel (the tracked ticks + closing pass of ONE align in one launch; single registrations only): hipEvent time per launch,
    # ticks per launch from the forced iteration count, algorithmic bytes = 80 N per tick + 64 N for the closing pass
    try:
        ctx.debug_set("prof_persist", 1); ctx.prof_reset(); ctx.prof_enable(True)
        for j in range(8):
            register(j)
        ctx.synchronize(); ctx.prof_enable(False); ctx.debug_set("prof_persist", 0)
        ps = ctx.prof_stats().get("align_persist", (0.0, 0))
        if ps[1] > 0:
            ms_l = ps[0] / ps[1]; ticks = GN_ITERS - 2.5        # hand-over after 2 or 3 unseeded iterations (adaptive), the rest in the launch
            pb = ab_bytes = 80 * N_PTS * ticks + 64 * N_PTS
            roofline["persistent_align"] = {"kernel": "k_align_persist<512, false>", "launches": int(ps[1]), "avg_launch_ms": round(ms_l, 5), "ticks_per_launch": ticks,
                                            "us_per_tick": round(1e3 * ms_l / (ticks + 1), 2), "algorithmic_bytes_per_launch": int(pb), "achieved_GBs": round(pb / (ms_l * 1e-3) / 1e9, 2),
                                            "frac": round(pb / (ms_l * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                                            "traffic": (json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json"))).get("align_persist", {}).get("hbm_bytes_per_launch") if os.path.exists(os.path.join(ROOT, "profiles", "pmc_latest.json")) else None)}
    except Exception as ex:
        roofline["persistent_align"] = {"error": repr(ex)}

    cpu = None
    if world == 1 and not args.no_cpu_baseline:
        from oracle import oracle as orc                      # CPU baseline leg only
        s_np, t_np = pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy()
        nthreads = orc.num_threads()
        def cpu_once():
            o = orc.GicpOracle(k=K_COV, max_iter=GN_ITERS, max_corr_dist=52.5, optimizer="gn", force_iterations=GN_ITERS)
            o.set_source(s_np); o.compute_covariances(0); o.set_target(t_np); o.compute_covariances(1)
            return o.align()
        tc = time.perf_counter(); ro = cpu_once(); first = time.perf_counter() - tc
        nrep = max(1, min(8, int(15.0 / max(first, 1e-3))))
        times = []
        for _ in range(nrep):
            tc = time.perf_counter(); cpu_once(); times.append(time.perf_counter() - tc)
        cpu_s = float(np.median(times))
        cpu = {"value": round(1.0 / cpu_s, 4), "unit": "registrations/s", "cores": nthreads, "kind": "port",
               "ms_per_registration": round(cpu_s * 1e3, 2), "ms_range": [round(1e3 * min(times), 2), round(1e3 * max(times), 2)],
               "sample": "%d full registrations of pair 0 (100k x 100k, k=20, 20 GN iterations) with the OpenMP C++ oracle; shared host, wall time varies run to run" % nrep}
        # parity spot check of the benched workload against the oracle: pair 0, the bench's own parameters re-bound to the context
        # (other NanoGICP objects may have used it), BEFORE any extra runs
        g.bind(); r = register(0)
        Tg = np.array(r.T64).reshape(4, 4)
        dtp = float(np.abs(Tg - ro["T"]).max()); dt_m, dr_rad = synth.pose_error(Tg, ro["T"])
        out_oracle = (ro["T"].tolist(), float(ro["fitness"]), int(ro["iterations"]))
        parity = {"pair": 0, "max_abs_T_diff": dtp, "dt_m": dt_m, "dr_rad": dr_rad, "iterations": [int(r.iterations), int(ro["iterations"])],
                  "score_rel_diff": abs(r.fitness - ro["fitness"]) / max(ro["fitness"], 1e-300), "ok": bool(dtp <= 1e-9 and r.iterations == ro["iterations"])}
    else:
        dtp, parity, out_oracle = None, None, (None, None, None)
    out = {"oracle_T": out_oracle[0], "oracle_fitness": out_oracle[1], "oracle_iterations": out_oracle[2], "single": single, "host": host, "align": align, "roofline": roofline, "cpu": cpu, "dtp": dtp, "parity": parity,
           "persistent_align_launches": int(ctx.debug_get("persist_launches")), "alone_in_process": bool(own)}
    if p80:
        # ---- SURVEY 8d's generator case (80 % overlap), one registration at a time: percentiles over 8 distinct pairs + kernel-family breakdown
        g.bind()
        def register80(j):
            s_, t_, _ = p80[j % len(p80)]
            g.setInputSourceDevice(s_.data_ptr(), N_PTS, 12); g.calculateSourceCovariances()
            g.setInputTargetDevice(t_.data_ptr(), N_PTS, 12); g.calculateTargetCovariances()
            return g.align()
        register80(0); register80(1); lat = []
        for j in range(24):
            tl = time.perf_counter(); register80(j); lat.append(1e3 * (time.perf_counter() - tl))
        out["overlap80_single"] = pct(lat)
        register80(0); ctx.synchronize(); lat = []
        for _ in range(20):
            ta = time.perf_counter(); g.align(); lat.append(1e3 * (time.perf_counter() - ta))
        out["overlap80_align"] = pct(lat)
        ctx.prof_reset(); ctx.prof_enable(True)
        for j in range(4):
            register80(j)
        ctx.synchronize(); ctx.prof_enable(False)
        st8 = ctx.prof_stats()
        out["overlap80_family_ms"] = {k: round(v[0] / 4, 4) for k, v in st8.items() if v[1] > 0}
    if not args.no_extras:
        # ---- BASELINE configs[0]: the reference's operating point: k = 15, LM, <= 32 iterations, real stopping rule,
        # clouds handed over as HOST buffers through qn_icp_alignment (PCIe inclusive), 30k and 100k points; CPU oracle beside it
        try:
            rop = {}
            for npts in (30000, N_PTS):
                sr, tr_, _ = synth.make_pair(700 + npts // 1000, npts)
                engine.icp_alignment(ctx, sr, tr_)
                lat = []
                for _ in range(15):
                    tq = time.perf_counter(); rr = engine.icp_alignment(ctx, sr, tr_); lat.append(1e3 * (time.perf_counter() - tq))
                e = {"gpu_ms_from_host_buffers": pct(lat), "iterations": rr["iterations"], "converged": rr["converged"], "score": rr["score"]}
                if not args.no_cpu_baseline:
                    from oracle import oracle as orc
                    tc = time.perf_counter(); ro2 = orc.icp_alignment(sr, tr_); c1 = time.perf_counter() - tc
                    reps = max(1, min(5, int(4.0 / max(c1, 1e-3)))); tc = time.perf_counter()
                    for _ in range(reps):
                        orc.icp_alignment(sr, tr_)
                    e["cpu_oracle_ms"] = round(1e3 * (time.perf_counter() - tc) / reps, 2); e["cpu_threads"] = orc.num_threads()
                    e["same_iterations_as_oracle"] = bool(ro2["iterations"] == rr["iterations"])
                    e["dT_vs_oracle_m_rad"] = list(synth.pose_error(rr["T"], ro2["T"]))
                rop["%dk" % (npts // 1000)] = e
            out["rop"] = {"config": "k=15, LM, max 32 iterations, eps_t 0.01, eps_r 2e-3, max_corr_dist 52.5 m, score thr 1.5 (SURVEY App. C)", **rop}
        except Exception as ex:
            out["rop"] = {"error": repr(ex)}
    # ---- Quatro coarse stage (BASELINE configs[2]): FPFH + optimizedMatching (cap 200) + GNC solve, 30k and 100k pairs from the host
    quatro = None
    if world == 1 and not args.no_quatro and not args.no_extras:
        try:
            from scipy.spatial import cKDTree
            quatro = {}
            for npts in (30000, N_PTS):
                qs, qt, _ = synth.make_pair(400 + npts // 1000, npts, mode="quatro")
                q = engine.Quatro(ctx)
                q.align(qs, qt)
                lat = []
                for _ in range(5):
                    tq = time.perf_counter(); Tq, qvalid = q.align(qs, qt); lat.append(1e3 * (time.perf_counter() - tq))
                host_wall = {"uploads_grids_enqueue": round(ctx.debug_get("quatro_wall_features_ms"), 3), "fpfh_wait_matching_tail": round(ctx.debug_get("quatro_wall_match_ms"), 3),
                             "clique_gnc_solve": round(ctx.debug_get("quatro_wall_solve_ms"), 3)}          # of the last timed align (before the profiled one)
                n_surv, n_fb = int(ctx.debug_get("feat_survivors")), int(ctx.debug_get("feat_fallbacks"))
                ctx.prof_reset(); ctx.prof_enable(True); q.align(qs, qt); ctx.synchronize(); ctx.prof_enable(False)
                st = ctx.prof_stats()
                stage = {k: round(st[k][0], 4) for k in ("grid_build", "fpfh_normals", "fpfh_spfh", "fpfh_fpfh", "feat_match", "match_tail") if st[k][1] > 0}
                tree = cKDTree(qs.astype(np.float64)); sel = np.random.default_rng(0).choice(len(qs), 4000, replace=False)
                m_n = float(np.mean(tree.query_ball_point(qs[sel].astype(np.float64), 0.9, return_length=True)))
                m_f = float(np.mean(tree.query_ball_point(qs[sel].astype(np.float64), 1.5, return_length=True)))
                ab_q = {"normals": npts * (16 + 16 * m_n + 12), "spfh": npts * (28 + 28 * m_f + 132), "fpfh": npts * (136 * m_f + 132)}     # per cloud, SURVEY 8d
                fm_ms = stage.get("feat_match", 0.0)
                flops = 2.0 * 33 * npts * npts                                   # forward direction; the lazy reverse search adds the hit fraction
                mm_flops = 2.0 * 112 * npts * npts * 1.25                        # what the matrix cores execute for it (K = 112, full pass + 1/4 sample)
                e = {"ms_per_align": pct(lat), "valid": bool(qvalid), "stage_ms": stage, "m_n": round(m_n, 1), "m_f": round(m_f, 1),
                     "algorithmic_bytes_per_cloud": {k: int(v) for k, v in ab_q.items()},
                     "frac_hbm": {k: round(ab_q[k] * 2 / (stage[s] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) for k, s in (("normals", "fpfh_normals"), ("spfh", "fpfh_spfh"), ("fpfh", "fpfh_fpfh")) if s in stage},
                     "feat_match": {"bound": "mfma", "kernel": "k_feat_mm<2>", "flops_f16_mfma": mm_flops, "achieved_TF_lower_bound": round(mm_flops / (fm_ms * 1e-3) / 1e12, 1) if fm_ms else None,
                                    "peak_TF": MFMA_F16_PEAK_TF, "frac_of_mfma_f16_peak": round(mm_flops / (fm_ms * 1e-3) / 1e12 / MFMA_F16_PEAK_TF, 4) if fm_ms else None,
                                    "effective_f32_TF": round(flops / (fm_ms * 1e-3) / 1e12, 2) if fm_ms else None,
                                    "survivors_exactly_re_evaluated": n_surv, "fallbacks_to_valu_search": n_fb,
                                    "note": "screening GEMM on v_mfma_f32_32x32x16_f16: K = 112 (f16 hi/lo split of 33 bins + bound terms), full pass + 1/4 sampled pass, forward search only "
                                            "(Ns x Nt); time = BOTH searches + de-duplication + operand images + exact stage, so the fraction is a lower bound. effective_f32_TF = 2*33*Ns*Nt / time"},
                     "host_wall_ms": host_wall}
                if npts == 30000 and not args.no_cpu_baseline:
                    # spot check of BASELINE configs[2] against the CPU oracle (quatro<>::align, loop_closure.cpp:144): same validity, the SAME correspondence set, pose within 1e-4 m / rad
                    from oracle import oracle as orc
                    rq = q.align(qs, qt, debug=True); oq = orc.quatro_align(qs, qt)
                    dtq, drq = synth.pose_error(rq["T"], oq["T"])
                    e["parity_vs_oracle"] = {"valid": [bool(rq["valid"]), bool(oq["valid"])], "correspondences": [int(len(rq["corres"])), int(len(oq["corres"]))],
                                             "same_correspondences": bool(np.array_equal(rq["corres"], oq["corres"])), "dt_m": dtq, "dr_rad": drq,
                                             "ok": bool(rq["valid"] == oq["valid"] and np.array_equal(rq["corres"], oq["corres"]) and dtq <= 1e-4 and drq <= 1e-4)}
                quatro["%dk" % (npts // 1000)] = e
        except Exception as ex:
            quatro = {"error": repr(ex)}
    out["quatro"] = quatro
    if own:
        ctx.close()
    return out


def single_process(args, engine, synth, json_fd):
    """`--gpus N --single-process`: ONE process drives all N GPUs through qn_multi_init(N) / qn_multi_align_best - pair i -> GPU i mod N on
    `in_flight` streams each, ncclCommInitAll(N) and ONE grouped ncclAllGather of the 96-byte records inside the C-ABI.  This is what a C++ host
    like the reference's single process (fast_lio_sam_qn.cpp:213-219) would call.  A step = one registration per GPU: K x N registrations timed."""
    n = args.gpus
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n:
        raise SystemExit("bench.py --gpus %d --single-process needs %d GPUs, %d visible (no GPU sharing, no CPU fallback)" % (n, n, have))
    torch.cuda.init()
    host_pairs = [synth.make_pair(j, N_PTS, shift=args.shift) for j in range(max(args.pairs, 1))]
    dev_pairs = []                                                   # clouds resident on EVERY GPU (distinct device buffers; clouds never move between GPUs)
    for g in range(n):
        dev_pairs.append([(torch.from_numpy(s).to("cuda:%d" % g), torch.from_numpy(t).to("cuda:%d" % g)) for s, t, _ in host_pairs])
    for g in range(n):
        torch.cuda.synchronize(g)
    mg = engine.MultiGpu(n, N_PTS + 1024, in_flight=max(1, args.in_flight))
    mg.debug_set("batch_lanes", max(1, args.lanes)); mg.debug_set("batch_share_source", 0)
    gg = engine.GicpParams(); engine.lib().qn_gicp_default_params(__import__("ctypes").byref(gg))
    gg.k_correspondences, gg.max_iterations, gg.max_corr_dist, gg.optimizer, gg.force_iterations = K_COV, GN_ITERS, 52.5, 1, GN_ITERS
    mg.set_params(gg)

    def descs(k_per_gpu):
        out = []
        for i in range(k_per_gpu * n):                                # pair i -> GPU i mod N
            g, j = i % n, (i // n) % len(host_pairs)
            s, t = dev_pairs[g][j]
            out.append((s.data_ptr(), N_PTS, t.data_ptr(), N_PTS, 12, 1))
        return out

    # fail fast, BEFORE anything is timed: the communicator must have the N ranks that were asked for (ncclCommCount, RCCL's own answer), and the gather of an
    # untimed call must have delivered the same record table to every GPU - a multi-GPU figure is never quoted on a communicator that is not what it claims to be
    rccl_ranks = mg.rccl_ranks()
    if rccl_ranks != n:
        raise SystemExit("bench.py --gpus %d --single-process: RCCL reports %d ranks in the communicator (%s)" % (n, rccl_ranks, engine.lib().qn_multi_last_error(mg.h).decode()))
    mg.align_best(descs(max(args.warmup, 1)))
    mg.verify_gather()
    for g in range(n):
        torch.cuda.synchronize(g)
    t0 = time.perf_counter()
    recs, best = mg.align_best(descs(args.steps))                    # EXACTLY `steps` registrations per GPU, the RCCL gather included
    for g in range(n):
        torch.cuda.synchronize(g)
    elapsed = time.perf_counter() - t0
    assert all(r.status == 0 for r in recs), [r.status for r in recs]
    per_gpu_ms, gather_ms = mg.timing()
    winner = best if best is not None else min(recs, key=lambda r: (r.fitness, r.pair_id))     # forced iterations never "converge": rank by score
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"T": np.array([list(r.T) for r in recs], dtype=np.float32).reshape(-1, 4, 4),
                                         **{f: np.array([getattr(r, f) for r in recs], dtype=np.float64) for f in ("fitness", "pair_id", "status", "valid", "converged", "iterations")}})
        np.save(os.path.join(args.dump_outputs, "winner.npy"), np.array([winner.pair_id, winner.converged, winner.fitness] + list(winner.T), dtype=np.float64))
    # roofline leg on GPU 0 with a context of its own (the same kernels the qn_multi contexts run)
    torch.cuda.set_device(0)
    ctx = engine.Context(N_PTS + 1024, device=0)
    g0 = engine.NanoGICP(ctx); g0.p = gg; g0.bind()
    def register(j):
        s, t = dev_pairs[0][j % len(host_pairs)]
        g0.setInputSourceDevice(s.data_ptr(), N_PTS, 12); g0.calculateSourceCovariances()
        g0.setInputTargetDevice(t.data_ptr(), N_PTS, 12); g0.calculateTargetCovariances()
        return g0.align()
    register(0); ctx.synchronize()
    lat = []
    for _ in range(30):
        ta = time.perf_counter(); g0.align(); lat.append(1e3 * (time.perf_counter() - ta))
    ms_step = 1e3 * elapsed / args.steps
    roofline = roofline_leg(ctx, register, ms_step / n, pct(lat)["median"])
    out = {"metric": "scan-pair registrations/sec on 100k-pt clouds", "value": round(n * args.steps / elapsed, 3), "unit": "registrations/s", "n_gpus": n,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32 search / f64 accumulate", "data": "synthetic",
           "config": {"workload": "Nano-GICP icpAlignment, synthetic 100k x 100k street-scene pairs, k=20 covariances, 20 forced GN iterations (BASELINE configs[1])",
                      "mode": "single process: qn_multi_init(%d) -> ncclCommInitAll(%d), qn_multi_align_best with %d pairs (pair i -> GPU i mod N), one grouped ncclAllGather of the 96-byte records" % (n, n, n * args.steps),
                      "points": N_PTS, "k": K_COV, "gn_iterations": GN_ITERS, "in_flight": max(1, args.in_flight), "distinct_pairs_per_gpu": len(host_pairs),
                      "rccl_ranks": rccl_ranks, "rccl_ranks_note": "ncclCommCount of every GPU's communicator, asserted == --gpus before timing; the gather of the untimed call was verified on every GPU (qn_multi_verify_gather)",
                      "per_gpu_pairs_per_s": [round(args.steps / (1e-3 * m), 2) if m > 0 else None for m in per_gpu_ms],
                      "per_gpu_ms": [round(m, 3) for m in per_gpu_ms], "gather_ms": round(gather_ms, 4),
                      "winner_pair": int(winner.pair_id), "winner_score": winner.fitness, "ms_per_align": pct(lat)["median"]},
           "roofline": roofline, "cpu_baseline": None}
    os.write(json_fd, (json.dumps(out) + "\n").encode())
    ctx.close(); mg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-quatro", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="only the headline measurement (profiling runs)")
    ap.add_argument("--pairs", type=int, default=8, help="distinct synthetic pairs (scenes) per rank, cycled over the steps (>= 2 x in-flight)")
    ap.add_argument("--in-flight", type=int, default=3, help="contexts (= hipStreams) per GPU; each registers `--lanes` candidate pairs per kernel launch")
    ap.add_argument("--lanes", type=int, default=8, help="candidate pairs per kernel launch of a context (qn_gicp_align_batch: the pair as a grid dimension); 1 = the classic one-registration-per-stream chain")
    ap.add_argument("--c2f-scenes", type=int, nargs="*", default=None, help="developer: synth pair ids (mode quatro, 30k) of the batched coarse-to-fine leg")
    ap.add_argument("--c2f-in-flight", type=int, default=4, help="contexts (streams) of the batched coarse-to-fine leg (batch64.coarse_to_fine)")
    ap.add_argument("--repeats", type=int, default=5, help="extra timed repeats of the --steps block for the spread of `value` (reported in config.value_repeats)")
    ap.add_argument("--shift", type=float, default=None, help="developer: scene-window shift of the synthetic pairs in metres (default: the generator's 5 m = ~96 %% overlap; 24 = 80 %%)")
    ap.add_argument("--batch-pairs", type=int, default=64, help="BASELINE configs[3]: candidate pairs of one query, sharded over the ranks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what they computed (one row per step) as DIR/<name>.npy (rank r > 0: DIR/rank<r>_<name>.npy)")
    ap.add_argument("--single-process", action="store_true", help="ONE process drives all --gpus N devices through qn_multi_init(N) / qn_multi_align_best (ncclCommInitAll + grouped ncclAllGather inside the C-ABI): the path a C++ host like the reference's single process would call")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1 (the timed block is exactly --steps registrations per rank)")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and not args.single_process:
        return spawn_ranks(args)
    # stdout carries ONE JSON line and nothing else: RCCL prints a version banner to fd 1 when a communicator comes up, so fd 1 is
    # pointed at stderr for the whole run and the line is written to the saved descriptor at the end
    sys.stdout.flush()
    json_fd = os.dup(1); os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.single_process and world != 1:
        raise SystemExit("bench.py --single-process is ONE process for all GPUs: do not launch it under torchrun with WORLD_SIZE=%d" % world)
    if world != args.gpus and not args.single_process:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (torchrun --nproc-per-node %d)" % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the engine has no CPU fallback")
    # one process per GPU (RCCL over xGMI).  QN_BENCH_BACKEND=gloo lets the N > 1 code path be exercised on a 1-GPU box
    # (all ranks share cuda:0, collectives on host tensors) - a plumbing test, not a measurement.
    backend = os.environ.get("QN_BENCH_BACKEND", "nccl")
    if backend == "nccl" and torch.cuda.device_count() <= local:
        raise SystemExit("bench.py: rank %d has no GPU of its own (%d visible)" % (rank, torch.cuda.device_count()))
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    torch.cuda.init()                       # torch's bundled HIP runtime first, then libqn_engine.so
    torch.cuda.set_device(local)
    cdev = "cuda" if backend == "nccl" else "cpu"
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from qn_amd import engine, synth
    engine.DEBUG_KNOBS_FROM_ENV = True       # developer tuning only (QN_DEBUG_KNOBS -> qn_debug_set on every context); unset in every reported run
    if args.single_process:
        return single_process(args, engine, synth, json_fd)
    # `in_flight` contexts (= hipStreams) per GPU: the candidate pairs of a loop-closure query are independent
    # registrations (BASELINE "batch of candidate keyframe pairs"), several are kept in flight to fill the chip
    ctxs = [engine.Context(N_PTS + 1024, device=local) for _ in range(max(1, args.in_flight))]
    for cx in ctxs:
        cx.debug_set("batch_lanes", max(1, args.lanes))
        cx.debug_set("batch_share_source", 0)       # a step is a FULL icpAlignment: every registration rebuilds its source (loop_closure.cpp:120-121) - the 8 scenes cycle over the lanes and would otherwise meet their own source again
    gs = []
    for cx in ctxs:
        gg = engine.NanoGICP(cx)
        gg.setCorrespondenceRandomness(K_COV); gg.setMaximumIterations(GN_ITERS); gg.setMaxCorrespondenceDistance(52.5)
        gg.setOptimizer("gn"); gg.setForceIterations(GN_ITERS)
        gs.append(gg)
    ctx, g = ctxs[0], gs[0]

    # candidate pairs of this rank: pair_id = rank + world * j   (pair i -> rank i mod N); distinct scenes, distinct device buffers
    npairs = max(args.pairs, 1)
    pairs = []
    for j in range(npairs):
        src, tgt, T = synth.make_pair(rank + world * j, N_PTS, shift=args.shift)
        pairs.append((torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), T))
    torch.cuda.synchronize()

    p80 = None
    if rank == 0 and not args.no_extras:      # SURVEY 8d's generator case: 80 % overlap (target window shifted 24 m; the headline pairs overlap ~96 %), 8 DISTINCT pairs
        p80 = []
        for j in range(8):
            s80, t80, _ = synth.make_pair(9000 + j, N_PTS, shift=24.0)
            p80.append((torch.from_numpy(s80).cuda(), torch.from_numpy(t80).cuda(), None))
        torch.cuda.synchronize()
    lat_legs = None

    def register(j, gg=g):
        s, t, _ = pairs[j % len(pairs)]
        gg.setInputSourceDevice(s.data_ptr(), N_PTS, 12); gg.calculateSourceCovariances()
        gg.setInputTargetDevice(t.data_ptr(), N_PTS, 12); gg.calculateTargetCovariances()
        return gg.align()

    def batch(n, plist=None):
        plist = plist or pairs
        descs = [(plist[j % len(plist)][0].data_ptr(), N_PTS, plist[j % len(plist)][1].data_ptr(), N_PTS, 12, 1) for j in range(n)]
        return engine.icp_alignment_batch(ctxs, descs, score_thr=1.5)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def gather_best(best):
        """the one exchange step: all_gather of every rank's best record (RCCL when backend = nccl) -> the winning loop"""
        if dist is None:
            return best
        mine = torch.tensor(best, dtype=torch.float64, device=cdev)
        allrec = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allrec, mine)
        return min((a.tolist() for a in allrec), key=lambda a: (a[2], a[0]))

    if args.warmup > 0:
        # untimed warm-up: at least `--warmup` registrations, at least four full runs of lanes per context (the lane sub-contexts are created on first use, and the first
        # launches of every kernel variant load its code object - multi-millisecond hiccups in the first few batches), and at least 0.25 s of sustained work (after the
        # seconds of CPU-side scene generation above the device sits in a low power state; a 30 ms warm-up left the first timed region 10 % slow)
        tw = time.perf_counter()
        batch(max(args.warmup, 4 * len(ctxs) * max(1, args.lanes)))
        while time.perf_counter() - tw < 0.25:
            batch(2 * len(ctxs) * max(1, args.lanes))
        # ... and ONE untimed run of exactly the block that is timed next (the pairs dealt to the contexts the same way): the first block behind a warm-up of another shape read 1-3 %
        # below its own repeats in every round's record (r5: 4064 against repeats of 4078-4209; r6: 3969 against 4084-4133) - the timed block and its repeats now start from the same state
        batch(args.steps)
    if dist is not None:          # untimed: bring up the communicator's channels (RCCL connects lazily on the first collective)
        gather_best([0.0] * 19)
        dist.all_reduce(torch.zeros(1, dtype=torch.float64, device=cdev), op=dist.ReduceOp.MAX)
    barrier()
    t0 = time.perf_counter()
    results, valid, status = batch(args.steps)                      # EXACTLY `steps` registrations
    assert all(st == 0 for st in status), status
    jb = min(range(len(results)), key=lambda j: results[j].fitness)      # (the rank's best record: the argmin first, ONE record built - twenty ctypes-array-to-list conversions inside a 4.9 ms region were 2 % of it)
    rb = results[jb]
    best = [float(rank + world * (jb % len(pairs))), float(rb.converged), rb.fitness] + list(rb.T)
    winner = gather_best(best)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {**gicp_result_arrays(results, valid, status), "pair_id": np.array([rank + world * (j % len(pairs)) for j in range(args.steps)], dtype=np.float64)},
                     prefix="" if rank == 0 else "rank%d_" % rank)
        if rank == 0:
            np.save(os.path.join(args.dump_outputs, "winner.npy"), np.array(winner, dtype=np.float64))
    # ---- spread of `value`: the same --steps block, `repeats` more times (a 60 ms timed region cannot resolve a few per cent on its own)
    rep_vals = []
    for _ in range(max(0, args.repeats)):
        barrier(); tr = time.perf_counter(); _, _, st_r = batch(args.steps); barrier(); wr = time.perf_counter() - tr
        assert all(x == 0 for x in st_r), st_r
        if dist is not None:
            tmax = torch.tensor([wr], dtype=torch.float64, device=cdev); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); wr = float(tmax.item())
        rep_vals.append(world * args.steps / wr)

    # ---- BASELINE configs[3], literally: ONE query with `batch_pairs` (64) DISTINCT candidate pairs, pair i -> rank i mod N, each rank
    # through qn_multi_align_best (its GPU, `in_flight` streams, the RCCL gather of its record table inside the C-ABI), then the
    # all_gather of the per-rank winners; pairs/s = 64 / wall.  The 64 pairs = the rank's scenes x rigid re-poses of the target.
    batch64 = None
    if not args.no_extras:
        nb = args.batch_pairs
        my_ids = [i for i in range(nb) if i % world == rank]
        bpairs = []
        for i in my_ids:
            s, t, _ = pairs[(i // world) % len(pairs)]
            v = i // (world * len(pairs))                              # variant: re-pose the target (distinct coordinates, distinct ground truth)
            if v:
                a = 0.01 * v; ca, sa = float(np.cos(a)), float(np.sin(a))
                R = torch.tensor([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=t.device)
                t = (t @ R.T + torch.tensor([0.05 * v, -0.03 * v, 0.0], dtype=torch.float32, device=t.device)).contiguous()
            bpairs.append((s, t))
        mg = engine.MultiGpu(1, N_PTS + 1024, in_flight=len(ctxs), device_ids=[local])
        mg.debug_set("batch_lanes", max(1, args.lanes))
        mg.debug_set("batch_share_source", 0)       # 64 DISTINCT pairs: no shared source preparation (the re-posed variants reuse a scene's source buffer)
        mg.set_params(g.p)
        descs = [(s.data_ptr(), N_PTS, t.data_ptr(), N_PTS, 12, 1) for s, t in bpairs]
        mg.align_best(descs[:min(len(descs), 4)])                     # untimed warm-up of the new contexts
        barrier()
        tb = time.perf_counter()
        recs, bestrec = mg.align_best(descs)
        if bestrec is None and recs:      # forced iterations never "converge" (no accept test): rank the records by score alone, as the headline loop does
            bestrec = min(recs, key=lambda r: (r.fitness, r.pair_id))
        mine = [float(my_ids[bestrec.pair_id]), float(bestrec.converged), bestrec.fitness] + list(bestrec.T) if bestrec is not None else [-1.0, 0.0, 1.7e308] + [0.0] * 16
        bwin = gather_best(mine)
        barrier()
        bwall = time.perf_counter() - tb
        if dist is not None:
            tmax = torch.tensor([bwall], dtype=torch.float64, device=cdev); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); bwall = float(tmax.item())
        assert all(r.status == 0 for r in recs), [r.status for r in recs]
        bwalls = [bwall]
        if world == 1:      # a one-shot 17 ms wall is at the mercy of one hiccup (a 64-pair call of the same build read 11.4 and 16.1 ms on two boxes): two more calls, the median is quoted
            for _ in range(2):
                barrier(); tb = time.perf_counter(); mg.align_best(descs); barrier(); bwalls.append(time.perf_counter() - tb)
            bwall = float(np.median(bwalls))
        batch64 = {"pairs": nb, "distinct_pairs": nb, "wall_ms": round(1e3 * bwall, 3), "wall_ms_runs": [round(1e3 * w, 3) for w in bwalls], "pairs_per_s": round(nb / bwall, 2), "ms_per_pair": round(1e3 * bwall / nb, 4),
                   "winner_pair": int(bwin[0]), "winner_score": bwin[2], "sharding": "pair i -> rank i mod %d; qn_multi_align_best per rank on its GPU (a process that owns several GPUs gathers its 96-byte records with RCCL inside the C-ABI), all_gather of the rank winners" % world,
                   "valid_pairs_this_rank": int(sum(r.valid for r in recs))}
        # ---- two of the 64 records against the CPU oracle (rank 0, when the CPU leg is on): a plain scene pair and a re-posed variant from the second half of the batch
        if rank == 0 and world == 1 and not args.no_cpu_baseline and recs:
            from oracle import oracle as orc                  # checker only
            chk = []
            for li in sorted({min(1, len(recs) - 1), len(recs) - 3 if len(recs) > 3 else 0}):
                s_np, t_np = bpairs[li][0].cpu().numpy(), bpairs[li][1].cpu().numpy()
                o = orc.GicpOracle(k=K_COV, max_iter=GN_ITERS, max_corr_dist=52.5, optimizer="gn", force_iterations=GN_ITERS)
                o.set_source(s_np); o.compute_covariances(0); o.set_target(t_np); o.compute_covariances(1)
                ro = o.align(); r = recs[li]
                dT = float(np.abs(np.array(r.T, dtype=np.float32).reshape(4, 4) - ro["Tf"]).max())
                chk.append({"pair": int(my_ids[li]), "max_abs_T_f32_diff": dT, "iterations": [int(r.iterations), int(ro["iterations"])],
                            "score_rel_diff": abs(r.fitness - ro["fitness"]) / max(ro["fitness"], 1e-300),
                            "ok": bool(dT <= 1e-6 and r.iterations == ro["iterations"] and abs(r.fitness - ro["fitness"]) <= 1e-6 * ro["fitness"])})
            batch64["parity_vs_oracle"] = {"records_checked": chk, "ok": bool(all(c["ok"] for c in chk)),
                                           "note": "the 96-byte records carry getFinalTransformation() (f32): compared with the oracle's f32 matrix"}
        # ---- what ONE rank does at N = 8 (BASELINE configs[3]: 64 pairs over 8 GPUs = 8 pairs per rank), measurable on one GPU: the walls of 8-pair qn_multi_align_best
        # calls over the SAME 64 pairs, eight blocks of 8 consecutive pairs (block v = the 8 scenes at re-pose variant v: the blocks differ in difficulty), median of 3 each.
        # projected_speedup_at_8 = wall(64 pairs on one GPU) / (mean block wall + gather): what 8 ranks holding one block each would need - a PROJECTION, no N > 1 run exists.
        if world == 1 and nb >= 16:
            share = max(1, nb // 8)
            blocks = []
            mg.align_best(descs[:share])
            for blk in range(nb // share):
                sub = descs[blk * share:(blk + 1) * share]; w8 = []
                for _ in range(3):
                    torch.cuda.synchronize(); t8 = time.perf_counter(); r8, _ = mg.align_best(sub); torch.cuda.synchronize(); w8.append(1e3 * (time.perf_counter() - t8))
                    assert all(r.status == 0 for r in r8)
                blocks.append(float(np.median(w8)))
            _, g_ms = mg.timing()
            batch64["per_rank_share_at_8"] = {"pairs": share, "block_wall_ms": [round(x, 3) for x in blocks], "mean_block_wall_ms": round(float(np.mean(blocks)), 3), "gather_ms_last": round(g_ms, 4),
                                              "projected_speedup_at_8": round(1e3 * bwall / (float(np.mean(blocks)) + g_ms), 2),
                                              "projected_speedup_easiest_block": round(1e3 * bwall / (min(blocks) + g_ms), 2),
                                              "note": "a rank's whole work at N = 8 is ONE short call: 8 pairs are latency, not throughput (2 contexts x 4 lanes serve them; the chain of ~42 launches is what lasts) - the eight "
                                                      "blocks together cost 1.5-1.6 x the 64-pair call.  projected = wall(%d pairs, 1 GPU) / (mean block wall + gather); the gather here is a 1-rank ncclAllGather - the 8-rank one "
                                                      "moves 8 x %d x 96 B over xGMI (latency-bound, tens of microseconds).  No N > 1 measurement exists in this repository." % (nb, share)}
        # ---- the same 64 distinct pairs at the reference's operating point (k = 15, LM, <= 32 iterations, the real stopping rule):
        # here the accept test `hasConverged() && score < thr` (loop_closure.cpp:129) is live, so `valid`, best_found and the arg-min of
        # qn_multi_align_best are exercised in a measured run, and the winner is the C-ABI's, not this script's
        import ctypes
        pref = engine.GicpParams(); engine.lib().qn_gicp_default_params(ctypes.byref(pref))
        pref.k_correspondences, pref.max_iterations, pref.max_corr_dist, pref.transformation_epsilon = 15, 32, 52.5, 0.01
        mg.set_params(pref)
        mg.align_best(descs[:min(len(descs), 4)])
        barrier()
        tb = time.perf_counter()
        rrecs, rbest = mg.align_best(descs)
        rmine = [float(my_ids[rbest.pair_id]), float(rbest.converged), rbest.fitness] + list(rbest.T) if rbest is not None else [-1.0, 0.0, 1.7e308] + [0.0] * 16
        rwin = gather_best(rmine)
        barrier()
        rwall = time.perf_counter() - tb
        if dist is not None:
            tmax = torch.tensor([rwall], dtype=torch.float64, device=cdev); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); rwall = float(tmax.item())
        assert all(r.status == 0 for r in rrecs), [r.status for r in rrecs]
        vrec = [r for r in rrecs if r.valid]
        own = min(vrec, key=lambda r: (r.fitness, r.pair_id)) if vrec else None
        batch64["reference_operating_point"] = {"config": "k=15, LM, max 32 iterations, eps_t 0.01, score thr 1.5", "pairs": nb, "wall_ms": round(1e3 * rwall, 3), "pairs_per_s": round(nb / rwall, 2),
                                                "valid_pairs_this_rank": len(vrec), "converged_this_rank": int(sum(r.converged for r in rrecs)), "best_found": rbest is not None,
                                                "winner_pair": int(rwin[0]), "winner_score": rwin[2],
                                                "argmin_matches_records": bool((own is None and rbest is None) or (own is not None and rbest is not None and own.pair_id == rbest.pair_id)),
                                                "iterations_min_max": [int(min(r.iterations for r in rrecs)), int(max(r.iterations for r in rrecs))]}
        mg.set_params(g.p)
        # ---- the same 64 candidates as ONE loop-closure query sees them: every pair shares the query's source cloud, which each context
        # prepares once (qn_icp_alignment_same_source inside qn_multi_align_best); the reference's single-candidate code path rebuilds it per call
        s0, t0_ = pairs[0][0], pairs[0][1]
        stg = []
        for v in range(len(my_ids)):                                   # this rank's candidates: rigid re-poses of the query scene's target
            a = 0.004 * (v + 1); ca, sa = float(np.cos(a)), float(np.sin(a))
            R = torch.tensor([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=t0_.device)
            stg.append((t0_ @ R.T + torch.tensor([0.02 * v, -0.01 * v, 0.0], dtype=torch.float32, device=t0_.device)).contiguous())
        sdescs = [(s0.data_ptr(), N_PTS, t.data_ptr(), N_PTS, 12, 1) for t in stg]
        mg.debug_set("batch_share_source", 1)       # here the shared source IS the workload
        mg.align_best(sdescs[:min(len(sdescs), 4)])
        swalls = []
        for _ in range(3 if world == 1 else 1):      # (median of three single-process calls, as above)
            barrier()
            tb = time.perf_counter()
            srecs, _ = mg.align_best(sdescs)
            barrier()
            swalls.append(time.perf_counter() - tb)
        swall = float(np.median(swalls))
        if dist is not None:
            tmax = torch.tensor([swall], dtype=torch.float64, device=cdev); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); swall = float(tmax.item())
        assert all(r.status == 0 for r in srecs), [r.status for r in srecs]
        batch64["shared_query"] = {"pairs": nb, "wall_ms": round(1e3 * swall, 3), "wall_ms_runs": [round(1e3 * w, 3) for w in swalls], "pairs_per_s": round(nb / swall, 2),
                                   "note": "64 candidate targets against ONE query cloud per rank: source grid + covariances prepared once per context"}
        mg.close()
        # ---- the reference's DEFAULT per-candidate path as a batch: coarseToFineAlignment (Quatro -> transformPcd -> Nano-GICP, loop_closure.cpp:138-159 with enable_quatro_) on
        # 64 distinct 30k-point candidate pairs (the reference's keyframe size, BASELINE configs[0]) at its operating point, through qn_coarse_to_fine_align_batch
        if world == 1 and not args.no_quatro:
            try:
                NQ = 30000
                c2f_ctxs = [engine.Context(NQ + 1024, device=local) for _ in range(max(1, args.c2f_in_flight))]
                for cx in c2f_ctxs:
                    cx.debug_set("batch_lanes", max(1, args.lanes))
                    gq = engine.NanoGICP(cx); gq.setCorrespondenceRandomness(15); gq.setMaximumIterations(32); gq.setMaxCorrespondenceDistance(52.5); gq.setTransformationEpsilon(0.01); gq.bind()
                    engine.Quatro(cx)
                # TRUE LOOPS: scenes on which the coarse estimate is right (the oracle says so too) - a revisited place, what the radius gate of fetchClosestKeyframeIdx
                # (loop_closure.cpp:34-56) hands over.  On this generator's near-symmetric street scenes Quatro's clique collapses (4 members) for about half of the
                # yaw-U(-180, 180) pairs, oracle and engine alike; Nano-GICP then runs its 32 iterations on misaligned clouds (every query "far") and the pair is rejected by
                # the score test: that mix is reported separately below (`mixed_scenes`), it measures the failure path, not the registration.
                scenes = [synth.make_pair(j, NQ, mode="quatro") for j in (args.c2f_scenes or C2F_TRUE_LOOP_SCENES)]
                qdev = [(torch.from_numpy(s_).cuda(), torch.from_numpy(t_).cuda()) for s_, t_, _ in scenes]
                qd = []
                for i in range(nb):
                    s_, t_ = qdev[i % len(qdev)]; v = i // len(qdev)
                    if v:
                        a = 0.004 * v; ca, sa = float(np.cos(a)), float(np.sin(a))
                        R = torch.tensor([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=t_.device)
                        t_ = (t_ @ R.T + torch.tensor([0.02 * v, -0.01 * v, 0.0], dtype=torch.float32, device=t_.device)).contiguous()
                    qd.append((s_, t_))
                torch.cuda.synchronize()
                qdescs = [(s_.data_ptr(), NQ, t_.data_ptr(), NQ, 12, 1) for s_, t_ in qd]
                engine.coarse_to_fine_align_batch(c2f_ctxs, qdescs[:2 * len(c2f_ctxs) * max(1, args.lanes)])           # untimed: lane contexts and their Quatro buffers are created on first use
                walls = []
                for _ in range(3):
                    torch.cuda.synchronize(); tq = time.perf_counter(); qr = engine.coarse_to_fine_align_batch(c2f_ctxs, qdescs); torch.cuda.synchronize(); walls.append(time.perf_counter() - tq)
                assert all(r["status"] == 0 for r in qr)
                qwall = float(np.median(walls))
                e = {"pairs": nb, "points": NQ, "in_flight": len(c2f_ctxs), "lanes": max(1, args.lanes), "wall_ms": round(1e3 * qwall, 3), "pairs_per_s": round(nb / qwall, 2),
                     "wall_ms_runs": [round(1e3 * w, 3) for w in walls], "valid_pairs": int(sum(r["valid"] for r in qr)),
                     "config": "Quatro (r_n 0.9, r_f 1.5, cap 200, thr 35 m, noise 0.3) + Nano-GICP k=15, LM, max 32 iterations, eps_t 0.01, score thr 1.5 (SURVEY App. C)"}
                # one pair at a time on one context, same pairs: what the batch replaces
                t1 = time.perf_counter()
                for (s_, t_) in qd[:8]:
                    engine.coarse_to_fine_alignment_device(c2f_ctxs[0], s_.data_ptr(), NQ, t_.data_ptr(), NQ, 12)
                e["one_pair_at_a_time_pairs_per_s"] = round(8 / (time.perf_counter() - t1), 2)
                if not args.no_cpu_baseline:
                    from oracle import oracle as orc              # checker only: record 1 and a re-posed one against the oracle
                    chk = []
                    for li in (1, nb - 3):
                        o = orc.coarse_to_fine_alignment(qd[li][0].cpu().numpy(), qd[li][1].cpu().numpy())
                        dtq, drq = synth.pose_error(qr[li]["T"], o["T"]) if o["valid"] else (0.0, 0.0)
                        chk.append({"pair": li, "valid": [bool(qr[li]["valid"]), bool(o["valid"])], "dt_m": dtq, "dr_rad": drq, "ok": bool(qr[li]["valid"] == o["valid"] and dtq <= 1e-4 and drq <= 1e-4)})
                    e["parity_vs_oracle"] = {"records_checked": chk, "ok": bool(all(c["ok"] for c in chk))}
                # the candidates of ONE query: 64 re-posed targets against scene 0's source cloud - per run of lanes the source's grid / normals / SPFH / FPFH are made once (batch_share_source)
                s0_, t0q = qdev[0]
                sq = []
                for v in range(nb):
                    a = 0.004 * (v + 1); ca, sa = float(np.cos(a)), float(np.sin(a))
                    R = torch.tensor([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=t0q.device)
                    sq.append((t0q @ R.T + torch.tensor([0.02 * v, -0.01 * v, 0.0], dtype=torch.float32, device=t0q.device)).contiguous())
                torch.cuda.synchronize()
                sqd = [(s0_.data_ptr(), NQ, t_.data_ptr(), NQ, 12, 1) for t_ in sq]
                engine.coarse_to_fine_align_batch(c2f_ctxs, sqd[:len(c2f_ctxs) * max(1, args.lanes)])
                sw = []
                for _ in range(3):
                    torch.cuda.synchronize(); tq = time.perf_counter(); sr = engine.coarse_to_fine_align_batch(c2f_ctxs, sqd); torch.cuda.synchronize(); sw.append(time.perf_counter() - tq)
                assert all(r["status"] == 0 for r in sr)
                e["shared_query"] = {"pairs": nb, "wall_ms": round(1e3 * float(np.median(sw)), 3), "pairs_per_s": round(nb / float(np.median(sw)), 2), "valid_pairs": int(sum(r["valid"] for r in sr)),
                                     "note": "64 candidate targets against ONE query cloud: the source's Quatro features are prepared once per run of lanes and borrowed by the other lanes"}
                # the failure mix: scenes 400..407 of the generator as they come (Quatro's estimate is wrong on five of them - see above)
                mixed = [synth.make_pair(400 + j, NQ, mode="quatro") for j in range(8)]
                mdev = [(torch.from_numpy(s_).cuda(), torch.from_numpy(t_).cuda()) for s_, t_, _ in mixed]; torch.cuda.synchronize()
                mdescs = [(mdev[i % 8][0].data_ptr(), NQ, mdev[i % 8][1].data_ptr(), NQ, 12, 1) for i in range(nb)]
                engine.coarse_to_fine_align_batch(c2f_ctxs, mdescs[:8])
                torch.cuda.synchronize(); tq = time.perf_counter(); mr = engine.coarse_to_fine_align_batch(c2f_ctxs, mdescs); torch.cuda.synchronize(); mwall = time.perf_counter() - tq
                e["mixed_scenes"] = {"pairs": nb, "wall_ms": round(1e3 * mwall, 3), "pairs_per_s": round(nb / mwall, 2), "valid_pairs": int(sum(r["valid"] for r in mr)),
                                     "note": "generator scenes 400-407 cycled: on five of the eight Quatro's maximum clique has 4 members and the coarse pose is wrong (oracle: same); Nano-GICP then spends its 32 LM "
                                             "iterations on misaligned clouds before the score test rejects the pair"}
                batch64["coarse_to_fine"] = e
                for cx in c2f_ctxs:
                    cx.close()
            except Exception as ex:
                batch64["coarse_to_fine"] = {"error": repr(ex)}

    out = None
    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        L = lat_legs if lat_legs is not None else latency_legs(engine, synth, pairs, args, world, ctx, p80=p80)
        single, host, align, chain_roofline, cpu, dtp, parity = L["single"], L["host"], L["align"], L["roofline"], L["cpu"], L["dtp"], L["parity"]
        align_ms = align["median"]
        # ---- the roofline object describes the path `value` ran: the batched launches (one context alone on the GPU, hipEvents on its stream); the classic chain's leg
        # (one registration per stream, what the latency figures time) rides along as `single_stream_chain`
        if max(1, args.lanes) >= 2:
            roofline = batched_roofline_leg(engine, ctx, pairs, max(1, args.lanes))
            roofline["single_stream_chain"] = chain_roofline
            # ---- the SAME kernel under the load `value` is measured at: hipEvents around every batched launch of EVERY in-flight context while all of them work (one more
            # --steps block, untimed).  This is the figure a `rocprofv3 --kernel-trace --stats` of this command reports (profiles/r5_*_kernel_stats.csv) - a launch that shares
            # the chip with the other contexts' kernels lasts 1.5-1.8 x longer than alone - and it is the one the top-level achieved / frac are quoted on; the context-alone
            # figures stay beside it as `alone_on_gpu`.
            try:
                n_l = max(min(args.steps, 96), 2 * len(ctxs) * max(1, args.lanes))
                fam = roofline["family"]; per_lane = {"knn_select": 2}.get(fam, 1); NL = max(1, args.lanes)
                trials = []
                for _ in range(3):                                        # three blocks, the median block is reported (a block that catches a clock transition reads 40 % long)
                    for cx in ctxs:
                        cx.prof_reset(); cx.prof_enable(True)
                    _, _, st_l = batch(n_l)
                    torch.cuda.synchronize()
                    assert all(x == 0 for x in st_l), st_l
                    tot, cnt = {}, {}
                    for cx in ctxs:
                        cx.synchronize(); cx.prof_enable(False)
                        for k, v in cx.prof_stats().items():
                            tot[k] = tot.get(k, 0.0) + v[0]; cnt[k] = cnt.get(k, 0) + v[1]
                    if cnt.get(fam, 0) > 0:
                        trials.append((tot[fam] / cnt[fam], tot, cnt))
                trials.sort(key=lambda x: x[0])
                if trials:
                    per_entry, tot, cnt = trials[len(trials) // 2]        # ms per table entry of a launch (a family's `launches` count the entries its launches carried)
                    roofline["under_load_trials_ms_per_entry"] = [round(x[0], 6) for x in trials]
                    bytes_entry = roofline["algorithmic_bytes_per_launch"] / (NL * per_lane)
                    ach = bytes_entry / (per_entry * 1e-3) / 1e9
                    alone = {k: roofline[k] for k in ("achieved", "frac", "avg_batched_launch_ms", "avg_launch_ms_per_entry")}
                    roofline["alone_on_gpu"] = dict(alone, note="one context alone on the GPU (the per-kernel table `kernels` below is measured this way)")
                    roofline["achieved"] = round(ach, 2); roofline["frac"] = round(ach / HBM_PEAK_GBS, 5)
                    roofline["avg_batched_launch_ms"] = round(per_entry * NL * per_lane, 5); roofline["avg_launch_ms_per_entry"] = round(per_entry, 6)
                    roofline["measured"] = "under the load `value` runs at: %d contexts x %d lanes in flight, hipEvents on every context's stream" % (len(ctxs), NL)
                    roofline["family_ms_per_registration_under_load"] = {k: round(tot[k] / n_l, 4) for k in tot if cnt.get(k, 0) > 0}
            except Exception as ex:
                roofline["under_load_error"] = repr(ex)
        else:
            roofline = chain_roofline
        roofline["whole_registration"] = whole_registration(ms_step)
        vb_path = os.path.join(ROOT, "profiles", "valu_budget_latest.json")
        if os.path.exists(vb_path):      # what the engine is actually bound by: VALU issue slots (SQ_ACTIVE_INST_VALU per kernel x launches per registration; tools/gpu_sq.sh + tools/valu_budget.py)
            try:
                vb = json.load(open(vb_path)); qc = float(vb["quad_cycles_per_registration"])
                chip_us = qc * 4.0 / (1024 * float(vb.get("clock_ghz", 2.1)) * 1e3)
                roofline["valu_issue"] = {"quad_cycles_per_registration": qc, "us_of_a_fully_issuing_chip": round(chip_us, 1), "frac_of_issue_slots": round(chip_us / (ms_step * 1e3), 4),
                                          "source": vb.get("source"), "measured_in_this_run": False, "stale": profile_stale(vb.get("csrc_sha1")),
                                          "note": "quad_cycles_per_registration is NOT measured in this run: it is read from profiles/valu_budget_latest.json (SQ_ACTIVE_INST_VALU passes of the build named in `source`; "
                                                  "the kernels of the GICP chain are unchanged since) - only the division by this run's step time is live.  1024 SIMDs x one wave64 VALU instruction per 4 cycles"}
            except Exception as ex:
                roofline["valu_issue"] = {"error": repr(ex)}
        # parity of the BATCHED path on the headline workload: the timed batch's own record of pair 0 against the oracle (the classic path's check is `parity`)
        if parity is not None and L.get("oracle_T") is not None:
            Tb = np.array(results[0].T64).reshape(4, 4); To = np.array(L["oracle_T"])
            dtb = float(np.abs(Tb - To).max())
            parity["batched_path"] = {"pair": 0, "max_abs_T_diff": dtb, "iterations": int(results[0].iterations), "score_rel_diff": abs(results[0].fitness - L["oracle_fitness"]) / max(L["oracle_fitness"], 1e-300),
                                      "ok": bool(dtb <= 1e-9 and results[0].iterations == L["oracle_iterations"])}
            parity["ok"] = bool(parity["ok"] and parity["batched_path"]["ok"])

        extras = {"latency_legs": {"alone_in_process": L["alone_in_process"], "persistent_align_launches": L["persistent_align_launches"],
                                   "note": "ms_per_registration_single_stream, ..._from_host_buffers, ms_per_align, overlap80 single-stream, reference_operating_point and quatro are one-registration-at-a-time figures "
                                           "(the reference's deployment: one candidate pair per timer tick), measured on the first in-flight context after the throughput legs"}}
        if not args.no_extras:
            try:
                # ---- SURVEY 8d's generator case as a throughput figure: same workload and in-flight setting as `value`, 8 DISTINCT 80 %-overlap pairs, `steps` timed registrations
                for gg in gs:
                    gg.bind()
                batch(8, p80); torch.cuda.synchronize()
                n80 = max(40, args.steps)
                t8 = time.perf_counter(); _, _, st80 = batch(n80, p80); torch.cuda.synchronize(); w80 = time.perf_counter() - t8
                assert all(x == 0 for x in st80), st80
                extras["overlap80"] = {"registrations_per_s": round(n80 / w80, 2), "ms_per_step": round(1e3 * w80 / n80, 4), "steps": n80, "distinct_pairs": len(p80), "in_flight": len(ctxs),
                                       "ms_per_registration_single_stream_stats": L.get("overlap80_single"), "ms_per_align_stats": L.get("overlap80_align"),
                                       "family_ms_per_registration": L.get("overlap80_family_ms"),
                                       "note": "SURVEY 8d generator: target scene window shifted so that the clouds overlap 80 % (20 % of the source has no counterpart)"}
                extras["reference_operating_point"] = L.get("rop")
                # ---- SURVEY 8d's generator text, literally: "80 % spatial overlap (target scene window shifted 10 m)" - on the 120 m scene a 10 m shift is 92 % overlap (the
                # 24 m of `overlap80` are the 80 %); same workload and in-flight setting as `value`, 8 distinct pairs
                p10 = []
                for j in range(8):
                    s10, t10, _ = synth.make_pair(9100 + j, N_PTS, shift=10.0)
                    p10.append((torch.from_numpy(s10).cuda(), torch.from_numpy(t10).cuda(), None))
                torch.cuda.synchronize()
                batch(8, p10); torch.cuda.synchronize()
                t8 = time.perf_counter(); _, _, st10 = batch(n80, p10); torch.cuda.synchronize(); w10 = time.perf_counter() - t8
                assert all(x == 0 for x in st10), st10
                extras["shift10"] = {"registrations_per_s": round(n80 / w10, 2), "ms_per_step": round(1e3 * w10 / n80, 4), "steps": n80, "distinct_pairs": len(p10), "in_flight": len(ctxs),
                                     "note": "target scene window shifted 10 m (SURVEY 8d's literal generator parameter; 92 % overlap on the 120 m scene)"}
            except Exception as ex:                                      # an extra must never cost the headline line
                extras["extras_error"] = repr(ex)
            # ---- the drop-in path's own latency: the compiled C++ programs that run the reference's call sequences against the header-only shims (tests/shim_icp_alignment.cpp =
            # loop_closure.cpp:113-135, tests/shim_coarse_to_fine.cpp = :138-159): pcl::PointXYZI clouds (32-byte stride) from the host, deep copies, aligned_ downloaded, a second
            # context for Quatro, CPU transformPcd, the target uploaded twice - what an UNMODIFIED LoopClosure would see per call (reference operating point: k = 15, LM, eps 0.01)
            try:
                extras["shim"] = shim_latency(synth)
            except Exception as ex:
                extras["shim"] = {"error": repr(ex)}

        quatro = L.get("quatro")

        # ---- BASELINE configs[4]: loopTimerFunc replay on a synthetic keyframe stream (tools/replay.py): candidate search, submaps assembled on the
        # device, registration (Nano-GICP scan-to-submap, and Quatro + Nano-GICP scan-to-scan), loop factors into a host pose graph (iSAM2 stand-in)
        if world == 1 and not args.no_extras:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import replay
                rp = {}
                for name, uq in (("nano_gicp", False), ("quatro_nano_gicp", True)):
                    replay.run(n_kf=20, seed=7, use_quatro=uq, verbose=False)            # warm-up (allocations)
                    o = replay.run(n_kf=60, seed=7, use_quatro=uq, verbose=False)
                    rp[name] = {"keyframes": o["n_keyframes"], "loop_attempts": o["attempts"], "loops_accepted": o["loops"],
                                "ms_per_attempt": round(o["ms_per_attempt"], 3) if o["ms_per_attempt"] else None,
                                "ate_odometry_m": round(o["ate_odometry"], 3), "ate_corrected_m": round(o["ate_corrected"], 3)}
                extras["replay"] = {"note": "assembly of both clouds on the device + registration per loop attempt; pose graph on the host", **rp}
            except Exception as ex:
                extras["replay"] = {"error": repr(ex)}

        out = {"metric": "scan-pair registrations/sec on 100k-pt clouds", "value": round(world * args.steps / elapsed, 3),
               "unit": "registrations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32 search / f64 accumulate", "data": "synthetic",
               "config": {"workload": "Nano-GICP icpAlignment, synthetic 100k x 100k street-scene pairs, k=20 covariances, 20 forced GN iterations (BASELINE configs[1])",
                          "points": N_PTS, "k": K_COV, "gn_iterations": GN_ITERS, "sharding": "pair i -> rank i mod N, all_gather of best record",
                          "in_flight": len(ctxs), "lanes": max(1, args.lanes), "distinct_pairs_per_rank": len(pairs),
                          "rccl_ranks": (dist.get_world_size() if dist is not None else 1), "collective_backend": (backend if dist is not None else None),
                          "launch_structure": "%d contexts (streams) x %d candidate pairs per kernel launch (qn_gicp_align_batch: k_lanes<F>, blockIdx.y = pair); launches per registration %.2f" % (len(ctxs), max(1, args.lanes), ctx.debug_get("batch_launches") / max(1.0, ctx.debug_get("batch_pairs"))),
                          "value_repeats": {"values": [round(v, 1) for v in rep_vals], "median": round(float(np.median(rep_vals)), 1) if rep_vals else None,
                                            "min": round(min(rep_vals), 1) if rep_vals else None, "max": round(max(rep_vals), 1) if rep_vals else None,
                                            "note": "the same --steps block timed `repeats` more times after the reported region"},
                          "ms_per_registration_single_stream": single["median"], "ms_per_registration_single_stream_stats": single,
                          "ms_per_registration_from_host_buffers": host["median"], "ms_per_registration_from_host_buffers_stats": host,
                          "ms_per_align": align_ms, "ms_per_align_stats": align, "winner_pair": int(winner[0]), "winner_score": winner[2],
                          "max_abs_T_diff_vs_oracle": dtp, "parity_vs_oracle": parity, "batch64": batch64, "quatro": quatro, **extras},
               "value_overlap80": (extras.get("overlap80") or {}).get("registrations_per_s"),
               "value_shift10": (extras.get("shift10") or {}).get("registrations_per_s"),
               "value_repeats": {"median": round(float(np.median(rep_vals)), 1) if rep_vals else None, "min": round(min(rep_vals), 1) if rep_vals else None,
                                 "max": round(max(rep_vals), 1) if rep_vals else None, "n": len(rep_vals)},
               "shim_ms_per_icpAlignment": {k: v.get("icpAlignment_ms") for k, v in (extras.get("shim") or {}).items() if isinstance(v, dict)} or None,
               "shim_ms_per_coarseToFine": {k: v.get("coarseToFine_ms") for k, v in (extras.get("shim") or {}).items() if isinstance(v, dict)} or None,
               "roofline": roofline, "cpu_baseline": cpu}
        os.write(json_fd, (json.dumps(out) + "\n").encode())
        if parity is not None and not parity["ok"]:
            raise SystemExit("bench.py: the benched workload does NOT match the oracle: %r" % (parity,))
        for name, par in (("batch64", (batch64 or {}).get("parity_vs_oracle")), ("batch64.coarse_to_fine", ((batch64 or {}).get("coarse_to_fine") or {}).get("parity_vs_oracle"))):
            if par is not None and not par["ok"]:
                raise SystemExit("bench.py: %s records do NOT match the oracle: %r" % (name, par))
        qpar = ((quatro or {}).get("30k") or {}).get("parity_vs_oracle") if isinstance(quatro, dict) else None
        if qpar is not None and not qpar["ok"]:
            raise SystemExit("bench.py: the Quatro stage (configs[2]) does NOT match the oracle: %r" % (qpar,))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    for cx in ctxs:
        cx.close()


if __name__ == "__main__":
    main()
