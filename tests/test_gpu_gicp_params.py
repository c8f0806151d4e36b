"""Nano-GICP on the GPU against the oracle (oracle/gicp_oracle.cpp) across its parameter space, on every align path.
Every test before this one ran at the reference's operating point; the branches that only other parameters reach are covered here:

- LM inner limit (lm_max_iterations 1/2/3, control 10) on lever-arm pairs that reject trials: the "lm not converged!!" path (lm_failed) and
  success after rejections - the device controller (solve_controller) and the host tick budgets;
- LM initial damping (lm_init_lambda_factor 0 ... 1e3): runs of tiny steps with accept/reject mixes, lambda = 0 repeating the same step;
- the stopping rule (rotation_epsilon x transformation_epsilon) with each epsilon deciding a stop, and the degenerate epsilons NaN / 0 (d_is_converged);
- iteration caps 0 / 1 / 2, LM and GN, with and without a guess; qn_gicp_align_batch at 0 iterations (its one-pair fallback, batch_supported);
- the correspondence gate in whole aligns (unseeded, tracked and far-refresh ticks, the LM trial-error re-gate), a gate below every NN distance (H = 0:
  the pivoted solve's zero step) and a gate that keeps a handful of correspondences;
- a lattice whose NN squared distances are exactly 0.25: the gate at 0.5 (strict <: all out) and one f32 step above (all in), bit for bit, through
  the tracked ticks (persist = 0) and the persistent kernel;
- small k (1 ... 8): covariances, then whole aligns;
- the same parameters on every path: the persistent kernel (persist_launches), qn_gicp_align_batch with 2 and 8 lanes (batch_launches),
  qn_icp_alignment_batch over 3 contexts and the fine stage of qn_coarse_to_fine_align_batch - bit for bit against the classic chain;
- parameter changes between calls on one context (and on a batch context's lanes), and getFitnessScore(max_range).

The bar against the oracle (check): iterations, converged, lm_failed, trace inner / accepted identical; y0 rtol 1e-8; lambda rtol 1e-6; rho, max_dR and
max_dt rtol 1e-6 (rho where the step is above rounding, see STEP_FLOOR); T within 1e-4 m / 1e-4 rad; Tf within 1e-5; fitness rel 1e-6; final H within
1e-9 of its largest entry."""
import ctypes as C
import numpy as np
import pytest
from qn_amd import synth

pytestmark = pytest.mark.gpu

TOL_T, TOL_R = 1e-4, 1e-4
NAN = float("nan")
# rho = (y0 - yi) / predicted decrease is compared on rows whose step is above rounding: a converged run that may not stop takes 1e-9 m steps, and
# both decreases are cancellation noise there.  max_dR / max_dt get an absolute floor of the same size.
STEP_FLOOR_T, STEP_FLOOR_R = 1e-5, 1e-6


def gicp_params(engine, *, k=15, max_iter=32, mcd=52.5, trans_eps=0.01, rot_eps=2e-3, optimizer="lm", lm_max_iter=10, lm_f=1e-9, force=0):
    p = engine.GicpParams(); engine.lib().qn_gicp_default_params(C.byref(p))
    p.k_correspondences, p.max_iterations, p.max_corr_dist, p.transformation_epsilon, p.rotation_epsilon = k, max_iter, mcd, trans_eps, rot_eps
    p.optimizer = 1 if optimizer == "gn" else 0; p.lm_max_iterations = lm_max_iter; p.lm_init_lambda_factor = lm_f; p.force_iterations = force
    return p


def set_params(engine, ctx, p):
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(p)))


def configure(g, *, k=15, max_iter=32, mcd=52.5, trans_eps=0.01, rot_eps=2e-3, optimizer="lm", lm_max_iter=10, lm_f=1e-9, force=0):
    """the NanoGICP setters"""
    g.setCorrespondenceRandomness(k); g.setMaximumIterations(max_iter); g.setMaxCorrespondenceDistance(mcd); g.setTransformationEpsilon(trans_eps)
    g.setRotationEpsilon(rot_eps); g.setOptimizer(optimizer); g.setLMMaxIterations(lm_max_iter); g.setLMInitLambdaFactor(lm_f); g.setForceIterations(force)


def gpu_align(engine, src, tgt, guess=None, knobs=None, ctx=None, **kw):
    """one registration through NanoGICP on a fresh context (or `ctx`) -> (result dict, persist_launches)"""
    own = ctx is None
    if own:
        ctx = engine.Context(max(len(src), len(tgt)) + 1024)
    for kk, v in (knobs or {}).items():
        ctx.debug_set(kk, v)
    g = engine.NanoGICP(ctx); configure(g, **kw)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
    assert g.align(None if guess is None else np.asarray(guess, np.float32)) is not None
    r = g.result_dict(); launches = ctx.debug_get("persist_launches")
    if own:
        ctx.close()
    return r, launches


def orc_align(oracle, src, tgt, guess=None, *, k=15, max_iter=32, mcd=52.5, trans_eps=0.01, rot_eps=2e-3, optimizer="lm", lm_max_iter=10, lm_f=1e-9, force=0):
    o = oracle.GicpOracle(k=k, max_iter=max_iter, max_corr_dist=mcd, trans_eps=trans_eps, rot_eps=rot_eps, optimizer=optimizer, lm_max_iter=lm_max_iter,
                          lm_init_lambda_factor=lm_f, force_iterations=force)
    o.set_source(src); o.compute_covariances(0); o.set_target(tgt); o.compute_covariances(1)
    # the f32 guess the product receives
    return o.align(None if guess is None else np.asarray(guess, np.float32).astype(np.float64)), o


def check(r, ro, what=""):
    assert (r["iterations"], r["converged"], r["lm_failed"]) == (ro["iterations"], ro["converged"], ro["lm_failed"]), what
    tr, tro = r["trace"], ro["trace"]
    assert tr.shape == tro.shape, what
    assert np.array_equal(tr[:, 5:], tro[:, 5:]), what                                    # inner tries, accepted flags
    assert np.allclose(tr[:, 0], tro[:, 0], rtol=1e-8, atol=0), what                      # y0
    assert np.allclose(tr[:, 1], tro[:, 1], rtol=1e-6, atol=0), what                      # lambda
    big = (tro[:, 4] > STEP_FLOOR_T) | (tro[:, 3] > STEP_FLOOR_R)
    assert np.allclose(tr[big, 2], tro[big, 2], rtol=1e-6, atol=1e-9), what               # rho
    assert np.allclose(tr[:, 3], tro[:, 3], rtol=1e-6, atol=1e-2 * STEP_FLOOR_R), what    # max_dR
    assert np.allclose(tr[:, 4], tro[:, 4], rtol=1e-6, atol=1e-2 * STEP_FLOOR_T), what    # max_dt
    assert np.isfinite(r["T"]).all(), what
    dt, dr = synth.pose_error(r["T"], ro["T"])
    assert dt <= TOL_T and dr <= TOL_R, (what, dt, dr)
    assert np.abs(r["Tf"] - ro["Tf"]).max() <= 1e-5, what
    assert abs(r["fitness"] - ro["fitness"]) <= 1e-6 * max(ro["fitness"], 1e-12), what
    assert np.abs(r["H"] - ro["H"]).max() <= 1e-9 * max(np.abs(ro["H"]).max(), 1e-300), what


def rec(r, v, s):
    return (s, v, r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.H).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def host_pairs(clouds):
    return [(s, len(s), t, len(t), 12, 0) for s, t in clouds]


def classic(engine, cap, p, clouds):
    """every pair on ONE classic context, one registration at a time, as a batch member"""
    ctx = engine.Context(cap)
    ctx.debug_set("batch_lanes", 1); ctx.debug_set("batch_member", 1); ctx.debug_set("pair_pipeline", 0)
    set_params(engine, ctx, p)
    res, val, st = engine.gicp_align_batch(ctx, host_pairs(clouds), score_thr=1.5)
    out = [rec(r, v, s) for r, v, s in zip(res, val, st)]
    ctx.close()
    return out


def batched(engine, cap, p, clouds, lanes):
    ctx = engine.Context(cap)
    ctx.debug_set("batch_lanes", lanes)
    set_params(engine, ctx, p)
    res, val, st = engine.gicp_align_batch(ctx, host_pairs(clouds), score_thr=1.5)
    out = [rec(r, v, s) for r, v, s in zip(res, val, st)]
    launches = ctx.debug_get("batch_launches")
    ctx.close()
    return out, launches


def lever(seed):
    src, tgt, guess = synth.lever_arm_pair(seed, rot_sigma=0.1)
    return src, tgt, guess.astype(np.float32)


def lever_moved(seed):
    """a lever-arm pair with its bad guess applied to the source: the batch entry points take no guess, and these pairs reject LM trials from the identity"""
    src, tgt, guess = synth.lever_arm_pair(seed, rot_sigma=0.1)
    return (src.astype(np.float64) @ guess[:3, :3].T + guess[:3, 3]).astype(np.float32), tgt


# ------------------------------------------------------------------------------------------------ LM knobs
@pytest.mark.parametrize("lm_max_iter", [1, 2, 3, 10])
def test_lm_inner_limit(oracle, lm_max_iter):
    from qn_amd import engine
    failed = succeeded_after_rejections = 0
    for seed in (0, 5, 9):
        src, tgt, guess = lever(seed)
        kw = dict(lm_max_iter=lm_max_iter)
        r, _ = gpu_align(engine, src, tgt, guess, **kw)
        ro, _ = orc_align(oracle, src, tgt, guess, **kw)
        check(r, ro, (seed, lm_max_iter))
        failed += r["lm_failed"]
        succeeded_after_rejections += int(((r["trace"][:, 5] > 1) & (r["trace"][:, 6] == 1)).any())
    if lm_max_iter == 10:
        assert failed == 0 and succeeded_after_rejections > 0
    elif lm_max_iter == 1:
        assert failed > 0
    else:
        assert failed + succeeded_after_rejections > 0


@pytest.mark.parametrize("lm_f", [0.0, 1e-6, 1e-3, 1.0, 1e3])
def test_lm_initial_damping(oracle, lm_f):
    from qn_amd import engine
    for seed in (0, 5):
        src, tgt, guess = lever(seed)
        r, _ = gpu_align(engine, src, tgt, guess, lm_f=lm_f)
        ro, _ = orc_align(oracle, src, tgt, guess, lm_f=lm_f)
        check(r, ro, (seed, lm_f))
        if lm_f == 0.0:
            assert (r["trace"][:, 1] == 0).all()          # lambda stays 0
        else:
            assert r["trace"][0, 1] > 0                   # the first trial is damped by lm_f * max |diag H|


def test_refused_lm_parameters():
    from qn_amd import engine
    ctx = engine.Context(4096)
    g = engine.NanoGICP(ctx)
    for f in (-1e-6, -1.0, NAN):
        with pytest.raises(engine.EngineError) as ei:
            g.setLMInitLambdaFactor(f)
        assert ei.value.status == engine.QN_ERR_INVALID_ARG
        g.p.lm_init_lambda_factor = 1e-9
    with pytest.raises(engine.EngineError) as ei:
        g.setLMMaxIterations(0)
    assert ei.value.status == engine.QN_ERR_INVALID_ARG
    g.p.lm_max_iterations = 10
    p = engine.GicpParams(); ctx.check(engine.lib().qn_gicp_get_params(ctx.h, C.byref(p)))
    assert p.lm_init_lambda_factor == 1e-9 and p.lm_max_iterations == 10          # the context kept its parameters
    ctx.close()


# ------------------------------------------------------------------------------------------------ stopping rule
def test_stopping_rule(oracle):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(31, 4000, extent=35.0)
    deciders = set()
    ctx = engine.Context(8192)
    for opt in ("lm", "gn"):
        for rot_eps in (1e-7, 1e-5, 2e-3, 0.1):
            for trans_eps in (1e-6, 5e-4, 0.01):
                kw = dict(rot_eps=rot_eps, trans_eps=trans_eps, optimizer=opt, max_iter=24)
                r, _ = gpu_align(engine, src, tgt, ctx=ctx, **kw)
                ro, _ = orc_align(oracle, src, tgt, **kw)
                check(r, ro, kw)
                if r["converged"]:
                    last, prev = r["trace"][-1], r["trace"][-2] if len(r["trace"]) > 1 else None
                    qr, qt = last[3] / rot_eps, last[4] / trans_eps
                    assert max(qr, qt) < 1
                    # the epsilon that decided: the other ratio was already below 1 one step earlier
                    if prev is not None and prev[3] / rot_eps < 1 <= prev[4] / trans_eps:
                        deciders.add("trans")
                    if prev is not None and prev[4] / trans_eps < 1 <= prev[3] / rot_eps:
                        deciders.add("rot")
    ctx.close()
    assert deciders == {"rot", "trans"}, deciders


@pytest.mark.parametrize("rot_eps,trans_eps", [(NAN, 0.01), (0.0, 0.01), (2e-3, 0.0), (2e-3, NAN), (0.0, 0.0), (NAN, NAN)])
@pytest.mark.parametrize("opt", ["lm", "gn"])
def test_degenerate_epsilons(oracle, rot_eps, trans_eps, opt):
    """converged = max(mr / rotation_epsilon, mt / transformation_epsilon) < 1, std::max's (a < b) ? b : a (include/qn_engine.h): a NaN rotation ratio never
    converges - fmax would drop it and stop on the translation alone - and a NaN translation ratio leaves the decision to the rotation's"""
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(31, 4000, extent=35.0)
    # (LM capped at 6: a run that may not stop reaches 1e-9 m steps after that, where accepting or rejecting a trial is cancellation noise)
    cap = 6 if opt == "lm" else 12
    kw = dict(rot_eps=rot_eps, trans_eps=trans_eps, optimizer=opt, max_iter=cap)
    r, _ = gpu_align(engine, src, tgt, **kw)
    ro, _ = orc_align(oracle, src, tgt, **kw)
    check(r, ro, kw)
    if rot_eps != rot_eps or rot_eps == 0.0 or trans_eps == 0.0:
        assert not r["converged"] and r["iterations"] == cap
    else:
        assert r["converged"]


def test_zero_rotation_epsilon_on_an_exact_identity_step(oracle):
    """rotation_epsilon = 0 and a step whose rotation is exactly the identity (0 / 0 = NaN): a gate below every NN distance gives H = 0 and the zero step.
    The translation alone (0 / 0.01 = 0) would stop it; the NaN rotation ratio must not."""
    from qn_amd import engine
    src, tgt, mcd = tiny_gate_pair(oracle)
    for opt in ("lm", "gn"):
        kw = dict(rot_eps=0.0, mcd=mcd, optimizer=opt, max_iter=3)
        r, _ = gpu_align(engine, src, tgt, **kw)
        ro, _ = orc_align(oracle, src, tgt, **kw)
        check(r, ro, kw)
        assert not r["converged"] and r["iterations"] == 3 and (r["trace"][:, 3:5] == 0).all()


# ------------------------------------------------------------------------------------------------ iteration caps
@pytest.mark.parametrize("max_iter", [0, 1, 2])
@pytest.mark.parametrize("opt", ["lm", "gn"])
def test_iteration_caps(oracle, max_iter, opt):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(32, 4000, extent=35.0)
    ctx = engine.Context(8192)
    for guess in (None, np.array([[1, 0, 0, 0.4], [0, 1, 0, -0.3], [0, 0, 1, 0.1], [0, 0, 0, 1]], np.float32)):
        kw = dict(max_iter=max_iter, optimizer=opt)
        r, _ = gpu_align(engine, src, tgt, guess, ctx=ctx, **kw)
        ro, _ = orc_align(oracle, src, tgt, guess, **kw)
        check(r, ro, (kw, guess is not None))
        assert r["iterations"] == max_iter
        if max_iter == 0:
            assert not r["converged"] and len(r["trace"]) == 0
            assert np.array_equal(r["Tf"], np.eye(4, dtype=np.float32) if guess is None else guess)
            assert np.array_equal(r["H"], ro["H"])
    ctx.close()


@pytest.mark.parametrize("opt", ["lm", "gn"])
def test_batch_at_zero_iterations_takes_the_one_pair_path(oracle, opt):
    from qn_amd import engine
    clouds = [synth.make_pair(33 + i, 3000 + 500 * i, extent=35.0)[:2] for i in range(3)]
    p = gicp_params(engine, max_iter=0, optimizer=opt)
    ref = classic(engine, 8192, p, clouds)
    got, launches = batched(engine, 8192, p, clouds, lanes=2)
    assert launches == 0                                  # batch_supported: no lanes at 0 iterations
    assert got == ref
    for (s, t), g in zip(clouds, got):
        ro, _ = orc_align(oracle, s, t, max_iter=0, optimizer=opt)
        assert g[2] == 0 and not g[3] and not g[4]
        assert abs(g[5] - ro["fitness"]) <= 1e-6 * ro["fitness"]
        assert np.frombuffer(g[8], np.float32).reshape(4, 4).tolist() == np.eye(4).tolist()


# ------------------------------------------------------------------------------------------------ correspondence gate
@pytest.mark.parametrize("mcd", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("mode", ["lm", "gn", "gn_forced"])
def test_gate_in_full_aligns(oracle, mcd, mode):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(63, 8000, extent=40.0, shift=8.0)
    kw = dict(mcd=mcd, optimizer="lm" if mode == "lm" else "gn", force=12 if mode == "gn_forced" else 0, max_iter=32)
    r, _ = gpu_align(engine, src, tgt, **kw)
    ro, o = orc_align(oracle, src, tgt, **kw)
    check(r, ro, kw)
    _, _, _, corr, _ = o.linearize(ro["T"])
    assert (corr < 0).mean() > 0.01, (corr < 0).mean()      # the gate rejects a real share of the points at the end


def tiny_gate_pair(oracle):
    src, tgt, _ = synth.make_pair(34, 3000, extent=35.0)
    o = oracle.GicpOracle(k=15); o.set_source(src); o.compute_covariances(0); o.set_target(tgt); o.compute_covariances(1)
    _, _, _, _, sqd = o.linearize(np.eye(4))
    return src, tgt, 0.25 * float(np.sqrt(sqd.min()))


@pytest.mark.parametrize("opt", ["lm", "gn"])
def test_gate_below_every_distance(oracle, opt):
    """H = 0: the unpivoted factorisation fails, the pivoted one gives the zero step - converged at iteration 1, T = guess, no NaN"""
    from qn_amd import engine
    src, tgt, mcd = tiny_gate_pair(oracle)
    guess = np.eye(4, dtype=np.float32); guess[:3, 3] = [1e-4, 0.0, 0.0]
    for gs in (None, guess):
        r, _ = gpu_align(engine, src, tgt, gs, mcd=mcd, optimizer=opt)
        ro, _ = orc_align(oracle, src, tgt, gs, mcd=mcd, optimizer=opt)
        check(r, ro, opt)
        assert r["converged"] and r["iterations"] == 1 and np.isfinite(r["T"]).all() and np.isfinite(r["trace"][:, [0, 1, 3, 4]]).all()      # (rho = 0 / 0, as the oracle's)
        assert np.array_equal(r["Tf"], np.eye(4, dtype=np.float32) if gs is None else gs)
        assert not r["H"].any()


def test_lm_with_a_handful_of_correspondences(oracle):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(35, 3000, extent=35.0)
    o = oracle.GicpOracle(k=15); o.set_source(src); o.compute_covariances(0); o.set_target(tgt); o.compute_covariances(1)
    _, _, _, _, sqd = o.linearize(np.eye(4))
    d = np.sort(np.unique(sqd))
    mcd = float(np.sqrt(0.5 * (float(d[7]) + float(d[8]))))        # between the 8th and the 9th smallest distance at the start
    r, _ = gpu_align(engine, src, tgt, mcd=mcd)
    ro, o2 = orc_align(oracle, src, tgt, mcd=mcd)
    _, _, _, corr, _ = o2.linearize(np.eye(4))
    assert 1 <= (corr >= 0).sum() <= 16
    check(r, ro, mcd)


def lattice_pair(n=48):
    """a square lattice (spacing 1, z = 0) and the same lattice 0.5 above it: every NN squared distance is exactly 0.25"""
    gx, gy = np.meshgrid(np.arange(n, dtype=np.float32) - n / 2, np.arange(n, dtype=np.float32) - n / 2)
    src = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n, np.float32)], 1).astype(np.float32)
    tgt = src.copy(); tgt[:, 2] = 0.5
    return src, tgt


def test_gate_exactly_on_the_threshold(oracle):
    from qn_amd import engine
    src, tgt = lattice_pair()
    ctx = engine.Context(8192)
    for mcd, gated_in in ((0.5, False), (float(np.nextafter(0.5, 1.0)), True)):
        g = engine.NanoGICP(ctx); configure(g, mcd=mcd)
        g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
        H, b, e, corr, sqd = g.linearize(np.eye(4))
        o = oracle.GicpOracle(k=15, max_corr_dist=mcd); o.set_source(src); o.compute_covariances(0); o.set_target(tgt); o.compute_covariances(1)
        Ho, bo, eo, co, so = o.linearize(np.eye(4))
        assert (sqd == np.float32(0.25)).all() and np.array_equal(sqd, so)
        assert np.array_equal(corr, co) and ((corr >= 0).all() if gated_in else (corr < 0).all())
        assert np.abs(H - Ho).max() <= 1e-9 * max(np.abs(Ho).max(), 1e-300)
    ctx.close()
    # forced GN at the gate 0.5: nothing survives, the pose stays put, and every tick - unseeded, tracked (persist = 0), persistent - re-gates the same 0.25
    kw = dict(mcd=0.5, optimizer="gn", force=10, max_iter=10)
    ro, _ = orc_align(oracle, src, tgt, **kw)
    assert not ro["H"].any()
    for knobs in ({"persist": 0}, {}):
        r, launches = gpu_align(engine, src, tgt, knobs=knobs, **kw)
        check(r, ro, knobs)
        assert np.array_equal(r["H"], ro["H"])
        if not knobs:
            assert launches > 0, "the persistent kernel did not run"
    # and one f32 step above: everything is in, the same path compared
    kw["mcd"] = float(np.nextafter(0.5, 1.0))
    ro, _ = orc_align(oracle, src, tgt, **kw)
    for knobs in ({"persist": 0}, {}):
        r, _ = gpu_align(engine, src, tgt, knobs=knobs, **kw)
        check(r, ro, ("in", knobs))


# ------------------------------------------------------------------------------------------------ small k
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_small_k(oracle, k):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(36, 5000, extent=35.0)
    ctx = engine.Context(8192)
    g = engine.NanoGICP(ctx); configure(g, k=k)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
    o = oracle.GicpOracle(k=k, max_iter=32, max_corr_dist=52.5, trans_eps=0.01)
    o.set_source(src); o.compute_covariances(0); o.set_target(tgt); o.compute_covariances(1)
    differ = 0
    for which, cloud in ((0, src), (1, tgt)):
        Cg, Co = g.covariances(which), o.covariances(which)
        if k == 1:
            # one point: a zero scatter matrix, whose eigenvectors are the Jacobi start - the identity - for both solvers
            assert np.abs(Cg - Co).max() < 1e-12
        for Cm in (Cg, Co):
            w = np.linalg.eigvalsh(Cm)
            assert np.allclose(w, [1e-3, 1, 1], atol=1e-12)               # PLANE regularisation, whatever the neighbourhood
        # where the normal is unique: the raw scatter's two smallest eigenvalues differ by a relative gap of 1e-6 of the largest
        idx, _ = o.knn(which, cloud, k)
        nb = cloud[idx].astype(np.float64); nb -= nb.mean(1, keepdims=True)
        ws = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", nb, nb) / k)
        unique = (ws[:, 1] - ws[:, 0]) > 1e-6 * np.maximum(ws[:, 2], 1e-300)
        diff = np.abs(Cg - Co).reshape(len(cloud), -1).max(1)
        assert (diff[unique] < 1e-9).all(), (k, which, int((diff[unique] >= 1e-9).sum()))
        differ += int((diff[~unique] >= 1e-9).sum())
    print("k = %d: %d covariances with a non-unique normal where the two solvers picked different planes" % (k, differ))
    g.align(); r = g.result_dict(); ro = o.align()
    if differ == 0:
        check(r, ro, k)
    else:                                   # different (equally valid) normals: the same registration within the north-star bar
        dt, dr = synth.pose_error(r["T"], ro["T"])
        assert dt <= TOL_T and dr <= TOL_R, (k, dt, dr)
    ctx.close()


# ------------------------------------------------------------------------------------------------ every path, same parameters
PATH_CASES = {
    "lm_limit": dict(lm_max_iter=2),
    "lm_damping": dict(lm_f=1e3),
    "gate": dict(mcd=1.0),
    "rot_eps_nan": dict(rot_eps=NAN, max_iter=10),
    "gn_forced_gate": dict(mcd=1.0, optimizer="gn", force=10, max_iter=10),
}


def path_clouds(name):
    if name in ("lm_limit", "lm_damping"):
        return [lever_moved(s) for s in (0, 5, 9)] + [synth.make_pair(37, 5000, extent=35.0, shift=6.0)[:2]]
    return [synth.make_pair(38 + i, 4000 + 1000 * i, extent=35.0, shift=2.0 + 2.0 * i)[:2] for i in range(5)]


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_every_path_same_parameters(oracle, name):
    from qn_amd import engine
    kw = PATH_CASES[name]
    clouds = path_clouds(name)
    cap = max(max(len(s), len(t)) for s, t in clouds) + 1024
    p = gicp_params(engine, **kw)
    ref = classic(engine, cap, p, clouds)
    for (s, t), rr in zip(clouds, ref):                 # the classic chain against the oracle
        ro, _ = orc_align(oracle, s, t, **kw)
        assert (rr[2], bool(rr[3]), bool(rr[4])) == (ro["iterations"], ro["converged"], ro["lm_failed"]), name
        dt, dr = synth.pose_error(np.frombuffer(rr[6]).reshape(4, 4), ro["T"])
        assert dt <= TOL_T and dr <= TOL_R, (name, dt, dr)
    if name == "lm_limit":
        assert any(rr[4] for rr in ref), "no lane took the lm-failed path"
    for lanes in (2, 8):                                # 2 lanes: ragged for the five-pair cases; 8 lanes: one partial run
        got, launches = batched(engine, cap, p, clouds, lanes)
        assert launches > 0 and got == ref, (name, lanes)
    ctxs = []
    for _ in range(3):
        c = engine.Context(cap); set_params(engine, c, p); ctxs.append(c)
    res, val, st = engine.icp_alignment_batch(ctxs, host_pairs(clouds), score_thr=1.5)
    assert [rec(r, v, s) for r, v, s in zip(res, val, st)] == ref, name
    for c in ctxs:
        c.close()
    if kw.get("force") and kw.get("optimizer") == "gn":
        launched = 0
        for s, t in clouds:                             # a lone registration (the persistent kernel where it takes over) against the chain alone
            a, la = gpu_align(engine, s, t, **kw)
            b, lb = gpu_align(engine, s, t, knobs={"persist": 0}, **kw)
            assert lb == 0 and a["T"].tobytes() == b["T"].tobytes() and a["H"].tobytes() == b["H"].tobytes() and a["fitness"] == b["fitness"]
            assert np.array_equal(a["trace"], b["trace"])
            launched += la
        assert launched > 0, "the persistent kernel never ran"


def test_persistent_kernel_with_non_default_parameters(oracle):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(39, 30000)
    for kw in (dict(optimizer="gn", force=12, max_iter=12, mcd=1.0, k=8),
               dict(optimizer="gn", force=10, max_iter=10, mcd=3.0, k=5, rot_eps=NAN, trans_eps=1e-6)):
        a, la = gpu_align(engine, src, tgt, **kw)
        b, lb = gpu_align(engine, src, tgt, knobs={"persist": 0}, **kw)
        assert la > 0 and lb == 0, "the persistent kernel did not run"
        for key in ("T", "H", "trace"):
            assert np.array_equal(a[key], b[key]), key
        assert a["fitness"] == b["fitness"]
        ro, _ = orc_align(oracle, src, tgt, **kw)
        check(a, ro, kw)


@pytest.mark.parametrize("name", ["lm_limit", "gate", "rot_eps_nan"])
def test_coarse_to_fine_batch_fine_stage(oracle, name):
    from qn_amd import engine
    kw = dict(PATH_CASES[name])
    clouds = [synth.make_pair(330 + i, 6000, extent=42.0, mode="quatro")[:2] for i in range(3)]
    p = gicp_params(engine, **kw)
    ctx = engine.Context(8192); ctx.debug_set("batch_lanes", 2); set_params(engine, ctx, p); engine.Quatro(ctx)
    got = engine.coarse_to_fine_align_batch([ctx], host_pairs(clouds))
    one = engine.Context(8192); set_params(engine, one, p); engine.Quatro(one)
    okw = dict(k=15, max_iter=kw.get("max_iter", 32), max_corr_dist=kw.get("mcd", 52.5), trans_eps=0.01, rot_eps=kw.get("rot_eps", 2e-3),
               lm_max_iter=kw.get("lm_max_iter", 10))
    for (s, t), g in zip(clouds, got):
        a, ns, stride = engine._cloud_arg(s); b, nt, _ = engine._cloud_arg(t)
        res = engine.GicpResult(); valid = C.c_int(); T = np.zeros((4, 4)); Tq = np.zeros((4, 4))
        one.check(engine.lib().qn_coarse_to_fine_alignment(one.h, engine._p(a), C.c_uint32(ns), engine._p(b), C.c_uint32(nt), C.c_uint32(stride), C.c_double(1.5),
                                                           C.byref(res), engine._p(T), engine._p(Tq), C.byref(valid)))
        assert g["status"] == 0 and g["valid"] == bool(valid.value) and g["iterations"] == res.iterations and g["score"] == res.fitness
        assert np.array_equal(g["T"], T) and np.array_equal(g["T_quatro"], Tq)
        o = oracle.coarse_to_fine_alignment(s, t, **okw)
        assert g["valid"] == o["valid"], name
        if o["valid"]:
            assert g["iterations"] == o["iterations"] and g["converged"] == o["converged"]
            dt, dr = synth.pose_error(g["T"], o["T"])
            assert dt <= TOL_T and dr <= TOL_R, (name, dt, dr)
    assert ctx.debug_get("batch_pairs") > 0, "the fine stage did not go through the lanes"
    ctx.close(); one.close()


# ------------------------------------------------------------------------------------------------ parameter changes between calls
A_KW = dict(mcd=52.5, lm_max_iter=10, lm_f=1e-9, rot_eps=2e-3, trans_eps=0.01)
B_KW = dict(mcd=1.0, lm_max_iter=3, lm_f=1e-3, rot_eps=1e-5, trans_eps=5e-4, max_iter=12)


def test_parameter_change_between_aligns():
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(37, 5000, extent=35.0, shift=6.0)
    guess = None
    ctx = engine.Context(8192)
    g = engine.NanoGICP(ctx); configure(g, **A_KW)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
    g.align(guess); ra = g.result_dict()
    configure(g, **B_KW)
    g.align(guess); rb = g.result_dict()
    fresh, _ = gpu_align(engine, src, tgt, guess, **B_KW)
    for key in ("T", "H", "trace"):
        assert np.array_equal(rb[key], fresh[key], equal_nan=True), key
    assert (rb["iterations"], rb["lm_failed"], rb["fitness"]) == (fresh["iterations"], fresh["lm_failed"], fresh["fitness"])
    assert ra["T"].tobytes() != rb["T"].tobytes()
    # changing k: the covariances must be recomputed (qn_gicp_set_params drops them) - an align without them is refused as not ready
    g.setCorrespondenceRandomness(8)
    assert g.align(guess) is None
    g.calculateSourceCovariances(); g.calculateTargetCovariances()
    g.align(guess); rk = g.result_dict()
    fk, _ = gpu_align(engine, src, tgt, guess, **dict(B_KW, k=8))
    assert np.array_equal(rk["T"], fk["T"]) and np.array_equal(rk["trace"], fk["trace"], equal_nan=True)
    ctx.close()


def test_parameter_change_between_batches():
    """two qn_gicp_align_batch calls on one context: the lanes' sub-contexts keep their clouds and must take the new parameters"""
    from qn_amd import engine
    clouds = [lever_moved(s) for s in (0, 5, 9)] + [synth.make_pair(40, 5000, extent=35.0, shift=6.0)[:2]]
    pa, pb = gicp_params(engine, **A_KW), gicp_params(engine, **B_KW)
    ctx = engine.Context(8192); ctx.debug_set("batch_lanes", 4)
    set_params(engine, ctx, pa)
    res, val, st = engine.gicp_align_batch(ctx, host_pairs(clouds))
    first = [rec(r, v, s) for r, v, s in zip(res, val, st)]
    set_params(engine, ctx, pb)
    res, val, st = engine.gicp_align_batch(ctx, host_pairs(clouds))
    second = [rec(r, v, s) for r, v, s in zip(res, val, st)]
    ctx.close()
    # against the classic chain, which reads the context's own parameters (the lanes of a fresh batch context would share a stale copy's error)
    assert first == classic(engine, 8192, pa, clouds)
    assert second == classic(engine, 8192, pb, clouds)
    assert second != first


# ------------------------------------------------------------------------------------------------ getFitnessScore(max_range)
def test_fitness_max_range(oracle):
    from qn_amd import engine
    src, tgt, _ = synth.make_pair(41, 6000, extent=40.0, shift=8.0)
    ctx = engine.Context(8192)
    g = engine.NanoGICP(ctx); configure(g)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
    g.align(); r = g.result_dict()
    ro, o = orc_align(oracle, src, tgt)
    Tf = r["Tf"]
    # the f32 squared NN distances at the result: one range exactly at a present distance (the comparison is <=)
    pts = o.transformed_source(Tf)
    _, d2 = o.knn(1, pts, 1)
    present = float(np.sort(d2[:, 0])[len(d2) // 2])
    # (pcl compares the SQUARED distance with max_range; the root of a present one is a range like any other)
    for max_range in (0.01, 0.25, 1.0, present, float(np.nextafter(present, 0.0)), float(np.sqrt(present)), 25.0):
        got, want = g.getFitnessScore(max_range), o.fitness(Tf, max_range)
        assert abs(got - want) <= 1e-9 * want, (max_range, got, want)
    ctx.close()
