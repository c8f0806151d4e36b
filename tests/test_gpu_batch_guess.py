"""qn_gicp_align_batch_guess: the batched registration from a per-pair initial guess (align(output, guess), what qn_gicp_align(guess) runs).  The guesses
reach each lane's k_init_state through the segment's argument upload, so a guessed batch must equal the one-pair path with the same guesses BIT FOR BIT -
lanes 3 and 8, a ragged tail, a shared source on and off; it must agree with the oracle's align(guess); guesses = None is qn_gicp_align_batch itself; and
non-finite or non-rigid guesses are refused before anything runs."""
import ctypes as C
import math
import numpy as np
import pytest
from qn_amd import synth

pytestmark = pytest.mark.gpu


def params(engine, *, k=15, max_iter=32, eps=0.01, max_corr=52.5):
    p = engine.GicpParams(); engine.lib().qn_gicp_default_params(C.byref(p))
    p.k_correspondences = k; p.max_iterations = max_iter; p.max_corr_dist = max_corr; p.transformation_epsilon = eps
    return p


def rec(r, v, s):
    return (s, v, r.iterations, r.converged, r.lm_failed, r.fitness, np.array(r.T64).tobytes(), np.array(r.H).tobytes(), np.array(r.T, dtype=np.float32).tobytes())


def run(engine, cap, pairs, guesses, lanes, knobs=None):
    """lanes = 1: every pair on ONE classic context, one registration at a time, as a batch member (the one-pair path with the guess)"""
    ctx = engine.Context(cap)
    ctx.debug_set("batch_lanes", lanes)
    if lanes == 1:
        ctx.debug_set("batch_member", 1); ctx.debug_set("pair_pipeline", 0)
    for k, v in (knobs or {}).items():
        ctx.debug_set(k, v)
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(params(engine))))
    res, val, st = engine.gicp_align_batch(ctx, pairs, score_thr=1.5, guesses=guesses)
    out = [rec(r, v, s) for r, v, s in zip(res, val, st)]
    ctx.close()
    return out


def _rz(deg, t=(0.0, 0.0, 0.0)):
    a = math.radians(deg)
    G = np.eye(4); G[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]; G[:3, 3] = t
    return G


GUESSES = [np.eye(4), _rz(0, (3.0, 0.0, 0.0)), _rz(90), _rz(180), _rz(0, (0.0, -3.0, 0.5)), _rz(90, (3.0, 0.0, 0.0)), _rz(180, (-2.0, 2.0, 0.0))]


def _cases():
    """seven pairs: four against ONE source buffer (the candidates of one query), three of their own; target i is the scene seen from guess i, so
    guess i (f32-rounded, as the engine receives it) starts each registration near its answer G_i T_i"""
    out = []
    s0, t0, T0 = synth.make_pair(910, 5000, extent=40.0, shift=2.0)
    for i in range(7):
        s, t, T = (s0, t0, T0) if i < 4 else synth.make_pair(910 + i, 4000 + 700 * i, extent=40.0, shift=2.0)
        G = GUESSES[i].astype(np.float32).astype(np.float64)
        tg = (t.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
        out.append((s, tg, G, G @ T))
    return out


def _pairs(cases):
    return [(s, len(s), t, len(t), 12, 0) for s, t, _, _ in cases]


@pytest.mark.parametrize("lanes", [3, 8])
@pytest.mark.parametrize("share", [1, 0])
def test_guessed_batches_equal_the_one_pair_path(lanes, share):
    from qn_amd import engine
    cases = _cases()
    pairs, guesses = _pairs(cases), [G for _, _, G, _ in cases]
    ref = run(engine, 20000, pairs, guesses, 1, {"batch_share_source": share})
    got = run(engine, 20000, pairs, guesses, lanes, {"batch_share_source": share})
    assert [g[0] for g in got] == [0] * 7
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, "pair %d differs from the one-pair path (lanes %d, share %d)" % (i, lanes, share)


def test_guessed_records_agree_with_the_oracle():
    from qn_amd import engine
    from oracle import oracle as orc
    cases = _cases()
    ctx = engine.Context(20000)
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(params(engine))))
    res, val, st = engine.gicp_align_batch(ctx, _pairs(cases), guesses=[G for _, _, G, _ in cases])
    both = 0
    for i, ((s, t, G, truth), r) in enumerate(zip(cases, res)):
        g = orc.GicpOracle(k=15, max_iter=32, max_corr_dist=52.5, trans_eps=0.01)
        g.set_source(s); g.compute_covariances(0); g.set_target(t); g.compute_covariances(1)
        o = g.align(G)
        assert st[i] == 0
        if not (r.converged and o["converged"]):
            continue
        both += 1
        T = np.array(r.T, dtype=np.float32).reshape(4, 4).astype(np.float64)
        dt, dr = synth.pose_error(T, o["Tf"].astype(np.float64))
        assert dt <= 1e-4 and dr <= 1e-4, (i, dt, dr)
        et, er = synth.pose_error(T, truth)
        assert et < 0.1 and er < math.radians(0.5), (i, et, er)          # the guess brought it home: yaw 90 / 180 included
    assert both >= 5, both
    ctx.close()


def test_no_guesses_is_the_unguessed_batch():
    from qn_amd import engine
    cases = _cases()[3:]
    pairs = _pairs(cases)
    ctx = engine.Context(20000)
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(params(engine))))
    plain = [rec(*x) for x in zip(*engine.gicp_align_batch(ctx, pairs))]
    n = len(pairs)
    descs = (engine.PairDesc * n)(*[engine.PairDesc(s.ctypes.data, ns, t.ctypes.data, nt, 12, 0) for s, ns, t, nt, _, _ in pairs])
    res = (engine.GicpResult * n)(); val = (C.c_int * n)(); st = (C.c_int * n)()
    ctx.check(engine.lib().qn_gicp_align_batch_guess(ctx.h, descs, None, C.c_uint32(n), C.c_double(1.5), res, val, st))
    assert [rec(*x) for x in zip(res, val, st)] == plain
    eye = [rec(*x) for x in zip(*engine.gicp_align_batch(ctx, pairs, guesses=[np.eye(4)] * n))]
    assert eye == plain                                                   # an identity guess starts from the same state
    ctx.close()


def test_bad_guesses_are_refused_before_anything_runs():
    from qn_amd import engine
    cases = _cases()[4:]
    pairs = _pairs(cases)
    ctx = engine.Context(20000)
    ctx.debug_set("batch_lanes", 3)
    ctx.check(engine.lib().qn_gicp_set_params(ctx.h, C.byref(params(engine))))
    good = [np.eye(4)] * len(pairs)
    before = ctx.debug_get("batch_pairs"), ctx.debug_get("batch_launches")
    for bad in [(1, 3, float("nan")), (2, 0, float("inf")), (0, 5, -float("inf")), (1, 14, 1.0), (2, 15, 2.0), (0, 12, 1e-3)]:
        gs = [g.copy() for g in good]
        i, j, v = bad
        gs[i].reshape(-1)[j] = v
        with pytest.raises(engine.EngineError) as e:
            engine.gicp_align_batch(ctx, pairs, guesses=gs)
        assert e.value.status == engine.QN_ERR_INVALID_ARG, bad
        assert (ctx.debug_get("batch_pairs"), ctx.debug_get("batch_launches")) == before, bad
    res, val, st = engine.gicp_align_batch(ctx, pairs, guesses=good)
    assert list(st) == [0] * len(pairs)
    ctx.close()
