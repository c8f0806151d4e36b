"""CPU-side tests of the Quatro path: oracle known-answer tests, and the PRODUCT's host solver
(qn_quatro_solve: max clique, yaw-only GNC-TLS rotation, TLS translation - pure host C++ inside
libqn_engine.so, no GPU call) against the oracle's independent implementation."""
import itertools
import numpy as np
import pytest
from qn_amd import synth


def yaw_T(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4); T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]; T[:3, 3] = t
    return T


def test_atan2_polynomial_accuracy(oracle):
    import ctypes as C
    f = oracle.lib().orc_atan2f; f.restype = C.c_float
    rng = np.random.default_rng(0)
    for y, x in rng.normal(size=(3000, 2)).astype(np.float32):
        assert abs(f(C.c_float(y), C.c_float(x)) - np.arctan2(float(y), float(x))) < 5e-7
    assert f(C.c_float(0), C.c_float(0)) == 0.0


def test_max_clique_lexicographic_vs_bruteforce(oracle):
    rng = np.random.default_rng(1)
    for n, p in [(9, 0.5), (12, 0.6), (14, 0.7)]:
        A = (rng.random((n, n)) < p).astype(np.uint8); A = np.triu(A, 1); A = A + A.T
        best = []
        for r in range(n, 0, -1):
            cl = [c for c in itertools.combinations(range(n), r) if all(A[i, j] for i, j in itertools.combinations(c, 2))]
            if cl:
                best = list(min(cl)); break
        assert oracle.max_clique(A).tolist() == best


def test_fpfh_plane_has_peaked_histograms(oracle):
    """All normals parallel on a plane => alpha = 0 (bin 5), phi = 0 (bin 5) for every pair."""
    g = np.stack(np.meshgrid(np.arange(0, 12, 0.3), np.arange(0, 12, 0.3)), -1).reshape(-1, 2)
    pts = np.c_[g + 5.0, np.full(len(g), 1.0)].astype(np.float32)
    nrm, sp, fp = oracle.quatro_fpfh(pts, 0.9, 1.5)
    inner = (g[:, 0] > 2) & (g[:, 0] < 9) & (g[:, 1] > 2) & (g[:, 1] < 9)
    assert np.allclose(np.abs(nrm[inner, 2]), 1.0, atol=1e-6)
    assert np.allclose(fp[inner, 11 + 5], 100.0, atol=1e-3) and np.allclose(fp[inner, 22 + 5], 100.0, atol=1e-3)
    assert np.allclose(fp[inner].reshape(-1, 3, 11).sum(2), 100.0, atol=1e-3)


def test_solver_recovers_planar_motion_with_outliers(oracle):
    rng = np.random.default_rng(2)
    src = rng.uniform(-20, 20, size=(60, 3)).astype(np.float32); src[:, 2] = rng.uniform(0, 3, 60)
    T = yaw_T(0.7, [3.0, -2.0, 0.1])
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.02, (60, 3))).astype(np.float32)
    dst[40:] = rng.uniform(-20, 20, size=(20, 3))                   # 1/3 outliers
    corres = np.c_[np.arange(60), np.arange(60)]
    r = oracle.quatro_solve(src, dst, corres)
    assert r["valid"] and set(range(40)) <= set(r["clique"].tolist())
    dt, dr = synth.pose_error(r["T"], T)
    assert dt < 0.1 and dr < 0.01


@pytest.mark.parametrize("seed", range(6))
def test_product_host_solver_matches_oracle(oracle, seed):
    from qn_amd import engine
    rng = np.random.default_rng(100 + seed)
    n = 80
    src = rng.uniform(-25, 25, size=(n, 3)).astype(np.float32); src[:, 2] = rng.uniform(0, 4, n)
    T = yaw_T(rng.uniform(-3, 3), [rng.uniform(-8, 8), rng.uniform(-8, 8), 0.05])
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    bad = rng.choice(n, n // 2, replace=False); dst[bad] = rng.uniform(-25, 25, size=(len(bad), 3))
    idx = np.sort(rng.permutation(n)[:70])
    corres = np.c_[idx, idx]
    a = engine.quatro_solve(src, dst, corres)
    b = oracle.quatro_solve(src, dst, corres)
    assert a["valid"] == b["valid"] and a["clique"].tolist() == b["clique"].tolist()
    assert np.abs(a["T"] - b["T"]).max() < 1e-9


@pytest.mark.parametrize("seed,true_scale,noise", [(0, 1.37, 0.05), (1, 0.8, 0.02), (2, 1.0, 0.05), (3, 2.5, 0.1), (4, 1.1, 0.0)])
def test_scale_estimation_three_implementations(oracle, seed, true_scale, noise):
    """estimate_scale = true (estimat_scale_, loop_closure.h:44 / loop_closure.cpp:24): TEASER++'s TLS scale solver over the TIM norm ratios in front of the consistency graph.
    The PRODUCT's host solver (qn_quatro_solve_scaled), the C++ oracle and the independent numpy restatement (oracle/py_quatro.py) on the same correspondences with a third of
    outliers: same clique, same scale (1e-12), same pose (1e-9), and the known scale / yaw / translation recovered."""
    from qn_amd import engine
    from oracle import py_quatro as pq
    rng = np.random.default_rng(900 + seed)
    M = 110
    src = rng.uniform(-20, 20, size=(M, 3)).astype(np.float32); src[:, 2] = rng.uniform(0, 4, M)
    T = yaw_T(rng.uniform(-3, 3), [rng.uniform(-6, 6), rng.uniform(-6, 6), 0.3])
    dst = (true_scale * (src.astype(np.float64) @ T[:3, :3].T) + T[:3, 3] + rng.normal(0, noise, (M, 3))).astype(np.float32)
    bad = rng.choice(M, M // 3, replace=False); dst[bad] = rng.uniform(-30, 30, size=(len(bad), 3))
    corres = np.c_[np.arange(M), np.arange(M)].astype(np.int32)
    ep = engine.quatro_default_params(); ep.estimate_scale = 1
    a = engine.quatro_solve(src, dst, corres, ep)
    b = oracle.quatro_solve_scaled(src, dst, corres, oracle.QuatroParams(estimate_scale=True))
    c = pq.solve(src, dst, corres, pq.Params(estimate_scale=True))
    assert a["valid"] and b["valid"] and c["valid"]
    assert a["clique"].tolist() == b["clique"].tolist() == list(c["clique"])
    assert abs(a["scale"] - b["scale"]) <= 1e-12 and abs(b["scale"] - c["scale"]) <= 1e-12
    assert np.abs(a["T"] - b["T"]).max() < 1e-9 and np.abs(b["T"] - c["T"]).max() < 1e-9
    good = sorted(set(range(M)) - set(bad.tolist()))
    assert len(set(good) & set(a["clique"].tolist())) >= 0.8 * len(good)
    assert abs(a["scale"] - true_scale) < 0.02 * true_scale + 3 * noise / 10
    dt, dr = synth.pose_error(a["T"], T)
    assert dt < 0.1 + 3 * noise and dr < 0.01 + noise / 5
    # and with the flag off the product still takes the fixed-scale path (the reference's shipped configuration): identical to before
    a1 = engine.quatro_solve(src, dst, corres); b1 = oracle.quatro_solve(src, dst, corres)
    assert a1["scale"] == 1.0 and a1["valid"] == b1["valid"] and a1["clique"].tolist() == b1["clique"].tolist()


def test_scalar_tls_with_ranges_known_answers():
    """the scale stage's estimator (numpy restatement): an exact consensus is returned exactly, outliers with tight ranges lose to a majority with loose ones, ties in the
    sweep resolve like the C++ sort"""
    from oracle import py_quatro as pq
    est, inl = pq._tls_ranges([2.0, 2.0, 2.0, 5.0], [0.1, 0.1, 0.1, 0.1])
    assert est == 2.0 and inl.tolist() == [True, True, True, False]
    est, inl = pq._tls_ranges([1.0, 1.02, 0.98, 3.0, 3.01], [0.05, 0.05, 0.05, 0.001, 0.001])
    assert abs(est - 1.0) < 0.02 and inl.tolist() == [True, True, True, False, False]
    est, inl = pq._tls_ranges([1.5], [0.2])
    assert est == 1.5 and inl.tolist() == [True]


def test_oracle_coarse_to_fine_recovers_large_yaw(oracle):
    src, tgt, T = synth.make_pair(300, 6000, extent=40.0, mode="quatro")
    r = oracle.coarse_to_fine_alignment(src, tgt)
    assert r["quatro"]["valid"]
    dt, dr = synth.pose_error(r["quatro"]["T"], T)
    assert dt < 3.0 and dr < 0.2                                   # coarse stage: loose
    dt, dr = synth.pose_error(r["T"], T)
    assert r["converged"] and dt < 0.05 and dr < 0.005             # after Nano-GICP refinement


@pytest.mark.parametrize("n,inlier_frac,noise,seed", [(177, 0.5, 0.05, 1), (200, 1.0, 0.02, 2), (120, 0.0, 0.0, 3), (300, 0.4, 0.08, 4),
                                                       (600, 0.2, 0.05, 5), (1100, 0.1, 0.05, 6), (2, 1.0, 0.0, 7), (1, 1.0, 0.0, 8), (260, 0.7, 0.15, 9)])
def test_product_clique_search_matches_oracle_on_hard_graphs(oracle, n, inlier_frac, noise, seed):
    """The product's maximum-clique search (stack bit sets, degree relabelling, k-core peeling, witness clique - qn_quatro_host.inc) against
    the oracle's independent implementation: dense consistency graphs (many inliers, loose noise: lots of near-maximum cliques), all
    inliers, none, sizes across the bit-set widths (<= 256, <= 1024, <= 4096).  Same lexicographically smallest maximum clique, same T."""
    from qn_amd import engine
    rng = np.random.default_rng(500 + seed)
    src = rng.uniform(-30, 30, size=(n, 3)).astype(np.float32); src[:, 2] = rng.uniform(0, 5, n)
    T = yaw_T(rng.uniform(-3, 3), [rng.uniform(-6, 6), rng.uniform(-6, 6), 0.1])
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (n, 3))).astype(np.float32)
    n_bad = int(round(n * (1.0 - inlier_frac)))
    if n_bad:
        bad = rng.choice(n, n_bad, replace=False); dst[bad] = rng.uniform(-30, 30, size=(n_bad, 3))
    corres = np.c_[np.arange(n), np.arange(n)]
    a = engine.quatro_solve(src, dst, corres)
    b = oracle.quatro_solve(src, dst, corres)
    assert a["valid"] == b["valid"] and a["clique"].tolist() == b["clique"].tolist()
    assert np.abs(a["T"] - b["T"]).max() < 1e-9


# ---- solver parameters away from the reference's operating point (noise_bound 0.3, gnc factor 1.4, cost threshold 1e-4, 50 iterations): the PRODUCT's host
# solver against the oracle on fixed correspondence sets - the golden fixtures' and one with half outliers.  Same valid, clique and GNC iteration count, T <= 1e-9.
def _solver_sets():
    import os
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for name in ("quatro_a", "quatro_b"):
        d = np.load(os.path.join(G, name + ".npz"))
        out[name] = (d["src"], d["tgt"], d["corres"])
    rng = np.random.default_rng(4242)
    n = 84
    src = rng.uniform(-25, 25, size=(n, 3)).astype(np.float32); src[:, 2] = rng.uniform(0, 4, n)
    T = yaw_T(1.1, [4.0, -3.0, 0.2])
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    bad = rng.choice(n, n // 2, replace=False); dst[bad] = rng.uniform(-25, 25, size=(len(bad), 3))
    out["outliers50"] = (src, dst, np.c_[np.arange(n), np.arange(n)].astype(np.int32))
    return out


@pytest.mark.parametrize("noise_bound", [0.0, 0.05, 1.0])
@pytest.mark.parametrize("which", ["quatro_a", "quatro_b", "outliers50"])
def test_product_solver_parameter_sweep_matches_oracle(oracle, which, noise_bound):
    from qn_amd import engine
    src, dst, corres = _solver_sets()[which]
    for gnc, cost_thr, max_iter in itertools.product([1.05, 4.0], [0.0, 1e-2], [1, 2, 200]):
        ep = engine.quatro_default_params()
        ep.noise_bound, ep.rot_gnc_factor, ep.rot_cost_diff_thr, ep.rot_max_iter = noise_bound, gnc, cost_thr, max_iter
        a = engine.quatro_solve(src, dst, corres, ep)
        b = oracle.quatro_solve(src, dst, corres, oracle.QuatroParams(noise_bound=noise_bound, rot_gnc_factor=gnc, rot_cost_diff_thr=cost_thr, rot_max_iter=max_iter))
        case = (which, noise_bound, gnc, cost_thr, max_iter)
        assert a["valid"] == b["valid"] and a["clique"].tolist() == b["clique"].tolist(), case
        assert a["rot_iterations"] == b["rot_iterations"] and 0 <= a["rot_iterations"] <= max_iter, (case, a["rot_iterations"], b["rot_iterations"])
        assert np.abs(a["T"] - b["T"]).max() <= 1e-9, case
        assert np.isfinite(a["T"]).all() and np.isfinite(b["T"]).all(), case
        if a["valid"]:
            assert len(a["clique"]) >= 2 and a["rot_iterations"] >= 1, case
    if which == "outliers50" and noise_bound == 0.05:                 # the sweep is not vacuous: the set registers
        assert a["valid"] and len(a["clique"]) >= 30


def test_zero_noise_bound_is_the_limit_of_the_tls_estimate(oracle):
    """noise_bound = 0 (accepted by qn_quatro_set_params): the TLS translation's 1 / bound^2 weights are infinite, and both implementations used to return
    t = 0 whatever the data, with valid = 1 as soon as two TIMs had exactly equal lengths.  Defined now (include/qn_engine.h): per axis, the value the most
    clique members share exactly (the estimate's limit for a bound going to 0), the smallest on a tie.  Exactly representable points under an exact shift:
    every TIM matches, the yaw is exactly 0, and the shift is recovered bit for bit - by the product and the oracle alike."""
    from qn_amd import engine
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    src = (g * [1.25, 0.75, 0.5] + [3.5, -8.25, 0.125]).astype(np.float32)
    shift = np.array([7.25, -2.5, 0.375])
    dst = (src.astype(np.float64) + shift).astype(np.float32)
    n = len(src)
    rng = np.random.default_rng(9)
    out = rng.choice(n, 12, replace=False); dst[out] += rng.uniform(-5, 5, size=(12, 3)).astype(np.float32)      # outliers: their TIMs do not match exactly
    corres = np.c_[np.arange(n), np.arange(n)].astype(np.int32)
    ep = engine.quatro_default_params(); ep.noise_bound = 0.0
    a = engine.quatro_solve(src, dst, corres, ep)
    b = oracle.quatro_solve(src, dst, corres, oracle.QuatroParams(noise_bound=0.0))
    assert a["valid"] and b["valid"] and a["clique"].tolist() == b["clique"].tolist() == sorted(set(range(n)) - set(out.tolist()))
    assert a["rot_iterations"] == b["rot_iterations"]
    assert np.array_equal(a["T"], b["T"])
    expect = np.eye(4); expect[:3, 3] = shift
    assert np.array_equal(a["T"], expect), a["T"]
    from oracle import py_quatro as pq                                                   # and the numpy restatement
    c = pq.solve(src, dst, corres, pq.Params(noise_bound=0.0))
    assert c["valid"] and list(c["clique"]) == a["clique"].tolist() and np.array_equal(c["T"], expect)
    # no exactly matching TIM at all: no clique of two, not a registration (and the identity, finite)
    dst2 = dst.copy(); dst2 += rng.normal(0, 1e-3, dst2.shape).astype(np.float32)
    a = engine.quatro_solve(src, dst2, corres, ep); b = oracle.quatro_solve(src, dst2, corres, oracle.QuatroParams(noise_bound=0.0))
    assert a["valid"] == b["valid"] and a["clique"].tolist() == b["clique"].tolist() and np.array_equal(a["T"], b["T"]) and np.isfinite(a["T"]).all()
