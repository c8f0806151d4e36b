"""Drift-free verification of Scan Context loop candidates (qn_gicp_align_batch_guess, qn_kf_verify_loop_candidates): the C-ABI surface, the
numpy twins of the engine's target poses and seeds (qn_amd/scancontext.py relative_pose / seed_from_yaw) against explicit restatements, the
sign of the seed against yaw_of_shift on a scan turned by whole sectors, and the C++ helper compiling against the stand-ins.  No GPU needed."""
import ctypes
import math
import os
import numpy as np
import pytest
from qn_amd import scancontext as sc
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_gicp_align_batch_guess", "qn_kf_verify_loop_candidates", "qn_kf_batch_count"]


def test_header_declares_and_library_exports_the_verify_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in SYMBOLS)


def _rigid(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    P = np.eye(4); P[:3, :3] = R; P[:3, 3] = rng.uniform(-300, 300, 3)
    return P


def _restated(Pc, Pi):
    """inv(P_c) P_i written out: [R^T | -R^T t] with the translation summed in order, then each entry of the product summed over k = 0..3 in order"""
    Pc = Pc.tolist(); Pi = Pi.tolist()
    inv = [[Pc[0][0], Pc[1][0], Pc[2][0], -(((0.0 + Pc[0][0] * Pc[0][3]) + Pc[1][0] * Pc[1][3]) + Pc[2][0] * Pc[2][3])],
           [Pc[0][1], Pc[1][1], Pc[2][1], -(((0.0 + Pc[0][1] * Pc[0][3]) + Pc[1][1] * Pc[1][3]) + Pc[2][1] * Pc[2][3])],
           [Pc[0][2], Pc[1][2], Pc[2][2], -(((0.0 + Pc[0][2] * Pc[0][3]) + Pc[1][2] * Pc[1][3]) + Pc[2][2] * Pc[2][3])],
           [0.0, 0.0, 0.0, 1.0]]
    return np.array([[(((0.0 + inv[r][0] * Pi[0][c]) + inv[r][1] * Pi[1][c]) + inv[r][2] * Pi[2][c]) + inv[r][3] * Pi[3][c] for c in range(4)] for r in range(4)])


def test_relative_pose_is_the_explicit_f64_product_bit_for_bit():
    rng = np.random.default_rng(11)
    for _ in range(200):
        Pc, Pi = _rigid(rng), _rigid(rng)
        got, want = sc.relative_pose(Pc, Pi), _restated(Pc, Pi)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert np.allclose(got, np.linalg.inv(Pc) @ Pi, atol=1e-9)


def test_relative_pose_of_a_pose_with_itself_is_the_identity():
    rng = np.random.default_rng(12)
    for _ in range(200):
        P = _rigid(rng)
        assert np.max(np.abs(sc.relative_pose(P, P) - np.eye(4))) <= 1e-15 * max(1.0, float(np.max(np.abs(P[:3, 3]))))


def test_seed_from_yaw_is_the_f32_rounding_of_rz_minus_yaw():
    for y in [0.0, 0.3, -1.2, math.pi / 2, -math.pi, 3.0, 2 * math.pi / 60 * 7]:
        g = sc.seed_from_yaw(y)
        c, s = math.cos(-y), math.sin(-y)
        want = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64).astype(np.float32)
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(g[3], np.array([0, 0, 0, 1], np.float32))


def _at(ring, sector, z, p=sc.Params()):
    r = (ring + 0.5) * p.max_radius / p.n_rings
    a = 2 * math.pi * (sector + 0.5) / p.n_sectors
    return [r * math.cos(a), r * math.sin(a), z]


@pytest.mark.parametrize("k", [1, 7, 30, 59])
def test_the_seed_from_the_shift_maps_the_query_onto_the_candidate(k):
    """the construction of test_turned_by_whole_sectors_is_exactly_zero_at_the_pinned_shift: the candidate is the query's cloud turned by +k sectors
    (what a sensor turned by -k sectors sees).  The seed from the query->candidate shift must carry the query's points onto the candidate's."""
    p = sc.Params()
    rng = np.random.default_rng(k)
    q = np.array([_at(r, s, z) for r, s, z in zip(rng.integers(0, 20, 3000), rng.integers(0, 60, 3000), rng.uniform(-1.5, 8, 3000))], np.float32)
    th = 2 * math.pi * k / p.n_sectors
    R = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
    c = (q.astype(np.float64) @ R.T).astype(np.float32)
    D, shift = sc.distance(sc.descriptor(q, p), sc.descriptor(c, p))
    assert D == 0.0 and shift == k
    G = sc.seed_from_yaw(sc.yaw_of_shift(shift, p.n_sectors)).astype(np.float64)
    mapped = q.astype(np.float64) @ G[:3, :3].T + G[:3, 3]
    assert np.max(np.abs(mapped - c)) <= 4 * 80.0 * 2.0 ** -23, np.max(np.abs(mapped - c))
    # the opposite sign would be far off
    Gw = sc.seed_from_yaw(-sc.yaw_of_shift(shift, p.n_sectors)).astype(np.float64)
    if k != 30:
        assert np.max(np.abs(q.astype(np.float64) @ Gw[:3, :3].T - c)) > 1.0


def test_verify_helper_compiles_against_the_standins(tmp_path):
    out = build_shim("shim_sc_verify.cpp", tmp_path)
    assert os.path.exists(out)
