"""The host build of the two 3 x 3 symmetric eigen solvers (csrc/qn_eig3.cuh through tests/eig3_host.cpp: the text the kernels compile) against a 50-digit
mpmath reference on the families of tests/eig3_cases.py: eigenvalues, residuals, orthonormality and - where an eigenvector is defined - its angle, each within
K eps ||A|| (K = 128 for qn_eig3_jacobi, 512 for sym_eig3; tests/eig3_checks.py has the metrics and where the bounds come from), and the contracts the call
sites rely on.  Each family's maxima are printed, numpy.linalg.eigh's under the same metrics beside them.  No GPU; the device build: tests/test_gpu_eig3.py."""
import numpy as np
import pytest
import eig3_cases as ec
import eig3_checks as chk

SOLVERS = [chk.JACOBI, chk.SYM]


def _host(which, name):
    batches = iter(chk.host_family(name))
    return lambda a6: next(batches)[which]


@pytest.mark.parametrize("name", ec.FINITE)
@pytest.mark.parametrize("which", SOLVERS, ids=[chk.SOLVER[s] for s in SOLVERS])
def test_family_within_the_bounds(which, name):
    top, _, columns = chk.check_family(which, name, _host(which, name))
    if name in ("random", "huge", "tiny", "seams"):
        assert columns >= 3 * sum(len(a) for a in ec.family(name)) - 6          # (well separated spectra: practically every eigenvector is compared)


@pytest.mark.parametrize("which", SOLVERS, ids=[chk.SOLVER[s] for s in SOLVERS])
def test_non_finite_rows_leave_their_neighbours_alone(which):
    chk.check_non_finite(which, lambda a6: chk.host_solve(a6)[which])


def test_device_entry_is_exported_wrapped_and_refuses_a_null_context():
    import ctypes as C
    from qn_amd import engine
    import test_capi_symbols
    assert "qn_debug_eig3" in test_capi_symbols.declared_symbols() and callable(engine.Context.debug_eig3)
    L = engine.lib()
    L.qn_debug_eig3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    a = np.ones(6); w = np.full(3, 7.0); V = np.full(9, 7.0)
    assert L.qn_debug_eig3(None, 0, a.ctypes.data_as(C.c_void_p), 1, w.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert (w == 7.0).all() and (V == 7.0).all()


def test_the_families_are_what_they_say():
    assert [len(a) for a in ec.family("seams")] == [1, 255, 256, 257]
    for name in ec.FINITE:
        for a6, (E, _) in zip(ec.family(name), chk.reference(name)):
            assert np.isfinite(a6).all() and (name == "seams" or len(a6) == 256 or name == "diagonal")
            if name in ("plane", "line", "iso"):                      # repeated up to the rounding of R diag(d) R'
                pair = E[:, 2] - E[:, 1] if name == "plane" else E[:, 1] - E[:, 0] if name == "line" else E[:, 2] - E[:, 0]
                assert float(pair.max()) <= 8 * chk.EPS
    d = ec.family("diagonal")[0]
    assert not d[:, [1, 2, 4]].any() and len({tuple(r) for r in d[:, [0, 3, 5]]}) == len(d) >= 40
    ints = ec.family("ints")[0]
    assert ((ints[:, [0, 3, 5]] == 0).any(axis=1) & (ints[:, [1, 2, 4]] != 0).any(axis=1)).sum() >= 50 and (ints == 0).sum() >= 150
    lat, (E, _) = ec.family("lattice-cov")[0], chk.reference("lattice-cov")[0]
    assert (np.abs(E[:, 0].astype(np.float64)) <= 64 * chk.EPS).sum() >= len(lat) // 3          # the coplanar third: a zero eigenvalue up to rounding


@pytest.mark.parametrize("name", ec.FINITE)
def test_long_double_eigenvalues_equal_the_reference(name):
    """eigenvalues_ld, the vectorised stand-in for mpmath where there are too many matrices (the map-normals test), within 2^-58 ||A|| of the 50-digit values"""
    for a6, (E, _) in zip(ec.family(name), chk.reference(name)):
        norm, e = chk._exponents(a6)
        got = chk.eigenvalues_ld(np.ldexp(a6, -e[:, None]))
        assert float(np.abs(got - E).max()) <= 2.0 ** -58, name


def test_rayleigh_excess_on_the_twin():
    """the map-normals check (tests/test_gpu_map_normals.py: excess <= 2^-44) on the twin's own LAPACK normals - a wavy sheet, a collinear run and a lattice plane
    with its ill-conditioned rim - and on wrong normals: one turned by 2^-18 rad out of a well separated eigenspace, and any unit vector where only unit length
    used to be asked (a collinear neighbourhood's normal along the line)"""
    from qn_amd import mapnormals as mn
    rng = np.random.default_rng(11)
    sheet = np.zeros((400, 3), np.float32); sheet[:, :2] = rng.uniform(-3, 3, (400, 2)); sheet[:, 2] = 0.1 * np.sin(sheet[:, 0])
    t = np.linspace(-3.0, 3.0, 61)
    line = (t[:, None] * np.array([1.0, 2.0, -0.5])[None, :] / 2.29 + np.array([4.0, 1.0, 2.0])).astype(np.float32)
    k = np.arange(-4, 5).astype(np.float32) * np.float32(0.3)
    x, y = np.meshgrid(k, k, indexing="ij")
    plane = np.stack([x.ravel(), y.ravel(), np.zeros(x.size, np.float32)], axis=1)
    for what, pts in (("sheet", sheet), ("line", line), ("plane", plane)):
        want = mn.normals(pts, (0.6, 5), [[0.0, 0.0, 9.0]])
        valid = np.isfinite(want["curvature"])
        C, tr = mn.covariance(want["count"], want["s1"], want["s2"])
        ex = chk.rayleigh_excess(C[valid], tr[valid], want["normals"][valid])
        print("%s: %d valid, largest Rayleigh excess 2^%.1f of the trace" % (what, valid.sum(), np.log2(max(ex.max(), 2.0 ** -99))))
        assert valid.sum() >= 40 and ex.max() <= 2.0 ** -44, (what, ex.max())
        if what == "sheet":
            w, U = np.linalg.eigh(C[valid])
            sep = (w[:, 1] - w[:, 0]) / w[:, 2] >= 0.1
            turned = U[:, :, 0] * np.cos(2.0 ** -18) + U[:, :, 1] * np.sin(2.0 ** -18)
            assert sep.sum() >= 100 and (chk.rayleigh_excess(C[valid], tr[valid], turned)[sep] > 2.0 ** -44).all()
        if what == "line":
            along = np.tile(np.array([1.0, 2.0, -0.5]) / 2.29, (int(valid.sum()), 1))
            assert (chk.rayleigh_excess(C[valid], tr[valid], along) > 0.9).all()


def test_the_metrics_see_a_small_turn():
    """the checks have teeth: the exact eigenvectors of a well separated matrix pass, and turned by 1e-11 rad in one plane they miss the vector and residual
    bounds by orders of magnitude while staying orthonormal"""
    a6 = ec.family("random")[0]
    ref = chk.reference("random")[0]
    w, V = chk.lapack(a6)
    good, _ = chk.maxima(a6, w, V, ref)
    assert max(good.values()) <= chk.K[chk.JACOBI], good
    c, s = np.cos(1e-11), np.sin(1e-11)
    G = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    bad, _ = chk.maxima(a6, w, V @ G, ref)
    assert bad["vector"] > 100 * chk.K[chk.SYM] and bad["residual"] > 100 * chk.K[chk.SYM] and bad["orthonormality"] <= 8, bad
    off, _ = chk.maxima(a6, w * (1.0 + 1e-12), V, ref)
    assert off["eigenvalue"] > chk.K[chk.SYM], off
