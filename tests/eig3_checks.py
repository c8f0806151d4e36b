"""What the two 3 x 3 symmetric eigen solvers (csrc/qn_eig3.cuh) must return for the families of tests/eig3_cases.py: the reference, the metrics, the bounds and
the contracts, shared by tests/test_eig3_cpu.py (the host build, tests/eig3_host.cpp) and tests/test_gpu_eig3.py (the device build, qn_debug_eig3).  No GPU.

Reference: mpmath.eigsy at 50 digits on the exact f64 entries, once per family and process (`reference`).  Every matrix is first scaled by the power of two
that brings ||A|| = max |entry| into [0.5, 1) - exact, and all bounds are relative to ||A|| - so the metrics, evaluated in np.longdouble (64-bit mantissa), round
about 2^-64 where the bounds start at 2^-52: the check's own error stays three decimal orders below what it measures.

Metrics, each in units of eps = 2^-52 (`metrics`; w, V as a solver returned them, column k of V with w[k]):
  eigenvalue       max_k |sorted(w)_k - E_k| / ||A||
  residual         max_k max_i |A v_k - w_k v_k|_i / ||A||
  orthonormality   max |V'V - I|
  vector           for every reference eigenvalue with gap_k = min_j |E_k - E_j| >= 2^-20 ||A||: sin(angle between its eigenvector and the column of the
                   computed eigenvalue of the same rank) gap_k / ||A|| (Davis-Kahan: a backward error of K eps ||A|| turns it by at most K eps ||A|| / gap_k).
                   Inside a cluster no single vector is defined; residual and orthonormality, which cover every column of every matrix, stand there.
Bound: K = 128 for qn_eig3_jacobi, 512 for sym_eig3, on every metric, whatever the conditioning.  A plane rotation applied in f64 perturbs the matrix by a
few eps ||A||, taken as 6; the solvers apply at most 18 and 96 rotations: 108 and 576, rounded to powers of two.  (Measured on the host build: at most 4 and 29.)

Contracts (`check_contracts`): sym_eig3's w is descending; a diagonal input gives - bit for bit - w = the diagonal and V = I from qn_eig3_jacobi (a rotation
with apq == 0 is skipped), the sorted diagonal and a permutation matrix from sym_eig3."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
import mpmath
import numpy as np
import eig3_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the metrics need a long double with a 64-bit mantissa"
EPS = 2.0 ** -52
GAP = 2.0 ** -20
JACOBI, SYM = 0, 1
SOLVER = {JACOBI: "qn_eig3_jacobi", SYM: "sym_eig3"}
K = {JACOBI: 128.0, SYM: 512.0}
METRICS = ("eigenvalue", "residual", "orthonormality", "vector")


def _ld(x):
    """an mpf -> long double, through its two leading f64 pieces"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _exponents(a6):
    """||A|| = max |entry| per matrix and the e with ||A|| 2^-e in [0.5, 1) (0 for the zero matrix)"""
    norm = np.abs(a6).max(axis=1)
    return norm, np.frexp(norm)[1].astype(np.int64)


def _reference(a6):
    norm, e = _exponents(a6)
    A = ec.full(np.ldexp(a6, -e[:, None]))
    n = len(A)
    E = np.zeros((n, 3), LD); Q = np.zeros((n, 3, 3), LD)
    with mpmath.workdps(50):
        for i in range(n):
            if norm[i] == 0.0:
                Q[i] = np.eye(3)
                continue
            ev, q = mpmath.eigsy(mpmath.matrix(A[i].tolist()))
            order = sorted(range(3), key=lambda k: ev[k])
            for k, j in enumerate(order):
                E[i, k] = _ld(ev[j])
                for r in range(3):
                    Q[i, r, k] = _ld(q[r, j])
    return E, Q


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> per batch of the family (E (n, 3) ascending, Q (n, 3, 3)) of the scaled matrices, long double.  Computed once, never written to."""
    out = []
    for a6 in ec.family(name):
        E, Q = _reference(a6)
        E.setflags(write=False); Q.setflags(write=False)
        out.append((E, Q))
    return tuple(out)


def eigenvalues_ld(a6):
    """-> (n, 3) ascending eigenvalues in long double: eight cyclic Jacobi sweeps vectorised over the matrices, for callers with too many matrices for mpmath
    (the map-normals test).  Error a few 2^-64 ||A||, whatever the spectrum; tests/test_eig3_cpu.py holds it to the 50-digit reference on every family."""
    A = ec.full(np.asarray(a6, np.float64)).astype(LD)
    n = len(A)
    for _ in range(8):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[:, p, q]
            nz = apq != 0
            with np.errstate(over="ignore"):                         # (theta or its square overflowing gives t = 0, the right limit)
                theta = (A[:, q, q] - A[:, p, p]) / (2 * np.where(nz, apq, LD(1)))
                t = np.where(nz, np.where(theta < 0, LD(-1), LD(1)) / (np.abs(theta) + np.sqrt(theta * theta + 1)), LD(0))
            c = 1 / np.sqrt(t * t + 1); s = t * c
            J = np.zeros((n, 3, 3), LD); J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1
            J[:, p, p] = c; J[:, q, q] = c; J[:, p, q] = s; J[:, q, p] = -s
            A = np.matmul(np.swapaxes(J, 1, 2), np.matmul(A, J))
            A[:, p, q] = A[:, q, p] = 0
    return np.sort(np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), axis=1)


def rayleigh_excess(C, trace, normals):
    """-> (n,) f64: ((n'Cn) / (n'n) - l0) / trace(C) in long double, l0 the smallest eigenvalue of C (eigenvalues_ld): how far a normal is, in energy, from
    the eigenspace it belongs to - defined and bounded for every spectrum, a repeated smallest eigenvalue included.  C (n, 3, 3) f64, trace (n,) > 0."""
    Cl = np.asarray(C, np.float64).astype(LD)
    v = np.asarray(normals).astype(np.float64).astype(LD)
    l0 = eigenvalues_ld(ec.a6_of(np.asarray(C, np.float64)))[:, 0]
    rq = (v[:, :, None] * Cl * v[:, None, :]).sum(axis=(1, 2)) / (v * v).sum(axis=1)
    return ((rq - l0) / np.asarray(trace, np.float64).astype(LD)).astype(np.float64)


def _units(err, den):
    """err / den in f64, with 0 / 0 = 0 and x / 0 = inf (the zero matrix allows no error at all)"""
    err = np.asarray(err, LD); den = np.asarray(den, LD)
    out = np.where(err == 0, LD(0), LD(np.inf))
    nz = den > 0
    out[nz] = err[nz] / den[nz]
    return out.astype(np.float64)


def metrics(a6, w, V, ref):
    """-> {metric: (n,) f64 in units of eps}, and the number of eigenvector columns compared"""
    E, Q = ref
    norm, e = _exponents(a6)
    A = ec.full(np.ldexp(a6, -e[:, None])).astype(LD)
    ws = np.ldexp(np.asarray(w, np.float64), -e[:, None]).astype(LD)
    Vl = np.asarray(V, np.float64).astype(LD)
    den = LD(EPS) * np.ldexp(norm, -e).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {}
        out["eigenvalue"] = _units(np.abs(np.sort(ws, axis=1) - E).max(axis=1), den)
        R = (A[:, :, :, None] * Vl[:, None, :, :]).sum(axis=2) - Vl * ws[:, None, :]
        out["residual"] = _units(np.abs(R).max(axis=(1, 2)), den)
        G = (Vl[:, :, :, None] * Vl[:, :, None, :]).sum(axis=1) - np.eye(3, dtype=LD)
        out["orthonormality"] = _units(np.abs(G).max(axis=(1, 2)), np.full(len(A), LD(EPS)))
        order = np.argsort(np.asarray(w, np.float64), axis=1, kind="stable")
        vec = np.zeros(len(A)); compared = 0
        for k in range(3):
            gap = np.minimum(np.abs(E[:, k] - E[:, (k + 1) % 3]), np.abs(E[:, k] - E[:, (k + 2) % 3]))
            use = gap >= LD(GAP) * np.ldexp(norm, -e).astype(LD)
            use &= norm > 0
            v = np.take_along_axis(Vl, order[:, None, k:k + 1], axis=2)[:, :, 0]
            q = Q[:, :, k]
            r = v - (v * q).sum(axis=1)[:, None] * q
            sin = np.sqrt((r * r).sum(axis=1) / (v * v).sum(axis=1))
            u = _units(sin * gap, den)
            vec = np.where(use, np.fmax(vec, np.where(np.isnan(u), np.inf, u)), vec)
            compared += int(use.sum())
        out["vector"] = vec
    return out, compared


def maxima(a6, w, V, ref):
    m, compared = metrics(a6, w, V, ref)
    # a NaN anywhere is a failure of any bound: max() would hide it behind a larger finite value
    return {k: (float("inf") if np.isnan(v).any() else float(v.max())) for k, v in m.items()}, compared


def lapack(a6):
    w, V = np.linalg.eigh(ec.full(a6))
    return w, V


def check_contracts(which, a6, w, V, diagonal):
    w = np.asarray(w); V = np.asarray(V)
    assert w.shape == (len(a6), 3) and V.shape == (len(a6), 3, 3) and w.dtype == np.float64 and V.dtype == np.float64
    if which == SYM:
        assert ((w[:, 0] >= w[:, 1]) & (w[:, 1] >= w[:, 2])).all(), "sym_eig3: w is not descending"
    if diagonal:
        d = a6[:, [0, 3, 5]]
        assert not a6[:, [1, 2, 4]].any()
        if which == JACOBI:
            assert np.array_equal(w.view(np.uint64), d.view(np.uint64)), "qn_eig3_jacobi: a diagonal input must come back as it is"
            assert np.array_equal(V.view(np.uint64), np.broadcast_to(np.eye(3), V.shape).copy().view(np.uint64)), "qn_eig3_jacobi: V of a diagonal input must be the identity"
        else:
            assert np.array_equal(w.view(np.uint64), (-np.sort(-d, axis=1)).view(np.uint64)), "sym_eig3: w of a diagonal input must be the sorted diagonal"
            one = np.float64(1.0).view(np.uint64)
            bits = np.ascontiguousarray(V).view(np.uint64)
            assert (((bits == 0) | (bits == one)).all() and ((bits == one).sum(axis=1) == 1).all() and ((bits == one).sum(axis=2) == 1).all()), "sym_eig3: V of a diagonal input must be a permutation matrix"
            assert np.array_equal(d[:, :, None] * V, V * w[:, None, :]), "sym_eig3: column k of the permutation must pick w[k] from the diagonal"


def check_family(which, name, solve, quiet=False):
    """all accuracy bounds and contracts of a finite family on solve(a6) -> (w, V); -> the family's maxima {metric: units of eps}, LAPACK's, columns compared"""
    top = dict.fromkeys(METRICS, 0.0); ltop = dict.fromkeys(METRICS, 0.0); columns = 0
    for a6, ref in zip(ec.family(name), reference(name)):
        w, V = solve(a6)
        check_contracts(which, a6, w, V, name == "diagonal")
        m, c = maxima(a6, w, V, ref)
        lm, _ = maxima(a6, *lapack(a6), ref)
        columns += c
        for k in METRICS:
            top[k] = max(top[k], m[k]); ltop[k] = max(ltop[k], lm[k])
    if not quiet:
        print("%-15s %-13s max in eps: %s | numpy.linalg.eigh: %s | %d eigenvector columns compared (bound %g)"
              % (SOLVER[which], name, " ".join("%s %.3g" % (k, top[k]) for k in METRICS), " ".join("%s %.3g" % (k, ltop[k]) for k in METRICS), columns, K[which]))
    for k in METRICS:
        assert top[k] <= K[which], (SOLVER[which], name, k, top[k], K[which])
    return top, ltop, columns


def check_non_finite(which, solve):
    """the finite rows of the poisoned batch give the bytes they give when run alone"""
    (a6,) = ec.family("non-finite")
    finite = np.isfinite(a6).all(axis=1)
    assert finite.sum() == 8 and not finite[0::2].any() and finite[1::2].all()
    w, V = solve(a6)
    wa, Va = solve(np.ascontiguousarray(a6[finite]))
    assert np.array_equal(np.ascontiguousarray(w[finite]).view(np.uint64), wa.view(np.uint64)), SOLVER[which]
    assert np.array_equal(np.ascontiguousarray(V[finite]).view(np.uint64), Va.view(np.uint64)), SOLVER[which]
    assert np.isfinite(wa).all() and np.isfinite(Va).all()


# ---- the host build of the solvers
_dir = None


@functools.lru_cache(maxsize=None)
def host_exe():
    """tests/eig3_host.cpp, built once per process the way the shim helpers are: g++, no contraction"""
    global _dir
    _dir = tempfile.mkdtemp(prefix="eig3_host_")
    atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    exe = os.path.join(_dir, "eig3_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "eig3_host.cpp"), "-o", exe])
    return exe


def host_solve(a6):
    """-> {JACOBI: (w, V), SYM: (w, V)} of the host build on the rows of a6"""
    exe = host_exe()
    a = np.ascontiguousarray(a6, np.float64).reshape(-1, 6)
    n = len(a)
    with tempfile.TemporaryDirectory(dir=_dir) as d:
        a.tofile(os.path.join(d, "in.bin"))
        subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], stdout=subprocess.DEVNULL)
        out = np.fromfile(os.path.join(d, "out.bin"), np.float64)
    assert out.size == 24 * n
    return {JACOBI: (out[:3 * n].reshape(n, 3), out[3 * n:12 * n].reshape(n, 3, 3)), SYM: (out[12 * n:15 * n].reshape(n, 3), out[15 * n:].reshape(n, 3, 3))}


@functools.lru_cache(maxsize=None)
def host_family(name):
    """the host build's results on every batch of a family, computed once"""
    return tuple(host_solve(a6) for a6 in ec.family(name))
