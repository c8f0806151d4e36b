"""What the Gauss-Newton step's small dense f64 routines (csrc/qn_step_math.cuh, d_propose of csrc/qn_gicp_kernels.cuh) must return for the families of
tests/step_math_cases.py: the references, the metrics, the bounds and the contracts, shared by tests/test_step_math_cpu.py (the host build,
tests/step_math_host.cpp, its sanitizer build, and the oracle's so3_exp and ldlt_solve6) and tests/test_gpu_step_math.py (the device build, qn_debug_step_math).
No GPU.  A build is a function run(which, records (n, stride_in)) -> (n, stride_out), `which` and the layouts as in include/qn_engine.h.

References: mpmath at 50 digits on the exact f64 inputs, once per family and process (`solve_reference`, `so3_reference`, `inv3_reference`).  Metrics are
evaluated in np.longdouble (64-bit mantissa: their own rounding is 2^-12 of what they measure), in units of eps = 2^-52.

6 x 6 solves of (A + lambda I) x = r, r = -b; M = A + lambda I, norms are infinity norms.
  backward  eta = ||M x - r|| / (||M|| ||x|| + ||r||) <= K_SOLVE eps on every finite result of the fast solve, the pivoted solve and the proposal, the rank
            deficient families included: what survives a pivot made of rounding noise, where x reaches 1e17.  K_SOLVE = 128: LDL' with the two triangular solves
            perturbs M by at most gamma_{3n+1} |L||D||L'| componentwise (Higham, Accuracy and Stability, 10.4 with 10.3), which in norm is at most n times that
            of ||M|| for a positive definite M: (3 n + 1) n = 114 roundoffs at n = 6, rounded up to a power of two, in eps although a roundoff is eps / 2; the
            rounding of A_ii + lambda, half an eps of M, is inside that room.  Not tuned to the code: measured at most 1.3 (host build).
  forward   where cond = ||M|| ||M^-1|| <= 2^40: ||x - x*|| / ||x*|| <= K_SOLVE cond eps, x* the 50-digit solution - the usual consequence of the backward bound,
            asked of both solves: it is the fast solve's comment "same solution as the pivoted factorisation up to rounding" as a number.
  paths     the fast solve accepts (ok) every `spd`, `graded`, `seams` and `lm-shift` matrix; it refuses every `gicp` line problem, every `ranks` problem of
            rank <= 2 and the zero matrix, and d_propose then reports the pivoted path and a finite step.  Everywhere d_propose's path is the fast solve's refusal.
  exact     `diagonal`: x = -b / d where d != 0 and 0 where d = 0, no rounding anywhere.  H = 0, b = 0: d = 0, delta = I, xi = x0, bit for bit.
  composed  d_propose's d is the fast or the pivoted solve's x of the same input, whichever its path says, bit for bit; delta's rotation is d_so3_exp of d[0:3]
            and its translation d[3:6], bit for bit; its last row (0, 0, 0, 1); xi = delta x0 within 4 eps (|delta| |x0|) entry by entry of the long double product
            (a dot product of four terms errs by gamma_4 = 2 eps of the sum of the terms' sizes; twice that for the comparison's own rounding), last row exact.

d_so3_exp, theta = |om|, R* = exp(om^) at 50 digits:
  accuracy  max |R - R*| <= K_SO3 (1 + theta) eps.  The square root rounds theta relatively, so the phase of sin and cos errs by theta eps / 2 and the error grows
            with theta.  glibc's sub-ulp sin and cos give at most 4.1 eps for theta <= 2 pi and about 0.38 theta eps at theta = 100, 1e6 and 1e15 (the host build,
            printed); the device library's are a couple of ulp, taken as a factor 4: 16.4, rounded to the power of two K_SO3 = 16.
  rotation  max |R'R - I| <= K_SO3 eps at every finite theta (the quaternion is normalised to rounding whatever the phase; measured at most 7); det R > 0;
            om = 0 gives I bit for bit; the Taylor and the closed branch at theta^2 = 1e-10, on inputs one step of om's largest component apart, differ by at most 2 eps.

m3_inverse, X* the 50-digit inverse, cond = ||M|| ||X*||: max |X - X*| / max |X*| <= 8 cond eps, and max |X - X'| / max |X*| within the same, on everything
  shaped like the product's C_B + R C_A R' (at most one small eigenvalue): cofactors of two products and a difference, a three-term determinant, one division
  and one product per entry are a handful of roundoffs; 8 is that handful as a power of two (measured at most 0.9 on the host build).  The adjugate is not
  backward stable in general: a cofactor and the determinant each carry an absolute error of a few eps ||M||^2 and eps ||M||^3, so relative to the inverse the
  error is a few eps ||M||^3 / |det M| - for eigenvalues (1, a, b) that is cond / a, the same as cond while the middle eigenvalue a stays near 1, and cond^2 when
  two eigenvalues are small.  The batch `spd-two-small` is there to show exactly that and is held to 8 (||M||^3 / |det M|) eps; under 8 cond eps it measures
  3e3.  An observation, not a defect of the product: a sum of two I - 0.999 nn' has two eigenvalues above 1.  Inputs are symmetric; a singular input may
  return anything.

d_is_converged: the flag, mr and mt equal the two-line expression restated in numpy (`converged_expected`), NaN and zero epsilons included.

Every build also: a rerun returns the same bytes; non-finite and singular rows leave the rows beside them as they are without them (`check_isolation`).

Measured maxima in the units of each bound, host build / device (MI355X) / oracle; the tests print them per family:
  solves, backward (128)   spd 0.76 / 0.76 / 0.59   graded 0.58 / 0.58 / 0.35   gicp 0.41 / 0.41 / 0.31   ranks 0.29 / 0.29 / 0.26   lm-shift 1.27 / 1.27 / 1.27
                           diagonal 0 / 0 / 0   seams 0.67 / 0.67 / 0.54   (the oracle has the pivoted solve only; the host and device figures are over both)
  solves, forward (128)    spd 1.12 / 1.12 / 1.04   graded 0.13 / 0.13 / 0.11   gicp 0.018 / 0.018 / 0.018   lm-shift 2.54 / 2.54 / 2.54   seams 0.97 / 0.97 / 0.97
  xi (4)                   1.42 / 1.42 / -
  d_so3_exp (16)           accuracy 0.59 / 0.59 / 0.59 (0.39 theta eps at theta >= 100), orthonormality 4.8 / 4.8 / 4.8, seam 8e-6 / 8e-6 / 8e-6 (bound 2)
  m3_inverse (8)           0.95 / 0.95 / -, asymmetry 0 (the cofactors of a symmetric input are computed from the same products)
The fast solve refused 215 of the 256 `ranks` problems (all of rank <= 2, and most of rank 3 to 5) and returned a finite x for 112 of them, all within the backward
bound.  Device against host: the two solves, the proposal's d and path, m3_inverse and d_is_converged returned the same bits on every record; d_so3_exp differed
on 1 of 245 inputs, and delta or xi on 116 of 3202 proposals (none of the `gicp` ones, whose steps are small) - the device's sin and cos are not glibc's; on the
device itself delta's rotation is d_so3_exp(d[0:3]) bit for bit, as `composed` asks."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
import mpmath
import numpy as np
import step_math_cases as sc
from step_math_cases import FAST, PIVOTED, PROPOSE, SO3, INV3, CONV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the metrics need a long double with a 64-bit mantissa"
EPS = 2.0 ** -52
K_SOLVE = 128.0
COND_MAX = 2.0 ** 40
K_SO3 = 16.0
K_INV3 = 8.0
K_XI = 4.0
SEAM = 2.0
ROUTINE = {FAST: "d_ldlt_solve6_fast", PIVOTED: "d_ldlt_solve6", PROPOSE: "d_propose", SO3: "d_so3_exp", INV3: "m3_inverse", CONV: "d_is_converged"}


def _ld(x):
    """an mpf -> long double, through its two leading f64 pieces"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _worst(v):
    """the largest of v, a NaN anywhere counting as infinity: max() would hide it behind a finite value"""
    v = np.asarray(v, np.float64)
    return 0.0 if v.size == 0 else float("inf") if np.isnan(v).any() else float(v.max())


# ---- references
def _mp_matrix(M):
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in M])


def _mp_norm(M, n):
    return max(sum(abs(M[i, j]) for j in range(n)) for i in range(n))


def _shifted(rec):
    """M = A + lambda I in long double (the sum itself exact to 2^-64), r = -b"""
    A, lam, b = sc.split(rec)
    M = A.astype(LD)
    M[:, np.arange(6), np.arange(6)] += lam.astype(LD)[:, None]
    return M, -b.astype(LD)


def _solve_reference(rec):
    A, lam, b = sc.split(rec)
    n = len(rec)
    cond = np.full(n, np.inf); xs = np.full((n, 6), np.nan, LD)
    Mf = A + lam[:, None, None] * np.eye(6)
    with np.errstate(all="ignore"):
        for i in range(n):                                           # an f64 estimate keeps the hopeless ones from the 50-digit inverse; the 50-digit cond decides
            try:
                est = np.linalg.cond(Mf[i], np.inf) if np.isfinite(Mf[i]).all() and np.isfinite(b[i]).all() else np.inf
            except np.linalg.LinAlgError:
                est = np.inf
            if not est <= 2.0 ** 46:
                continue
            with mpmath.workdps(50):
                M = _mp_matrix(A[i]) + mpmath.mpf(float(lam[i])) * mpmath.eye(6)
                try:
                    X = mpmath.inverse(M)
                except ZeroDivisionError:
                    continue
                cond[i] = float(_mp_norm(M, 6) * _mp_norm(X, 6))
                x = X * mpmath.matrix([-mpmath.mpf(float(v)) for v in b[i]])
                for k in range(6):
                    xs[i, k] = _ld(x[k])
    cond.setflags(write=False); xs.setflags(write=False)
    return cond, xs


@functools.lru_cache(maxsize=None)
def solve_reference(name):
    """-> per batch (cond (n,) f64 - infinity where singular, non-finite or beyond 2^46 -, x* (n, 6) long double).  Computed once, never written to."""
    return tuple(_solve_reference(rec) for rec in sc.solve_family(name))


@functools.lru_cache(maxsize=None)
def so3_reference():
    """-> theta (n,) f64 (NaN where om is not finite or theta^2 overflows), R* (n, 3, 3) long double: I + sin(t)/t K + (1 - cos t)/t^2 K^2 at 50 digits"""
    om, _ = sc.so3()
    n = len(om)
    theta = np.full(n, np.nan); R = np.full((n, 3, 3), np.nan, LD)
    with np.errstate(over="ignore"):
        fine = np.isfinite(om).all(axis=1) & np.isfinite((om * om).sum(axis=1))
    with mpmath.workdps(60):
        for i in np.flatnonzero(fine):
            x, y, z = (mpmath.mpf(float(v)) for v in om[i])
            t = mpmath.sqrt(x * x + y * y + z * z)
            K = mpmath.matrix([[0, -z, y], [z, 0, -x], [-y, x, 0]])
            E = mpmath.eye(3) if t == 0 else mpmath.eye(3) + (mpmath.sin(t) / t) * K + ((1 - mpmath.cos(t)) / (t * t)) * (K * K)
            theta[i] = float(t)
            for a in range(3):
                for b in range(3):
                    R[i, a, b] = _ld(E[a, b])
    theta.setflags(write=False); R.setflags(write=False)
    return theta, R


@functools.lru_cache(maxsize=None)
def inv3_reference():
    """-> per batch (cond (n,) f64, infinity where singular; X* (n, 3, 3) long double; ||M||^3 / |det M| (n,) f64)"""
    out = []
    for rec in sc.inv3():
        n = len(rec)
        cond = np.full(n, np.inf); X = np.full((n, 3, 3), np.nan, LD); growth = np.full(n, np.inf)
        with mpmath.workdps(50):
            for i in range(n):
                M = _mp_matrix(rec[i].reshape(3, 3))
                det = mpmath.det(M)
                if det == 0:
                    continue
                Xi = mpmath.inverse(M)
                cond[i] = float(_mp_norm(M, 3) * _mp_norm(Xi, 3)); growth[i] = float(_mp_norm(M, 3) ** 3 / abs(det))
                for a in range(3):
                    for b in range(3):
                        X[i, a, b] = _ld(Xi[a, b])
        cond.setflags(write=False); X.setflags(write=False); growth.setflags(write=False)
        out.append((cond, X, growth))
    return tuple(out)


# ---- the solves
def backward_error(rec, x):
    """-> (n,) f64 in units of eps, NaN where x is not finite"""
    M, r = _shifted(rec)
    x = np.asarray(x, np.float64)
    fin = np.isfinite(x).all(axis=1)
    xl = np.where(fin[:, None], x, 0.0).astype(LD)
    with np.errstate(all="ignore"):
        res = np.abs((M * xl[:, None, :]).sum(axis=2) - r).max(axis=1)
        den = np.abs(M).sum(axis=2).max(axis=1) * np.abs(xl).max(axis=1) + np.abs(r).max(axis=1)
        eta = np.where(res == 0, LD(0), res / np.where(den > 0, den, LD(1)) / LD(EPS))
        eta = np.where((den == 0) & (res != 0), LD(np.inf), eta)
    return np.where(fin, eta.astype(np.float64), np.nan)


def forward_error(x, ref):
    """-> (n,) f64: ||x - x*|| / ||x*|| / (cond eps), NaN where cond > 2^40 or x is not finite"""
    cond, xs = ref
    x = np.asarray(x, np.float64)
    use = (cond <= COND_MAX) & np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        err = np.abs(x.astype(LD) - xs).max(axis=1); nx = np.abs(xs).max(axis=1)
        rel = np.where(err == 0, LD(0), err / np.where(nx > 0, nx, LD(1))) / (cond.astype(LD) * LD(EPS))
        rel = np.where((nx == 0) & (err != 0), LD(np.inf), rel)
    return np.where(use, rel.astype(np.float64), np.nan)


def _refused(name, batch, rec):
    """the problems the fast solve must refuse"""
    n = len(rec)
    if name == "gicp":
        return np.full(n, sc.LAYOUTS[batch] == "line")
    if name == "ranks":
        return np.array([sc.rank_of(i) <= 2 for i in range(n)])
    if name == "diagonal":
        return ~rec[:, :36].any(axis=1)
    return np.zeros(n, bool)


def _accepted(name, batch, rec):
    """the problems the fast solve must accept"""
    return np.full(len(rec), name in ("spd", "graded", "seams", "lm-shift"))


def check_solves(name, run, quiet=False, label=""):
    """every bound and contract of a finite solve family on one build; -> its maxima {(routine, metric): units of the bound's constant}"""
    top = {}
    counts = dict(refused=0, finite=0, forward=0, n=0)
    for batch, (rec, ref) in enumerate(zip(sc.solve_family(name), solve_reference(name))):
        n = len(rec)
        A, lam, b = sc.split(rec)
        fast = run(FAST, rec); piv = run(PIVOTED, rec)
        prec = sc.propose_records(rec); prop = run(PROPOSE, prec)
        assert fast.shape == (n, 7) and piv.shape == (n, 6) and prop.shape == (n, 39)
        ok = fast[:, 6]
        assert np.isin(ok, (0.0, 1.0)).all() and np.isin(prop[:, 38], (0.0, 1.0)).all()
        # paths
        must_refuse, must_accept = _refused(name, batch, rec), _accepted(name, batch, rec)
        assert (ok[must_refuse] == 0.0).all(), (name, batch, "the fast solve accepted a problem it must refuse", np.flatnonzero(must_refuse & (ok != 0))[:8])
        assert (ok[must_accept] == 1.0).all(), (name, batch, "the fast solve refused a problem it must accept", np.flatnonzero(must_accept & (ok != 1))[:8])
        assert np.array_equal(prop[:, 38], 1.0 - ok), (name, batch, "d_propose's path is not the fast solve's refusal")
        assert np.isfinite(prop[must_refuse]).all(), (name, batch, "the pivoted step of a refused problem is not finite")
        assert np.isfinite(piv).all(), (name, batch, "the pivoted solve of a finite problem is not finite")
        assert np.isfinite(fast[ok == 1.0]).all(), (name, batch, "an accepted fast solve is not finite")
        # accuracy
        for routine, x in ((FAST, fast[:, :6]), (PIVOTED, piv), (PROPOSE, prop[:, :6])):
            eta = backward_error(rec, x); fwd = forward_error(x, ref)
            for metric, v in (("backward", eta), ("forward", fwd)):
                w = _worst(v[~np.isnan(v)])
                top[routine, metric] = max(top.get((routine, metric), 0.0), w)
                assert w <= K_SOLVE, (label, ROUTINE[routine], name, batch, metric, w, K_SOLVE, int(np.nanargmax(v)))
            if routine == PIVOTED:
                counts["forward"] += int((~np.isnan(fwd)).sum())
        counts["refused"] += int((ok == 0).sum()); counts["finite"] += int(np.isfinite(fast[:, :6]).all(axis=1).sum()); counts["n"] += n
        # composition
        d = prop[:, :6]; delta = prop[:, 6:22].reshape(n, 4, 4); xi = prop[:, 22:38].reshape(n, 4, 4); x0 = prec[:, 43:59].reshape(n, 4, 4)
        assert same_bits(d, np.where((ok == 1.0)[:, None], fast[:, :6], piv)), (name, batch, "d_propose's d is not the solve's x")
        fin = np.isfinite(delta).all(axis=(1, 2))
        assert fin[must_refuse | must_accept].all()
        if fin.any():
            R = run(SO3, np.ascontiguousarray(d[fin, :3])).reshape(-1, 3, 3)
            assert same_bits(np.ascontiguousarray(delta[fin, :3, :3]), R), (name, batch, "delta's rotation is not d_so3_exp(d[0:3])")
        assert same_bits(np.ascontiguousarray(delta[:, :3, 3]), np.ascontiguousarray(d[:, 3:6])), (name, batch, "delta's translation is not d[3:6]")
        assert same_bits(np.ascontiguousarray(delta[:, 3, :]), np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))) and same_bits(np.ascontiguousarray(xi[:, 3, :]), np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
        finx = fin & np.isfinite(xi).all(axis=(1, 2))
        dl, xl = delta[finx].astype(LD), x0[finx].astype(LD)
        err = np.abs((dl[:, :, :, None] * xl[:, None, :, :]).sum(axis=2) - xi[finx].astype(LD))[:, :3, :]
        size = (np.abs(dl)[:, :, :, None] * np.abs(xl)[:, None, :, :]).sum(axis=2)[:, :3, :]
        w = _worst((err / (size * LD(EPS))).astype(np.float64))
        top[PROPOSE, "xi"] = max(top.get((PROPOSE, "xi"), 0.0), w)
        assert w <= K_XI, (label, name, batch, "xi", w)
        # exact families
        if name == "diagonal":
            dg = np.diagonal(A, axis1=1, axis2=2)
            with np.errstate(all="ignore"):
                want = np.where(dg != 0, -b / np.where(dg != 0, dg, 1.0), 0.0)
            assert np.array_equal(piv, want), "d_ldlt_solve6: a diagonal system has an exact answer"
            pos = (dg > 0).all(axis=1)
            assert pos.sum() >= 20 and np.array_equal(ok, pos.astype(np.float64)) and np.array_equal(fast[pos, :6], want[pos]), "d_ldlt_solve6_fast: a diagonal system has an exact answer"
            zero = np.flatnonzero(~rec[:, :36].any(axis=1))
            assert len(zero) == 1 and not b[zero].any()
            z = zero[0]
            assert same_bits(d[z], np.zeros(6)) and same_bits(delta[z], np.eye(4)) and same_bits(xi[z], x0[z]), "H = 0: d = 0, delta = I, xi = x0, bit for bit"
    if not quiet:
        print("%-8s %-9s max: %s | fast solve refused %d of %d, finite %d; forward error compared on %d (bounds: backward, forward %g; xi %g)"
              % (label, name, "  ".join("%s %s %.3g" % (ROUTINE[r].replace("d_ldlt_", ""), m, v) for (r, m), v in sorted(top.items())), counts["refused"], counts["n"], counts["finite"], counts["forward"], K_SOLVE, K_XI))
    return top, counts


# ---- d_so3_exp
def so3_metrics(R):
    """-> accuracy / (1 + theta), orthonormality, both in eps, and det, over the finite rows; NaN elsewhere"""
    theta, Rs = so3_reference()
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    fin = ~np.isnan(theta)
    Rl = np.where(fin[:, None, None], R, 0.0).astype(LD)
    with np.errstate(invalid="ignore"):
        acc = (np.abs(Rl - Rs).max(axis=(1, 2)) / (LD(1) + np.where(fin, theta, 0.0).astype(LD)) / LD(EPS)).astype(np.float64)
    G = (Rl[:, :, :, None] * Rl[:, :, None, :]).sum(axis=1) - np.eye(3, dtype=LD)
    orth = (np.abs(G).max(axis=(1, 2)) / LD(EPS)).astype(np.float64)
    det = np.linalg.det(np.where(fin[:, None, None], R, np.eye(3)))
    return np.where(fin, acc, np.nan), np.where(fin, orth, np.nan), np.where(fin, det, np.nan)


def check_so3(run, quiet=False, label=""):
    om, tags = sc.so3()
    tags = np.array(tags)
    R = run(SO3, om)
    assert R.shape == (len(om), 9)
    theta, _ = so3_reference()
    fin = ~np.isnan(theta)
    assert np.array_equal(fin, tags != "non-finite") and np.isfinite(R[fin]).all()
    acc, orth, det = so3_metrics(R)
    top = {}
    for tag in sorted(set(tags[fin])):
        m = tags == tag
        top[tag] = (_worst(acc[m]), _worst(orth[m]), _worst(acc[m] * (1.0 + theta[m]) / np.maximum(theta[m], 1e-300)) if tag == "large" else None)
    if not quiet:
        print("%-8s so3 max in eps, accuracy / (1 + theta) and orthonormality (bound %g both): %s | at theta >= 100 the accuracy is %.3g theta eps"
              % (label, K_SO3, "  ".join("%s %.3g %.3g" % (t, v[0], v[1]) for t, v in top.items()), top["large"][2]))
    for tag, v in top.items():
        assert v[0] <= K_SO3 and v[1] <= K_SO3, (label, "d_so3_exp", tag, v)
    assert (det[fin] > 0).all()
    zero = np.flatnonzero(tags == "zero")
    assert len(zero) == 1 and same_bits(R[zero[0]].reshape(3, 3), np.eye(3)), "d_so3_exp(0) is the identity, bit for bit"
    lo, hi = R[tags == "seam-lo"], R[tags == "seam-hi"]
    with np.errstate(over="ignore", invalid="ignore"):
        tsq = (om * om)[:, 0] + (om * om)[:, 1] + (om * om)[:, 2]
    assert len(lo) == len(hi) >= 8 and (tsq[tags == "seam-lo"] < 1e-10).all() and (tsq[tags == "seam-hi"] >= 1e-10).all()
    seam = float(np.abs(lo.astype(LD) - hi.astype(LD)).max() / LD(EPS))
    if not quiet:
        print("%-8s so3 the two branches at theta^2 = 1e-10 differ by at most %.3g eps (bound %g)" % (label, seam, SEAM))
    assert seam <= SEAM, (label, seam)
    return top, seam


# ---- m3_inverse
def check_inv3(run, quiet=False, label=""):
    top = {}
    for name, rec, (cond, Xs, growth) in zip(sc.INV3_BATCHES, sc.inv3(), inv3_reference()):
        X = run(INV3, rec).reshape(-1, 3, 3)
        fin = np.isfinite(cond)
        assert fin.all() or name == "singular"
        assert np.isfinite(X[fin]).all()
        amp = growth if name == "spd-two-small" else cond             # (the docstring: the adjugate's own amplification, cond only while one eigenvalue is small)
        Xl = X[fin].astype(LD); scale = np.abs(Xs[fin]).max(axis=(1, 2)) * amp[fin].astype(LD) * LD(EPS)
        err = (np.abs(Xl - Xs[fin]).max(axis=(1, 2)) / scale).astype(np.float64)
        asym = (np.abs(Xl - np.swapaxes(Xl, 1, 2)).max(axis=(1, 2)) / scale).astype(np.float64)
        top[name] = (_worst(err), _worst(asym), float(cond[fin].max()))
        assert top[name][0] <= K_INV3 and top[name][1] <= K_INV3, (label, "m3_inverse", name, top[name])
    if not quiet:
        print("%-8s inv3 max in cond eps (spd-two-small: in ||M||^3 / |det M| eps), error and asymmetry (bound %g), and the largest cond: %s" % (label, K_INV3, "  ".join("%s %.3g %.3g %.3g" % ((t,) + v) for t, v in top.items())))
    return top


# ---- d_is_converged
def converged_expected(rec):
    """the routine's two lines restated: -> (n, 3) flag, mr, mt"""
    d = rec[:, :16].reshape(-1, 4, 4)
    mr = np.abs(d[:, :3, :3] - np.eye(3)).max(axis=(1, 2)); mt = np.abs(d[:, :3, 3]).max(axis=1)
    with np.errstate(all="ignore"):
        qr = mr / rec[:, 16]; qt = mt / rec[:, 17]
        flag = np.where(qr < qt, qt, qr) < 1.0
    return np.stack([flag.astype(np.float64), mr, mt], axis=1)


def check_conv(run, quiet=False, label=""):
    rec = sc.conv()
    got = run(CONV, rec); want = converged_expected(rec)
    assert same_bits(got, want), (label, "d_is_converged", np.flatnonzero((bits(got) != bits(want)).any(axis=1))[:8])
    if not quiet:
        print("%-8s conv %d records, %d converged: equal to the restated expression" % (label, len(rec), int(want[:, 0].sum())))
    return int(want[:, 0].sum())


# ---- every routine
def isolation_cases():
    """-> [(which, records, keep)]: batches with non-finite or singular rows, and the rows that are neither"""
    (poison,) = sc.solve_family("non-finite")
    keep = np.isfinite(poison).all(axis=1)
    assert keep.sum() == 16 and not keep[0::2].any() and keep[1::2].all()
    om, tags = sc.so3()
    sing = sc.inv3()[sc.INV3_BATCHES.index("singular")]
    ksing = np.isfinite(inv3_reference()[sc.INV3_BATCHES.index("singular")][0])
    assert ksing.sum() == 8
    cv = sc.conv()
    (ranks,) = sc.solve_family("ranks")
    full = np.array([sc.rank_of(i) == 5 for i in range(len(ranks))])
    return [(FAST, poison, keep), (PIVOTED, poison, keep), (PROPOSE, sc.propose_records(poison), keep), (SO3, om, np.array(tags) != "non-finite"),
            (INV3, sing, ksing), (CONV, cv, np.isfinite(cv[:, 16:]).all(axis=1) & (cv[:, 16:] != 0).all(axis=1)), (FAST, ranks, full), (PIVOTED, ranks, full)]


def check_isolation(run):
    """the rows that are finite and regular come out of the mixed batch with the bytes they have in a batch of their own"""
    for which, rec, keep in isolation_cases():
        mixed = run(which, rec); alone = run(which, np.ascontiguousarray(rec[keep]))
        assert same_bits(np.ascontiguousarray(mixed[keep]), alone), ROUTINE[which]
        if which != FAST:
            assert np.isfinite(alone).all(), ROUTINE[which]


def all_batches():
    """-> [(family, which, records)]: everything a build is asked, for the rerun, the sanitizer and the device-against-host comparisons"""
    out = []
    for name in sc.SOLVE_FAMILIES:
        for rec in sc.solve_family(name):
            out += [(name, FAST, rec), (name, PIVOTED, rec), (name, PROPOSE, sc.propose_records(rec))]
    out.append(("so3", SO3, sc.so3()[0]))
    out += [("inv3", INV3, rec) for rec in sc.inv3()]
    out.append(("conv", CONV, sc.conv()))
    return out


def count_differences(run_a, run_b, quiet=False, labels=("device", "host")):
    """-> {(family, routine): (records that differ in any bit, records)} between two builds over all_batches(); a NaN equals a NaN.  For d_propose the step d
    and the path are counted apart from delta and xi, as (family, "d_propose d"): with them the solve ends and d_so3_exp's sin and cos begin"""
    out = {}

    def add(key, differ, n):
        k = out.get(key, (0, 0))
        out[key] = (k[0] + int(differ.sum()), k[1] + n)
    for name, which, rec in all_batches():
        a, b = run_a(which, rec), run_b(which, rec)
        differ = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
        add((name, ROUTINE[which]), differ.any(axis=1), len(rec))
        if which == PROPOSE:
            add((name, "d_propose d"), differ[:, [0, 1, 2, 3, 4, 5, 38]].any(axis=1), len(rec))
    if not quiet:
        for (name, routine), (k, n) in out.items():
            print("%-10s %-18s %d of %d results of the %s build differ from the %s build in some bit" % (name, routine, k, n, labels[0], labels[1]))
    return out


# ---- the host builds of the routines
_dir = None


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False):
    """tests/step_math_host.cpp, built once per process the way eig3_checks.host_exe builds its program: g++, no contraction; sanitize: the same stand-alone
    program with the address and undefined-behaviour sanitizers, every finding fatal"""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="step_math_host_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    exe = os.path.join(_dir, "step_math_host" + ("_san" if sanitize else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
                          + ["-I" + os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc"), os.path.join(ROOT, "tests", "step_math_host.cpp"), "-o", exe])
    return exe


def host_run(which, rec, sanitize=False):
    exe = host_exe(sanitize)
    si, so = sc.STRIDES[which]
    a = np.ascontiguousarray(rec, np.float64).reshape(-1, si)
    with tempfile.TemporaryDirectory(dir=_dir) as d:
        a.tofile(os.path.join(d, "in.bin"))
        subprocess.check_call([exe, str(which), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], stdout=subprocess.DEVNULL)
        out = np.fromfile(os.path.join(d, "out.bin"), np.float64)
    assert out.size == so * len(a)
    return out.reshape(len(a), so)


_host_cache = {}


def host(which, rec):
    """the host build's result, computed once per (routine, batch)"""
    key = (which, rec.shape, rec.tobytes())
    if key not in _host_cache:
        out = host_run(which, rec)
        out.setflags(write=False)
        _host_cache[key] = out
    return _host_cache[key]


def oracle(which, rec):
    """the oracle's ldlt_solve6 (as the pivoted solve: on A + lambda I formed in f64, as the routine forms it) and so3_exp behind the same interface"""
    from oracle import oracle as orc
    if which == PIVOTED:
        A, lam, b = sc.split(rec)
        M = A + lam[:, None, None] * np.eye(6)
        return np.array([orc.ldlt_solve6(M[i], -b[i]) for i in range(len(rec))]).reshape(-1, 6)
    if which == SO3:
        return np.array([orc.so3_exp(np.ascontiguousarray(o)).ravel() for o in rec]).reshape(-1, 9)
    raise KeyError(which)
