"""What the GICP linearisation and its fixed-order sums must return for the inputs of tests/linearize_cases.py: the reference, the bounds, the restated orders
and the host build, shared by tests/test_linearize_cpu.py (the host build of accumulate_point_n, tests/linearize_host.cpp, its sanitizer build and its mutants)
and tests/test_gpu_linearize.py (the device: qn_debug_linearize).  No GPU.  A build of the per-correspondence arithmetic is a function run(records (n, 37)) ->
(n, 28): the 21 upper entries of H = J'MJ row major, the 6 of b = J'Me, the cost e'Me, as added to accumulators that start at zero.

Reference (`reference`): the dense formula in mpmath at 50 digits from the exact f64 inputs - C_A = I - c n_A n_A', C_B = I - c n_B n_B' with c the double 0.999,
S = C_B + R C_A R' with the given R as it is (no assumption that R R' = I), M = S^-1, e = mu_B - (T mu_A + t), J = [skew(T mu_A + t) | -I] as a 3 x 6 matrix,
H = J'MJ, b = J'Me, cost = e'Me; once per family and process, kept as two f64 pieces, the errors evaluated in np.longdouble.

Bounds.  With kappa = cond_2(S), mu = ||M||_2 = 1 / lambda_min(S), s = 1 + |T mu_A + t|, r = |e|, g = |T| |mu_A| + |t| + |mu_B| (what the residual is formed
from; |T| the 2-norm of the rotation block) and eps = 2^-53, entry by entry:
    H     <= C eps kappa mu s^2
    b     <= C eps mu s (kappa r + g)
    cost  <= C eps mu r (kappa r + g) + C eps^2 mu g^2
Derivation, to first order.  S is formed from products and sums of O(1) terms with an absolute error of a few eps |S|; an inverse computed from it - by any
stable method, the adjugate on this shape of matrix included (tests/step_math_checks.py holds m3_inverse to 8 cond eps) - has the relative error kappa eps, i.e.
an absolute error dM of kappa eps mu in every entry.  T mu_A + t and e are sums of terms of size g: absolute error eps g each, so dJ and de are eps g.  Every
entry of J is at most s in size (the skew part |T mu_A + t|, the identity part 1).  Then  dH = J' dM J  gives kappa eps mu s^2 (the term 2 J' M dJ = mu s eps g
is below it unless g >> kappa s, which needs T mu_A and t to cancel: none of the families does that);  db = J' dM e + J' M de  gives  eps mu s (kappa r + g);
d cost = e' dM e + 2 e' M de + de' M de  gives  eps mu r (kappa r + g)  and the second-order  eps^2 mu g^2,  which is all that is left when r = 0.
The constant.  The rule was fixed before any build of the text was looked at: a dense numpy f64 evaluation of the same formula with the same adjugate inverse
(`dense`) is measured against the reference on the final table; C = 16 - eight times two, room for the different but equally stable association of the expanded
terms - while it stays within 2 of the bounds at C = 1, otherwise the next power of two at or above eight times its largest ratio.  On 1500 random records of
these families it had measured 1.8 (H), 0.92 (b), 1.24 (cost); on this table it measures 2.24 (H, a zero-normal record with cond 1 and s near 1, where
kappa mu s^2 is smallest against the roundings of T mu_A + t), 0.66 (b) and 1.21 (cost), so C = 32 (tests/test_linearize_cpu.py::
test_dense_evaluation_sets_the_constant recomputes the rule and asserts C_BOUND equals it).  Never set from the host's or the device's own results.

Exact, on every build: `same-point` b = 0 and cost = 0; `origin` the rotation block, the cross block and b[0:3] = 0; `axis` row and column k of the rotation and
cross blocks and b[k] = 0; lin = 0 leaves entries 0 .. 26 at +0.0 and gives entry 27 the bits it has with lin = 1.

Orders restated from the source (`fold_rows`, `reduce_rows_order`), every addition a numpy f64 addition in the order of the device code:
  fold7       lane (c, s), c = lane / 8 the component, s = lane % 8, adds the values of lanes s, s + 8, .., s + 56 of component c in that order to 0.0; then three
              exchange steps v += v[lane ^ 1], v += v[lane ^ 2], v += v[7 - s]; lane (c, 0) holds the wave's sum.  first: it replaces the wave's row, later
              trips add to the row (row + v).  A lane without a correspondence contributes 0.  The block's row adds the four wave rows to 0.0 in wave order.
  reduce_rows sub-sum s of component c adds rows s, s + 18, .. in order to 0.0, in batches of 32 rows that continue the same running sum (a batch's missing
              rows add +0.0); component c then adds its 18 sub-sums in order to 0.0.  The same for every block size and either kind of load.

Measured maxima in units of the bounds at C = 1, H / b / cost.  The host build of accumulate_point_n, the device build (MI355X) and the device's emit_point (one
live lane per wave) returned the same bits on every record, so they share a column; the tests print these lines:
  family          dense numpy           host = device accumulate_point_n = device emit_point
  random          1.54  0.455 0.92      1.54  0.636 0.788
  parallel        0.953 0.55  0.63      1.77  0.967 0.825
  perpendicular   1.96  0.664 0.894     2.93  0.888 0.947
  zero-normal     2.24  0.459 0.959     2.24  0.533 1.15
  f32-pose        0.856 0.466 0.992     1.02  0.653 0.992
  trial           1.17  0.445 1.21      1.4   0.564 1.26
  same-point      1.03  0     0         0.896 0     0
  origin          1.48  0.646 0.686     1.34  1.02  1.13
  axis            1.26  0.339 0.399     2.06  0.47  0.612
  over the table  2.24  0.664 1.21      2.93  1.02  1.26      (bound: 32)
The mutants of the host text: transposed-cross-block 1e15 (H), gram-is-identity 2.3e8 on f32-pose, one-normal-unregularised 4e12.
Device against host: 0 of 73168 records (the families and every correspondence of the fold blocks) differ in any bit.  emit_point against accumulate_point_n:
0 of 5376 wave rows, the live lane at all 64 positions, the other lanes holding zeros, NaN, +Inf, -Inf or 1e300.  fold7 and the block rows against the restated
order: 0 of 480 wave rows and 0 of 120 block rows at 1, 2 and 4 trips.  reduce_rows: the four instantiations equal the restated order at all 13 row counts."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
import mpmath
import numpy as np
import linearize_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the metrics need a long double with a 64-bit mantissa"
EPS = 2.0 ** -53
C_BOUND = 32.0
H_SLICE, B_SLICE, COST = slice(0, 21), slice(21, 27), 27


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the reference
def _reference(rec):
    Rx, Tx, pa, pb, na, nb, lin = lc.split(rec)
    n = len(rec)
    hi = np.zeros((n, lc.NPART)); lo = np.zeros((n, lc.NPART)); scal = np.zeros((n, 5))
    mp = mpmath.mpf
    with mpmath.workdps(50):
        c = mp(0.999)                                                # the double
        for i in range(n):
            R = mpmath.matrix([[mp(float(Rx[i, a, b])) for b in range(3)] for a in range(3)])
            T = mpmath.matrix([[mp(float(Tx[i, a, b])) for b in range(3)] for a in range(3)])
            t = mpmath.matrix([mp(float(Tx[i, a, 3])) for a in range(3)])
            vA, vB, nA, nB = (mpmath.matrix([mp(float(x)) for x in v[i]]) for v in (pa, pb, na, nb))
            CA = mpmath.eye(3) - c * nA * nA.T; CB = mpmath.eye(3) - c * nB * nB.T
            S = CB + R * CA * R.T
            M = mpmath.inverse(S)
            tA = T * vA + t
            e = vB - tA
            J = mpmath.zeros(3, 6)
            sk = [[0, -tA[2], tA[1]], [tA[2], 0, -tA[0]], [-tA[1], tA[0], 0]]
            for a in range(3):
                for b in range(3):
                    J[a, b] = sk[a][b]
                J[a, 3 + a] = -1
            MJ = M * J; Me = M * e
            H = J.T * MJ; bb = J.T * Me; cost = (e.T * Me)[0]
            full = [H[r, k] for r, k in lc.UPPER] + [bb[k] for k in range(6)] + [cost]
            if not lin[i]:
                full[:27] = [mp(0)] * 27
            for k, x in enumerate(full):
                hi[i, k] = float(x); lo[i, k] = float(x - mp(hi[i, k]))
            ev = np.linalg.eigvalsh(np.array([[float(S[a, b]) for b in range(3)] for a in range(3)]))
            g = np.linalg.norm(Tx[i, :, :3], 2) * np.linalg.norm(pa[i]) + np.linalg.norm(Tx[i, :, 3]) + np.linalg.norm(pb[i])
            scal[i] = (ev[2] / ev[0], 1.0 / ev[0], 1.0 + float(mpmath.norm(tA)), float(mpmath.norm(e)), g)
    for a in (hi, lo, scal):
        a.setflags(write=False)
    return hi, lo, scal


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> hi, lo (n, 28): the 50-digit values as two f64 pieces (lin = 0: entries 0 .. 26 are 0), and (n, 5): kappa, mu, s, r, g.  Computed once, never written to."""
    return _reference(lc.family(name))


def bounds(scal):
    """(n, 28) at C = 1"""
    kappa, mu, s, r, g = scal.T
    out = np.empty((len(scal), lc.NPART))
    out[:, H_SLICE] = (EPS * kappa * mu * s * s)[:, None]
    out[:, B_SLICE] = (EPS * mu * s * (kappa * r + g))[:, None]
    out[:, COST] = EPS * mu * r * (kappa * r + g) + EPS * EPS * mu * g * g
    return out


def ratios(name, got):
    """-> (n, 3): the largest error over the entries of H, of b, and the cost's, in units of the bounds at C = 1; a non-finite result counts as infinity"""
    hi, lo, scal = reference(name)
    got = np.asarray(got, np.float64)
    assert got.shape == hi.shape, (got.shape, hi.shape)
    with np.errstate(all="ignore"):
        err = np.abs((got.astype(LD) - hi.astype(LD)) - lo.astype(LD))
        q = np.where(err == 0, LD(0), err / bounds(scal).astype(LD)).astype(np.float64)
    q = np.where(np.isfinite(got), q, np.inf)
    return np.stack([q[:, H_SLICE].max(axis=1), q[:, B_SLICE].max(axis=1), q[:, COST]], axis=1)


def check_family(name, run, label="", quiet=False):
    """the bounds and the exact structure of one family on one build -> its maxima (H, b, cost) in units of the bounds at C = 1"""
    rec = lc.family(name)
    got = run(rec)
    q = ratios(name, got)
    top = tuple(float(v) for v in q.max(axis=0))
    if not quiet:
        print("%-22s %-13s %4d records, cond up to %7.1f: max H %.3g  b %.3g  cost %.3g of the bound at C = 1 (C = %g)" % (label, name, len(rec), reference(name)[2][:, 0].max(), top[0], top[1], top[2], C_BOUND))
    assert max(top) <= C_BOUND, (label, name, top, int(q.max(axis=1).argmax()))
    lin = lc.split(rec)[6]
    assert same_bits(np.ascontiguousarray(got[~lin, :27]), np.zeros(((~lin).sum(), 27))), (label, name, "lin = 0 must leave entries 0 .. 26 at +0.0")
    if name == "trial":
        h = len(rec) // 2
        assert lin[:h].all() and not lin[h:].any() and same_bits(np.ascontiguousarray(got[:h, 27]), np.ascontiguousarray(got[h:, 27])), (label, "the cost of a trial pass has the bits of a linearisation pass'")
    if name == "same-point":
        assert (got[:, 21:] == 0).all(), (label, name, "b and the cost are exactly 0")
    if name == "origin":
        assert (got[:, list(lc.ROTATION_AND_CROSS) + [21, 22, 23]] == 0).all() and (got[:, 15:21] != 0).any(axis=1).all(), (label, name)
    if name == "axis":
        for k, idx in lc.AXIS_ZERO.items():
            m = np.array(lc.tags(name)) == k
            rest = [j for j in range(27) if j not in idx and j not in (16, 17, 19)]      # (M's own off-diagonal entries may be anything)
            assert m.sum() == 16 and (got[m][:, list(idx)] == 0).all() and (got[m][:, rest] != 0).all(), (label, name, k)
    return top


def dense(rec, gram=True):
    """The dense formula in numpy f64 with the adjugate inverse of m3_inverse: what sets the bounds' constant.  gram = False: R R' taken to be I."""
    Rx, Tx, pa, pb, na, nb, lin = lc.split(rec)
    out = np.zeros((len(rec), lc.NPART))
    for i in range(len(rec)):
        R = Rx[i, :, :3]
        m = R @ na[i]
        G = R @ R.T if gram else np.eye(3)
        a = (np.eye(3) - 0.999 * np.outer(nb[i], nb[i])) + (G - 0.999 * np.outer(m, m))
        c = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                      [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                      [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]])
        det = a[0, 0] * c[0, 0] + a[0, 1] * c[1, 0] + a[0, 2] * c[2, 0]
        M = c * (1.0 / det)
        tA = Tx[i, :, :3] @ pa[i] + Tx[i, :, 3]
        e = pb[i] - tA
        J = np.hstack([np.array([[0, -tA[2], tA[1]], [tA[2], 0, -tA[0]], [-tA[1], tA[0], 0]]), -np.eye(3)])
        H = J.T @ M @ J; b = J.T @ M @ e
        out[i, 27] = e @ M @ e
        if lin[i]:
            out[i, :21] = [H[r, k] for r, k in lc.UPPER]; out[i, 21:27] = b
    return out


# ---- the orders, restated
XOR1, XOR2, MIRROR = [1, 0, 3, 2, 5, 4, 7, 6], [2, 3, 0, 1, 6, 7, 4, 5], [7, 6, 5, 4, 3, 2, 1, 0]


def fold_rows(contrib, have, order="device"):
    """fold7 and what its callers do with the rows.  contrib (trips, 256, 28): every lane's 28 values (accumulate_point_n's of its correspondence); have
    (trips, 256) -> the four wave rows (4, 28) and the block's row (28,).  order: "device", or a permutation of it for the tests of the inputs - "down" (u from
    7 to 0), "steps" (the exchange steps in the order mirror, ^2, ^1), "waves" (the block's row from wave 3 to wave 0), "trips" (the trips from last to first)."""
    contrib = np.asarray(contrib, np.float64); have = np.asarray(have, bool)
    trips = len(contrib)
    assert contrib.shape == (trips, lc.BLOCK, lc.NPART) and have.shape == (trips, lc.BLOCK)
    x = np.where(have[:, :, None], contrib, 0.0).reshape(trips, 4, 8, 8, lc.NPART)      # [trip, wave, u, s, component]: lane = 8 u + s
    rows = None
    for t in (range(trips) if order != "trips" else reversed(range(trips))):
        v = np.zeros((4, 8, lc.NPART))
        for u in (range(8) if order != "down" else reversed(range(8))):
            v = v + x[t, :, u]
        for perm in ((XOR1, XOR2, MIRROR) if order != "steps" else (MIRROR, XOR2, XOR1)):
            v = v + v[:, perm]
        rows = v[:, 0] if rows is None else rows + v[:, 0]
    blk = np.zeros(lc.NPART)
    for w in (range(4) if order != "waves" else reversed(range(4))):
        blk = blk + rows[w]
    return rows, blk


def reduce_rows_order(rows, segs=18, batch=32):
    """reduce_rows: (n, 28) -> (28,)"""
    rows = np.asarray(rows, np.float64).reshape(-1, lc.NPART)
    n = len(rows)
    v = np.zeros(lc.NPART)
    for s in range(segs):
        a = np.zeros(lc.NPART)
        for r0 in range(s, n, segs * batch):
            for u in range(batch):
                r = r0 + segs * u
                a = a + (rows[r] if r < n else 0.0)
        v = v + a
    return v


# ---- the host builds of accumulate_point_n
MUTANTS = {                                                            # name -> (text of csrc/qn_linearize.cuh, what replaces it, the family whose check must fail)
    "transposed-cross-block": ("acc[4] += -MS[1][0];", "acc[4] += -MS[0][1];", "random"),
    "gram-is-identity": ("const double g = Rx[a][0] * Rx[b][0] + Rx[a][1] * Rx[b][1] + Rx[a][2] * Rx[b][2];", "const double g = a == b ? 1.0 : 0.0;", "f32-pose"),
    "one-normal-unregularised": ("(g - 0.999 * m[a] * m[b])", "(g - m[a] * m[b])", "random"),
}
_dir = None


@functools.lru_cache(maxsize=None)
def host_exe(sanitize=False, mutant=None):
    """tests/linearize_host.cpp, built once per process the way step_math_checks.host_exe builds its program: g++, no contraction; sanitize: the same stand-alone
    program with the address and undefined-behaviour sanitizers, every finding fatal; mutant: against a copy of the header with one piece of text replaced"""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="linearize_host_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    inc = []
    if mutant is not None:
        old, new, _ = MUTANTS[mutant]
        txt = open(os.path.join(CSRC, "qn_linearize.cuh")).read()
        assert txt.count(old) == 1, (mutant, txt.count(old))
        d = os.path.join(_dir, mutant); os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "qn_linearize.cuh"), "w").write(txt.replace(old, new))
        inc = ["-I" + d]
    exe = os.path.join(_dir, "linearize_host" + ("_san" if sanitize else "") + ("_" + mutant if mutant else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
                          + inc + ["-I" + CSRC, os.path.join(ROOT, "tests", "linearize_host.cpp"), "-o", exe])
    return exe


def host_run(rec, sanitize=False, mutant=None):
    exe = host_exe(sanitize, mutant)
    a = np.ascontiguousarray(rec, np.float64).reshape(-1, lc.POINT)
    with tempfile.TemporaryDirectory(dir=_dir) as d:
        a.tofile(os.path.join(d, "in.bin"))
        subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], stdout=subprocess.DEVNULL)
        out = np.fromfile(os.path.join(d, "out.bin"), np.float64)
    assert out.size == lc.NPART * len(a)
    return out.reshape(len(a), lc.NPART)


_host_cache = {}


def host(rec):
    """the host build's result, computed once per table"""
    key = (rec.shape, rec.tobytes())
    if key not in _host_cache:
        out = host_run(rec)
        out.setflags(write=False)
        _host_cache[key] = out
    return _host_cache[key]
