"""The problem families of the Gauss-Newton step's small dense f64 routines (csrc/qn_step_math.cuh: d_ldlt_solve6_fast, d_ldlt_solve6, d_so3_exp, d_iso_mul,
d_is_converged, m3_inverse; d_propose of csrc/qn_gicp_kernels.cuh).  Deterministic, seeded inputs only - what a routine must return for them is in
tests/step_math_checks.py.  tests/test_step_math_cpu.py runs the host build of the routines over them, tests/test_gpu_step_math.py the device build
(qn_debug_step_math).  Pure numpy, no GPU.

A family is a tuple of batches; a batch is an (n, stride) f64 array of records that goes through one call, in the layouts of qn_debug_step_math
(include/qn_engine.h).  Unless said otherwise a family is one batch of N = 256 problems.

6 x 6 solves (`solve_family`; records A (36, symmetric, row major), lambda, b (6): the system is (A + lambda I) x = -b; `propose_records` appends a pose x0):
  spd         Q diag(d) Q', Q orthogonal, d = 10^-U(0, c) with the extremes 1 and 10^-c pinned, c = U(0, 3) per matrix: condition 1 to 1e3
  graded      the same with c = 4, 8, 12, 15, one batch each: the unpivoted factorisation must still see six positive pivots
  gicp        H = sum J'MJ, b = sum J'Me over 50 synthetic correspondences, J = (skew(p), -I), M = (2I - 0.999 (nn' + mm'))^-1, one batch per layout:
              box (random points and normals), plane (all normals z: condition about 3e5), walls (two parallel walls: sliding along them is held by the
              in-plane 1/2 of M only), line (points on the x axis, normals z: the rotation about x is free, row and column 0 of H and b[0] are exactly 0)
  ranks       integer B (6 x r, entries -3 .. 3), A = BB', b = -Az with integer z, r = i mod 6: exactly singular, exactly consistent systems
  lm-shift    H = BB', B 6 x 3 normal: rank 3; lambda = 10^(-12, -6, 0, 6) max diag, by i mod 4: the LM shift alone makes the system definite
  diagonal    power-of-two diagonals (every pivot, quotient and product exact), the identity and the zero matrix; b = 0 wherever the diagonal is 0
  seams       `spd` at n = 1, 63, 64, 65, 129: the launch seams of the device entry (64 lanes a block)
  non-finite  16 problems with a NaN or an infinity in one entry of A or b, interleaved with 16 finite `spd` ones

`so3` (records om (3)), `inv3` (records M (9), seven batches), `conv` (records delta (16), rotation_epsilon, transformation_epsilon): see the functions."""
import functools
import numpy as np

N = 256
BLOCK = 64                                                           # lanes a block of k_debug_step_math (csrc/qn_selftest.cuh)
SOLVE_FAMILIES = ("spd", "graded", "gicp", "ranks", "lm-shift", "diagonal", "seams", "non-finite")
SOLVE_FINITE = tuple(f for f in SOLVE_FAMILIES if f != "non-finite")
GRADES = (4, 8, 12, 15)
LAYOUTS = ("box", "plane", "walls", "line")
SEAMS = (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
FAST, PIVOTED, PROPOSE, SO3, INV3, CONV = range(6)                   # `which` of qn_debug_step_math
STRIDES = ((43, 7), (43, 6), (59, 39), (3, 9), (9, 9), (18, 3))


def _rng(name):
    return np.random.default_rng([5, sum(map(ord, name)), len(name)])


def _ro(a):
    a = np.ascontiguousarray(a, np.float64)
    a.setflags(write=False)
    return a


def rotations(rng, n):
    """n rotation matrices from random unit quaternions"""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def records(A, lam, b):
    """(n, 6, 6) symmetric, (n,), (n, 6) -> (n, 43)"""
    A = np.asarray(A, np.float64); n = len(A)
    assert np.array_equal(A, np.swapaxes(A, 1, 2), equal_nan=True)
    return np.concatenate([A.reshape(n, 36), np.asarray(lam, np.float64).reshape(n, 1), np.asarray(b, np.float64).reshape(n, 6)], axis=1)


def split(rec):
    """(n, 43) -> A (n, 6, 6), lambda (n,), b (n, 6)"""
    rec = np.asarray(rec)
    return rec[:, :36].reshape(-1, 6, 6), rec[:, 36], rec[:, 37:43]


def _sym(M):
    return 0.5 * (M + np.swapaxes(M, 1, 2))


def _spd(rng, n, c):
    """Q diag(d) Q' with d = 10^-U(0, c), 1 and 10^-c among them; c a number or one per matrix"""
    Q = np.linalg.qr(rng.normal(size=(n, 6, 6)))[0]
    c = np.broadcast_to(np.asarray(c, np.float64), (n,))
    d = 10.0 ** (-rng.uniform(0.0, 1.0, (n, 6)) * c[:, None])
    d[:, 0] = 1.0; d[:, 1] = 10.0 ** -c
    d = rng.permuted(d, axis=1)
    return records(_sym(np.einsum("nij,nj,nkj->nik", Q, d, Q)), np.zeros(n), rng.normal(size=(n, 6)))


def _adjugate_inverse(S):
    """the inverse of (n, 3, 3) by cofactors: exact zeros stay exact zeros (numpy.linalg.inv pivots)"""
    c = np.empty_like(S)
    for i in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            c[:, j, i] = (-1) ** (i + j) * (S[:, a[0], b[0]] * S[:, a[1], b[1]] - S[:, a[0], b[1]] * S[:, a[1], b[0]])
    det = S[:, 0, 0] * c[:, 0, 0] + S[:, 0, 1] * c[:, 1, 0] + S[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _gicp(rng, n, layout, m=50):
    z = np.array([0.0, 0.0, 1.0]); x = np.array([1.0, 0.0, 0.0])
    if layout == "box":
        p = rng.uniform(-10.0, 10.0, (n, m, 3)); nb = _unit(rng.normal(size=(n, m, 3))); na = _unit(nb + 0.05 * rng.normal(size=(n, m, 3)))
    elif layout == "plane":
        p = rng.uniform(-27.0, 27.0, (n, m, 3)); p[:, :, 2] = 0.0; nb = np.broadcast_to(z, (n, m, 3)); na = nb
    elif layout == "walls":
        p = rng.uniform(-10.0, 10.0, (n, m, 3)); p[:, :, 0] = np.where(np.arange(m) % 2 == 0, -5.0, 5.0); nb = np.broadcast_to(x, (n, m, 3)); na = nb
    else:
        p = np.zeros((n, m, 3)); p[:, :, 0] = rng.uniform(-10.0, 10.0, (n, m)); nb = np.broadcast_to(z, (n, m, 3)); na = nb
    S = 2.0 * np.eye(3) - 0.999 * (nb[..., :, None] * nb[..., None, :] + na[..., :, None] * na[..., None, :])
    M = _adjugate_inverse(S.reshape(n * m, 3, 3)).reshape(n, m, 3, 3)
    J = np.zeros((n, m, 3, 6))
    J[..., 0, 1] = -p[..., 2]; J[..., 0, 2] = p[..., 1]; J[..., 1, 0] = p[..., 2]; J[..., 1, 2] = -p[..., 0]; J[..., 2, 0] = -p[..., 1]; J[..., 2, 1] = p[..., 0]
    J[..., 0, 3] = J[..., 1, 4] = J[..., 2, 5] = -1.0
    e = 0.1 * rng.normal(size=(n, m, 3))
    H = _sym(np.einsum("nmai,nmab,nmbj->nij", J, M, J))
    b = np.einsum("nmai,nmab,nmb->ni", J, M, e)
    return records(H, np.zeros(n), b)


def _ranks(rng, n):
    A = np.zeros((n, 6, 6)); b = np.zeros((n, 6))
    for i in range(n):
        B = rng.integers(-3, 4, size=(6, i % 6)).astype(np.float64)
        A[i] = B @ B.T
        b[i] = -(A[i] @ rng.integers(-3, 4, size=6).astype(np.float64))
    return records(A, np.zeros(n), b)


def rank_of(i):
    """the rank of problem i of `ranks`"""
    return i % 6


def _lm_shift(rng, n):
    B = rng.normal(size=(n, 6, 3))
    H = _sym(np.einsum("nik,njk->nij", B, B))
    lam = 10.0 ** np.array([-12.0, -6.0, 0.0, 6.0])[np.arange(n) % 4] * np.abs(np.diagonal(H, axis1=1, axis2=2)).max(axis=1)
    return records(H, lam, rng.normal(size=(n, 6)))


def _diagonal(rng):
    rows = [np.ones(6), np.zeros(6), 2.0 ** np.arange(6), 2.0 ** -np.arange(6), 2.0 ** np.array([40, -40, 0, 3, -7, 12]), 2.0 ** np.array([-500, 500, 0, 1, -1, 2]),
            np.array([1.0, 0.0, 4.0, 0.0, 0.25, 0.0]), np.array([0.0, 0.0, 0.0, 0.0, 0.0, 8.0]), np.full(6, 2.0 ** -30), np.full(6, 2.0 ** 30)]
    rows += [rng.permutation(2.0 ** rng.integers(-20, 21, size=6).astype(np.float64)) for _ in range(22)]
    d = np.array(rows)
    b = rng.integers(-8, 9, size=d.shape).astype(np.float64) * (d != 0)
    A = np.zeros((len(d), 6, 6)); A[:, np.arange(6), np.arange(6)] = d
    return records(A, np.zeros(len(d)), b + 0.0)


def _poison(rng):
    rec = _spd(rng, 32, 2.0).copy()
    where = [0, 7, 14, 21, 35, 6, 1, 29, 37, 40, 42, 38, 36, 36, 28, 39]       # entries of the record: A (diagonal and off-diagonal, mirrored below), lambda (36), b (37 ..)
    what = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, np.inf, np.nan, np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan, np.inf]
    for i, (k, v) in enumerate(zip(where, what)):
        rec[2 * i, k] = v                                            # the even rows are poisoned, the odd rows finite
        if k < 36:
            rec[2 * i, 6 * (k % 6) + k // 6] = v
    return rec


@functools.lru_cache(maxsize=None)
def solve_family(name):
    """-> the tuple of (n, 43) batches of a solve family (read only)"""
    rng = _rng(name)
    if name == "spd":
        out = [_spd(rng, N, rng.uniform(0.0, 3.0, N))]
    elif name == "graded":
        out = [_spd(rng, N, float(c)) for c in GRADES]
    elif name == "gicp":
        out = [_gicp(rng, N, layout) for layout in LAYOUTS]
    elif name == "ranks":
        out = [_ranks(rng, N)]
    elif name == "lm-shift":
        out = [_lm_shift(rng, N)]
    elif name == "diagonal":
        out = [_diagonal(rng)]
    elif name == "seams":
        out = [_spd(rng, n, rng.uniform(0.0, 3.0, n)) for n in SEAMS]
    elif name == "non-finite":
        out = [_poison(rng)]
    else:
        raise KeyError(name)
    return tuple(_ro(a) for a in out)


@functools.lru_cache(maxsize=None)
def poses(n, seed=17):
    """n isometries (n, 4, 4): the x0 of the proposal records"""
    rng = np.random.default_rng([5, seed, n])
    T = np.zeros((n, 4, 4)); T[:, :3, :3] = rotations(rng, n); T[:, :3, 3] = 10.0 * rng.normal(size=(n, 3)); T[:, 3, 3] = 1.0
    return _ro(T)


def propose_records(rec):
    """(n, 43) solve records -> (n, 59) records of d_propose: H (36), b (6), lambda, x0 (16)"""
    A, lam, b = split(rec)
    n = len(rec)
    return np.ascontiguousarray(np.concatenate([A.reshape(n, 36), b, lam.reshape(n, 1), poses(n).reshape(n, 16)], axis=1))


# ---- d_so3_exp
def _seam_pair(u):
    """om = s u on either side of the branch of d_so3_exp: theta_sq - evaluated as the routine evaluates it - the largest below 1e-10 and the next step of
    om's largest component, at or above it"""
    def tsq(o):
        return o[0] * o[0] + o[1] * o[1] + o[2] * o[2]
    lo = np.asarray(u, np.float64) / np.linalg.norm(u) * 1e-5 * (1.0 - 1e-13)
    k = int(np.argmax(np.abs(lo)))
    assert tsq(lo) < 1e-10
    for _ in range(20000):
        hi = lo.copy(); hi[k] = np.nextafter(hi[k], np.inf * np.sign(hi[k]))
        if tsq(hi) >= 1e-10:
            return lo, hi
        lo = hi
    raise AssertionError("no seam found")


@functools.lru_cache(maxsize=None)
def so3():
    """-> (om (n, 3), tags): one batch of rotation vectors.  tags[i] names the group of row i: zero, tiny (theta 1e-300, 1e-160: theta_sq underflows), seam-lo /
    seam-hi (theta_sq the last below and the first at or above 1e-10, rows paired), small (1e-3), one, pi, 2pi (each with -4 .. 4 ulp on the angle), large (100, 1e6,
    1e15), axis (axis-aligned at all of these angles), random (theta = 10^U(-8, 1)), non-finite (NaN, infinities, and 1e200: theta_sq overflows)"""
    rng = _rng("so3")
    rows, tags = [], []

    def add(tag, v):
        rows.append(np.asarray(v, np.float64)); tags.append(tag)
    dirs = _unit(rng.normal(size=(6, 3)))
    add("zero", [0.0, 0.0, 0.0])
    for t in (1e-300, 1e-160):
        for u in dirs[:3]:
            add("tiny", t * u)
    for u in list(dirs) + [[1.0, 0.0, 0.0], [1.0, 1e-3, 0.0]]:
        lo, hi = _seam_pair(u)
        add("seam-lo", lo); add("seam-hi", hi)
    for tag, t in (("small", 1e-3), ("one", 1.0)):
        for u in dirs:
            add(tag, t * u)
    for tag, t in (("pi", np.pi), ("2pi", 2.0 * np.pi)):
        for k in range(-4, 5):
            tk = t
            for _ in range(abs(k)):
                tk = np.nextafter(tk, np.inf if k > 0 else 0.0)
            add(tag, [tk, 0.0, 0.0]); add(tag, tk * dirs[abs(k) % 6])
    for t in (100.0, 1e6, 1e15):
        for u in dirs[:4]:
            add("large", t * u)
    for t in (1e-160, 1e-5, 1e-3, 1.0, np.pi, 2.0 * np.pi, 100.0, 1e6, 1e15):
        for a in range(3):
            for s in (1.0, -1.0):
                v = np.zeros(3); v[a] = s * t
                add("axis", v)
    for u, t in zip(_unit(rng.normal(size=(96, 3))), 10.0 ** rng.uniform(-8.0, 1.0, 96)):
        add("random", t * u)
    for v in ([np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0, 2.0, -np.inf], [1e200, 0.0, 0.0], [1e160, 1e160, 1e160], [np.nan, np.nan, np.nan]):
        add("non-finite", v); add("one", dirs[0])                    # (a finite neighbour after each)
    return _ro(np.array(rows)), tuple(tags)


# ---- m3_inverse
INV3_BATCHES = ("random", "parallel", "close", "f32-pose", "spd", "spd-two-small", "singular")


def _rcr(nb, m, G):
    """C_B + R C_A R' as emit_point (csrc/qn_tick.cuh) forms it, the same expression: the upper triangle, mirrored.  nb the target normal, m the rotated source
    normal, G = R R'"""
    n = len(nb)
    S = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            S[:, a, b] = ((1.0 if a == b else 0.0) - 0.999 * nb[:, a] * nb[:, b]) + (G[:, a, b] - 0.999 * m[:, a] * m[:, b])
            S[:, b, a] = S[:, a, b]
    return S


@functools.lru_cache(maxsize=None)
def inv3():
    """-> the tuple of (n, 9) batches, by INV3_BATCHES: the sums of two I - 0.999 nn' with random normals; with the same normal twice (condition 1e3); with normals
    1e-6 apart; with R R' of an f32-rounded rotation in place of I; SPD matrices Q diag(1, U(1/4, 1), 10^-U(0, 6)) Q' of condition up to 1e6 with ONE small
    eigenvalue - the shape of C_B + R C_A R', a sum of two matrices with two unit eigenvalues each, taken past its 0.002; SPD matrices Q diag(1, 10^-U(0, 6),
    10^-U(0, 6)) Q' with TWO small eigenvalues, which the product cannot form and where the adjugate loses more (tests/step_math_checks.py); and 8 exactly singular
    matrices (integer, rank 2 and below) between 8 finite neighbours"""
    rng = _rng("inv3")
    I = np.broadcast_to(np.eye(3), (N, 3, 3))
    nb = _unit(rng.normal(size=(N, 3)))
    out = [_rcr(nb, _unit(rng.normal(size=(N, 3))), I), _rcr(nb, nb, I), _rcr(nb, _unit(nb + 1e-6 * rng.normal(size=(N, 3))), I)]
    R = rotations(rng, N).astype(np.float32).astype(np.float64)
    na = _unit(nb + 0.05 * rng.normal(size=(N, 3)))
    out.append(_rcr(nb, np.einsum("nij,nj->ni", R, na), np.einsum("nik,njk->nij", R, R)))
    for two in (False, True):
        Q = rotations(rng, N); d = 10.0 ** -rng.uniform(0.0, 6.0, (N, 3)); d[:, 0] = 1.0
        if not two:
            d[:, 1] = rng.uniform(0.25, 1.0, N); d[:8, 2] = 1e-6
        out.append(_sym(np.einsum("nij,nj,nkj->nik", Q, d, Q)))
    S = out[0][:16].copy()
    for i in range(0, 16, 2):
        B = rng.integers(-3, 4, size=(3, (i // 2) % 3)).astype(np.float64)
        S[i] = B @ B.T
    out.append(S)
    return tuple(_ro(a.reshape(len(a), 9)) for a in out)


# ---- d_is_converged
@functools.lru_cache(maxsize=None)
def conv():
    """-> (n, 18) records delta (16), rotation_epsilon, transformation_epsilon: the truth table.  The rotation and translation deviations mr, mt of delta are set
    through single entries, so they are exact; ratios mr / epsilon exactly 1, one ulp below, well below and above on either side, crossed; epsilons of 0, NaN and
    infinity; the exact identity; and random steps with random epsilons"""
    rng = _rng("conv")
    rows = []

    def add(mr, mt, er, et, slot=0):
        d = np.eye(4)
        a, b = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))[slot % 6]      # (off the diagonal: 1 + mr would round)
        d[a, b] = mr if slot % 2 == 0 else -mr
        d[slot % 3, 3] = mt if slot % 2 == 0 else -mt
        rows.append(np.concatenate([d.ravel(), [er, et]]))
    below = lambda v: np.nextafter(v, 0.0)
    er, et = 2e-3, 5e-4                                              # the defaults of the engine
    slot = 0
    for mr, e_r in ((0.25, 0.25), (0.25, np.nextafter(0.25, 1.0)), (below(0.25), 0.25), (0.125, 0.25), (0.5, 0.25), (0.0, 0.25)):
        for mt, e_t in ((0.125, 0.125), (0.125, np.nextafter(0.125, 1.0)), (below(0.125), 0.125), (0.0625, 0.125), (0.25, 0.125), (0.0, 0.125)):
            add(mr, mt, e_r, e_t, slot); slot += 1
    for e_r in (0.0, np.nan, np.inf, -1.0, er):
        for e_t in (0.0, np.nan, np.inf, -1.0, et):
            for mr, mt in ((0.0, 0.0), (2.0 ** -12, 0.0), (0.0, 2.0 ** -12), (2.0 ** -12, 2.0 ** -12), (2.0 ** -8, 2.0 ** -13), (2.0 ** -13, 2.0 ** -8)):
                add(mr, mt, e_r, e_t, slot); slot += 1
    out = np.array(rows)
    T = np.zeros((64, 4, 4)); T[:, :3, :3] = np.eye(3) + 10.0 ** rng.uniform(-5.0, -2.0, (64, 1, 1)) * rng.normal(size=(64, 3, 3)); T[:, 3, 3] = 1.0
    T[:, :3, 3] = 10.0 ** rng.uniform(-5.0, -2.0, (64, 1)) * rng.normal(size=(64, 3))
    rnd = np.concatenate([T.reshape(64, 16), 10.0 ** rng.uniform(-4.0, -2.0, (64, 2))], axis=1)
    return _ro(np.concatenate([out, rnd]))
