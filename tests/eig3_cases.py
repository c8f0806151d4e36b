"""The matrix families of the two 3 x 3 symmetric eigen solvers (csrc/qn_eig3.cuh: qn_eig3_jacobi, six fixed sweeps, behind every map normal; qn::sym_eig3,
up to 32 sweeps with an early exit and a descending sort, behind the GICP covariances and the Quatro normals).  Deterministic, seeded inputs only - what a
solver must return for them is in tests/eig3_checks.py.  tests/test_eig3_cpu.py runs the host build of the solvers over them, tests/test_gpu_eig3.py the
device build (qn_debug_eig3).  Pure numpy, no GPU.

A matrix is a record a6 = (xx, xy, xz, yy, yz, zz) of f64; a family is a list of batches, each an (n, 6) array that goes through one call.  Unless said
otherwise a family is one batch of N = 256 matrices R diag(d) R', R the rotation of a random unit quaternion, symmetrised by (M + M') / 2.

  random         symmetric, N(0, 1) entries, indefinite: the general case
  graded         d = (1, 1e-8, 1e-16), and d = 10^U(-16, 0) per axis: eigenvalues far below eps ||A|| must still come out to eps ||A||, and the vectors of the
                 large ones must not be spoilt by the small
  plane          d = (1, 1, 0): the covariance of a flat neighbourhood with an isotropic spread; the repeated pair leaves only the normal defined
  line           d = (1, 0, 0): a collinear neighbourhood; the repeated zero leaves only the line's direction defined
  iso            d = (1, 1, 1): a multiple of the identity up to rounding - every off-diagonal entry is rounding noise, the rotations turn noise
  near-repeated  d = 1 + U(-1, 1)^3 10^U(-16, -1) (one exponent per matrix), and (1, 1 + 1e-15, 0.3): theta = (aqq - app) / (2 apq) is a quotient of two
                 small numbers; gaps on every scale between a cluster and a well separated spectrum
  huge, tiny     `random` times 2^500 and 2^-500: nothing in the solvers may compare an entry with an absolute number (beyond sym_eig3's 1e-300), and
                 theta * theta must be allowed to overflow.  (Below about 2^-960 the products theta * theta and t * apq underflow and accuracy is lost:
                 no family goes there.)
  ints           entries uniform in -3 .. 3, not rotated: many exact zeros (skipped rotations), zero diagonals beside non-zero off-diagonals
                 (theta = 0, a 45 degree turn), exact ties
  lattice-cov    what k_map_normals forms: the covariance, by qn_amd.mapnormals.covariance, of the integer moments of 3 .. 8 lattice points in -4 .. 4;
                 a third of the neighbourhoods coplanar (an axis plane, or the tilted plane z = x + c), so rank two and below in exact arithmetic
  diagonal       every ordering of distinct diagonals, with ties, zeros and negatives; no rotation may happen at all, the answer is exact
  seams          `random` at n = 1, 255, 256, 257: the launch seams of the device entry (256 lanes a block), one batch each
  non-finite     8 matrices with a NaN or an infinity in one entry, interleaved with 8 finite ones: a poisoned lane must not touch its neighbours"""
import functools
import itertools
import numpy as np

N = 256
BLOCK = 256                                                          # lanes a block of k_debug_eig3 (csrc/qn_selftest.cuh)
FAMILIES = ("random", "graded", "plane", "line", "iso", "near-repeated", "huge", "tiny", "ints", "lattice-cov", "diagonal", "seams", "non-finite")
FINITE = tuple(f for f in FAMILIES if f != "non-finite")


def _rng(name):
    return np.random.default_rng([3, FAMILIES.index(name)])


def rotations(rng, n):
    """n rotation matrices from random unit quaternions"""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def a6_of(M):
    """(n, 3, 3) -> (n, 6), the upper triangle by rows of (M + M') / 2"""
    S = 0.5 * (M + np.swapaxes(M, 1, 2))
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))


def full(a6):
    """(n, 6) -> (n, 3, 3)"""
    a = np.asarray(a6)
    return np.stack([a[:, [0, 1, 2]], a[:, [1, 3, 4]], a[:, [2, 4, 5]]], axis=1)


def rotated(rng, d):
    """R diag(d) R' for every row of d (n, 3)"""
    d = np.asarray(d, np.float64)
    R = rotations(rng, len(d))
    return a6_of(np.einsum("nij,nj,nkj->nik", R, d, R))


def _random(rng, n):
    return a6_of(rng.normal(size=(n, 3, 3)))


def _lattice_cov(rng, n):
    from qn_amd import mapnormals as mn
    count = np.zeros(n, np.uint32); s1 = np.zeros((n, 3), np.int64); s2 = np.zeros((n, 6), np.int64)
    for i in range(n):
        k = int(rng.integers(3, 9))
        p = rng.integers(-4, 5, size=(k, 3)).astype(np.int64)
        if i % 3 == 0:
            if i % 2 == 0:
                p[:, int(rng.integers(0, 3))] = int(rng.integers(-4, 5))               # an axis plane
            else:
                p[:, 0] = rng.integers(-2, 3, size=k); p[:, 2] = p[:, 0] + int(rng.integers(-2, 3))      # the plane z = x + c
        count[i] = k; s1[i] = p.sum(axis=0)
        s2[i] = [(p[:, a] * p[:, b]).sum() for a in range(3) for b in range(a, 3)]
    return a6_of(mn.covariance(count, s1, s2)[0])


def _diagonal():
    triples = [(3.0, 2.0, 1.0), (1.0, 1e-8, 1e-16), (-1.0, 0.0, 2.0), (5.0, -5.0, 0.5), (-3.0, -2.0, -1.0), (2.0 ** 500, 1.0, 2.0 ** -500),      # distinct
               (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-2.0, -2.0, 3.0), (0.0, 0.0, -1.0), (7.0, 7.0, -7.0),                                        # ties
               (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-4.0, -4.0, -4.0)]
    rows = []
    for t in triples:
        rows += sorted(set(itertools.permutations(t)))
    a = np.zeros((len(rows), 6)); a[:, [0, 3, 5]] = rows
    return a


def _poison():
    rng = _rng("non-finite")
    a = _random(rng, 16)
    bad = [(0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, np.nan), (3, -np.inf), (1, np.nan)]
    for i, (k, v) in enumerate(bad):
        a[2 * i, k] = v                                              # the even rows are poisoned, the odd rows finite
    return a


@functools.lru_cache(maxsize=None)
def family(name):
    """-> the tuple of (n, 6) f64 batches of a family (read only)"""
    rng = _rng(name)
    if name == "random":
        out = [_random(rng, N)]
    elif name == "graded":
        out = [np.concatenate([rotated(rng, np.tile([1.0, 1e-8, 1e-16], (N // 2, 1))), rotated(rng, 10.0 ** rng.uniform(-16.0, 0.0, (N // 2, 3)))])]
    elif name in ("plane", "line", "iso"):
        out = [rotated(rng, np.tile({"plane": [1.0, 1.0, 0.0], "line": [1.0, 0.0, 0.0], "iso": [1.0, 1.0, 1.0]}[name], (N, 1)))]
    elif name == "near-repeated":
        d = 1.0 + rng.uniform(-1.0, 1.0, (N // 2, 3)) * 10.0 ** rng.uniform(-16.0, -1.0, (N // 2, 1))
        out = [np.concatenate([rotated(rng, d), rotated(rng, np.tile([1.0, 1.0 + 1e-15, 0.3], (N // 2, 1)))])]
    elif name in ("huge", "tiny"):
        out = [np.ldexp(_random(rng, N), 500 if name == "huge" else -500)]
    elif name == "ints":
        out = [rng.integers(-3, 4, size=(N, 6)).astype(np.float64)]
    elif name == "lattice-cov":
        out = [_lattice_cov(rng, N)]
    elif name == "diagonal":
        out = [_diagonal()]
    elif name == "seams":
        out = [_random(rng, n) for n in (1, BLOCK - 1, BLOCK, BLOCK + 1)]
    elif name == "non-finite":
        out = [_poison()]
    else:
        raise KeyError(name)
    for a in out:
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 6
        a.setflags(write=False)
    return tuple(out)
