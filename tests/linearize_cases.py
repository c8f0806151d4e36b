"""Inputs for the direct tests of the GICP linearisation and its fixed-order sums (qn_debug_linearize; the record layouts are those of include/qn_engine.h):
correspondences for accumulate_point_n (csrc/qn_linearize.cuh) and emit_point (csrc/qn_tick.cuh), blocks of 256 lanes for emit_point's folds, tables of partial
rows for reduce_rows.  Pure numpy, seeded, no GPU; nothing here comes from engine output.  tests/linearize_checks.py has the references and the bounds.

A correspondence (37 f64): Rx (12), Tx (12) - 3 x 4 poses, row major -, pa, pb (3 each, exactly f32), na, nb (3 each), lin.  The families (`family(name)`,
192 records each unless said: one for every combination of rotation angle, translation, point magnitude and residual of the grids below):
  random          random unit normals
  parallel        R n_A parallel or antiparallel to n_B, exactly (to the rounding of R n_A; exactly under the identity) and off by 1e-9, 1e-5, 1e-2: cond reaches 1000
  perpendicular   n_B perpendicular to R n_A
  zero-normal     n_A, n_B or both zero: the "no neighbour: C = I" record
  f32-pose        the rotation rounded to f32 and widened (a caller's guess: R R^T is I to 6e-8 only), normals parallel as above
  trial           Rx != Tx, the LM trial geometry; 384 records: every geometry with lin = 1, then the same with lin = 0, side by side
  same-point      identity pose, mu_A = mu_B: b and the cost are exactly 0 (48)
  origin          mu_A = 0 and t = 0 under every rotation: the rotation block, the cross block and b[0:3] are exactly 0 (48)
  axis            identity pose, T mu_A on one axis: that axis' row and column of the rotation and cross blocks are exactly 0 (48)"""
import functools
import numpy as np

POINT, NPART, HEAD, LANE, BLOCK = 37, 28, 25, 13, 256
ANGLES = (0.0, 1e-3, 0.3, 3.0)                 # rad
SHIFTS = (0.0, 1.0, 100.0, 1e4)                # m
SIZES = (1e-2, 1.0, 50.0, 1e3)                 # |mu_A|
RESIDUALS = (1e-6, 1e-2, 1.0)                  # |mu_B - T mu_A| before mu_B is rounded to f32
OFFS = (0.0, 1e-9, 1e-5, 1e-2)
N = len(ANGLES) * len(SHIFTS) * len(SIZES) * len(RESIDUALS)
FAMILIES = ("random", "parallel", "perpendicular", "zero-normal", "f32-pose", "trial", "same-point", "origin", "axis")
UPPER = [(r, c) for r in range(6) for c in range(r, 6)]            # entry k of the 21 -> (row, column) of H
AXIS_ZERO = {0: (0, 1, 2, 3, 4, 5, 21), 1: (1, 6, 7, 8, 9, 10, 22), 2: (2, 7, 11, 12, 13, 14, 23)}      # T mu_A on axis k: J[:, k] = 0, so row and column k of H and b[k]
ROTATION_AND_CROSS = tuple(range(15))


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def unit(v):
    return v / np.linalg.norm(v)


def rot(w):
    """exp(w^) in f64 (Rodrigues)"""
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose(R, t):
    return np.hstack([R, np.asarray(t, np.float64).reshape(3, 1)])


def record(Rx, Tx, pa, pb, na, nb, lin):
    r = np.concatenate([np.ravel(Rx), np.ravel(Tx), pa, pb, na, nb, [1.0 if lin else 0.0]]).astype(np.float64)
    assert r.shape == (POINT,) and np.array_equal(f32(r[24:30]), r[24:30])
    return r


def split(rec):
    """(n, 37) -> Rx (n, 3, 4), Tx (n, 3, 4), pa, pb, na, nb (n, 3), lin (n,) bool"""
    rec = np.asarray(rec, np.float64).reshape(-1, POINT)
    return rec[:, :12].reshape(-1, 3, 4), rec[:, 12:24].reshape(-1, 3, 4), rec[:, 24:27], rec[:, 27:30], rec[:, 30:33], rec[:, 33:36], rec[:, 36] != 0.0


def _geometry(rng, i):
    """combination i of the grids: a pose, mu_A and the direction of the residual"""
    angle = ANGLES[i % 4]; shift = SHIFTS[(i // 4) % 4]; size = SIZES[(i // 16) % 4]; res = RESIDUALS[(i // 64) % 3]
    R = rot(unit(rng.normal(size=3)) * angle)
    t = unit(rng.normal(size=3)) * shift
    pa = f32(unit(rng.normal(size=3)) * size)
    return R, t, pa, unit(rng.normal(size=3)) * res


def _parallel(rng, R, na):
    off = OFFS[rng.integers(4)]; sign = (1.0, -1.0)[rng.integers(2)]
    return unit(R @ na + off * rng.normal(size=3)) * sign, (off, sign)


@functools.lru_cache(maxsize=None)
def _family(name):
    rng = np.random.default_rng([20260, FAMILIES.index(name)])
    out, tags = [], []
    if name in ("random", "parallel", "perpendicular", "zero-normal", "f32-pose", "trial"):
        for i in range(N):
            R, t, pa, dres = _geometry(rng, i)
            if name == "f32-pose":
                R = f32(R)
            Rx = Tx = pose(R, t)
            if name == "trial":
                Tx = pose(rot(rng.normal(size=3) * 0.01) @ R, t + rng.normal(size=3) * 0.05)
            pb = f32(Tx[:, :3] @ pa + Tx[:, 3] + dres)
            na = unit(rng.normal(size=3)); nb = unit(rng.normal(size=3)); tag = None
            if name in ("parallel", "f32-pose"):
                nb, tag = _parallel(rng, R, na)
            elif name == "perpendicular":
                nb = unit(np.cross(R @ na, rng.normal(size=3)))
            elif name == "zero-normal":
                tag = i % 3
                if tag in (0, 2):
                    na = np.zeros(3)
                if tag in (1, 2):
                    nb = np.zeros(3)
            out.append(record(Rx, Tx, pa, pb, na, nb, True)); tags.append(tag)
        if name == "trial":
            out += [np.concatenate([r[:36], [0.0]]) for r in out]; tags += tags
    elif name == "same-point":
        for i in range(48):
            pa = f32(unit(rng.normal(size=3)) * SIZES[i % 4])
            out.append(record(pose(np.eye(3), np.zeros(3)), pose(np.eye(3), np.zeros(3)), pa, pa, unit(rng.normal(size=3)), unit(rng.normal(size=3)), True)); tags.append(None)
    elif name == "origin":
        for i in range(48):
            P = pose(rot(unit(rng.normal(size=3)) * ANGLES[i % 4]), np.zeros(3))
            if i % 8 >= 4:
                P = f32(P)
            out.append(record(P, P, np.zeros(3), f32(unit(rng.normal(size=3)) * RESIDUALS[i % 3]), unit(rng.normal(size=3)), unit(rng.normal(size=3)), True)); tags.append(None)
    elif name == "axis":
        for i in range(48):
            k = i % 3
            pa = np.zeros(3); pa[k] = f32(SIZES[(i // 3) % 4] * (1.0 + rng.random()) * (-1.0) ** i)
            P = pose(np.eye(3), np.zeros(3))
            out.append(record(P, P, pa, f32(pa + unit(rng.normal(size=3)) * RESIDUALS[i % 3]), unit(rng.normal(size=3)), unit(rng.normal(size=3)), True)); tags.append(k)
    else:
        raise KeyError(name)
    a = np.array(out); a.setflags(write=False)
    return a, tuple(tags)


def family(name):
    return _family(name)[0]


def tags(name):
    return _family(name)[1]


@functools.lru_cache(maxsize=None)
def all_records():
    """every family's records, one table"""
    a = np.concatenate([family(name) for name in FAMILIES]); a.setflags(write=False)
    return a


# ---- blocks for emit_point (which 1)
def block(Rx, Tx, lin, lanes):
    """lanes (trips, 256, 13): have, pa, pb, na, nb per trip and lane -> one packed block"""
    lanes = np.asarray(lanes, np.float64)
    assert lanes.shape[1:] == (BLOCK, LANE)
    return np.concatenate([np.ravel(Rx), np.ravel(Tx), [1.0 if lin else 0.0], lanes.ravel()])


POISONS = (None, np.nan, np.inf, -np.inf, 1e300)


def single_live(rec, poison=None):
    """one block of one trip per correspondence i: alive in lane (i + 16 w) mod 64 of every wave w, the other 63 lanes of each wave without a correspondence -
    holding zeros, or `poison` in points and normals.  -> blocks (n, 25 + 256 x 13), the live lane of wave 0 (n,).  Over 64 consecutive records the live lane
    visits every position of every wave."""
    rec = np.asarray(rec, np.float64).reshape(-1, POINT)
    n = len(rec)
    lanes = np.zeros((n, 1, BLOCK, LANE))
    if poison is not None:
        lanes[:, :, :, 1:] = poison
    at = np.arange(n) % 64
    for w in range(4):
        lane = 64 * w + (at + 16 * w) % 64
        lanes[np.arange(n), 0, lane, 0] = 1.0
        lanes[np.arange(n), 0, lane, 1:] = rec[:, 24:36]
    out = np.concatenate([rec[:, :24], rec[:, 36:37], lanes.reshape(n, -1)], axis=1)
    return out, at


def _mask(k):
    lane = np.arange(BLOCK)
    return [np.ones(BLOCK, bool), np.zeros(BLOCK, bool), lane // 64 != 2, lane % 2 == 0, lane % 64 == 63][k]


MASKS = ("all", "none", "one wave empty", "every other lane", "only lane 63")


@functools.lru_cache(maxsize=None)
def fold_blocks(trips):
    """Full blocks whose sums show the order they were formed in: |mu_A| and the residual log-uniform over 1e-4 .. 1e4 with mixed signs (the rotation block and the
    cost then span 1e-8 .. 1e8, the cross block and b 1e-4 .. 1e4) and normals from random to parallel within 1e-5 (M's entries from 0.25 to 500, either sign off
    the diagonal).  Four pose pairs - identity; 0.3 rad and 1 m; an f32 rotation of 3 rad and 100 m; a trial pair Rx != Tx - each with lin = 1 and lin = 0 under
    the five `have` masks; trip t of a block uses mask (k + t) mod 5.  -> blocks (40, ...), points (40, trips, 256, 37): every lane's correspondence as a which-0
    record, have (40, trips, 256), lin (40,), and twin (40,): the block with the same inputs and the other lin."""
    rng = np.random.default_rng([20261, trips])
    R1 = rot(unit(rng.normal(size=3)) * 0.3); R2 = f32(rot(unit(rng.normal(size=3)) * 3.0)); R3 = rot(unit(rng.normal(size=3)) * 0.3)
    poses = [(pose(np.eye(3), np.zeros(3)),) * 2, (pose(R1, unit(rng.normal(size=3))),) * 2, (pose(R2, unit(rng.normal(size=3)) * 100.0),) * 2,
             (pose(R3, [1.0, -2.0, 0.5]), pose(rot(rng.normal(size=3) * 0.01) @ R3, [1.02, -2.03, 0.51]))]
    blocks, points, haves, lins, twin = [], [], [], [], []
    for Rx, Tx in poses:
        for k in range(len(MASKS)):
            lanes = np.zeros((trips, BLOCK, LANE)); pts = np.zeros((trips, BLOCK, POINT))
            for t in range(trips):
                for l in range(BLOCK):
                    pa = f32(unit(rng.normal(size=3)) * 10.0 ** rng.uniform(-4, 4))
                    pb = f32(Tx[:, :3] @ pa + Tx[:, 3] + unit(rng.normal(size=3)) * 10.0 ** rng.uniform(-4, 4))
                    na = unit(rng.normal(size=3))
                    nb = unit(rng.normal(size=3)) if l % 2 else unit(Rx[:, :3] @ na + 10.0 ** rng.uniform(-5, 0) * rng.normal(size=3)) * (-1.0) ** (l // 2)
                    lanes[t, l, 1:] = np.concatenate([pa, pb, na, nb])
                lanes[t, :, 0] = _mask((k + t) % len(MASKS))
            for lin in (True, False):
                pts[:, :, :24] = np.concatenate([Rx.ravel(), Tx.ravel()]); pts[:, :, 24:36] = lanes[:, :, 1:]; pts[:, :, 36] = float(lin)
                twin.append(len(blocks) + (1 if lin else -1))
                blocks.append(block(Rx, Tx, lin, lanes)); points.append(pts.copy()); haves.append(lanes[:, :, 0] != 0.0); lins.append(lin)
    out = (np.array(blocks), np.array(points), np.array(haves), np.array(lins), np.array(twin))
    for a in out:
        a.setflags(write=False)
    return out


def dead_blocks(trips):
    """blocks without a single correspondence, under a finite pose, a pose with a NaN in its rotation and one with a NaN in its translation, the lanes holding
    every poison in turn; lin = 1 and lin = 0 -> (12, ...)"""
    out = []
    for bad in (None, 5, 3):
        P = pose(rot(np.array([0.1, -0.2, 0.3])), [1.0, 2.0, 3.0]).ravel()
        if bad is not None:
            P[bad] = np.nan
        for lin in (True, False):
            for fill in ((0.0, np.nan), (np.inf, 1e300)):
                lanes = np.zeros((trips, BLOCK, LANE))
                lanes[:, 0::2, 1:] = fill[0]; lanes[:, 1::2, 1:] = fill[1]
                out.append(block(P, P, lin, lanes))
    return np.array(out)


# ---- tables for reduce_rows (which 2)
ROW_COUNTS = (1, 2, 17, 18, 19, 35, 36, 37, 512, 513, 576, 577, 1153)      # 18: the sub-sums; 513: 512 blocks and the far row, the most a caller passes; 576 = 18 x 32: a batch
ROW_KINDS = ((256, 0), (256, 1), (512, 0), (512, 1))                      # NT, COHERENT; arg = NT + COHERENT


@functools.lru_cache(maxsize=None)
def rows_table(n):
    """n rows of 28: magnitudes log-uniform over 1e-8 .. 1e8, mixed signs"""
    rng = np.random.default_rng([20262, n])
    a = 10.0 ** rng.uniform(-8, 8, size=(n, NPART)) * rng.choice([-1.0, 1.0], size=(n, NPART))
    a.setflags(write=False)
    return a


NAN_ROW, NAN_COMPONENTS = 300, (3, 20, 27)


def nan_table():
    """513 rows, row 300 a NaN in three of its components"""
    a = rows_table(513).copy()
    a[NAN_ROW, list(NAN_COMPONENTS)] = np.nan
    return a
