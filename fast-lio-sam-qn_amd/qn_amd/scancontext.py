"""Scan Context (Kim & Kim, IROS 2018) place descriptors and loop candidates: the numpy twin of csrc/qn_sc.hip.

This module is the specification the kernels match bit for bit (descriptors, ring keys, column norms, every distance, shift and the
order of the result), the way synth.lidar_scan is the ray-caster's.  The definition (include/qn_engine.h, qn_sc_params):

  descriptor   Nr x Ns f32 max-height image of a keyframe's resident records in its SENSOR frame (PosePcd::pcd_), no pose applied.
               A point is dropped when x, y or z is not finite, x == y == 0, or r2 = x*x + y*y >= max_radius^2 (f64 from the f32 inputs).
               ring   = #{i in 1..Nr-1 : r2 >= edges2[i]},  edges2[i] = (i * max_radius / Nr)^2 (host f64 table)
               sector = #{j in 1..Ns-1 : azimuth(p) >= azimuth(b_j)},  b_j = (cos, sin)(2 pi j / Ns) (host f64 table), the comparison
                        decided without a transcendental: by half plane (y > 0 or y == 0 and x > 0 is the upper one), then by the
                        sign of the f64 cross product b_j.x * y - b_j.y * x >= 0 (no fused multiply-add)
               value  = max over the bin's points of (f32)((f64)z + lidar_height); a bin with no point is 0
  ring key     rk[i] = (sum over j in order of (f64)d[i, j]) / Ns                        (f64)
  column norm  cn[j] = sqrt(sum over i in order of (f64)d[i, j]^2)                         (f64, correctly rounded sqrt)
  distance     for each shift s in [0, Ns): V_s = {j : cn_q[j] != 0 and cn_c[(j + s) % Ns] != 0},
               D_s = (sum over j in V_s in order of (1 - dot_j / sqrt(ss_q[j] * ss_c[k]))) / |V_s|,  k = (j + s) % Ns,
               dot_j = sum over i in order of (f64)q[i, j] * (f64)c[i, k], ss[j] = cn[j]^2 before the sqrt (the column's sum of squares);
               D_s = 1 when V_s is empty.  The denominator is the sqrt of the product of the sums of squares, not the product of the two
               norms: a column against itself then gives dot_j / sqrt(ss * ss) = ss / ss = 1 exactly (sqrt(x * x) = x under correct
               rounding), so a scan against itself, or against itself turned by whole sectors, is at distance exactly 0.
               D = min_s D_s, shift = the lowest s reaching it.  Candidate column (j + shift) matches query column j: the candidate's
               heading minus the query's is yaw = -shift * 2 pi / Ns (yaw_of_shift).
  query        admissible candidates of query q: c != q, stamps[q] - stamps[c] > tdiff (loop_closure.cpp:45), c described; with
               ringkey_prefilter = P > 0 only the P admissible ones with the smallest sum over i in order of (rk_q[i] - rk_c[i])^2
               (ties: lower id) get the full distance.  Result: the top_k by ascending D, ties to the lower id, as (id, D, shift).

The tables are built with Python's math.cos / math.sin, which call the C library's cos / sin - the functions the engine's host code
calls for the tables it uploads - so both sides start from the same f64 values.  Every sum below is an explicit loop in a fixed order
(numpy's own reductions sum pairwise), and nothing here fuses a multiply with an add."""
import math
from dataclasses import dataclass
import numpy as np

MAX_RINGS, MAX_SECTORS = 64, 360


@dataclass
class Params:
    """qn_sc_params: the original Scan Context's PC_NUM_RING / PC_NUM_SECTOR / PC_MAX_RADIUS / LIDAR_HEIGHT, and the ring-key
    prefilter (0: every admissible keyframe gets the full distance; P > 0: the P nearest by ring key, the original's tree search made exact)."""
    n_rings: int = 20
    n_sectors: int = 60
    max_radius: float = 80.0
    lidar_height: float = 2.0
    ringkey_prefilter: int = 0


def tables(p):
    """-> (edges2 [Nr + 1], cos [Ns], sin [Ns]) f64: the ring edges squared (edges2[Nr] = max_radius^2) and the sector boundary directions."""
    nr, ns, R = int(p.n_rings), int(p.n_sectors), float(p.max_radius)
    e = np.empty(nr + 1)
    for i in range(nr):
        r = float(i) * R / nr
        e[i] = r * r
    e[nr] = R * R
    c = np.array([math.cos(2.0 * math.pi * j / ns) for j in range(ns)])
    s = np.array([math.sin(2.0 * math.pi * j / ns) for j in range(ns)])
    return e, c, s


def _upper(x, y):
    """0 for the half plane [0, pi) of azimuths (y > 0, or y == 0 and x > 0), 1 for [pi, 2 pi)"""
    return np.where((y > 0.0) | ((y == 0.0) & (x > 0.0)), 0, 1)


def bins(xyz, p):
    """-> (ring, sector, keep) of every point of an (n, >=3) f32 cloud: keep = not dropped"""
    a = np.asarray(xyz, dtype=np.float32)
    a = a.reshape(-1, a.shape[-1]) if a.ndim == 2 else a.reshape(-1, 3)
    x = a[:, 0].astype(np.float64); y = a[:, 1].astype(np.float64); z = a[:, 2].astype(np.float64)
    e, c, s = tables(p)
    nr, ns = int(p.n_rings), int(p.n_sectors)
    with np.errstate(all="ignore"):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r2 = x * x + y * y
        keep = fin & ~((x == 0.0) & (y == 0.0)) & (r2 < e[nr])
        ring = np.zeros(len(x), np.int64)
        for i in range(1, nr):
            ring += r2 >= e[i]
        hp = _upper(x, y)
        sector = np.zeros(len(x), np.int64)
        for j in range(1, ns):
            hb = 0 if (s[j] > 0.0 or (s[j] == 0.0 and c[j] > 0.0)) else 1
            cross = c[j] * y - s[j] * x
            sector += (hp > hb) | ((hp == hb) & (cross >= 0.0))
    return ring, sector, keep


def _ordered(v):
    """f32 -> uint32 whose unsigned order is the float order (the kernel's atomicMax key); 0 is below every float"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _unordered(k):
    k = np.asarray(k, dtype=np.uint32)
    b = np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k)
    return np.where(k == 0, np.uint32(0), b).astype(np.uint32).view(np.float32)


def descriptor(xyz, p=None):
    """-> (desc (Nr, Ns) f32, ring key (Nr,) f64, column norms (Ns,) f64) of one keyframe cloud (sensor frame)"""
    p = Params() if p is None else p
    nr, ns = int(p.n_rings), int(p.n_sectors)
    a = np.asarray(xyz, dtype=np.float32)
    a = a.reshape(-1, a.shape[-1]) if a.ndim == 2 else a.reshape(-1, 3)
    ring, sector, keep = bins(a, p)
    key = np.zeros(nr * ns, np.uint32)
    if keep.any():
        v = (a[keep, 2].astype(np.float64) + float(p.lidar_height)).astype(np.float32)
        np.maximum.at(key, ring[keep] * ns + sector[keep], _ordered(v))
    d = _unordered(key).reshape(nr, ns)
    return (d,) + keys(d)


def keys(d):
    """-> (ring key, column norms) of a descriptor, summed in the definition's order"""
    d64 = np.asarray(d, dtype=np.float32).astype(np.float64)
    acc = np.zeros(d64.shape[0])
    for j in range(d64.shape[1]):
        acc = acc + d64[:, j]
    return acc / float(d64.shape[1]), np.sqrt(column_squares(d))


def column_squares(d):
    """-> ss (Ns,) f64: each column's sum over rings in order of (f64)d[i, j]^2 (the column norm squared, before its rounding)"""
    d64 = np.asarray(d, dtype=np.float32).astype(np.float64)
    acc = np.zeros(d64.shape[1])
    for i in range(d64.shape[0]):
        acc = acc + d64[i, :] * d64[i, :]
    return acc


def distances(q, cands):
    """q = (desc, rk, cn) of the query; cands = list of (desc, rk, cn).  -> (D (M,) f64, shift (M,) int64), the definition's D and shift"""
    if len(cands) > 256:                                                    # in pieces: the work arrays are 8 Ns^2 bytes per candidate
        parts = [distances(q, cands[a:a + 256]) for a in range(0, len(cands), 256)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    dq = q[0]
    M = len(cands)
    if M == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    nr, ns = dq.shape
    Q = dq.astype(np.float64)
    nq = column_squares(dq)
    C = np.stack([c[0] for c in cands]).astype(np.float64)                 # (M, Nr, Ns)
    NC = np.stack([column_squares(c[0]) for c in cands])                    # (M, Ns)
    jj = np.arange(ns)
    K = (jj[None, :] + jj[:, None]) % ns                                    # K[s, j] = (j + s) % Ns
    dot = np.zeros((M, ns, ns))                                             # [m, s, j]
    for i in range(nr):
        dot = dot + Q[i][None, None, :] * C[:, i, :][:, K]
    nck = NC[:, K]                                                          # [m, s, j]
    valid = (nq[None, None, :] != 0.0) & (nck != 0.0)
    with np.errstate(all="ignore"):
        term = 1.0 - dot / np.sqrt(nq[None, None, :] * nck)
    acc = np.zeros((M, ns)); cnt = np.zeros((M, ns))
    for j in range(ns):
        v = valid[:, :, j]
        acc = np.where(v, acc + term[:, :, j], acc)
        cnt = cnt + v
    with np.errstate(all="ignore"):
        Ds = np.where(cnt > 0, acc / np.maximum(cnt, 1.0), 1.0)
    shift = np.argmin(Ds, axis=1)                                           # the first minimum: the lowest shift on ties
    return Ds[np.arange(M), shift], shift


def distance(q, c):
    """-> (D, shift) of one pair"""
    D, s = distances(q, [c])
    return float(D[0]), int(s[0])


def yaw_of_shift(shift, n_sectors):
    """the candidate's heading minus the query's [rad] for a shift, wrapped to [-pi, pi)"""
    y = -2.0 * math.pi * int(shift) / int(n_sectors)
    return (y + math.pi) % (2.0 * math.pi) - math.pi


def ringkey_distance(rq, rc):
    acc = 0.0
    for a, b in zip(np.asarray(rq, np.float64), np.asarray(rc, np.float64)):
        d = float(a) - float(b)
        acc = acc + d * d
    return acc


def query(descs, q, stamps, tdiff, top_k, prefilter=0):
    """descs: dict id -> (desc, rk, cn) of the described keyframes; q: the query id (described).
    -> list of (id, D, shift), at most top_k, by ascending D then id"""
    cand = [c for c in sorted(descs) if c != q and stamps[q] - stamps[c] > tdiff]
    if prefilter > 0:
        rq = descs[q][1]
        cand = sorted(cand, key=lambda c: (ringkey_distance(rq, descs[c][1]), c))[:prefilter]
        cand.sort()
    D, sh = distances(descs[q], [descs[c] for c in cand])
    order = sorted(range(len(cand)), key=lambda m: (D[m], cand[m]))[:top_k]
    return [(cand[m], float(D[m]), int(sh[m])) for m in order]


# ---- drift-free verification of a candidate (qn_kf_verify_loop_candidates, csrc/qn_verify.hip): the engine's target poses and seeds, bit for bit
def relative_pose(P_c, P_i):
    """inv(P_c) P_i in f64: inv(P) = [R^T | -R^T t] (each -R^T t entry summed over k = 0..2 in order), every entry of the product summed over
    k = 0..3 in order, no fused multiply-add.  Keyframe i of candidate c's window enters the target with this pose (the candidate's sensor frame)."""
    Pc = [[float(v) for v in row] for row in np.asarray(P_c, np.float64).reshape(4, 4)]
    Pi = [[float(v) for v in row] for row in np.asarray(P_i, np.float64).reshape(4, 4)]
    A = [[0.0] * 4 for _ in range(4)]
    for r in range(3):
        acc = 0.0
        for k in range(3):
            A[r][k] = Pc[k][r]
            acc = acc + Pc[k][r] * Pc[k][3]
        A[r][3] = -acc
    A[3] = [0.0, 0.0, 0.0, 1.0]
    Q = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + A[r][k] * Pi[k][c]
            Q[r, c] = acc
    return Q


def seed_from_yaw(yaw):
    """the initial guess of a candidate whose heading minus the query's is yaw: Rz(-yaw) as f32 (4x4), from the C library's cos / sin in f64.
    R(inv(P_c) P_q) = Rz(h_q - h_c) = Rz(-yaw)."""
    c, s = math.cos(-float(yaw)), math.sin(-float(yaw))
    return np.array([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]).astype(np.float32)
