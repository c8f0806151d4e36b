"""The objects of a cloud - PCL's EuclideanClusterExtraction over the points that are not ground: the numpy twin of csrc/qn_mapclusters.inc (qn_kf_map_clusters /
qn_kf_map_cluster_points / qn_kf_map_cluster_list / qn_kf_map_drop_rejected_clusters) and its specification.  Pure numpy, no GPU.

For the n records of a cloud (x y z, anything behind carried along) and ClusterParams(tolerance, min_size, max_size, class_mask) - tolerance f64 finite > 0,
min_size an integer >= 1, max_size an integer >= min_size (both u32), class_mask with bits 0 .. 4 only:
  members      class_mask == 0: every finite record (x, y and z all finite).  class_mask != 0: a finite record whose ground class c (mapground's, one byte per
               record, given as `classes`) has its bit 1 << c set in the mask; (1 << OBSTACLE) | (1 << OVERHEAD) is the intended use.
  edges        two members at DIFFERENT indices are joined when sqdist3(p, q) <= float32(tolerance * tolerance), inclusive - overlap.sqdist3_block's f32
               arithmetic (f32 differences, dx dx + dy dy + dz dz left to right, no fused multiply-add), symmetric in p and q.  A duplicate at another index is
               joined at distance 0.  edges = the number of unordered joined pairs.
  components   the connected components of that graph.  root[p] = the smallest index in p's component (u32), size[p] = its member count; a record that is not
               a member has root 0xffffffff and size 0.
  clusters     a component with min_size <= size <= max_size, numbered 0 .. C - 1 in ascending order of root.  label[p] (int32) = the number; REJECTED = -1 for
               the members of the other components, NONE = -2 for the records that are not members.
  per cluster  root, size, lo[3] and hi[3] - the f32 minimum and maximum of the members' coordinates in the total order of the sign-magnitude-to-ordered-
               integer image of the f32 (so -0 < +0) - and sum_q[3], the int64 sums of xq = int64(rint(x * 2^e)), half to even, the f32 widened to f64 first
               (the product is exact), e = quant_exponent(tolerance): the largest integer with tolerance * 2^e <= 2^10 (kept within [-126, 127]).  A member
               with |xq| >= 2^31 on any axis: CapacityError; below that the sums of fewer than 2^32 members are exact.  centroid = sum_q / size * 2^-e (f64).
  statistics   n, n_finite, members; components, clusters, too_small, too_large (components); clustered_points, rejected_points; largest (the largest
               component's size); quant_exp; edges.
Everything is an integer or an f32 selected by an order-free rule, so no order of meeting neighbours or of joining components changes a byte.

The components are computed as the GPU cannot be asked to: candidate pairs from a binning into cells of a little more than the tolerance, the f32 test, then
min-label hooking (every root under the smallest root it has an edge to) with pointer jumping until nothing changes."""
import math
from collections import namedtuple
import numpy as np
from . import overlap

ClusterParams = namedtuple("ClusterParams", "tolerance min_size max_size class_mask", defaults=(0.5, 10, 0xffffffff, 0))      # interface choices, not measurements
ClusterStats = namedtuple("ClusterStats", "n n_finite members components clusters too_small too_large clustered_points rejected_points largest quant_exp edges")
INFO_DTYPE = np.dtype([("root", "<u4"), ("size", "<u4"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("sum_q", "<i8", (3,))])        # qn_cluster_info, 56 bytes
REJECTED = -1
NONE = -2
NO_ROOT = 0xffffffff
LIMIT = 1 << 31
PAIR_BUDGET = 1 << 22                                # candidate pairs expanded at a time


class CapacityError(ValueError):
    """what the C library answers with QN_ERR_CAPACITY"""


def check_params(p):
    overlap.radius2(p.tolerance)
    for name in ("min_size", "max_size", "class_mask"):
        v = getattr(p, name)
        if int(v) != v or not (0 <= int(v) <= 0xffffffff):
            raise ValueError("mapclusters: %s must be an unsigned 32-bit integer" % name)
    if int(p.min_size) < 1:
        raise ValueError("mapclusters: min_size must be >= 1")
    if int(p.max_size) < int(p.min_size):
        raise ValueError("mapclusters: max_size must be >= min_size")
    if int(p.class_mask) & ~31:
        raise ValueError("mapclusters: class_mask may have the bits 0 .. 4 only")


def quant_exponent(tolerance):
    """the largest e with tolerance * 2^e <= 2^10 (f64; exact through frexp), clamped to the exponents of normal f32 powers of two"""
    overlap.radius2(tolerance)
    m, x = math.frexp(float(tolerance))              # tolerance = m 2^x, 0.5 <= m < 1
    e = 11 - x if m == 0.5 else 10 - x
    return max(-126, min(127, e))


def ordered(x):
    """the ordered-integer image of f32 values (u32): ascending with the value, -0 below +0"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unordered(u):
    """the f32 whose ordered image is u"""
    u = np.ascontiguousarray(u, np.uint32)
    return np.where(u >> 31 != 0, u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def members_of(a, class_mask, classes):
    fin = np.isfinite(a).all(axis=1)
    if int(class_mask) == 0:
        return fin, fin
    if classes is None:
        raise ValueError("mapclusters: class_mask != 0 needs the ground classes")
    c = np.asarray(classes)
    if c.shape != (len(a),):
        raise ValueError("mapclusters: one class per record")
    return fin, fin & (((int(class_mask) >> c.astype(np.int64)) & 1) == 1)


def joined_pairs(b, tolerance):
    """-> (u, v) int64 arrays, u < v: every unordered pair of the finite points b (m, 3) f32 with sqdist3 <= float32(tolerance^2), each once.  Cells of
    1.001 tolerance (the f32 distance of a joined pair is within 2^-21 of the tolerance along an axis): a partner lies in the 27 cells around a point's; each
    point meets the points behind it in its own cell and all points of the 13 cells that follow it in key order."""
    m = len(b)
    r2 = overlap.radius2(tolerance)
    z = np.zeros(0, np.int64)
    if m < 2:
        return z, z
    edge = float(tolerance) * 1.001
    c = np.floor(b.astype(np.float64) / edge)
    cmin = c.min(axis=0)
    span = [int(v) + 3 for v in (c.max(axis=0) - cmin)]                        # one empty cell on either side: no offset wraps
    if span[0] * span[1] * span[2] >= 1 << 62:
        raise CapacityError("mapclusters: the extent of the cloud needs more than 2^62 cells of the tolerance")
    ci = (c - cmin).astype(np.int64) + 1
    key = (ci[:, 2] * span[1] + ci[:, 1]) * span[0] + ci[:, 0]
    order = np.argsort(key, kind="stable")
    ks = key[order]; bs = b[order]
    us = []; vs = []
    pos = np.arange(m, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for dz in (0, 1):
            for dy in (-1, 0, 1):
                if dz == 0 and dy < 0:
                    continue
                # one run of consecutive keys per (dy, dz): x - 1 .. x + 1, or for the point's own row the cell itself (behind the point) and x + 1
                own = dz == 0 and dy == 0
                k0 = ks + (dz * span[1] + dy) * span[0] + (0 if own else -1)
                lo = np.searchsorted(ks, k0, "left"); hi = np.searchsorted(ks, k0 + (1 if own else 2), "right")
                if own:
                    lo = np.maximum(lo, pos + 1)
                cnt = np.maximum(hi - lo, 0)
                cum = np.cumsum(cnt)
                s = 0
                while s < m:
                    base = cum[s - 1] if s else 0
                    e = max(s + 1, int(np.searchsorted(cum, base + PAIR_BUDGET, "right")))
                    k = cnt[s:e]
                    tot = int(k.sum())
                    if tot:
                        qi = np.repeat(pos[s:e], k)
                        start = np.cumsum(k) - k
                        cj = np.arange(tot, dtype=np.int64) - np.repeat(start, k) + np.repeat(lo[s:e], k)
                        d = bs[qi] - bs[cj]
                        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                        ok = d2 <= r2
                        us.append(order[qi[ok]]); vs.append(order[cj[ok]])
                    s = e
    if not us:
        return z, z
    u = np.concatenate(us); v = np.concatenate(vs)
    return np.minimum(u, v), np.maximum(u, v)


def components(m, u, v):
    """-> root (m,) int64: the smallest index of each vertex's component of the graph with the edges (u, v)"""
    parent = np.arange(m, dtype=np.int64)
    while len(u):
        ru = parent[u]; rv = parent[v]
        live = ru != rv
        if not live.any():
            break
        u = u[live]; v = v[live]; ru = ru[live]; rv = rv[live]
        np.minimum.at(parent, np.maximum(ru, rv), np.minimum(ru, rv))          # every root under the smallest root it has an edge to
        while True:                                                              # pointer jumping to a flat forest
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def classify(points_xyzi, params=None, classes=None):
    """-> dict(label (n,) i32, root (n,) u32, size (n,) u32, clusters: a structured array of INFO_DTYPE, centroid (C, 3) f64, stats: a ClusterStats)"""
    p = ClusterParams() if params is None else ClusterParams(*params)
    check_params(p)
    a = overlap._xyz(points_xyzi)
    n = len(a)
    fin, mem = members_of(a, p.class_mask, classes)
    idx = np.flatnonzero(mem)
    b = a[idx]
    m = len(idx)
    e = quant_exponent(p.tolerance)
    xq = np.rint(b.astype(np.float64) * np.float64(math.ldexp(1.0, e)))
    if m and not (np.abs(xq) < LIMIT).all():
        raise CapacityError("mapclusters: a member's coordinate is 2^31 units of 2^-e m or more")
    xq = xq.astype(np.int64)
    u, v = joined_pairs(b, p.tolerance)
    croot = components(m, u, v)                                                  # ascending members: the smallest member index is the smallest map index
    csize = np.bincount(croot, minlength=m)
    root = np.full(n, NO_ROOT, np.uint32); size = np.zeros(n, np.uint32); label = np.full(n, NONE, np.int32)
    root[idx] = idx[croot].astype(np.uint32); size[idx] = csize[croot].astype(np.uint32)
    roots = np.flatnonzero(croot == np.arange(m))                                # ascending
    rs = csize[roots]
    kept = (rs >= int(p.min_size)) & (rs <= int(p.max_size))
    number = np.full(m, REJECTED, np.int64)
    number[roots[kept]] = np.arange(int(kept.sum()))
    cl = number[croot]
    label[idx] = cl.astype(np.int32)
    C = int(kept.sum())
    info = np.zeros(C, INFO_DTYPE)
    info["root"] = idx[roots[kept]]; info["size"] = rs[kept]
    inc = cl >= 0
    lo = np.full((C, 3), 0xffffffff, np.uint32); hi = np.zeros((C, 3), np.uint32); sq = np.zeros((C, 3), np.int64)
    o = ordered(b[inc])
    for ax in range(3):
        np.minimum.at(lo[:, ax], cl[inc], o[:, ax]); np.maximum.at(hi[:, ax], cl[inc], o[:, ax])
        np.add.at(sq[:, ax], cl[inc], xq[inc, ax])
    info["lo"] = unordered(lo); info["hi"] = unordered(hi); info["sum_q"] = sq
    centroid = sq.astype(np.float64) / info["size"].astype(np.float64)[:, None] * math.ldexp(1.0, -e)
    stats = ClusterStats(n, int(fin.sum()), m, len(roots), C, int((rs < int(p.min_size)).sum()), int((rs > int(p.max_size)).sum()), int(inc.sum()),
                         int(m - inc.sum()), int(rs.max()) if len(rs) else 0, e, len(u))
    return dict(label=label, root=root, size=size, clusters=info, centroid=centroid, stats=stats)


def drop_rejected(points, params=None, classes=None):
    """-> the kept records of `points`, in order and with every column: all but the members of rejected components (what qn_kf_map_drop_rejected_clusters
    leaves in the map slot; records that are not members - non-finite ones, excluded ground - stay)"""
    c = np.asarray(points)
    return np.ascontiguousarray(c[classify(c, params, classes)["label"] != REJECTED])
