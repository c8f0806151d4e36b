"""Exploration frontiers of the occupancy map - the FREE voxels that border UNKNOWN space, grouped into connected regions: the numpy twin of
csrc/qn_mapfrontier.inc (qn_kf_map_frontiers / _frontier_grid / _frontier_regions / _frontier_list / _frontier_costs) and its specification.  Pure numpy, no GPU.

  input        the class bytes of a 3-D occupancy map, (D, H, W) uint8 with x the fastest axis (mapoccupancy.classify, or KeyframeStore.map_occupancy_grid).
  params       FrontierParams(free_mask, unknown_mask, edge_unknown, min_size, iz_lo, iz_hi): both masks have at least one of the class bits 0 .. 2, no other,
               and share none (1 << FREE, 1 << UNKNOWN); edge_unknown 0 or 1 (1); min_size >= 1 (8); iz_lo .. iz_hi (0, INT32_MAX) the band of layers,
               inclusive, clipped to the grid, iz_lo > iz_hi is refused.  The defaults are interface choices, not measurements.
  candidate    a voxel whose class bit is in free_mask and whose layer lies in the band.
  frontier     a candidate with at least one of its 6 face neighbours unknown: a neighbour inside the grid is unknown iff its class bit is in unknown_mask
               (the band does not apply to neighbours), a neighbour outside the grid iff edge_unknown - the grid is the bounding box of the rays, nothing was
               seen beyond it.  faces[v] = the number of unknown face neighbours, 1 .. 6.
  components   the connected components of the frontier voxels under 26-connectivity; root = the smallest linear index (iz H + iy) W + ix, size = the count.
  regions      the components with size >= min_size, numbered 0 .. R - 1 in ascending root.
  labels       one int32 per voxel: the region number, REJECTED = -1 for the frontier voxels of smaller components, NONE = -2 for everything else.
  info         per region (INFO_DTYPE, 64 bytes): root, size, lo[3], hi[3] (the box of the grid indices ix, iy, iz), faces (the sum of faces[v]: the opening's
               area in voxel faces), reserved (0), sum[3] (u64: the sums of ix, iy, iz; centroid() = sum / size, mapoccupancy.centres turns it to metres).
  stats        FrontierStats(candidates, frontier, components, regions, too_small, region_voxels, rejected_voxels, largest, unknown_faces): too_small counts
               components, largest is the size of the largest component (kept or not), unknown_faces the sum of faces[v] over all frontier voxels.
  costs        with a route field (maproute.field's cost, (D, H, W) or planar (1, H, W): a voxel reads its column's cell): per region the smallest cost below
               BLOCKED over its voxels and the voxel attaining it, the smallest linear index on a tie; UNREACHED and voxel (0, 0, 0) when none is reached.
  frontier()   min-label propagation over the 26 shifts, vectorised on the list of frontier voxels; brute() is the definition literally - a flood fill per
               component (scipy.ndimage.label with the 3 x 3 x 3 structure, or a plain stack without scipy) - the second, independent statement.
Components are a set property and root, number, box and sums are order-free integers, so any exact algorithm gives the same bytes."""
from collections import namedtuple
import numpy as np
from . import mapoccupancy as mo, maproute as mr

INT32_MAX = 0x7fffffff
FrontierParams = namedtuple("FrontierParams", "free_mask unknown_mask edge_unknown min_size iz_lo iz_hi",
                            defaults=(1 << mo.FREE, 1 << mo.UNKNOWN, 1, 8, 0, INT32_MAX))      # interface choices
FrontierStats = namedtuple("FrontierStats", "candidates frontier components regions too_small region_voxels rejected_voxels largest unknown_faces")
INFO_DTYPE = np.dtype([("root", "<u4"), ("size", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("faces", "<u4"), ("reserved", "<u4"),
                       ("sum", "<u8", (3,))])                          # qn_frontier_info, 64 bytes
REJECTED = -1
NONE = -2
BLOCKED, UNREACHED = mr.BLOCKED, mr.UNREACHED
# the 6 face neighbours and the 26 neighbours of the components, (dx, dy, dz)
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
SHIFTS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def check_params(p):
    """raises ValueError on a value outside its range"""
    fm, um, edge, ms, lo, hi = p
    for name, m in (("free_mask", fm), ("unknown_mask", um)):
        if int(m) != m or int(m) == 0 or int(m) & ~7:
            raise ValueError("mapfrontier: %s must have at least one of the bits 0 .. 2 set and no other" % name)
    if int(fm) & int(um):
        raise ValueError("mapfrontier: free_mask and unknown_mask must share no class")
    if int(edge) != edge or int(edge) not in (0, 1):
        raise ValueError("mapfrontier: edge_unknown must be 0 or 1")
    if int(ms) != ms or not (1 <= int(ms) <= 0xffffffff):
        raise ValueError("mapfrontier: min_size must be an integer in 1 .. 2^32 - 1")
    for v in (lo, hi):
        if int(v) != v or not (-INT32_MAX - 1 <= int(v) <= INT32_MAX):
            raise ValueError("mapfrontier: iz_lo and iz_hi must be 32-bit integers")
    if int(lo) > int(hi):
        raise ValueError("mapfrontier: iz_lo > iz_hi")


def _params(params):
    p = FrontierParams() if params is None else FrontierParams(*params)
    check_params(p)
    return FrontierParams(*(int(v) for v in p))


def _classes(classes):
    cls = np.asarray(classes, np.uint8)
    if cls.ndim != 3:
        raise ValueError("mapfrontier: classes must be (D, H, W)")
    return cls


def mark(classes, params=None):
    """-> (candidate (D, H, W) bool, faces (D, H, W) uint8: the unknown face neighbours of a candidate, 0 elsewhere); a frontier voxel has faces > 0"""
    p = _params(params)
    cls = _classes(classes)
    D, H, W = cls.shape
    lo, hi = max(p.iz_lo, 0), min(p.iz_hi, D - 1)
    z = np.arange(D)
    cand = (((p.free_mask >> cls.astype(np.int64)) & 1) == 1) & ((z >= lo) & (z <= hi))[:, None, None]
    pad = np.full((D + 2, H + 2, W + 2), bool(p.edge_unknown))
    pad[1:-1, 1:-1, 1:-1] = ((p.unknown_mask >> cls.astype(np.int64)) & 1) == 1
    faces = np.zeros(cls.shape, np.uint8)
    for dx, dy, dz in FACES:
        faces += pad[1 + dz:D + 1 + dz, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
    faces[~cand] = 0
    return cand, faces


def _assemble(shape, p, lin, root_of, faces_of, candidates):
    """labels, info and stats from the frontier voxels lin (ascending linear indices), the root (a linear index) of each and its faces"""
    D, H, W = shape
    labels = np.full(D * H * W, NONE, np.int32)
    roots, inv, sizes = np.unique(root_of, return_inverse=True, return_counts=True)      # ascending root
    kept = sizes >= p.min_size
    number = np.where(kept, np.cumsum(kept) - 1, REJECTED).astype(np.int32)
    lab = number[inv] if len(lin) else np.zeros(0, np.int32)
    labels[lin] = lab
    R = int(kept.sum())
    info = np.zeros(R, INFO_DTYPE)
    info["root"] = roots[kept]; info["size"] = sizes[kept]
    inc = lab >= 0
    k = lab[inc]; v = lin[inc]
    ijk = np.stack([v % W, (v // W) % H, v // (W * H)], axis=1) if len(v) else np.zeros((0, 3), np.int64)
    lo = np.full((R, 3), INT32_MAX, np.int64); hi = np.full((R, 3), -INT32_MAX - 1, np.int64); sm = np.zeros((R, 3), np.uint64)
    fc = np.zeros(R, np.int64)
    for a in range(3):
        np.minimum.at(lo[:, a], k, ijk[:, a]); np.maximum.at(hi[:, a], k, ijk[:, a])
        if len(k):                                                    # (sums below 2^53: exact in the f64 weights of bincount)
            sm[:, a] = np.bincount(k, ijk[:, a].astype(np.float64), minlength=R).astype(np.uint64)
    if len(k):
        fc = np.bincount(k, faces_of[inc].astype(np.float64), minlength=R).astype(np.int64)
    info["lo"] = lo; info["hi"] = hi; info["sum"] = sm; info["faces"] = fc
    rv = int(sizes[kept].sum())
    stats = FrontierStats(int(candidates), len(lin), len(roots), R, len(roots) - R, rv, len(lin) - rv, int(sizes.max()) if len(sizes) else 0,
                          int(faces_of.sum(dtype=np.int64)))
    return dict(labels=labels.reshape(D, H, W), info=info, stats=stats)


def frontier(classes, params=None):
    """-> dict(labels (D, H, W) int32, info: a structured array of INFO_DTYPE, stats: a FrontierStats), by min-label propagation over the 26 shifts"""
    p = _params(params)
    cls = _classes(classes)
    D, H, W = cls.shape
    cand, faces = mark(cls, p)
    front = faces > 0
    lin = np.flatnonzero(front.ravel())
    n = len(lin)
    # the place of every frontier voxel in the list, in a volume padded by one voxel (-1: no frontier voxel); the list is in ascending linear index, so the
    # smallest place in a component is its root's
    where = np.full((D + 2, H + 2, W + 2), -1, np.int64)
    where[1:-1, 1:-1, 1:-1][front] = np.arange(n)
    z, y, x = lin // (W * H) + 1, (lin // W) % H + 1, lin % W + 1
    me = np.arange(n)
    nb = []
    for dx, dy, dz in SHIFTS:
        t = where[z + dz, y + dy, x + dx]
        if (t >= 0).any():
            nb.append(np.where(t >= 0, t, me))
    lab = me.copy()
    while n:
        new = lab
        for t in nb:
            new = np.minimum(new, lab[t])
        new = new[new]                                                # (a label names a voxel of the same component: its label is no larger)
        if np.array_equal(new, lab):
            break
        lab = new
    return _assemble(cls.shape, p, lin, lin[lab] if n else lin, faces.ravel()[lin].astype(np.int64), cand.sum())


def brute(classes, params=None):
    """the definition literally -> dict(labels, info, stats) as frontier(): the unknown neighbours counted one direction at a time, a flood fill per component
    (scipy.ndimage.label with the 3 x 3 x 3 structure where scipy imports, a plain stack without it), every region's numbers from its own voxels"""
    p = _params(params)
    cls = _classes(classes)
    D, H, W = cls.shape
    unknown = np.isin(cls, [c for c in range(3) if (p.unknown_mask >> c) & 1])
    free = np.isin(cls, [c for c in range(3) if (p.free_mask >> c) & 1])
    for iz in range(D):
        if iz < p.iz_lo or iz > p.iz_hi:
            free[iz] = False
    faces = np.zeros(cls.shape, np.int64)
    for axis in range(3):
        for step in (-1, 1):
            nbr = np.full(cls.shape, bool(p.edge_unknown))
            src = [slice(None)] * 3; dst = [slice(None)] * 3
            src[axis] = slice(1, None) if step == 1 else slice(None, -1)
            dst[axis] = slice(None, -1) if step == 1 else slice(1, None)
            nbr[tuple(dst)] = unknown[tuple(src)]
            faces += nbr
    front = free & (faces > 0)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        comp, ncomp = ndimage.label(front, structure=np.ones((3, 3, 3), bool))
    else:
        comp = np.zeros(cls.shape, np.int64); ncomp = 0
        for seed in np.argwhere(front):
            if comp[tuple(seed)]:
                continue
            ncomp += 1
            comp[tuple(seed)] = ncomp
            stack = [tuple(int(v) for v in seed)]
            while stack:
                cz, cy, cx = stack.pop()
                for dx, dy, dz in SHIFTS:
                    t = (cz + dz, cy + dy, cx + dx)
                    if 0 <= t[0] < D and 0 <= t[1] < H and 0 <= t[2] < W and front[t] and not comp[t]:
                        comp[t] = ncomp
                        stack.append(t)
    labels = np.full(cls.shape, NONE, np.int32)
    flat = comp.ravel()
    lin = np.flatnonzero(flat)
    order = np.argsort(flat[lin], kind="stable")
    groups = np.split(lin[order], np.cumsum(np.bincount(flat[lin], minlength=ncomp + 1)[1:])[:-1]) if ncomp else []
    groups.sort(key=lambda g: int(g.min()))                           # ascending root
    rows = []
    largest = 0
    for g in groups:
        largest = max(largest, len(g))
        gz, gy, gx = np.unravel_index(g, cls.shape)
        if len(g) < p.min_size:
            labels[gz, gy, gx] = REJECTED
            continue
        labels[gz, gy, gx] = len(rows)
        rows.append((int(g.min()), len(g), (gx.min(), gy.min(), gz.min()), (gx.max(), gy.max(), gz.max()), int(faces[gz, gy, gx].sum()), 0,
                     (int(gx.sum()), int(gy.sum()), int(gz.sum()))))
    info = np.array(rows, INFO_DTYPE) if rows else np.zeros(0, INFO_DTYPE)
    rv = int(info["size"].sum())
    stats = FrontierStats(int(free.sum()), int(front.sum()), ncomp, len(rows), ncomp - len(rows), rv, int(front.sum()) - rv, largest, int(faces[front].sum()))
    return dict(labels=labels, info=info, stats=stats)


def voxel_list(labels):
    """-> (ijk (m, 3) int32 grid indices (ix, iy, iz), label (m,) int32) of every frontier voxel (label != NONE), in ascending linear index (what
    qn_kf_map_frontier_list returns)"""
    lab = np.asarray(labels, np.int32)
    z, y, x = np.nonzero(lab != NONE)
    return np.stack([x, y, z], axis=1).astype(np.int32).reshape(-1, 3), lab[z, y, x]


def costs(labels, regions, cost):
    """labels (D, H, W) int32 with `regions` regions and a route field cost, (D, H, W) or planar (1, H, W) uint32 -> (cost (R,) uint32, ijk (R, 3) int32): per
    region the smallest cost below BLOCKED over its voxels and the voxel attaining it, the smallest linear index on a tie; UNREACHED and (0, 0, 0) without one"""
    lab = np.asarray(labels, np.int32); c = np.asarray(cost, np.uint32)
    D, H, W = lab.shape
    if c.shape not in ((D, H, W), (1 if W * H else 0, H, W)):
        raise ValueError("mapfrontier: the route field must be (D, H, W) or (1, H, W)")
    R = int(regions)
    lin = np.flatnonzero(lab.ravel() >= 0)
    k = lab.ravel()[lin]
    at = c.ravel()[lin % (W * H) if c.shape[0] != D else lin].astype(np.uint64)
    key = np.full(R, 0xffffffffffffffff, np.uint64)
    ok = at < BLOCKED
    np.minimum.at(key, k[ok], (at[ok] << np.uint64(32)) | lin[ok].astype(np.uint64))
    none = key == 0xffffffffffffffff
    v = (key & np.uint64(0xffffffff)).astype(np.int64)
    out = np.where(none, UNREACHED, key >> np.uint64(32)).astype(np.uint32)
    ijk = np.stack([v % max(W, 1), (v // max(W, 1)) % max(H, 1), v // max(W * H, 1)], axis=1).astype(np.int32)
    ijk[none] = 0
    return out, ijk


def centroid(info):
    """the regions' centroids in grid indices, sum / size -> (R, 3) f64; mapoccupancy.centres(centroid, grid) turns them to metres"""
    i = np.asarray(info)
    return i["sum"].astype(np.float64) / np.maximum(i["size"], 1).astype(np.float64)[:, None]
