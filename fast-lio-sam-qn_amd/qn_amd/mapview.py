"""View gain over the occupancy map: how much unknown space a sensor would see from a candidate viewpoint.  The numpy twin of csrc/qn_mapview.inc
(qn_kf_map_view_gain / qn_kf_map_view_grid) and its specification.  Pure numpy, no GPU.

  input        the class bytes (D, H, W) and the grid of the live occupancy result (mapoccupancy.classify), Q viewpoints in world coordinates (f64) and a ray
               table `offsets`, R rows of three int32: a ray's end relative to its start in the occupancy map's fixed point, 1024ths of a voxel.  The table is
               data of the caller (sensor_offsets makes one), so no sine or cosine is part of the rule.  1 <= Q <= 2^16, 1 <= R <= 2^20, every |component| <=
               MAX_OFFSET = 2^25.
  params       ViewParams(gain_mask, stop_mask, max_through, iz_lo, iz_hi): gain_mask class bits 0 .. 2, not 0 (1 << UNKNOWN); stop_mask class bits 0 .. 2, may
               be 0, no bit of gain_mask (1 << OCCUPIED); max_through a u32, 0: no limit (0); the band iz_lo <= iz_hi of layers (0, INT32_MAX).  The defaults
               are interface choices, not measurements.
  viewpoint    A_k = int64(rint((x_k * inv) * 1024)), inv = 1.0 / voxel, exactly as mapoccupancy.quantise: f64, each operation rounded on its own, half to even.
               Status OUTSIDE (1) when a coordinate is not finite, when |x_k * inv| >= 2^20 or when the voxel c(A) = A >> 10 lies outside the grid; otherwise OK
               (0).  An OUTSIDE viewpoint casts nothing and its row is zero apart from the status; ijk is the viewpoint's grid voxel, (0, 0, 0) when OUTSIDE.
  ray          B = A + offsets[r]; the visited voxels v_0 = c(A) .. v_n = c(B) are those of mapoccupancy.walk(A, B) - the same integer rule, a tie going to the
               lowest axis, an origin on a face heading down stepping at once.  They are examined in order, v_0 included:
                 1. v_i outside the grid: the ray ESCAPED; it ends and v_i is not counted in steps.
                 2. otherwise steps += 1; if the class bit of v_i is in stop_mask the ray is BLOCKED and ends.
                 3. otherwise, if its class bit is in gain_mask: the pair (viewpoint, v_i) is marked if the layer iz lies in the band iz_lo .. iz_hi (inclusive,
                    clipped to the grid); through += 1, band or not; if max_through != 0 and through == max_through the ray is SPENT and ends.
                 4. if v_n has been examined without an end, the ray REACHED.
               Every ray of an OK viewpoint ends in exactly one of the four ray ends: blocked, escaped, spent, reached.  A ray with offset (0, 0, 0) examines v_0 only.
  results      gain[q] = the number of distinct voxels marked for viewpoint q; cover[v] = the number of viewpoints that marked voxel v, one u32 per voxel,
               (D, H, W), x fastest.  Sum cover = sum gain.  Distinct is a set property and the tallies are integer sums, so no schedule, pass split or ray
               order changes a byte.
  stats        ViewStats(viewpoints = Q, outside, rays = R, covered = the voxels with cover >= 1, max_cover, total_gain, steps = the sum of the rows' steps).
The engine's kernels are k_mv_origin, k_mv_cast and k_mv_stats, and its call has one synchronisation with the host whatever the number of passes; the engine's
`passes` is a diagnostic of the GPU schedule that the twin does not have.
"""
import math
from collections import namedtuple
import numpy as np
from . import mapoccupancy as mo

OK, OUTSIDE = 0, 1
MAX_OFFSET = 1 << 25
MAX_VIEWPOINTS = 1 << 16
MAX_RAYS = 1 << 20
INT32_MAX = 0x7fffffff
ViewParams = namedtuple("ViewParams", "gain_mask stop_mask max_through iz_lo iz_hi", defaults=(1 << mo.UNKNOWN, 1 << mo.OCCUPIED, 0, 0, INT32_MAX))   # interface choices
ViewStats = namedtuple("ViewStats", "viewpoints outside rays covered max_cover total_gain steps")
VIEW_DTYPE = np.dtype([("status", "<u4"), ("gain", "<u4"), ("blocked", "<u4"), ("escaped", "<u4"), ("spent", "<u4"), ("reached", "<u4"), ("ijk", "<i4", (3,)),
                       ("reserved", "<u4"), ("steps", "<u8")])          # qn_view_info, 48 bytes
assert VIEW_DTYPE.itemsize == 48


def check_params(p):
    g, s, m, lo, hi = (int(v) for v in p)
    if any(int(v) != v for v in p):
        raise ValueError("mapview: integer parameters")
    if g == 0 or g & ~7:
        raise ValueError("mapview: gain_mask must have at least one of the bits 0 .. 2 set and no other")
    if s & ~7 or s < 0 or s & g:
        raise ValueError("mapview: stop_mask has the bits 0 .. 2 only and shares none with gain_mask")
    if not 0 <= m <= 0xffffffff:
        raise ValueError("mapview: max_through must be a u32")
    if not (-INT32_MAX - 1 <= lo <= hi <= INT32_MAX):
        raise ValueError("mapview: iz_lo <= iz_hi, both int32")
    return ViewParams(g, s, m, lo, hi)


def check_offsets(offsets):
    off = np.asarray(offsets)
    if off.ndim != 2 or off.shape[1] != 3 or not 1 <= len(off) <= MAX_RAYS:
        raise ValueError("mapview: a ray table of 1 .. 2^20 rows of three")
    off = off.astype(np.int64)
    if (np.abs(off) > MAX_OFFSET).any():
        raise ValueError("mapview: an offset beyond 2^25")
    return off


def sensor_offsets(voxel, max_range, n_beams, n_azimuth, elev_lo_deg, elev_hi_deg):
    """the ray table of a spinning sensor -> (n_beams * n_azimuth, 3) int32, beam-major (row = beam * n_azimuth + azimuth step): beam b at elevation e_b (n_beams
    values from elev_lo_deg to elev_hi_deg, ends included), azimuth a_j = 2 pi j / n_azimuth, direction (cos e cos a, cos e sin a, sin e),
    offset = rint(direction * (max_range / voxel) * 1024).  ValueError beyond the offset limit."""
    e = np.deg2rad(np.linspace(float(elev_lo_deg), float(elev_hi_deg), int(n_beams)))[:, None]
    a = (2.0 * math.pi * np.arange(int(n_azimuth)) / int(n_azimuth))[None, :]
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e) * np.ones_like(a)], axis=2).reshape(-1, 3)
    off = np.rint(d * (float(max_range) / float(voxel)) * 1024.0)
    if not np.isfinite(off).all() or (np.abs(off) > MAX_OFFSET).any():
        raise ValueError("mapview: a ray of the table reaches beyond the offset limit 2^25")
    return off.astype(np.int32)


def origins(grid, viewpoints):
    """-> (A (Q, 3) int64 fixed point, ijk (Q, 3) int64 grid voxel, ok (Q,) bool) of the viewpoints by the map's own quantisation"""
    g = mo.OccupancyGrid(*grid)
    x = np.asarray(viewpoints, np.float64).reshape(-1, 3)
    if not 1 <= len(x) <= MAX_VIEWPOINTS:
        raise ValueError("mapview: 1 .. 2^16 viewpoints")
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * (np.float64(1.0) / np.float64(g.voxel))
        fin = np.abs(t) < mo.COORD_LIMIT                             # (a NaN fails the comparison, an infinity too)
        A = np.rint(np.where(fin, t, 0.0) * np.float64(1024.0)).astype(np.int64)
    c = (A >> mo.S) - np.asarray(g.minc, np.int64)
    ok = fin.all(axis=1) & (c >= 0).all(axis=1) & (c < np.array([g.width, g.height, g.depth], np.int64)).all(axis=1)
    return A, np.where(ok[:, None], c, 0), ok


def _band(p, depth):
    return max(p.iz_lo, 0), min(p.iz_hi, depth - 1)


def _finish(info, cover, Q, R):
    stats = ViewStats(Q, int((info["status"] == OUTSIDE).sum()), R, int((cover > 0).sum()), int(cover.max(initial=0)), int(cover.sum(dtype=np.uint64)),
                      int(info["steps"].sum(dtype=np.uint64)))
    return dict(info=info, cover=cover, stats=stats)


def gain(classes, grid, viewpoints, offsets, params=None):
    """-> dict(info: (Q,) of VIEW_DTYPE, cover: (D, H, W) uint32, stats: a ViewStats).  All rays of a viewpoint advance together, one walk step a round, as
    mapoccupancy.classify does."""
    p = check_params(ViewParams() if params is None else ViewParams(*params))
    off = check_offsets(offsets)
    cls = np.asarray(classes, np.uint8)
    Dd, Hd, Wd = cls.shape
    flat = cls.reshape(-1)
    dims = np.array([Wd, Hd, Dd], np.int64)
    stride = np.array([1, Wd, Wd * Hd], np.int64)
    A, ijk, ok = origins(grid, viewpoints)
    minc = np.asarray(mo.OccupancyGrid(*grid).minc, np.int64)
    lo, hi = _band(p, Dd)
    Q, R = len(A), len(off)
    info = np.zeros(Q, VIEW_DTYPE)
    info["status"] = np.where(ok, OK, OUTSIDE); info["ijk"] = ijk
    cover = np.zeros(cls.size, np.uint32)
    for q in np.flatnonzero(ok):
        a = A[q][None, :]; b = a + off
        c = a >> mo.S; cend = b >> mo.S
        s = np.sign(b - a); D = np.abs(b - a)
        rem = np.abs(cend - c)
        r = np.where(s > 0, ((c + 1) << mo.S) - a, a - (c << mo.S)) * np.ones_like(b)
        pos = (c - minc) * np.ones_like(b)                           # grid coordinates, (R, 3)
        through = np.zeros(R, np.int64)
        seen = np.zeros(cls.size, bool)
        idx = np.arange(R)
        tally = dict(blocked=0, escaped=0, spent=0, reached=0)
        steps = 0
        while len(idx):
            pp = pos[idx]
            inside = ((pp >= 0) & (pp < dims)).all(axis=1)
            tally["escaped"] += int((~inside).sum())
            idx = idx[inside]; pp = pp[inside]
            steps += len(idx)
            lin = (pp * stride).sum(axis=1)
            bit = np.int64(1) << flat[lin].astype(np.int64)
            stop = (bit & p.stop_mask) != 0
            tally["blocked"] += int(stop.sum())
            g = ~stop & ((bit & p.gain_mask) != 0)
            seen[lin[g & (pp[:, 2] >= lo) & (pp[:, 2] <= hi)]] = True
            through[idx[g]] += 1
            spent = g & (p.max_through != 0) & (through[idx] == p.max_through)
            tally["spent"] += int(spent.sum())
            live = ~stop & ~spent
            done = live & (rem[idx].sum(axis=1) == 0)
            tally["reached"] += int(done.sum())
            idx = idx[live & ~done]
            if not len(idx):
                break
            rr = r[idx]; DD = D[idx]; on = rem[idx] > 0
            best = np.where(on[:, 0], 0, np.where(on[:, 1], 1, 2))
            for k in (1, 2):
                rb = np.take_along_axis(rr, best[:, None], 1)[:, 0]; Db = np.take_along_axis(DD, best[:, None], 1)[:, 0]
                better = on[:, k] & (k > best) & (rr[:, k] * Db < rb * DD[:, k])
                best = np.where(better, k, best)
            pos[idx, best] += s[idx, best]
            r[idx, best] += mo.ONE
            rem[idx, best] -= 1
        row = info[q]
        row["gain"] = int(seen.sum()); row["steps"] = steps
        for f, v in tally.items():
            row[f] = v
        cover += seen
    return _finish(info, cover.reshape(Dd, Hd, Wd), Q, R)


def brute(classes, grid, viewpoints, offsets, params=None):
    """the definition literally: a Python loop over mapoccupancy.walk -> what gain() returns"""
    p = check_params(ViewParams() if params is None else ViewParams(*params))
    off = check_offsets(offsets)
    cls = np.asarray(classes, np.uint8)
    Dd, Hd, Wd = cls.shape
    A, ijk, ok = origins(grid, viewpoints)
    minc = [int(v) for v in mo.OccupancyGrid(*grid).minc]
    lo, hi = _band(p, Dd)
    info = np.zeros(len(A), VIEW_DTYPE)
    cover = np.zeros((Dd, Hd, Wd), np.uint32)
    for q in range(len(A)):
        info[q]["status"] = OK if ok[q] else OUTSIDE
        if not ok[q]:
            continue
        info[q]["ijk"] = ijk[q]
        marked = set()
        n = dict(blocked=0, escaped=0, spent=0, reached=0)
        steps = 0
        a = [int(v) for v in A[q]]
        for o in off:
            through = 0
            end = "reached"
            for v in mo.walk(a, [a[k] + int(o[k]) for k in range(3)]):
                x, y, z = (v[k] - minc[k] for k in range(3))
                if not (0 <= x < Wd and 0 <= y < Hd and 0 <= z < Dd):
                    end = "escaped"
                    break
                steps += 1
                bit = 1 << int(cls[z, y, x])
                if bit & p.stop_mask:
                    end = "blocked"
                    break
                if bit & p.gain_mask:
                    if lo <= z <= hi:
                        marked.add((x, y, z))
                    through += 1
                    if p.max_through != 0 and through == p.max_through:
                        end = "spent"
                        break
            n[end] += 1
        info[q]["gain"] = len(marked); info[q]["steps"] = steps
        for f, v in n.items():
            info[q][f] = v
        for x, y, z in marked:
            cover[z, y, x] += 1
    return _finish(info, cover, len(A), len(off))
