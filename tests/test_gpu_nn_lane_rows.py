"""The one-query-per-lane first 1-NN pass (NnLaneK, knob nn_lane = 1) where a probe row crosses an 8-cell tile boundary: the row's two runs of the cell-sorted
points are walked as ONE merged run.  Target clouds of ~3000 points on grids of 9, 13 and 17 cells in x (knob `cell` = 1 m: the tile boundaries at x-cell 8 and 16
lie inside), with emptied regions (rows with no point in the first part, the second part, or at all) and ~6 points per cell (rows of 3 cells hold well over four
candidates: several four-candidate trips, the last one partial).  Queries within one cell on either side of x-cell 8 and 16, at and beyond the grid's six faces, and
spread over the volume.  The first iteration's correspondences and squared distances with nn_lane = 1 and nn_lane = 0 (the cooperative pass) are equal element
for element, and both equal a numpy brute force in the kernels' f32 arithmetic, lowest index on ties (exact duplicates are in the target)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL = 1.0
LY, LZ = 6.5, 3.5


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def make_target(lx, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform([0, 0, 0], [lx, LY, LZ], (3400, 3))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    keep = ~((y >= 2.0) & (y < 3.0) & (z >= 1.0) & (z < 2.0))                       # a (y, z) row empty over the whole length
    keep &= ~((x >= 5.0) & (x < 8.0) & (y >= 4.0) & (y < 5.0))                      # rows whose part left of the tile boundary at x-cell 8 is empty
    keep &= ~((x >= 8.0) & (x < 11.0) & (y >= 5.0) & (y < 6.0))                     # ... and right of it
    keep &= ~((x >= 15.0) & (y >= 0.0) & (y < 1.0))                                 # the same at x-cell 16 (17-cell grid)
    p = p[keep][:2990]
    p = np.concatenate([p, [[0, 0, 0], [lx, LY, LZ]], p[[5, 5, 900, 1500]]])      # the box's corners pin the grid; exact duplicates: ties
    return f32(p)


def make_queries(lx, seed):
    rng = np.random.default_rng(seed)
    q = [rng.uniform([0, 0, 0], [lx, LY, LZ], (700, 3))]
    for b in (8.0, 16.0):                                                           # within one cell on either side of a tile boundary (and exactly on it)
        if b < lx + 1.0:
            s = rng.uniform([b - 1.0, 0, 0], [min(b + 1.0, lx), LY, LZ], (500, 3)); s[:40, 0] = b; s[40:60, 0] = np.nextafter(np.float32(b), np.float32(0))
            q.append(s)
    for a, L in enumerate((lx, LY, LZ)):                                            # the six faces: on them, just inside, and up to 0.4 cells outside
        for side in (0.0, L):
            s = rng.uniform([0, 0, 0], [lx, LY, LZ], (90, 3))
            s[:30, a] = side; s[30:60, a] = side + rng.uniform(-0.05, 0.05, 30); s[60:, a] = side + np.sign(side - 0.5 * L) * rng.uniform(0.0, 0.4, 30)
            q.append(s)
    return f32(np.concatenate(q))


def brute(src, tgt):
    """(index, f32 squared distance) of the nearest target point, (dx^2 + dy^2) + dz^2 in f32 as the kernels form it, lowest index on ties"""
    idx = np.zeros(len(src), np.int32); d2 = np.zeros(len(src), np.float32)
    for i, s in enumerate(src):
        d = (tgt - s) ** 2
        dd = (d[:, 0] + d[:, 1]) + d[:, 2]
        j = int(np.argmin(dd))                                                      # (the first of equal minima)
        idx[i] = j; d2[i] = dd[j]
    return idx, d2


@pytest.mark.parametrize("lx", [8.5, 12.5, 16.5])
def test_rows_across_tile_boundaries(lx):
    from qn_amd import engine
    tgt, src = make_target(lx, int(lx * 2)), make_queries(lx, 100 + int(lx * 2))
    assert 2900 <= len(tgt) <= 3100 and tgt.dtype == np.float32 and src.dtype == np.float32
    bi, bd = brute(src, tgt)
    out = {}
    for lane in (1, 0):
        ctx = engine.Context(4096)
        ctx.debug_set("cell", CELL); ctx.debug_set("nn_lane", lane)
        g = engine.NanoGICP(ctx); g.setCorrespondenceRandomness(15); g.setMaxCorrespondenceDistance(52.5)
        g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
        gi = ctx.grid_info(1)
        assert abs(gi["cell"] - CELL) < 1e-6 and int(gi["dims"][0]) == int(lx) + 1 and 9 <= int(gi["dims"][0]) <= 17, gi
        _, _, _, corr, sqd = g.linearize(np.eye(4))
        out[lane] = (corr.copy(), sqd.copy())
        ctx.close()
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    for lane in (1, 0):
        bad = np.nonzero(out[lane][0] != bi)[0]
        assert bad.size == 0, ("nn_lane", lane, bad.size, bad[:5].tolist(), out[lane][0][bad[:5]].tolist(), bi[bad[:5]].tolist())
        assert np.array_equal(out[lane][1], bd), ("nn_lane", lane)
