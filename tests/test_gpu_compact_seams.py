"""The seams of the block scan and the block rank (csrc/qn_map_compact.cuh: scan_row / k_scan_rows, lane_rank / block_rank) through every consumer's call
site: the outlier filter, the clusters (with and without a class mask), the occupancy list, the crop and the shared compaction.  Not workloads: hand-made
clouds whose kept pattern is known in closed form.

The map slot gets its exact size through the voxel grid's overflow guard (leaf 1e-4: the records pass through, see tests/test_gpu_cell_walk.py).  A compaction
must leave map[removed == 0], in order; the removed bytes are the classifying call's own and are compared with the construction first.

Rank (MO_BLOCK = 256, four waves): 63, 64, 65, 255, 256 and 257 records - a wave and a block one short, full, one over - with the kept lanes none, all,
alternating, only lane 63 of each wave, only lane 0 of the waves after the first.
Scan (MO_SCAN_BLOCK = 1024 threads, thread i sums chunk blocks): 1 block; 1024 (chunk 1, every thread); 1025 (chunk 2: 513 threads used, the last thread's
range is empty and it still writes the total); 2049 (chunk 3, ragged) - each with a full last block and with a last block of one record, the kept counts
different from block to block.  k_static_scan, the kernel with a tail of its own, has its 2050 tiles in tests/test_gpu_range_edges.py.

The clouds: a record that must be alone sits on its own site of a lattice 4 r apart; records that must have a partner share a site two by two, r / 4 apart
(three on the last site when their number is odd), so every one of them has a neighbour within r and none has one from another site."""
import numpy as np
import pytest
from qn_amd import maplocalize as ml, mapclusters as mc, mapground as mg, mapoccupancy as mocc

F = np.float32
R = 0.25                                                                         # the outlier radius and the cluster tolerance: the lattice is 1 m apart
BLOCK, SCAN_BLOCK = 256, 1024
SIZES = (63, 64, 65, 255, 256, 257)
PATTERNS = ("none", "all", "alternating", "lane63", "lane0_later_waves")
BAD = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf]], F)


def pattern(name, n):
    i = np.arange(n)
    return {"none": i < 0, "all": i >= 0, "alternating": i % 2 == 0, "lane63": i % 64 == 63, "lane0_later_waves": (i % 64 == 0) & (i >= 64)}[name]


def split(sel):
    """the records of `sel` -> (those that share sites, those that are non-finite): three non-finite records from the middle of sel, fewer where sel is short
    or where that would leave one record to share a site with nobody"""
    pos = np.flatnonzero(sel)
    nf = min(3, len(pos))
    if len(pos) - nf == 1:
        nf -= 1
    bad = np.zeros(len(sel), bool)
    bad[pos[(len(pos) - nf) // 2:][:nf]] = True
    return sel & ~bad, bad


def cloud(paired, bad=None):
    """-> (n, 3) f32: the records of `paired` two by two on a site, those of `bad` non-finite, every other record alone on its site"""
    n = len(paired)
    bad = np.zeros(n, bool) if bad is None else bad
    m = int(paired.sum())
    assert m != 1 and not (paired & bad).any()
    k = np.arange(m)
    site = np.zeros(n, np.int64); slot = np.zeros(n, np.int64)
    site[paired] = np.minimum(k // 2, max(m // 2 - 1, 0)); slot[paired] = k - 2 * site[paired]
    alone = ~paired
    site[alone] = m // 2 + np.arange(int(alone.sum()))
    a = max(2, int(np.ceil((int(site.max()) + 1) ** (1.0 / 3.0))))
    while a ** 3 <= int(site.max()):
        a += 1
    pts = np.stack([site % a, (site // a) % a, site // (a * a)], axis=1) * (4.0 * R)
    pts[:, 0] += slot * (R / 4.0)
    pts = pts.astype(F)
    pts[bad] = BAD[np.arange(int(bad.sum())) % 3]
    if n == 1:
        pts[0, 0] = 3.0e5                                                        # (a lone record trips the guard by its coordinate, not by an extent)
    return pts


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def as_map(store, pts):
    """pts as the store's map slot -> the map as the store downloads it"""
    n = store.build_map([store.add(pts)], [np.eye(4)], 1e-4)
    got = store.download_map(n)
    fin = np.isfinite(pts).all(axis=1)
    assert n == len(pts) and got[fin, :3].tobytes() == pts[fin].tobytes() and not np.isfinite(got[~fin, :3]).all(axis=1).any(), "the cloud did not pass through"
    return got


def filter_outliers(store, keep, bad=None):
    """the cloud of `keep` through map_outliers and map_remove_outliers: the removed bytes are the construction's, the slot is map[removed == 0]"""
    from qn_amd import engine
    bad = np.zeros(len(keep), bool) if bad is None else bad
    got = as_map(store, cloud(keep & ~bad, bad))
    stats, cnt, _, rm = store.map_outliers(engine.OutlierParams(R, 1.0, 1))
    assert np.array_equal(rm == 0, keep), "the classification is not the construction's"
    assert stats["removed"] == int((~keep).sum())
    _, n = store.map_remove_outliers()
    assert n == int(keep.sum())
    if n:
        assert store.download_map(n).tobytes() == got[rm == 0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_rank_seams_of_the_outlier_filter(store, n):
    """k_mo_flag's count, k_scan_rows, k_mo_compact's block_rank: an isolated point is removed, a point with a partner stays, a non-finite record stays"""
    for name in PATTERNS:
        keep = pattern(name, n)
        paired, bad = split(keep)
        filter_outliers(store, keep, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_rank_seams_of_the_cluster_labels(store, n):
    """k_mc_root_label's block_rank, min_size = 1: every kept record is alone, more than the tolerance from all others, so it is its own cluster and its label
    its rank among the kept.  The others are non-finite (no label) or share a site and are turned down by max_size = 1 - the only way to a finite record
    whose root is not kept, which the pattern `none` needs - so their root, the lower index of the site, takes the other branch."""
    from qn_amd import engine
    for name in PATTERNS:
        keep = pattern(name, n)
        paired, bad = split(~keep)
        as_map(store, cloud(paired, bad))
        stats, label, root, size, clusters = store.map_clusters(engine.ClusterParams(R, 1, 1, 0))
        want = np.full(n, mc.REJECTED, np.int32)
        want[bad] = mc.NONE
        want[keep] = np.arange(int(keep.sum()))
        assert np.array_equal(label, want), name
        assert np.array_equal(root[keep], np.flatnonzero(keep)) and (root[bad] == mc.NO_ROOT).all() and (size[keep] == 1).all(), name
        assert stats["clusters"] == int(keep.sum()) and np.array_equal(clusters["root"], np.flatnonzero(keep)), name


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_rank_seams_of_the_cluster_members(store, n):
    """k_mc_member's count, k_scan_rows, k_mc_pick's block_rank: the members under a class mask after map_ground.  Every record has a column of its own on a
    flat 4 m lattice; the members lie at z = 0 (GROUND), the others 1 m up (OBSTACLE: the envelope rises 2^-10 m a column, 1 / 16 m across the lattice).
    Without a member all records are ground and the mask asks for obstacles.  Every member is its own cluster: its label is its rank among the members, and
    its root comes back through the compacted cloud's map indices."""
    from qn_amd import engine
    a = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    for name in PATTERNS:
        keep = pattern(name, n)
        pts = np.stack([4.0 * (i % a), 4.0 * (i // a), np.where(keep, 0.0, 1.0)], axis=1).astype(F)
        as_map(store, pts)
        _, cls, _ = store.map_ground(engine.GroundParams(1.0, 1e-4, 0.2, 2.0, 1))
        want_cls = np.where(keep, mg.GROUND, mg.OBSTACLE) if keep.any() else np.full(n, mg.GROUND)
        assert np.array_equal(cls, want_cls), name
        mask = 1 << mg.GROUND if keep.any() else 1 << mg.OBSTACLE
        stats, label, root, size, _ = store.map_clusters(engine.ClusterParams(1.0, 1, 0xffffffff, mask))
        assert stats["members"] == stats["clusters"] == int(keep.sum()), name
        assert np.array_equal(label, np.where(keep, np.cumsum(keep) - 1, mc.NONE)), name
        assert np.array_equal(root, np.where(keep, i, mc.NO_ROOT)), name


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_rank_seams_of_the_occupancy_list(store, n):
    """k_dg_list_flag's count, k_scan_rows, k_dg_list_pick's block_rank (qn_dense_grid.cuh, on OcList) on a grid of n x 1 x 1 voxels, for each of the three single-class masks.  One keyframe of
    one record a quarter of a voxel from the sensor, listed once per hit with the sensor in the middle of a voxel: the ray ends in the voxel it starts in, a hit
    and no miss.  min_hits = 2: two hits make a voxel OCCUPIED, one FREE, none UNKNOWN.  The grid spans the rays' ends, so its first and its last voxel cannot
    be UNKNOWN: there the pattern gives way."""
    from qn_amd import engine
    kid = store.add(np.array([[0.25, 0.0, 0.0]], F))
    params = engine.OccupancyParams(1.0, 0.0, 60.0, 0, 2, 2)
    for name in PATTERNS:
        p = pattern(name, n)
        for c, other in ((mocc.OCCUPIED, mocc.FREE), (mocc.FREE, mocc.OCCUPIED), (mocc.UNKNOWN, mocc.FREE)):
            want = np.where(p, c, other)
            if c == mocc.UNKNOWN:
                want[[0, n - 1]] = other
            vox = np.repeat(np.arange(n), want)                                  # (the class is the number of hits)
            poses = np.tile(np.eye(4), (len(vox), 1, 1))
            poses[:, 0, 3] = vox + 0.5; poses[:, 1, 3] = 0.5; poses[:, 2, 3] = 0.5
            stats = store.map_occupancy([kid] * len(vox), poses, params)
            assert (stats["width"], stats["height"], stats["depth"]) == (n, 1, 1) and stats["total_misses"] == 0, name
            for m in (mocc.UNKNOWN, mocc.FREE, mocc.OCCUPIED):
                ijk, hits, misses = store.map_occupancy_list(1 << m)
                k = np.flatnonzero(want == m)
                assert np.array_equal(ijk, np.stack([k, 0 * k, 0 * k], axis=1)) and (hits == m).all() and not misses.any(), (name, c, m)


def block_counts(nb, last):
    """-> keep (n,) bool over nb blocks, the last of `last` records: block b keeps (37 b + 11) mod 257 of its records, at seeded places"""
    n = (nb - 1) * BLOCK + last
    want = np.minimum((37 * np.arange(nb) + 11) % 257, BLOCK)
    order = np.argsort(np.random.default_rng(nb).random((nb, BLOCK)), axis=1)
    keep = (order < want[:, None]).reshape(-1)[:n]
    if int(keep.sum()) == 1:
        keep[:] = False                                                          # (a kept point needs a partner)
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("last", [BLOCK, 1], ids=["full", "one"])
@pytest.mark.parametrize("nb", [1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
def test_scan_seams_of_the_outlier_filter(store, nb, last):
    keep = block_counts(nb, last)
    per_block = np.add.reduceat(keep, np.arange(0, len(keep), BLOCK))
    assert len(per_block) == nb and (nb < 3 or len(set(per_block[:-1])) > min(nb - 1, 200))
    filter_outliers(store, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("last", [BLOCK, 1], ids=["full", "one"])
@pytest.mark.parametrize("nc", [1, 65])
def test_scan_seams_of_the_crop(store, nc, last):
    """k_scan_rows in place, a block per centre, at 1025 blocks (65 centres: a second pass of one), against maplocalize.crop_indices"""
    n = SCAN_BLOCK * BLOCK + last
    got = as_map(store, cloud(np.zeros(n, bool)))
    side = float(np.ceil(n ** (1.0 / 3.0)))
    centres = np.random.default_rng(nc).uniform(0.0, side, (nc, 3))
    centres[0] = got[n - 1, :3]                                                  # (the first crop holds the last record)
    crops = store.map_crop(centres, 6.0)
    for c, r in zip(centres, crops):
        want = ml.crop_indices(got, c, 6.0)
        assert len(want) > 100 and np.array_equal(r["idx"], want) and r["xyzi"].tobytes() == got[want].tobytes()
    assert crops[0]["idx"][-1] == n - 1
    per_block = np.bincount(crops[-1]["idx"] // BLOCK, minlength=SCAN_BLOCK + 1)
    assert len(set(per_block)) > 10 and (per_block == 0).any()


@pytest.mark.gpu
def test_scan_seams_of_the_occupancy_list(store):
    """64 x 64 x 65 voxels: 1040 blocks, chunk 2, the last 504 threads without a block; a handful of long rays from one corner, against the twin"""
    from qn_amd import engine
    ends = np.array([[63.0, 63.0, 64.0], [63.0, 0.0, 0.0], [0.0, 63.0, 0.0], [0.0, 0.0, 64.0], [63.0, 63.0, 0.0], [40.0, 63.0, 64.0], [63.0, 20.0, 64.0],
                     [63.0, 63.0, 30.0]], F)
    pose = np.eye(4); pose[:3, 3] = 0.5
    kid = store.add(ends)
    params = engine.OccupancyParams(1.0, 0.0, 200.0, 1, 1, 2)
    stats = store.map_occupancy([kid], [pose], params)
    assert (stats["width"], stats["height"], stats["depth"]) == (64, 64, 65) and stats["n_rays"] == len(ends)
    want = mocc.classify([ends], [pose], params.twin())
    assert (64 * 64 * 65 + BLOCK - 1) // BLOCK > SCAN_BLOCK
    for m in (mocc.UNKNOWN, mocc.FREE, mocc.OCCUPIED):
        ijk, hits, misses = store.map_occupancy_list(1 << m)
        w_ijk, w_hits, w_misses = mocc.voxel_list(want, 1 << m)
        assert len(w_ijk) > 0 and np.array_equal(ijk, w_ijk) and np.array_equal(hits, w_hits) and np.array_equal(misses, w_misses), m
