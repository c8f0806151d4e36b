"""The range-image kernels (k_range_bin, k_freespace_check, k_freespace_reduce, k_static_vote, k_static_scan, k_static_compact: csrc/qn_range.cuh's
fs_project / fs_window / fs_class) on the edge cases of tests/range_edge_cases.py, bit for bit against the numpy twins qn_amd/freespace.py and
qn_amd/staticmap.py, and against what the generators state by construction wherever they state it (tests/test_range_edges_cpu.py holds the twin to the
same statements and to a scalar restatement of the specification, without a GPU).

What the cases reach that ray-cast scenes and Gaussian clouds do not:
  knife edges   transformed points within an ulp of a column boundary and a row edge (diagonal transforms, through freespace_batch and as witness votes), at
                32 x 720 (column table in LDS) and 2 x 4608 (in global memory).  A build that contracts c y - s x, x x + y y or the transform into a fused
                multiply-add gives other class bytes here (what a contracted rebuild showed).
  thresholds    tol = 0 (class by the rounding of float32(r)), r == min_range and one f32 ulp below, r beyond the f32 maximum, -0.0, f32 subnormals.
  seams         record counts 1 .. 4097 around the wave (64), the round (FS_BLOCK 512) and the tile (FS_TILE 2048) in all six kernels, with the compaction's
                removal patterns; more than SV_SCAN_BLOCK = 1024 tiles in the scan (chunk = 3); more than SV_CHUNK = 32768 entries (a second launch);
                more than 256 tiles in one direction of the reduce; 255 witnesses (the u8 counters full).
Everything runs on ONE store, each case adding its keyframes, so the image slots grow (range_reserve) from case to case; the cases of another image shape or
min_range come last (new image parameters discard every image), and the first keyframe's images are compared again before them and re-made after them.
Not covered: the describe path's own chunking (more than 32768 keyframes in one range_describe) - filling a store with that many keyframes was not measured."""
import os
import sys
import numpy as np
import pytest
from qn_amd import freespace as fs, staticmap as sm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import range_edge_cases as rc

pytestmark = pytest.mark.gpu
FIELDS = ("n", "n_finite", "in_fov", "observed", "seen_through", "occluded", "agree")


def _bits_equal(got, want, what):
    for g, w, name in zip(got, want, ("near", "far")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


class World:
    def __init__(self, engine):
        self.engine = engine
        self.store = engine.KeyframeStore()
        self.image_params = None
        self.discards = 0
        self.use(rc.EDGE)
        self.early_cloud, self.early_expect = rc.pattern_records(rc.EDGE, rc.mixed(777, 5))
        self.early = self.store.add(self.early_cloud)
        assert self.store.range_describe([self.early]) == [0]
        self.early_images = self.store.range_images(self.early)

    def use(self, p):
        key = (p.n_rows, p.n_cols, p.el_lo, p.el_hi, p.min_range)
        if self.image_params is not None and key != self.image_params:
            self.discards += 1
        self.image_params = key
        self.store.range_set_params(p)

    def load(self, case):
        """the case's keyframes into the store, described -> (keyframe ids, the twin's images)"""
        self.use(case.params)
        kids = [self.store.add(c) for c in case.clouds]
        status = self.store.range_describe(kids)
        images = rc.twin_images(case)
        assert status == [0 if np.isfinite(n).any() else self.engine.QN_ERR_EMPTY_CLOUD for n, _ in images], case.name
        return kids, images

    def check_images(self, case, kids, images, which=None):
        for k in (range(len(kids)) if which is None else which):
            got = self.store.range_images(kids[k])
            _bits_equal(got, images[k], (case.name, k))
            if k in case.expect["pixels"]:
                pix, near, far = case.expect["pixels"][k]
                assert np.array_equal(np.isfinite(got[0]), pix) and np.array_equal(got[1] > 0, pix), (case.name, "pixels", k)
                assert np.allclose(got[0][pix], near[pix], rtol=1e-5, atol=0) and np.allclose(got[1][pix], far[pix], rtol=1e-5, atol=0), (case.name, k)

    def check_pairs(self, case, kids, images):
        """all pairs of the case in one freespace_batch: counts and every class byte of both directions"""
        recs = self.store.freespace_batch([kids[q] for q, _, _ in case.pairs], [kids[c] for _, c, _ in case.pairs], [T for _, _, T in case.pairs])
        want = rc.twin_pairs(case, images)
        wrong = []
        for j, rec in enumerate(recs):
            for d, key in enumerate(("q_in_c", "c_in_q")):
                cls = self.store.freespace_points(j, d)
                if not np.array_equal(cls, want[j][d]["classes"]):
                    bad = np.flatnonzero(cls != want[j][d]["classes"])
                    wrong.append((j, d, case.meta["edges"][j] if "edges" in case.meta else None, len(bad), bad[:6].tolist(), cls[bad[:6]].tolist(),
                                  want[j][d]["classes"][bad[:6]].tolist()))
                    continue
                assert {f: rec[key][f] for f in FIELDS} == {f: want[j][d][f] for f in FIELDS}, (case.name, j, key)
                if (j, d) in case.expect["cls"]:
                    assert np.array_equal(cls, case.expect["cls"][(j, d)]), (case.name, j, d, "by construction")
                    assert {f: rec[key][f] for f in FIELDS} == rc.counts_of(cls, case.meta["finite"][(j, d)]), (case.name, j, key, "by construction")
        assert not wrong, (case.name, "(pair, direction, (column, row edge, shift), wrong bytes, where, got, twin):", wrong[:10], len(wrong))
        return recs

    def check_votes(self, case, kids, images, points=None, with_map=False):
        """static_classify under every rule of the case: removed of every entry, static_points of the entries in `points` (None: all)"""
        e = case.entries
        ids = [kids[i] for i in e["ids"]]
        votes = rc.twin_votes(case, images)
        for rule in case.rules:
            got = self.store.static_classify(ids, e["poses"], witnesses=(e["wit_off"], e["wit"]), params=self.engine.StaticParams(*rule))
            removed = [sm.removed(st, ag, sm.StaticParams(*rule)) for st, ag in votes]
            assert got["removed"].tolist() == [int(r.sum()) for r in removed], (case.name, rule, np.flatnonzero(got["removed"] != [int(r.sum()) for r in removed])[:10])
            assert got["status"] == [0 if len(r) else self.engine.QN_ERR_EMPTY_CLOUD for r in removed], (case.name, rule)
            wrong = []
            for k in (range(len(ids)) if points is None else points):
                st, ag, rm = self.store.static_points(k)
                ok = np.array_equal(st, votes[k][0]) and np.array_equal(ag, votes[k][1]) and np.array_equal(rm, removed[k].astype(np.uint8))
                if not ok:
                    wrong.append((k, case.meta["edges"][k - 1] if "edges" in case.meta and k else None, int((st != votes[k][0]).sum()), int((ag != votes[k][1]).sum())))
                if k in case.expect["votes"]:
                    assert np.array_equal(st, case.expect["votes"][k][0]) and np.array_equal(ag, case.expect["votes"][k][1]), (case.name, rule, k, "by construction")
            assert not wrong, (case.name, rule, "(entry, (column, row edge, shift), wrong seen_through, wrong agree):", wrong[:10], len(wrong))
            if with_map:
                self.check_map(case, e, removed, 0.5)
        return votes

    def check_map(self, case, e, removed, leaf):
        """build_map_static against build_map, on a second store, of the records the twin keeps (each distinct kept cloud added once; ids repeat)"""
        n = self.store.build_map_static(leaf)
        got = self.store.download_map(n)
        other = self.engine.KeyframeStore()
        try:
            memo, ids2 = {}, []
            for kf, rm in zip(e["ids"], removed):
                key = (kf, rm.tobytes())
                if key not in memo:
                    memo[key] = other.add(case.clouds[kf][~rm])
                ids2.append(memo[key])
            ref = other.download_map(other.build_map(ids2, e["poses"], leaf))
        finally:
            other.close()
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (case.name, leaf, got.shape, ref.shape)
        assert n > 0


@pytest.fixture(scope="module")
def world():
    from qn_amd import engine
    w = World(engine)
    yield w
    w.store.close()


# ---- the first image shape (8 x 64): seams
def test_seam_counts_in_all_six_kernels(world):
    case = rc.get("seams")
    kids, images = world.load(case)
    world.check_images(case, kids, images)
    recs = world.check_pairs(case, kids, images)
    assert sorted({r["q_in_c"]["n"] for r in recs}) == rc.SEAM_COUNTS and len(recs) == 7 * len(rc.SEAM_COUNTS)
    world.check_votes(case, kids, images, with_map=True)


def test_more_than_1024_tiles_in_the_scan(world):
    case = rc.get("scan-tiles")
    assert case.meta["tiles"] > 2 * rc.SV_SCAN_BLOCK
    kids, images = world.load(case)
    votes = world.check_votes(case, kids, images, with_map=True)
    assert sum(int(v[0].sum()) for v in votes) > 1000               # (the comparison is not of empty sets)


def test_more_than_32768_entries(world):
    case = rc.get("many-entries")
    count = len(case.entries["ids"])
    kids, images = world.load(case)
    votes = world.check_votes(case, kids, images, points=[0, 1, 2] + list(range(rc.SV_CHUNK - 2, rc.SV_CHUNK + 3)))
    assert count == rc.SV_CHUNK + 3 and sum(int(v[0].sum()) for v in votes[rc.SV_CHUNK:]) > 0


def test_more_than_256_tiles_in_one_direction(world):
    case = rc.get("reduce-tiles")
    kids, images = world.load(case)
    world.check_images(case, kids, images)
    rec, = world.check_pairs(case, kids, images)
    assert rec["q_in_c"]["n"] == rc.REDUCE_SLOTS * rc.FS_TILE + 1 and min(rec["q_in_c"][f] for f in FIELDS) > 50000


def test_255_witnesses_fill_the_counters(world):
    case = rc.get("full-counters")
    kids, images = world.load(case)
    world.check_votes(case, kids, images, points=[0, 1, 2, 200, 383])
    st, ag, _ = world.store.static_points(0)
    seq = case.expect["votes"][0]
    assert (st[seq[0] > 0] == 255).all() and (ag[seq[1] > 0] == 255).all() and (seq[0] > 0).sum() > 30 and (seq[1] > 0).sum() > 30


def test_zero_tolerance_and_ranges_beyond_f32(world):
    for name in ("zero-tolerance", "beyond-f32"):
        case = rc.get(name)
        kids, images = world.load(case)
        world.check_images(case, kids, images)
        world.check_pairs(case, kids, images)
        world.check_votes(case, kids, images)
    near, far = world.store.range_images(kids[0])
    r, c = case.meta["inf_pixel"]
    assert near[r, c] == np.inf and far[r, c] == np.inf


def test_an_early_keyframe_keeps_its_images_while_the_slots_grow(world):
    store = world.store
    if world.discards:                                              # (run out of order: the images were discarded with their parameters; make them again)
        world.use(rc.EDGE)
        assert store.range_describe([world.early]) == [0]
    tiny = [store.add(rc.checkerboard(rc.EDGE, 20.0 + k)[k::7]) for k in range(40)]       # 40 more slots: the block grows at least once here
    assert store.range_describe(tiny) == [0] * 40
    got = store.range_images(world.early)
    _bits_equal(got, world.early_images, "early")
    _bits_equal(got, fs.range_images(world.early_cloud, rc.EDGE), "early, twin")
    assert np.array_equal(np.isfinite(got[0]), world.early_expect["pixels"])
    _bits_equal(store.range_images(tiny[3]), fs.range_images(rc.checkerboard(rc.EDGE, 23.0)[3::7], rc.EDGE), "tiny")


# ---- other image shapes and other min_range: every set of new parameters discards the images, each case describes its own keyframes
@pytest.mark.parametrize("name", ["knife-32x720", "knife-2x4608"])
def test_knife_edges_through_the_check_and_the_votes(world, name):
    case = rc.get(name)
    assert len(case.pairs) >= 32
    kids, images = world.load(case)
    world.check_images(case, kids, images, which=[0, 1, len(kids) - 1])
    world.check_pairs(case, kids, images)
    world.check_votes(case, kids, images)


def test_seam_counts_with_the_table_in_global_memory(world):
    case = rc.get("seams-wide")
    assert case.params.n_cols > 4096
    kids, images = world.load(case)
    world.check_images(case, kids, images, which=range(0, len(kids), 3))
    world.check_pairs(case, kids, images)
    world.check_votes(case, kids, images, with_map=True)


@pytest.mark.parametrize("name", ["min-range-5", "min-range-1.25", "min-range-40", "subnormals"])
def test_min_range_and_subnormals(world, name):
    case = rc.get(name)
    kids, images = world.load(case)
    world.check_images(case, kids, images)
    rec, = world.check_pairs(case, kids, images)
    world.check_votes(case, kids, images)
    cls = world.store.freespace_points(0, 0)
    if "dropped" in case.meta:
        assert np.array_equal(cls == 0, case.meta["dropped"][(0, 0)]) and rec["q_in_c"]["in_fov"] == 12
    else:
        assert {2, 3, 4} <= set(cls.tolist())                       # subnormal ranges are told apart: a quarter, three times and once the range


def test_back_at_the_first_shape_the_early_keyframe_gets_the_same_images(world):
    world.use(rc.EDGE)
    assert world.store.range_describe([world.early]) == [0]
    _bits_equal(world.store.range_images(world.early), world.early_images, "early, again")
