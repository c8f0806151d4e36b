"""The map's clusters on the GPU (qn_kf_map_clusters / qn_kf_map_cluster_points / qn_kf_map_cluster_list / qn_kf_map_drop_rejected_clusters) against their
specification, the numpy twin qn_amd/mapclusters.py, run on the map the store itself downloads.  Everything is an integer or an f32 picked by an order-free
rule, so everything is compared bit for bit: label, root and size of every point, the cluster list, every field of the statistics, and a rerun.  The kernels'
block is 256 points (the sizes 1, 2, 255, 256, 257 and 513 are its launch seams).  Hand-made points (tests/test_map_clusters_twin.py, with their answers worked
out by hand) reach the map slot unchanged through the voxel grid's overflow guard: at leaf 1e-4 a cloud that spans half a metre on every axis passes through
as it is, duplicates, signed zeros and non-finite records included."""
import ctypes as C
import math
import subprocess
import numpy as np
import pytest
from qn_amd import mapclusters as mc, mapground as mg, synth
import test_map_clusters_twin as T

pytestmark = pytest.mark.gpu
B = 256                                                              # MO_BLOCK of csrc/qn_mapclusters.inc
F = np.float32
SEN = synth.SpinningLidar(n_beams=16, n_cols=300)
POSES = [synth.sensor_pose(-6.0, 0.5, 0.1), synth.sensor_pose(0.0, -0.4, 0.3), synth.sensor_pose(6.5, 0.8, -0.2), synth.sensor_pose(12.0, -0.2, 0.4)]
STAT_FIELDS = mc.ClusterStats._fields
OBJECTS = (1 << mg.OBSTACLE) | (1 << mg.OVERHEAD)
ALL = 0xffffffff


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


@pytest.fixture(scope="module")
def scans(store):
    prims = synth.Scene(np.random.default_rng(7), 120.0).primitives()
    return [int(i) for i in store.add_lidar_scans(prims, SEN, POSES, [11, 12, 13, 14])]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _gpu(store, params):
    """map_clusters in the form of the twin's result"""
    from qn_amd import engine
    stats, label, root, size, cl = store.map_clusters(engine.ClusterParams(*params))
    info = np.zeros(len(cl["root"]), mc.INFO_DTYPE)
    for f in ("root", "size", "lo", "hi", "sum_q"):
        info[f] = cl[f]
    return dict(label=label, root=root, size=size, clusters=info, centroid=cl["centroid"], stats=mc.ClusterStats(*[stats[f] for f in STAT_FIELDS]))


def equal_the_twin(store, params, what, classes=None):
    """map_clusters of the store's map against the twin on the downloaded map -> (the GPU result in the twin's form, the map)"""
    pts = store.download_map(store._map_n)
    got = _gpu(store, params)
    want = mc.classify(pts, params, classes)
    s = got["stats"]
    print("%s: %d points, %d members, %d edges, %d components (largest %d), %d clusters, %d too small, %d too large" %
          (what, s.n, s.members, s.edges, s.components, s.largest, s.clusters, s.too_small, s.too_large))
    assert len(got["label"]) == len(pts) and got["label"].dtype == np.int32 and got["root"].dtype == np.uint32 and got["size"].dtype == np.uint32
    for f in ("root", "size", "label"):
        assert np.array_equal(got[f], want[f]), (what, f, int((got[f] != want[f]).sum()))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert _same(got["clusters"], want["clusters"]), what            # all 56 bytes of every record: -0 and +0 are different bytes
    assert _same(got["centroid"], want["centroid"]), what
    again = _gpu(store, params)                                      # a rerun returns the same bytes
    assert again["stats"] == got["stats"] and all(_same(again[f], got[f]) for f in ("label", "root", "size", "clusters")), what
    return got, pts


def _map_of(store, clouds, poses, leaf):
    ids = [store.add(c) for c in clouds]
    return store.build_map(ids, poses, leaf)


def _as_it_is(store, pts, pose=None):
    """the records themselves as the map (leaf 1e-4: the overflow guard passes them through)"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = _map_of(store, [pts], [np.eye(4) if pose is None else pose], 1e-4)
    got = store.download_map(n)
    assert n == len(pts) and _same(got[:, :3], pts[:, :3]), "the cloud did not pass through"
    return pts


@pytest.mark.parametrize("n", [1, 2, B - 1, B, B + 1, 2 * B + 1])
def test_launch_seams(store, n):
    rng = np.random.default_rng(100 + n)
    side = int(math.ceil(math.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    pts = np.zeros((n, 3), np.float32)
    pts[:, :2] = ij * 0.3 + rng.uniform(-0.05, 0.05, (n, 2)); pts[:, 2] = 0.02 * np.sin(ij[:, 0]) + rng.uniform(-0.01, 0.01, n)
    assert _map_of(store, [pts], [np.eye(4)], 0.1) == n              # at least 0.2 apart on an axis: every point is a voxel of its own
    got, _ = equal_the_twin(store, (0.5, 2, ALL, 0), "map of %d points" % n)
    s = got["stats"]                                                 # grid neighbours are at most 0.41 m apart: one component
    assert (s.components, s.largest, s.clusters, s.too_small) == (1, n, int(n >= 2), int(n < 2)) and (got["root"] == 0).all()


def test_a_long_thin_component(store):
    pts, p, order = T.case_line()
    _as_it_is(store, pts)
    got, _ = equal_the_twin(store, p, "a snaking line of 3000 points")
    T.check_line(got, order)
    pts, p, order = T.case_line(opened=1310)
    _as_it_is(store, pts)
    got, _ = equal_the_twin(store, p, "the line with one link opened")
    T.check_line(got, order, 1310)


def test_the_knife_edge(store):
    pts, p = T.case_knife_edge()
    _as_it_is(store, pts)
    T.check_knife_edge(equal_the_twin(store, p, "on the tolerance / just beyond")[0])
    pts, p = T.case_lattice_on_the_radius()
    _as_it_is(store, pts)
    T.check_lattice_on_the_radius(equal_the_twin(store, p, "lattice with partners on the tolerance")[0])


def test_duplicates_at_distinct_indices_join(store):
    pts, p = T.case_duplicates()
    _as_it_is(store, pts)
    T.check_duplicates(equal_the_twin(store, p, "duplicates")[0])


def test_size_seams(store):
    pts, p, clump, sizes = T.case_size_seams()
    _as_it_is(store, pts)
    T.check_size_seams(equal_the_twin(store, p, "clumps of min - 1, min, max, max + 1 points")[0], clump, sizes)


def test_numbering_follows_the_roots_across_blocks(store):
    pts, p, pair = T.case_numbering()
    _as_it_is(store, pts)
    T.check_numbering(equal_the_twin(store, p, "700 isolated pairs")[0], pair)


def test_one_dense_blob(store):
    pts, p = T.case_blob()
    _as_it_is(store, pts)
    T.check_blob(equal_the_twin(store, p, "one blob")[0], pts)


def test_signed_zeros_at_a_box_face(store):
    pts, p = T.case_signed_zeros()
    pose = np.where(np.eye(4) == 1.0, 1.0, -0.0)                     # the identity with every zero entry -0: (-0) x + ... + (-0) keeps a -0 where +0 would lose it
    _as_it_is(store, pts, pose)
    T.check_signed_zeros(equal_the_twin(store, p, "-0 and +0 at a box face")[0])


def test_non_finite_records_are_no_members_and_are_never_dropped(store):
    pts, p = T.case_non_finite()
    n = _map_of(store, [pts], [np.eye(4)], 1e-4)                     # passed through; the transform leaves a non-finite record non-finite, not its bytes
    fin = np.isfinite(pts).all(axis=1)
    assert n == len(pts) and _same(store.download_map(n)[fin, :3], pts[fin])
    got, m = equal_the_twin(store, p, "a map with non-finite records")
    T.check_non_finite(got, m)
    _, left = store.map_drop_rejected_clusters()
    kept = store.download_map(left)
    assert left == len(m) - got["stats"].rejected_points and _same(kept, mc.drop_rejected(m, p)) and (~np.isfinite(kept[:, :3]).all(axis=1)).sum() == 4


def test_ray_cast_street_scene_with_and_without_the_ground(store, scans):
    from qn_amd import engine
    n = store.build_map(scans, POSES, 0.3)
    assert 3000 <= n <= 40000, n
    got, pts = equal_the_twin(store, (0.5, 10, ALL, 0), "street scene, every finite point")
    assert got["stats"].largest > n // 2                             # the ground welds almost everything into one component
    # class_mask != 0 without a ground classification of this map: refused
    st = engine.ClusterStats()
    assert store._l.qn_kf_map_clusters(store.h, C.byref(engine.ClusterParams(0.5, 10, ALL, OBJECTS)), C.byref(st)) == engine.QN_ERR_NOT_READY
    _, cls, _ = store.map_ground(engine.GroundParams())
    assert _same(cls, mg.classify(pts)["classes"])
    obj, _ = equal_the_twin(store, (0.5, 10, ALL, OBJECTS), "street scene, what stands on the ground", cls)
    s = obj["stats"]
    member = ((OBJECTS >> cls.astype(np.int64)) & 1) == 1
    assert s.members == member.sum() and s.clusters > 1 and s.largest < s.members
    assert (obj["label"][cls == mg.GROUND] == mc.NONE).all() and (obj["label"][member] != mc.NONE).all()      # no ground point has a label >= 0
    # the cluster results ended nothing: the ground is still served
    assert store._l.qn_kf_map_ground_points(store.h, np.zeros(n, np.uint8).ctypes.data_as(C.c_void_p), None) == engine.QN_OK


def test_neighbours_across_cell_borders_on_every_axis(store):
    """tolerance 0.25 in a box of 3 x 3 x 2 m: cells of about the tolerance, more than ten a side on every axis, so most edges cross a cell border in x, in y and
    in z"""
    rng = np.random.default_rng(3)
    a = rng.uniform(0.0, 1.0, (4000, 3)) * (3.0, 3.0, 2.0)
    for c in range(3):
        idx = rng.choice(4000, 4000 // 6, replace=False)
        a[idx] = rng.uniform(0.2, 0.8, 3) * (3.0, 3.0, 2.0) + rng.normal(0.0, 0.15, (len(idx), 3))
    _as_it_is(store, a.astype(np.float32))
    got, _ = equal_the_twin(store, (0.25, 3, ALL, 0), "across cell borders")
    s = got["stats"]                                                 # 222 points a cubic metre, 14 expected partners within 0.25 m: far above percolation
    assert s.edges > 4000 and s.largest > 2000 and s.components > 1   # one component through hundreds of cells, and a few stragglers
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) * F(0.125)
    _as_it_is(store, g)
    got, _ = equal_the_twin(store, (0.25, 3, ALL, 0), "a cubic lattice of spacing 2^-3, tolerance 2^-2")
    # by hand: offsets (a, b, c) h with a^2 + b^2 + c^2 <= 4: per axis pair counts along 12, 12, 6 points
    cnt = lambda d: (12 - abs(d[0])) * (12 - abs(d[1])) * max(6 - abs(d[2]), 0)
    offs = [(a_, b_, c_) for a_ in range(-2, 3) for b_ in range(-2, 3) for c_ in range(-2, 3) if 0 < a_ * a_ + b_ * b_ + c_ * c_ <= 4]
    assert len(offs) == 32 and got["stats"].edges == sum(cnt(d) for d in offs) // 2 and got["stats"].components == 1


def test_drop_serves_the_filtered_map_and_ends_what_was_computed_from_the_old_one(store, scans):
    from qn_amd import engine
    n = store.build_map(scans, POSES, 0.3)
    views = np.array([[p[0, 3], p[1, 3], p[2, 3]] for p in POSES])
    store.map_normals(engine.NormalParams(0.6, 5), views)
    store.map_outliers(engine.OutlierParams())
    _, cls, _ = store.map_ground(engine.GroundParams())
    p = (0.5, 10, ALL, OBJECTS)
    got, pts = equal_the_twin(store, p, "before the drop", cls)
    s = got["stats"]
    assert 0 < s.rejected_points < n
    nrm = np.zeros((n, 4), np.float32)
    assert store._l.qn_kf_download_map_normals(store.h, nrm.ctypes.data_as(C.c_void_p), None, None) == engine.QN_OK       # the classify did not touch the slot
    ptr, m = store.map_drop_rejected_clusters()
    want = mc.drop_rejected(pts, p, cls)
    assert m == n - s.rejected_points == len(want) and ptr
    assert _same(store.download_map(m), want)                        # byte for byte, all 16 bytes of each kept record, in order
    # the slot's generation moved: what was computed from the old map is refused
    L = store._l
    w = np.zeros(n, np.uint32); cnt = C.c_uint32(77)
    assert L.qn_kf_download_map_normals(store.h, nrm.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_outlier_points(store.h, w.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_ground_points(store.h, np.zeros(n, np.uint8).ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_cluster_points(store.h, None, w.ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_cluster_list(store.h, None, C.c_uint32(0), C.byref(cnt)) == engine.QN_ERR_NOT_READY and cnt.value == 77
    p2 = C.c_void_p(); m2 = C.c_uint32()
    assert L.qn_kf_map_drop_rejected_clusters(store.h, C.byref(p2), C.byref(m2)) == engine.QN_ERR_NOT_READY
    assert _same(store.download_map(m), want)                        # the refused drop left the slot as it was
    # a new classify sees the filtered map
    again, _ = equal_the_twin(store, (0.5, 10, ALL, 0), "after the drop")
    assert again["stats"].n == m


def test_lifecycle_and_refusals(store, scans):
    from qn_amd import engine
    n = store.build_map(scans[:2], POSES[:2], 0.3)
    p = (0.5, 5, 400, 0)
    keep, _ = equal_the_twin(store, p, "two keyframes")
    count = keep["stats"].clusters
    assert count >= 2
    L = store._l
    st = engine.ClusterStats(); st.n = 12345
    bad = [engine.ClusterParams(*v) for v in [(0.0, 5, 400, 0), (-1.0, 5, 400, 0), (float("nan"), 5, 400, 0), (float("inf"), 5, 400, 0), (0.5, 0, 400, 0),
                                               (0.5, 5, 4, 0), (0.5, 5, 400, 32), (0.5, 5, 400, 0x80000000)]]
    q = engine.ClusterParams(); q.reserved = 1
    bad.append(q)
    for q in bad:
        assert L.qn_kf_map_clusters(store.h, C.byref(q), C.byref(st)) == engine.QN_ERR_INVALID_ARG, (q.tolerance, q.min_size, q.max_size, q.class_mask, q.reserved)
    assert L.qn_kf_map_clusters(store.h, None, C.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_clusters(store.h, C.byref(engine.ClusterParams()), None) == engine.QN_ERR_INVALID_ARG
    # class_mask != 0 without a live ground result
    assert L.qn_kf_map_clusters(store.h, C.byref(engine.ClusterParams(0.5, 5, 400, OBJECTS)), C.byref(st)) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_cluster_points(store.h, None, None, None) == engine.QN_ERR_INVALID_ARG
    cnt = C.c_uint32(77)
    info = np.zeros(count + 1, mc.INFO_DTYPE); info["root"] = 99
    assert L.qn_kf_map_cluster_list(store.h, info.ctypes.data_as(C.c_void_p), C.c_uint32(count), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_cluster_list(store.h, info.ctypes.data_as(C.c_void_p), C.c_uint32(count - 1), C.byref(cnt)) == engine.QN_ERR_CAPACITY
    assert cnt.value == 77 and (info["root"] == 99).all()            # nothing written
    ptr = C.c_void_p(); m = C.c_uint32()
    assert L.qn_kf_map_drop_rejected_clusters(store.h, None, C.byref(m)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_drop_rejected_clusters(store.h, C.byref(ptr), None) == engine.QN_ERR_INVALID_ARG
    assert st.n == 12345                                             # nothing was written
    # every refusal left the previous results readable and unchanged; each output alone is served
    label = np.zeros(n, np.int32); root = np.zeros(n, np.uint32); size = np.zeros(n, np.uint32)
    assert L.qn_kf_map_cluster_points(store.h, label.ctypes.data_as(C.c_void_p), None, None) == engine.QN_OK
    assert L.qn_kf_map_cluster_points(store.h, None, root.ctypes.data_as(C.c_void_p), None) == engine.QN_OK
    assert L.qn_kf_map_cluster_points(store.h, None, None, size.ctypes.data_as(C.c_void_p)) == engine.QN_OK
    assert _same(label, keep["label"]) and _same(root, keep["root"]) and _same(size, keep["size"])
    assert L.qn_kf_map_cluster_list(store.h, None, C.c_uint32(0), C.byref(cnt)) == engine.QN_OK and cnt.value == count      # the count only
    assert L.qn_kf_map_cluster_list(store.h, info.ctypes.data_as(C.c_void_p), C.c_uint32(count + 1), C.byref(cnt)) == engine.QN_OK and cnt.value == count
    assert _same(info[:count], keep["clusters"]) and info["root"][count] == 99
    # a rebuild replaces the slot: the results are refused until the next classify, and so is the drop
    n2 = store.build_map(scans[:3], POSES[:3], 0.3)
    assert L.qn_kf_map_cluster_points(store.h, label.ctypes.data_as(C.c_void_p), None, None) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_cluster_list(store.h, None, C.c_uint32(0), C.byref(cnt)) == engine.QN_ERR_NOT_READY
    assert L.qn_kf_map_drop_rejected_clusters(store.h, C.byref(ptr), C.byref(m)) == engine.QN_ERR_NOT_READY
    assert store._map_n == n2 and len(store.download_map(n2)) == n2
    equal_the_twin(store, p, "the map built afterwards")
    # a member beyond the quantisation's range: refused, and the results of the map just classified stay
    far = np.array([[2.0 ** 20, 0, 0], [0, 0, 0], [0, 1, 1]], np.float32)
    _as_it_is(store, far)
    assert L.qn_kf_map_clusters(store.h, C.byref(engine.ClusterParams(0.5, 1, 2, 0)), C.byref(st)) == engine.QN_ERR_CAPACITY and st.n == 12345
    with pytest.raises(mc.CapacityError):
        mc.classify(far, (0.5, 1, 2, 0))


def test_not_ready_without_a_map():
    from qn_amd import engine
    s = engine.KeyframeStore()
    try:
        st = engine.ClusterStats(); ptr = C.c_void_p(); m = C.c_uint32(); out = np.zeros(4, np.uint32)
        assert s._l.qn_kf_map_clusters(s.h, C.byref(engine.ClusterParams()), C.byref(st)) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_cluster_points(s.h, None, out.ctypes.data_as(C.c_void_p), None) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_cluster_list(s.h, None, C.c_uint32(0), C.byref(m)) == engine.QN_ERR_NOT_READY
        assert s._l.qn_kf_map_drop_rejected_clusters(s.h, C.byref(ptr), C.byref(m)) == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_clusters()
        assert ei.value.status == engine.QN_ERR_NOT_READY
        with pytest.raises(engine.EngineError) as ei:
            s.map_drop_rejected_clusters()
        assert ei.value.status == engine.QN_ERR_NOT_READY
    finally:
        s.close()


def _fnv(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return h


def test_cpp_helper_gives_the_python_result(store, scans, tmp_path):
    from shim_build import build_shim
    from qn_amd import engine
    exe = build_shim("shim_map_clusters.cpp", tmp_path)
    ids, poses = scans[:2], POSES[:2]
    with open(tmp_path / "kf.bin", "wb") as f:
        for i in ids:
            c = store.keyframe(i)
            f.write(np.uint32(len(c)).tobytes()); f.write(np.ascontiguousarray(c, np.float32).tobytes())
    np.ascontiguousarray(np.array(poses, np.float64)).tofile(str(tmp_path / "poses.bin"))
    txt = subprocess.check_output([exe, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "0.3", "0.5", "5", "400"], text=True)
    n = store.build_map(ids, poses, 0.3)
    stats, label, root, size, cl = store.map_clusters(engine.ClusterParams(0.5, 5, 400, 0))
    hp = _fnv(label[i].tobytes() + root[i].tobytes() + size[i].tobytes() for i in range(n))
    hc = _fnv(cl["root"][j].tobytes() + cl["size"][j].tobytes() + cl["lo"][j].tobytes() + cl["hi"][j].tobytes() + cl["centroid"][j].tobytes()
              for j in range(stats["clusters"]))
    _, m = store.map_drop_rejected_clusters()
    kept = store.download_map(m)
    hm = _fnv(kept[i].tobytes() for i in range(m))
    assert txt.splitlines() == ["clusters %d %d %d %d %016x %016x" % (n, stats["components"], stats["clusters"], stats["edges"], hp, hc),
                                "filtered %d %016x" % (m, hm)], txt
