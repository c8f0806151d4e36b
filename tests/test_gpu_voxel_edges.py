"""The voxel-grid pipeline (voxel_submaps, csrc/qn_cloud.hip) against its references on every case of tests/voxel_cases.py, through its three entry
points: qn_kf_assemble (slot 0), qn_kf_assemble_batch (the case's lists, and the same lists reversed so that prefixes and sort groups move) and
qn_kf_build_map (single-list cases; intensity on some keyframes).  All 16 bytes of every record: xyz against the C++ oracle, w = 1 for assemble
and the batch, w = the mean intensity against the numpy restatement for the map; the status and the note in last_error against the references'
flags; one rerun of the batch bitwise identical.  No tolerance anywhere.  tests/test_voxel_reference_cpu.py shows on the CPU that the two
references agree on these very inputs.  Two consumers on a few cases: qn_kf_quatro_describe's cloud is assemble([id], identity), and
qn_kf_overlap_batch (whose cell index reuses the guard, the sort groups and the radix passes) gives what the numpy twin qn_amd/overlap.py gives -
every integer and every per-point result; sum_d2, an f64 sum in no fixed order, is compared between two runs only."""
import ctypes as C
import numpy as np
import pytest

import voxel_cases as vc
from test_voxel_reference_cpu import references, same_bits

pytestmark = pytest.mark.gpu
EYE = np.eye(4)
WARNING = "warning: leaf size is too small"
NOTE = "note: non-finite points dropped"


def _records(ptr, n):
    """the n float4 records at a device pointer, all 16 bytes"""
    from qn_amd import engine
    out = np.zeros((n, 4), np.float32)
    if n:
        l = engine.lib(); l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; l.hipMemcpy.restype = C.c_int
        assert l.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), 16 * n, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _note(store):
    return store._l.qn_kf_last_error(store.h).decode()


def _same_records(got, want):
    """all 16 bytes; a NaN (a passed-through non-finite point: its payload is not part of any specification) matches a NaN"""
    if got.shape != want.shape:
        return False
    g, w = got.view(np.uint32), want.view(np.uint32)
    return bool(((g == w) | (np.isnan(got) & np.isnan(want))).all())


def _expected_note(refs):
    live = [r for r in refs if len(r["fin"])]
    if any(r["tripped"] for r in live):
        return WARNING
    return NOTE if any(len(r["cat"]) > len(r["fin"]) for r in live) else ""


def _new_store(case):
    from qn_amd import engine
    store = engine.KeyframeStore()
    ids = [store.add(k, i) for k, i in zip(case.kfs, case.inten)]
    assert ids == list(range(len(case.kfs)))
    return store


def _check_submap(name, what, s, rec, status, ref):
    """one submap of assemble / the batch: status, the oracle's xyz, w = 1"""
    from qn_amd import engine
    if not len(ref["fin"]):
        assert status == engine.QN_ERR_EMPTY_CLOUD and (rec is None or len(rec) == 0), (name, what, s, status)
        return
    assert status == 0, (name, what, s, status)
    assert len(rec) == len(ref["xyz"]), (name, what, s, len(rec), len(ref["xyz"]))
    assert same_bits(rec[:, :3], ref["xyz"]), (name, what, s, int((rec[:, :3].view(np.uint32) != ref["xyz"].view(np.uint32)).any(1).sum()))
    assert same_bits(rec[:, 3], np.ones(len(rec), np.float32)), (name, what, s)


def _batch(store, case, lists):
    out = store.assemble_batch(lists, case.pose_lists(lists), case.leaf)
    return out, [_records(p, n) if st == 0 else None for p, n, st in out], _note(store)


@pytest.mark.parametrize("name", vc.NAMES)
def test_every_entry_point_equals_the_references(oracle, name):
    from qn_amd import engine
    case = vc.get(name)
    vc.check(case)
    refs = [references(oracle, case, l) for l in case.lists]
    store = _new_store(case)
    try:
        # qn_kf_assemble, slot 0 (it does not clear last_error: the note is checked where this call must have written it)
        for s, (l, ref) in enumerate(zip(case.lists, refs)):
            before = _note(store)
            try:
                ptr, n = store.assemble(l, case.pose_lists([l])[0], case.leaf, 0)
                rec, status = _records(ptr, n), 0
            except engine.EngineError as e:
                rec, status = None, e.status
            _check_submap(name, "assemble", s, rec, status, ref)
            want = _expected_note([ref])
            assert _note(store).startswith(want) if want else _note(store) == before, (name, "assemble", s, _note(store))
            if status == 0:
                assert same_bits(store.download(0, len(rec)), rec[:, :3]), (name, "download", s)
        # qn_kf_assemble_batch, the lists as given and reversed; one rerun
        first = None
        for what, lists, rr in (("batch", case.lists, refs), ("reversed", case.lists[::-1], refs[::-1]), ("rerun", case.lists, refs)):
            out, got, note = _batch(store, case, lists)
            for s, ref in enumerate(rr):
                _check_submap(name, what, s, got[s], out[s][2], ref)
            want = _expected_note(rr)
            assert note.startswith(want) if want else note == "", (name, what, note)
            if what == "batch":
                first = (out, got)
            elif what == "rerun":
                assert [o[1:] for o in out] == [o[1:] for o in first[0]], (name, what)
                assert all((a is None and b is None) or same_bits(a, b) for a, b in zip(got, first[1])), (name, what)
        # qn_kf_build_map: the restatement's records, intensity included; a tripped map is the whole concatenation
        if len(case.lists) == 1:
            ref = refs[0]
            for what in ("map", "map rerun"):
                if not len(ref["fin"]):
                    with pytest.raises(engine.EngineError) as ei:
                        store.build_map(case.lists[0], case.pose_lists()[0], case.leaf)
                    assert ei.value.status == engine.QN_ERR_EMPTY_CLOUD, (name, what)
                    continue
                n = store.build_map(case.lists[0], case.pose_lists()[0], case.leaf)
                m = store.download_map(n)
                assert n == len(ref["xyzi"]), (name, what, n, len(ref["xyzi"]))
                assert _same_records(m, ref["xyzi"]), (name, what)
                assert same_bits(m[np.isfinite(m[:, :3]).all(1)][:, :3], ref["xyz"] if not ref["tripped"] else ref["fin"][:, :3]), (name, what)   # xyz: the oracle
                assert _note(store).startswith(WARNING) if ref["tripped"] else _note(store) == "", (name, what, _note(store))
    finally:
        store.close()


# ---- consumers of the pipeline: a tile edge, a far cloud, a tripped one
def _consumer_clouds():
    sizes = vc.get("sizes-batch")
    far = vc.get("far-8km-0.3"); utm = vc.get("far-utm-0.1")
    trip = vc.get("guard-pd-ok-cells-over-nan"); wide = vc.get("guard-floor-out-of-int"); out19 = vc.get("guard-outlier-1e19-nan")
    return dict(tile_4097=(sizes.kfs[7], 0.3), tile_4096=(sizes.kfs[6], 0.3), far_8km=(far.concat(far.lists[0])[:, :3].copy(), 0.3),
                far_utm=(utm.concat(utm.lists[0])[:, :3].copy(), 0.1), tripped_box=(trip.kfs[0], 1.0), tripped_1e9=(wide.kfs[0], 0.3),
                tripped_1e19=(out19.kfs[0], 0.3))


@pytest.mark.parametrize("which", ["tile_4097", "tile_4096", "far_8km", "tripped_box"])
def test_quatro_describe_cloud_is_assemble_with_the_identity(oracle, which):
    from qn_amd import engine
    xyz, leaf = _consumer_clouds()[which]
    fin = xyz[np.isfinite(xyz).all(1)]
    store = engine.KeyframeStore(); ctx = engine.Context(16384); engine.Quatro(ctx)
    try:
        k = store.add(xyz)
        assert store.quatro_describe(ctx, [k], leaf) == [0]
        p, n = store.quatro_cloud(k)
        got = _records(p, n)
        ap, an = store.assemble([k], [EYE], leaf, 0)
        assert n == an and same_bits(got, _records(ap, an)), which
        assert same_bits(got[:, :3], oracle.voxel_grid(fin, leaf)) and oracle.voxel_guard(fin, leaf) == (which == "tripped_box"), which
    finally:
        ctx.close(); store.close()


@pytest.mark.parametrize("pair,radius", [(("tile_4097", "tile_4096"), 0.6), (("far_utm", "far_utm"), 1.0), (("far_8km", "far_8km"), 0.6),
                                         (("tripped_1e9", "tripped_1e9"), 100.0), (("tripped_1e19", "tile_4096"), 0.6)])
def test_overlap_batch_equals_the_twin(pair, radius):
    import torch
    from qn_amd import engine, overlap as ov
    clouds = _consumer_clouds()
    a, b = clouds[pair[0]][0], clouds[pair[1]][0]
    if pair[0] == pair[1]:
        b = np.ascontiguousarray(b[::-1][: len(b) - 7])                               # the same cloud in another order, a few points short
    dev = []
    for x in (a, b):
        r = np.ones((len(x), 4), np.float32); r[:, :3] = x
        dev.append(torch.from_numpy(r).cuda())
    store = engine.KeyframeStore()
    try:
        arg = [(dev[0].data_ptr(), len(a), dev[1].data_ptr(), len(b))]
        rec = store.overlap_batch(arg, radius)[0]
        pts = [store.overlap_points(0, d) for d in (0, 1)]
        again = store.overlap_batch(arg, radius)[0]
        assert rec["status"] == 0 and again == rec, (pair, rec, again)
        for d, key, x, y in ((0, "a_to_b", a, b), (1, "b_to_a", b, a)):
            want = ov.direction(x, y, radius, points=True)
            got = rec[key]
            assert (got["n"], got["n_finite"], got["inliers"]) == (want["n"], want["n_finite"], want["inliers"]), (pair, key, got, want["inliers"])
            assert np.array_equal(pts[d][1], want["nn_idx"]), (pair, key)
            assert same_bits(pts[d][0], want["nn_d2"]), (pair, key)
            assert want["inliers"] > 0, (pair, key)
    finally:
        store.close()
