"""Many loop-closure submaps in one pass (qn_kf_assemble_batch, loop_closure.cpp:58-108 for one query and its candidates): every submap
equals qn_kf_assemble of the same list in all 16 bytes of every record and the oracle's assemble_submap, the batch slot
is isolated from slots 0/1 and the map slot, and the batch outputs registered through gicp_align_batch / coarse_to_fine_align_batch give
the records of the one-pair device entry points on the same clouds assembled through slots 0/1."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from qn_amd import synth

from test_kf_batch_api import build_loop_program, LOOP_BIN
from test_gpu_c2f_batch import make_ctx, same_record

pytestmark = pytest.mark.gpu


def _records(ptr, n):
    """the n float4 records at a device pointer, all 16 bytes (hipMemcpy of the runtime the engine library is linked against)"""
    from qn_amd import engine
    out = np.zeros((n, 4), np.float32)
    if n:
        l = engine.lib(); l.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; l.hipMemcpy.restype = C.c_int
        assert l.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), 16 * n, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _loop_records(store, ids, poses, leaf, slot=0):
    """qn_kf_assemble of one list -> (records, status)"""
    from qn_amd import engine
    try:
        ptr, n = store.assemble(ids, poses, leaf, slot)
    except engine.EngineError as e:
        return None, e.status
    return _records(ptr, n), 0


def _check_batch(store, lists, pose_lists, leaf):
    """assemble_batch, then every submap against qn_kf_assemble of its list -> the batch output"""
    out = store.assemble_batch(lists, pose_lists, leaf)
    note = store._l.qn_kf_last_error(store.h).decode()
    got = [_records(p, n) if st == 0 else None for p, n, st in out]
    for s, (l, P) in enumerate(zip(lists, pose_lists)):
        want, st = _loop_records(store, l, P, leaf)
        assert out[s][2] == st, (s, out[s][2], st)
        if st == 0:
            assert got[s].shape == want.shape and np.array_equal(got[s].view(np.uint32), want.view(np.uint32)), "submap %d differs from qn_kf_assemble" % s
            assert np.array_equal(store.download_batch(s, out[s][1]).view(np.uint32), got[s][:, :3].view(np.uint32))
        else:
            assert out[s][1] == 0
    return out, got, note


def _world_keyframes(nkf, npts, seed, world_pts=60000, extent=60.0, step=(1.2, 0.4, 0.01)):
    """keyframes sampled from one synthetic world along a path: sensor-frame clouds and their poses"""
    rng = np.random.default_rng(seed)
    world = synth.make_pair(seed, world_pts, extent=extent, leaf=0.1)[0]
    kfs, poses = [], []
    for k in range(nkf):
        P = np.eye(4); P[:3, :3] = synth._rot_zyx(0.04 * k, 0.01 * rng.normal(), 0.01 * rng.normal()); P[:3, 3] = [step[0] * k - 15, step[1] * k - 5, step[2] * k]
        sel = rng.choice(len(world), npts, replace=False)
        w = world[sel].astype(np.float64) + rng.normal(0, 0.01, (npts, 3))
        kfs.append(((w - P[:3, 3]) @ P[:3, :3]).astype(np.float32))
        poses.append(P)
    return kfs, poses


@pytest.fixture
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def test_query_and_sixteen_candidates_with_overlaps_and_repeats(store, oracle):
    kfs, poses = _world_keyframes(30, 5000, 1)
    for k in kfs:
        store.add(k)
    from qn_amd import engine
    lists = [engine.loop_submap_ids(29, 29, 10, True, True, 30)[0]]
    lists += [engine.loop_submap_ids(29, c, 4, False, False, 30)[1] for c in (0, 2, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 28, 3)]
    lists[3] = lists[3] + [5, 5, 1]                                    # repeats inside one submap
    lists[8] = [4]                                                     # a single-keyframe submap
    out, got, _ = _check_batch(store, lists, [[poses[i] for i in l] for l in lists], 0.3)
    assert all(st == 0 for _, _, st in out) and len(out) == 17
    for s in range(len(lists)):                                        # the oracle's setSrcAndDstCloud, every submap
        ref = oracle.assemble_submap(kfs, poses, lists[s], 0.3)
        assert np.array_equal(got[s][:, :3].view(np.uint32), ref.view(np.uint32)) and (got[s][:, 3] == 1.0).all()


def test_non_finite_tripped_and_empty_submaps_beside_normal_ones(store, oracle):
    rng = np.random.default_rng(2)
    kfs, poses = _world_keyframes(6, 4000, 2)
    dirty = kfs[1].copy(); dirty[::7, 0] = np.nan; dirty[3::11, 2] = np.inf; dirty[5::13, 1] = -np.inf
    huge = rng.uniform(-2e4, 2e4, (3000, 3)).astype(np.float32); huge[::9] = np.nan     # trips PCL's guard at leaf 0.3, with non-finite points
    allbad = np.full((500, 3), np.nan, np.float32); allbad[::2, 1] = np.inf
    ids = [store.add(k) for k in kfs] + [store.add(dirty), store.add(huge), store.add(allbad), store.add(np.zeros((0, 3), np.float32))]
    P = poses + [poses[1], np.eye(4), np.eye(4), np.eye(4)]
    lists = [[0, 1, 2], [6], [7], [2, 3, 6], [8], [4, 5], [8, 9], [9], [], [0]]
    out, got, note = _check_batch(store, lists, [[P[i] for i in l] for l in lists], 0.3)
    assert "too small" in note, note                                   # the tripped submap's warning
    st = [o[2] for o in out]
    from qn_amd import engine
    assert st == [0, 0, 0, 0, engine.QN_ERR_EMPTY_CLOUD, 0, engine.QN_ERR_EMPTY_CLOUD, engine.QN_ERR_EMPTY_CLOUD, engine.QN_ERR_EMPTY_CLOUD, 0], st
    fin = huge[np.isfinite(huge).all(1)]
    assert out[2][1] == len(fin) and np.array_equal(got[2][:, :3].view(np.uint32), fin.view(np.uint32))       # unfiltered, concatenation order
    assert out[1][1] < len(dirty) and out[0][1] < 12000                 # the others are filtered
    ref = oracle.voxel_grid(oracle.transform_pcd(dirty, P[6])[np.isfinite(dirty).all(1)], 0.3)
    assert np.array_equal(got[1][:, :3].view(np.uint32), ref.view(np.uint32))


def test_group_split_of_submaps_with_large_extent(store):
    """leaf 0.1 over 300 m x 300 m x 10 m: ~9e8 cells (30 leaf bits), so at most 4 submaps share the 32 key bits: 9 submaps sort in groups"""
    rng = np.random.default_rng(3)
    wide = [np.c_[rng.uniform(-150, 150, (6000, 2)), rng.uniform(-5, 5, 6000)].astype(np.float32) for _ in range(5)]
    kfs, poses = _world_keyframes(3, 3000, 3)
    ids = [store.add(w) for w in wide] + [store.add(k) for k in kfs]
    P = [np.eye(4)] * 5 + poses
    lists = [[0], [1, 5], [2], [6, 7], [3], [4], [0, 1], [2, 3, 0], [5]]
    out, got, _ = _check_batch(store, lists, [[P[i] for i in l] for l in lists], 0.1)
    assert all(o[2] == 0 for o in out)
    inv = np.float32(1) / np.float32(0.1)
    mn, mx = wide[0].min(0), wide[0].max(0)
    cells = int(np.prod(np.floor(mx * inv).astype(np.int64) - np.floor(mn * inv).astype(np.int64) + 1))
    assert 2 ** 29 < cells < 2 ** 31 - 1, cells


def test_slots_and_map_are_isolated(store):
    kfs, poses = _world_keyframes(10, 4000, 4)
    for k in kfs:
        store.add(k)
    p0, n0 = store.assemble([0, 1], poses[:2], 0.3, 0)
    p1, n1 = store.assemble([2, 3, 4], poses[2:5], 0.3, 1)
    a0, a1 = _records(p0, n0), _records(p1, n1)
    nm = store.build_map(list(range(10)), poses, 0.3)
    m = store.download_map(nm)
    lists = [[5, 6], [7], [8, 9, 0]]
    out = store.assemble_batch(lists, [[poses[i] for i in l] for l in lists], 0.3)
    b = [_records(p, n) for p, n, _ in out]
    assert np.array_equal(_records(p0, n0).view(np.uint32), a0.view(np.uint32)) and np.array_equal(_records(p1, n1).view(np.uint32), a1.view(np.uint32))
    assert np.array_equal(store.download_map(nm).view(np.uint32), m.view(np.uint32))
    store.assemble(list(range(10)), poses, 0.2, 0)                     # larger than before: slot 0 and the shared scratch grow
    store.assemble([9], poses[9:], 0.4, 1)
    store.build_map([1, 2], poses[1:3], 0.5)
    for (p, n, _), r in zip(out, b):
        assert np.array_equal(_records(p, n).view(np.uint32), r.view(np.uint32))
    assert np.array_equal(store.download_batch(1, out[1][1]).view(np.uint32), b[1][:, :3].view(np.uint32))


def test_argument_errors_return_invalid_before_running(store):
    from qn_amd import engine
    store.add(np.zeros((10, 3), np.float32))
    l = store._l
    ids = np.array([0, 0], np.int32); T = np.tile(np.eye(4).reshape(1, 16), (2, 1)); seg = np.array([0, 2, 1], np.uint32)
    ptrs = (C.c_void_p * 2)(); n = np.zeros(2, np.uint32); st = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda ids, seg, S, leaf: l.qn_kf_assemble_batch(store.h, p(ids), p(T), p(seg), C.c_uint32(S), C.c_double(leaf), ptrs, p(n), p(st))
    assert call(ids, seg, 2, 0.3) == engine.QN_ERR_INVALID_ARG                           # non-monotone seg_off
    assert call(ids, np.array([0, 1, 2], np.uint32), 2, 0.0) == engine.QN_ERR_INVALID_ARG
    assert call(ids, np.array([0, 1, 2], np.uint32), 0, 0.3) == engine.QN_ERR_INVALID_ARG
    assert call(np.array([0, 7], np.int32), np.array([0, 1, 2], np.uint32), 2, 0.3) == engine.QN_ERR_INVALID_ARG
    assert call(ids, np.array([0, 1, 2], np.uint32), 2, 0.3) == engine.QN_OK


def _gicp_ctx(engine, cap, lanes):
    ctx = engine.Context(cap, device=0); ctx.debug_set("batch_lanes", lanes)
    g = engine.NanoGICP(ctx); g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(52.5); g.setTransformationEpsilon(0.01); g.bind()
    return ctx, g


def test_fine_registration_of_batch_outputs_equals_the_device_path(store):
    """1 query + 8 candidates (icpAlignment: query scan vs candidate submap) through gicp_align_batch with 8 lanes, against qn_icp_alignment_device"""
    from qn_amd import engine
    kfs, poses = _world_keyframes(30, 6000, 5)
    for k in kfs:
        store.add(k)
    corrected = list(poses)
    drift = np.eye(4); drift[:3, :3] = synth._rot_zyx(0.03, 0, 0); drift[:3, 3] = [0.4, -0.3, 0.05]
    corrected[29] = drift @ poses[29]
    cands = [3, 6, 9, 12, 15, 18, 21, 26]
    pairs, st = store.loop_submap_pairs(corrected, 29, cands, 2, 0.3, enable_quatro=False, enable_submap_matching=False)
    assert all(s == 0 for s in st) and len({p[0] for p in pairs}) == 1
    cap = max(max(p[1], p[3]) for p in pairs) + 1024
    ctx, g = _gicp_ctx(engine, cap, 8)
    res, val, bst = engine.gicp_align_batch(ctx, pairs, score_thr=1.5)
    one, g1 = _gicp_ctx(engine, cap, 1)
    for c, r, v, s in zip(cands, res, val, bst):
        src, dst = engine.loop_submap_ids(29, c, 2, False, False, 30)
        ps, ns = store.assemble(src, [corrected[i] for i in src], 0.3, 0)
        pd, nd = store.assemble(dst, [corrected[i] for i in dst], 0.3, 1)
        r1 = engine.GicpResult(); v1 = C.c_int()
        one.check(one._l.qn_icp_alignment_device(one.h, C.c_void_p(ps), C.c_uint32(ns), C.c_void_p(pd), C.c_uint32(nd), C.c_uint32(16), C.c_double(1.5), C.byref(r1), C.byref(v1)))
        assert s == 0 and bool(v) == bool(v1.value) and r.converged == r1.converged and r.iterations == r1.iterations, (c, v, v1.value, r.iterations, r1.iterations)
        assert np.array_equal(np.array(r.T, np.float32).view(np.uint32), np.array(r1.T, np.float32).view(np.uint32)) and r.fitness == r1.fitness, c
    assert sum(val) >= 1
    ctx.close(); one.close()


def test_coarse_to_fine_of_batch_outputs_equals_the_device_path(store):
    """4 pairs of ~30k-point submaps (submap matching, range 1) through coarse_to_fine_align_batch, against qn_coarse_to_fine_alignment_device"""
    from qn_amd import engine
    kfs, poses = _world_keyframes(24, 20000, 6, world_pts=150000, extent=70.0)
    for k in kfs:
        store.add(k)
    cands = [4, 9, 14, 19]
    pairs, st = store.loop_submap_pairs(poses, 22, cands, 1, 0.3, enable_quatro=True, enable_submap_matching=True)
    assert all(s == 0 for s in st)
    assert 15000 < pairs[0][1] < 60000, pairs[0][1]
    cap = max(max(p[1], p[3]) for p in pairs) + 1024
    ctx = make_ctx(engine, cap, 4)
    got = engine.coarse_to_fine_align_batch([ctx], pairs)
    one = engine.Context(cap)
    for c, gr in zip(cands, got):
        src, dst = engine.loop_submap_ids(22, c, 1, True, True, 24)
        ps, ns = store.assemble(src, [poses[i] for i in src], 0.3, 0)
        pd, nd = store.assemble(dst, [poses[i] for i in dst], 0.3, 1)
        r = engine.coarse_to_fine_alignment_device(one, ps, ns, pd, nd, 16)
        assert gr["status"] == 0 and same_record(gr, r), (c, {k: gr[k] for k in ("valid", "score", "iterations")}, {k: r[k] for k in ("valid", "score", "iterations")})
    ctx.close(); one.close()


def test_cpp_helper_gives_the_python_submaps(store, tmp_path):
    if not os.path.exists(LOOP_BIN):
        build_loop_program()
    kfs, poses = _world_keyframes(16, 3000, 7)
    with open(tmp_path / "kf.bin", "wb") as f:
        for x in kfs:
            f.write(np.uint32(len(x)).tobytes()); f.write(np.ascontiguousarray(x, np.float32).tobytes())
    np.ascontiguousarray(poses, np.float64).tofile(tmp_path / "poses.bin")
    cands = [2, 5, 9, 14]
    out = subprocess.check_output([LOOP_BIN, str(tmp_path / "kf.bin"), str(tmp_path / "poses.bin"), "15", "3", "0.3", "0", "1", str(tmp_path / "sub.bin")] + [str(c) for c in cands],
                                  timeout=120).decode().split()
    assert out == ["4", "1"], out
    raw = np.fromfile(tmp_path / "sub.bin", np.uint8); subs, o = [], 0
    while o < len(raw):
        m = int(raw[o:o + 4].view(np.uint32)[0]); subs.append(raw[o + 4:o + 4 + 12 * m].view(np.float32).reshape(m, 3)); o += 4 + 12 * m
    for k in kfs:
        store.add(k)
    pairs, st = store.loop_submap_pairs(poses, 15, cands, 3, 0.3, enable_quatro=False, enable_submap_matching=True)
    assert len(subs) == 5 and all(s == 0 for s in st)
    want = [_records(pairs[0][0], pairs[0][1])] + [_records(p[2], p[3]) for p in pairs]
    for a, b in zip(subs, want):
        assert np.array_equal(a.view(np.uint32), b[:, :3].view(np.uint32))


def test_scale_ten_million_input_points(store):
    """1 query + 32 candidate submaps x 21 keyframes x 15k points (1.04e7 input points) in one call: each equals qn_kf_assemble"""
    kfs, poses = _world_keyframes(48, 15000, 8, world_pts=200000, extent=80.0)
    for k in kfs:
        store.add(k)
    lists = [list(range(26, 47))] + [[(c + j) % 47 for j in range(21)] for c in range(0, 32)]
    assert sum(len(l) for l in lists) * 15000 >= 10 ** 7
    out, got, _ = _check_batch(store, lists, [[poses[i] for i in l] for l in lists], 0.3)
    assert all(o[2] == 0 for o in out)
