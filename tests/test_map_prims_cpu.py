"""What the direct tests of the map units' shared device primitives need without a GPU: the entry point is declared, exported, wrapped and refuses a null
store for every routine, and the case table of tests/map_prims_cases.py is what it says it is - the counts of distinct keys, which sums wrap, the
component counts of the graph families - with its references checked on inputs whose answers are known in closed form.  The device: tests/test_gpu_map_prims.py."""
import ctypes as C
import os
import re
import numpy as np
import map_prims_cases as mc


def test_device_entry_is_declared_wrapped_and_refuses_a_null_store():
    from qn_amd import engine
    import test_capi_symbols
    assert "qn_kf_debug_map_prims" in test_capi_symbols.declared_symbols() and callable(engine.KeyframeStore.debug_map_prims)
    L = engine.lib()
    L.qn_kf_debug_map_prims.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    a = np.zeros(4096, np.uint32); out = np.full(4096, 7, np.uint32)
    for which in range(9):
        for n in (0, 1):
            assert L.qn_kf_debug_map_prims(None, which, a.ctypes.data_as(C.c_void_p), n, 1, out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert (out == 7).all()
    K = engine.KeyframeStore
    for mine, theirs in ((mc.LANE, K.MAP_PRIMS_LANE), (mc.WAVE_OUT, K.MAP_PRIMS_WAVE), (mc.KEY_IN, K.MAP_PRIMS_KEY_IN), (mc.KEY_OUT, K.MAP_PRIMS_KEY),
                         (mc.BLOCK_IN, K.MAP_PRIMS_BLOCK_IN), (mc.BLOCK_OUT, K.MAP_PRIMS_BLOCK), (mc.VOXEL, K.MAP_PRIMS_VOXEL)):
        assert mine == theirs
    assert [d.itemsize for d in (mc.LANE, mc.WAVE_OUT, mc.KEY_IN, mc.KEY_OUT, mc.BLOCK_IN, mc.BLOCK_OUT, mc.VOXEL)] == [32, 64, 8, 24, 40, 232, 32]      # include/qn_engine.h
    assert K.MAP_PRIMS_GRID == 8 and re.search(r"#define\s+QN_DEBUG_MAP_PRIMS_WHICH\s+9\b", open(os.path.join(test_capi_symbols.ROOT, "include", "qn_engine.h")).read())


def test_the_wave_cases_are_what_they_say():
    names, waves = mc.wave_cases()
    ref = dict(zip(names, mc.wave_reference(waves)))
    assert len(names) % 4 == 0 and len(set(names)) == len(names)
    for lane in (0, 31, 32, 63):
        lo, hi = ref["low@%d" % lane], ref["high@%d" % lane]
        assert (lo["imin"], lo["umin"], lo["fmin"], lo["qmin"], lo["ssum"]) == (-3, 5, -1.5, (1 << 40) + 3, -(1 << 40) - 1)
        assert (hi["imax"], hi["umax"], hi["fmax"], hi["usum"], hi["qsum"], hi["ssum"]) == (3, 0x80000001, 2.5, 0x80000001, (1 << 63) + 9, 1 << 41)
    # which sums wrap: the true sum is not the modular one
    true = lambda name, f: sum(int(v) for v in waves[names.index(name)][f])
    assert true("sums wrap", "u") >= 1 << 32 and true("sums wrap", "q") >= 1 << 64 and true("sums wrap", "s") >= 1 << 63
    assert true("u64 sum above 2^40", "u") == 64 * ((1 << 26) - 1) < 1 << 32 and 1 << 46 <= true("u64 sum above 2^40", "q") < 1 << 47
    assert int(ref["u64 sum above 2^40"]["qsum"]) == 64 * (1 << 40) + 2016 and int(ref["u64 sum above 2^40"]["ssum"]) == -64 * (1 << 40) - 2016
    w = waves[names.index("top bit beside small")]
    assert (w["u"] >= 1 << 31).sum() >= 20 and (w["u"] < 100).sum() >= 40 and int(ref["top bit beside small"]["umin"]) < 100 <= 1 << 31 <= int(ref["top bit beside small"]["umax"])
    assert {mc.INT_MIN, -1, 0, 1, mc.INT_MAX} <= set(w["i"].tolist()) and (waves[names.index("all top bit")]["u"] >> 31).all()
    hi, lo = waves[names.index("u64 high word only")], waves[names.index("u64 low word only")]
    assert len(set((hi["q"] & np.uint64(mc.M32)).tolist())) == 1 and len(set((hi["q"] >> np.uint64(32)).tolist())) == 64
    assert len(set((lo["q"] >> np.uint64(32)).tolist())) == 1 and len(set((lo["q"] & np.uint64(mc.M32)).tolist())) == 64
    den = waves[names.index("denormals")]["f"]
    assert (den != 0).all() and (np.abs(den) < np.finfo(np.float32).tiny).all() and (den < 0).any() and (den > 0).any()
    assert np.isnan(ref["NaN everywhere"]["fmin"]) and np.isnan(ref["NaN everywhere"]["fmax"]) and ref["NaN but lane 5"]["fmin"] == ref["NaN but lane 5"]["fmax"] == 4.5
    for lane in (0, 32, 63):
        f = waves[names.index("NaN@%d" % lane)]["f"]
        assert np.isnan(f).sum() == 1 and np.isnan(f[lane]) and ref["NaN@%d" % lane]["fmin"] == np.nanmin(f) and ref["NaN@%d" % lane]["fmax"] == np.nanmax(f)
    assert ref["inf"]["fmin"] == -np.inf and ref["inf"]["fmax"] == np.inf
    assert mc.same_floats(np.float32([0.0, np.nan]), np.float32([-0.0, np.nan])) and not mc.same_floats(np.float32([1.0]), np.float32([np.nan]))
    assert not mc.same_floats(np.float32([np.nan]), np.float32([1.0])) and not mc.same_floats(np.float32([1.0]), np.float32([1.0000001]))


def test_the_key_cases_are_what_they_say():
    names, waves = mc.key_cases()
    out, trips = mc.key_reference(waves)
    assert len(names) == 64 and all(sorted(names[4 * b + w] for b in range(16)) == sorted(set(names)) for w in range(4))      # every case in every wave position
    distinct = dict(zip(names, trips.tolist()))
    assert [distinct[k] for k in ("none", "one key", "64 distinct", "two alternating", "only lane 63", "lanes 0 and 63", "0 and ffffffff", "negative")] == [0, 1, 64, 2, 1, 1, 2, 4]
    assert distinct["low 16 bits equal"] == distinct["high 16 bits equal"] == 6 and 10 <= distinct["twenty random"] <= 20 and distinct["runs"] == 13
    w, o = waves[names.index("dead carriers")], out[names.index("dead carriers")]
    assert distinct["dead carriers"] == 2 and not w["has"][0] and w["key"][0] == 7 and o["lead"][2] == 2 and o["same"][2] & 0xaaaaaaaaaaaaaaab == 0
    w, o = waves[names.index("dead lane holds the only copy")], out[names.index("dead lane holds the only copy")]
    assert distinct["dead lane holds the only copy"] == 4 and o["trip"][20] == mc.NONE and not (out["same"][names.index("dead lane holds the only copy")] >> np.uint64(20) & np.uint64(1)).any()
    o = out[names.index("lanes 0 and 63")]
    assert o["same"][0] == o["same"][63] == (1 << 63) | 1 and o["lead"][63] == 0 and o["served"].sum() == 2
    o = out[names.index("two alternating")]
    assert o["trip"][:4].tolist() == [0, 1, 0, 1] and o["key"][:2].tolist() == [77, 3] and o["same"][0] == 0x5555555555555555 and o["same"][1] == 0xaaaaaaaaaaaaaaaa
    neg = waves[names.index("negative")]["key"].astype(np.int32)
    assert {-1, -2, mc.INT_MIN} <= set(neg.tolist())


def test_the_block_cases_are_what_they_say():
    names, blocks = mc.block_cases()
    ref = dict(zip(names, mc.block_reference(blocks)))
    for wave in range(4):
        for lane in (0, 31, 32, 63):
            r = ref["one lane %d.%d" % (wave, lane)]
            assert r["count"].tolist() == [1] * 15 and r["sum32"].tolist() == r["max32"].tolist() == [0x80000001, 0x80000001, 5, 0x80000001, 5, mc.M32]
            assert r["sum64"].tolist() == r["max64"].tolist() == [(1 << 63) + 9, (1 << 63) + 9, (1 << 40) + 3, (1 << 63) + 9, (1 << 40) + 3, 1]
            assert (r["again32"], r["again64"], r["wide"].tolist()) == (5, (1 << 40) + 3, [0x80000001, 5])
    r = ref["all equal"]
    assert r["count"].tolist() == [256, 256, 0, 256, 0, 256, 256, 0, 256, 0, 256, 0, 256, 0, 256] and r["sum32"][0] == 0 and r["wide"][0] == 256 * 0x90000000      # a u32 sum that wraps
    assert r["sum64"][2] == 0 and r["max64"][2] == 1 << 56                                                                          # and a u64 one
    r = ref["all set"]
    assert (r["count"] == 256).all() and r["sum32"][0] == mc.M32 - 255 and r["sum64"][0] == mc.M64 - 255 and r["sum64"][2] == 0
    r = ref["per wave extremes"]
    assert r["max32"][0] == 0x80000003 and r["max64"][0] == (1 << 63) + 3 and r["count"][:3].tolist() == [252, 252, 4]
    assert int(ref["u64 sums above 2^40"]["sum64"][0]) == 256 * (1 << 40) + 255 * 128 and int(ref["sums wrap"]["sum32"][0]) == (256 * 0xff000000 + 255 * 128) & mc.M32


def test_the_slot_scan_and_rank_references():
    for nb in mc.NBS:
        a = mc.slots("last slot only", nb, 3)
        assert not a[:-1].any() and (a[-1] >= 1 << 31).all() and np.array_equal(mc.fold_reference(a), a[-1])
        a = mc.slots("second trip only", nb, 2, True)
        assert not a[:1024].any() and not a[2048:].any() and (nb <= 1024 or a.any())
        assert not mc.slots("zeros", nb, 5).any()
        big = mc.slots("large, the total wraps", nb, 1)
        if nb >= 63:
            assert int(big.astype(np.int64).sum()) >= 1 << 32
        off, tot = mc.scan_reference(np.ascontiguousarray(big.T))
        assert off[0, 0] == 0 and int(tot[0]) == int(big.astype(np.int64).sum()) & mc.M32 and (nb < 2 or off[0, 1] == big[0, 0])
    off, tot = mc.scan_reference(np.array([[1, 2, 3], [0xffffffff, 2, 0]], np.uint32))
    assert off.tolist() == [[0, 1, 3], [0, 0xffffffff, 1]] and tot.tolist() == [6, 1]
    keep, bases = mc.rank_cases()
    assert len(keep) == 256 * len(bases) and (bases != 0).all() and (bases.astype(np.int64) + 256 > mc.M32).sum() >= 10
    want = mc.rank_reference(keep, bases)
    assert np.array_equal(want[::256], bases) and want[256 + 255] == (int(bases[1]) + int(keep[256:511].sum())) & mc.M32


def test_the_graph_families_are_what_they_say():
    sizes = {}
    for name in mc.UF_FAMILIES:
        n, edges, forest = mc.uf_family(name)
        want = mc.uf_reference(name)
        mc.check_forest(want, want, name)                                        # (the flat forest of the reference passes the raw array's checks)
        sizes[name] = np.bincount(np.bincount(want)[np.unique(want)])            # sizes[name][k] = the components of k nodes
        assert len(edges) <= 1 << 18 and (name.startswith("tiny") or name == "bipartite") == (n != mc.N)
    one = lambda name: sizes[name].sum() == 1
    assert all(one(k) for k in ("path ascending", "path descending", "path bit-reversed", "star high", "star low", "comb", "bipartite", "tiny 1", "tiny 2"))
    n, edges, _ = mc.uf_family("star high")
    assert (edges[:, 1] == n - 1).all() and len(edges) == n - 1
    n, edges, _ = mc.uf_family("path bit-reversed")
    assert sorted(edges[:, 0].tolist()) == list(range(n - 1)) and abs(int(edges[1, 0]) - int(edges[0, 0])) == 1 << 15
    assert sizes["same edge"].tolist() == [0, mc.N - 2, 1] and sizes["cliques"].tolist() == [0] * 64 + [1024]
    assert sizes["random sparse"][2:].sum() >= 5000 and sizes["random sparse"][1] >= 20000 and sizes["random dense"].sum() < 100
    n, edges, _ = mc.uf_family("same edge")
    assert (edges[:, 0] == edges[:, 1]).sum() >= 1 << 12 and len({tuple(e) for e in edges.tolist()}) == 4 and len(edges) == 1 << 16
    for name in ("forest of runs", "forest of scattered groups", "deep forest"):
        n, edges, forest = mc.uf_family(name)
        start = mc.components(n, np.zeros((0, 2), np.uint32), forest)
        depth2 = (forest[forest] != forest).sum()
        assert (depth2 > 1000) == (name == "deep forest") and len(np.unique(mc.uf_reference(name))) < len(np.unique(start))      # the edges join groups
    _, _, runs = mc.uf_family("forest of runs")
    lengths = np.diff(np.flatnonzero(np.r_[runs == np.arange(mc.N), True]))
    assert lengths.min() >= 1 and lengths.max() <= 512 and len(lengths) > 100 and (np.diff(runs.astype(np.int64)) >= 0).all()
    bad = np.array([0, 0, 1, 2], np.uint32)
    for wrong in ([0, 1, 1, 2], [0, 0, 3, 2], [0, 0, 0, 3]):                         # a cycle-free but wrong forest, a parent above its node, a root too many
        try:
            mc.check_forest(np.array(wrong, np.uint32), mc.components(4, np.array([[0, 1], [2, 3], [1, 2]], np.uint32)), "wrong")
        except AssertionError:
            continue
        raise AssertionError("check_forest let %r through" % (wrong,))
    mc.check_forest(bad, np.zeros(4, np.uint32), "a chain")


def test_the_grid_references_agree_and_are_what_they_say():
    """numpy's unravel_index / ravel_multi_index against a serial divmod loop, on the shapes the device runs; then what the shapes are there for"""
    for W, H, D in mc.GRID_SHAPES:
        a, b = mc.grid_reference(W, H, D), mc.grid_reference_divmod(W, H, D)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)), (W, H, D)
        vox, origin, walk = a
        assert np.array_equal(vox["index"], np.arange(W * H * D)) and vox["x"].max() == W - 1 and vox["y"].max() == H - 1 and vox["z"].max() == D - 1
        assert len(origin) == int(vox["tile"].max()) + 1 and (vox["place"] < 512).all() and (vox["pos"] < 1000).all()
        first = np.flatnonzero(vox["place"] == 0)                                    # the voxel at place 0 of a tile is the tile's origin
        assert np.array_equal(np.stack([vox[f][first] for f in "xyz"], axis=1)[np.argsort(vox["tile"][first])], origin[:, :3])
        assert len({(int(t), int(p)) for t, p in zip(vox["tile"], vox["place"])}) == W * H * D      # a tile and a place name one voxel
    assert walk.shape == (26, 3) and walk[0].tolist() == [-1, -1, -1] and walk[1].tolist() == [0, -1, -1] and walk[12].tolist() == [-1, 0, 0] and walk[13].tolist() == [1, 0, 0]
    assert walk[25].tolist() == [1, 1, 1] and len({tuple(w) for w in walk.tolist()}) == 26 and (0, 0, 0) not in {tuple(w) for w in walk.tolist()}
    sides = {axis: sorted({s[axis] for s in mc.GRID_SHAPES}) for axis in range(3)}
    for axis in range(3):                                                            # below, at and above the tile side on each axis; a one-voxel axis in each position
        assert 1 in sides[axis] and mc.TILE in sides[axis] and any(mc.TILE > s > 0 for s in sides[axis]) and any(s > mc.TILE and s % mc.TILE for s in sides[axis])
    assert any(W * H * D > 256 and (W * H * D) % 256 for W, H, D in mc.GRID_SHAPES) and max(W * H * D for W, H, D in mc.GRID_SHAPES) < 5000
    vox, origin, _ = mc.grid_reference(9, 17, 1)
    assert origin.tolist() == [[0, 0, 0, 0], [8, 0, 0, 0], [0, 8, 0, 0], [8, 8, 0, 0], [0, 16, 0, 0], [8, 16, 0, 0]]
    assert tuple(vox[8 + 9 * 16]) == (8, 16, 0, 152, 5, 0, 111, 0) and tuple(vox[7 + 9 * 7]) == (7, 7, 0, 70, 0, 63, 188, 0)
