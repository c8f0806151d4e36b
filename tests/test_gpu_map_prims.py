"""The device builds of what the map units share - the wave and block folds, the key walk, the slot folds, the row scan and the block rank of
csrc/qn_map_compact.cuh, the two linkers of csrc/qn_union_find.cuh, the index, tile and rim arithmetic and the neighbourhood walk of csrc/qn_dense_grid.cuh - called directly through qn_kf_debug_map_prims (csrc/qn_map_selftest.hip) on the inputs of
tests/map_prims_cases.py, which no unit can produce, against that file's serial references.  Every comparison is exact: integers by value, floats by value
with +0 and -0 equal and a NaN lane ignored unless every lane is NaN.  The sign of a zero minimum or maximum is whatever fminf / fmaxf give, and no caller
reads it: the only float callers, k_mg_extent and k_mg_extent_sum, hand the extremes to qn_kf_map_ground, which takes floor(x / cell) of them, compares and
converts to integers - a zero of either sign gives column 0 and a grid origin equal to 0.0 by value.

No caller can reach nb = 0 in a slot fold or a scan - a map slot has at least one record, and the grid calls launch them only behind `if (cells)`,
`if (nt)` or `if (nc)` - and the entry point writes nothing for n = 0, so nb starts at 1 here.

The union-find runs are the production text on graphs the units' geometry cannot make: after the unite launch the raw parent array must have
parent[x] <= x, every parent[x] in x's component, every walk ending within n steps, the roots exactly the component minima; after the flatten root[x] is
the smallest node of x's component; a rerun gives the same roots (the raw array may differ).  Every interleaving, on tiny forests: tests/test_union_find_model.py."""
import ctypes as C
import numpy as np
import pytest
import map_prims_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def store():
    from qn_amd import engine
    s = engine.KeyframeStore()
    yield s
    s.close()


def _fields(got, want, names, what):
    for k, name in enumerate(names):
        for f in want.dtype.names:
            g, w = got[k][f], want[k][f]
            same = mc.same_floats(g, w) if want.dtype[f].kind == "f" else np.array_equal(g, w)
            assert same, "%s, %s.%s: %s, the reference has %s" % (what, name, f, g, w)


def test_wave_folds(store):
    names, waves = mc.wave_cases()
    want = mc.wave_reference(waves)
    for again in range(2):                                                       # (and a rerun: the same values)
        got = store.debug_map_prims(store.MAP_PRIMS_WAVES, waves.reshape(-1))
        _fields(got, want, names, "wave folds")


@pytest.mark.parametrize("signed", [0, 1], ids=["uint32_t", "int32_t"])
def test_key_walk(store, signed):
    names, waves = mc.key_cases()
    want, want_trips = mc.key_reference(waves)
    got, trips = store.debug_map_prims(store.MAP_PRIMS_KEYS, waves.reshape(-1), signed)
    got = got.reshape(waves.shape)
    for w, name in enumerate(names):
        g, has = got[w], waves[w]["has"] != 0
        ballot = sum(1 << int(l) for l in np.flatnonzero(has))
        served = g["trip"] != mc.NONE
        # the properties, from the device's own output: a trip per distinct key, in ascending order of first lane, lead the lowest bit of same, the masks
        # disjoint with the ballot of has as their union - so a lane without a key is in no mask, whatever key it carries
        assert trips[w] == len(set(waves[w]["key"][has].tolist())), name
        assert np.array_equal(served, has) and (g["served"] == has).all(), name
        masks = {}
        for lane in np.flatnonzero(served):
            masks.setdefault(int(g["trip"][lane]), set()).add((int(g["same"][lane]), int(g["lead"][lane]), int(g["key"][lane])))
        assert sorted(masks) == list(range(int(trips[w]))) and all(len(v) == 1 for v in masks.values()), name
        union, leads = 0, []
        for trip in range(int(trips[w])):
            (same, lead, key), = masks[trip]
            assert same & union == 0 and same != 0 and lead == (same & -same).bit_length() - 1, name
            assert same == sum(1 << int(l) for l in np.flatnonzero(served & (g["trip"] == trip))), name
            assert all(int(waves[w]["key"][l]) == key for l in range(64) if (same >> l) & 1), name
            union |= same; leads.append(lead)
        assert union == ballot and leads == sorted(leads), name
    _fields(got.reshape(-1, 1), want.reshape(-1, 1), ["%s, lane %d" % (n, l) for n in names for l in range(64)], "key walk")
    assert np.array_equal(trips, want_trips)


def test_block_folds(store):
    names, blocks = mc.block_cases()
    want = mc.block_reference(blocks)
    got = store.debug_map_prims(store.MAP_PRIMS_BLOCKS, blocks.reshape(-1))
    _fields(got, want, names, "block folds")


@pytest.mark.parametrize("nb", mc.NBS)
def test_slot_folds(store, nb):
    """k_slot_fold<uint32_t, K> and <unsigned long long, K> for every K the units launch, and k_slot_max<uint32_t>"""
    for pattern in mc.SLOT_PATTERNS:
        for wide, ks in ((False, mc.FOLD_K32), (True, mc.FOLD_K64)):
            for k in ks:
                a = mc.slots(pattern, nb, k, wide)
                got = store.debug_map_prims(store.MAP_PRIMS_SLOTS, a, (store.MAP_PRIMS_U64 if wide else 0) | k)
                assert np.array_equal(got, mc.fold_reference(a)), (pattern, wide, k, got, mc.fold_reference(a))
        a = mc.slots(pattern, nb, 1)[:, 0]
        got = store.debug_map_prims(store.MAP_PRIMS_SLOTS, a, store.MAP_PRIMS_MAX)
        assert got.shape == (1,) and int(got[0]) == max(int(v) for v in a), (pattern, got)


@pytest.mark.parametrize("nb", mc.NBS)
def test_scan_rows(store, nb):
    """out of place and in place (cnt == off), one row and three rows at once"""
    for pattern in mc.SLOT_PATTERNS:
        for rows in (1, 3):
            cnt = np.ascontiguousarray(mc.slots(pattern, nb, rows).T)
            want_off, want_tot = mc.scan_reference(cnt)
            for in_place in (0, store.MAP_PRIMS_IN_PLACE):
                off, tot = store.debug_map_prims(store.MAP_PRIMS_SCAN, cnt, rows | in_place)
                assert np.array_equal(off, want_off) and np.array_equal(tot, want_tot), (pattern, rows, bool(in_place))


def test_block_rank(store):
    keep, bases = mc.rank_cases()
    got = store.debug_map_prims(store.MAP_PRIMS_RANK, (keep, bases))
    want = mc.rank_reference(keep, bases)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "block_rank differs in block %d, lane %d: %d, the reference has %d" % (bad[0] // 256, bad[0] % 256, got[bad[0]], want[bad[0]])


LINKERS = {"uf_unite": 6, "uf_unite_min": 7}


@pytest.mark.parametrize("per", mc.EDGE_LANES)
@pytest.mark.parametrize("family", mc.UF_FAMILIES)
@pytest.mark.parametrize("linker", list(LINKERS))
def test_union_find(store, linker, family, per):
    n, edges, forest = mc.uf_family(family)
    want = mc.uf_reference(family)
    parent, root = store.debug_map_prims(LINKERS[linker], (n, edges, forest), per)
    mc.check_forest(parent, want, "%s, %s, %d edges a lane" % (linker, family, per))
    assert np.array_equal(root, want)
    _, again = store.debug_map_prims(LINKERS[linker], (n, edges, forest), per)
    assert np.array_equal(again, want)


@pytest.mark.parametrize("per", mc.EDGE_LANES)
@pytest.mark.parametrize("family", ["random dense", "comb", "forest of runs"])
@pytest.mark.parametrize("linker", list(LINKERS))
def test_union_find_in_two_launches(store, linker, family, per):
    """the edges split over two calls, the second starting from the raw forest the first one left: the components of all of them"""
    n, edges, forest = mc.uf_family(family)
    half = len(edges) // 2
    parent, root = store.debug_map_prims(LINKERS[linker], (n, edges[:half], forest), per)
    first = mc.components(n, edges[:half], forest)
    mc.check_forest(parent, first, "%s, %s, first half" % (linker, family))
    assert np.array_equal(root, first)
    parent2, root2 = store.debug_map_prims(LINKERS[linker], (n, edges[half:], parent), per)
    mc.check_forest(parent2, mc.uf_reference(family), "%s, %s, second half" % (linker, family))
    assert np.array_equal(root2, mc.uf_reference(family))


@pytest.mark.parametrize("shape", mc.GRID_SHAPES, ids=["%dx%dx%d" % s for s in mc.GRID_SHAPES])
def test_grid_geometry(store, shape):
    """oc_ijk, dg_index, dg_tile_of, dg_in_tile, dg_lane_pos, dg_tile_origin and the order of dg_each_neighbour against numpy's unravel_index: exact"""
    vox, origin, walk = store.debug_map_prims(store.MAP_PRIMS_GRID, shape)
    want_vox, want_origin, want_walk = mc.grid_reference(*shape)
    _fields(vox.reshape(-1, 1), want_vox.reshape(-1, 1), ["%s, index %d" % (shape, i) for i in range(len(want_vox))], "grid geometry")
    assert np.array_equal(origin, want_origin), (shape, origin, want_origin)
    assert np.array_equal(walk, want_walk), (walk, want_walk)


def test_refusals_and_the_empty_input(store):
    from qn_amd import engine
    L = store._l
    L.qn_kf_debug_map_prims.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    a = np.zeros(1 << 14, np.uint32); out = np.full(1 << 14, 7, np.uint32)
    call = lambda *args: L.qn_kf_debug_map_prims(*args)
    for which in range(9):
        arg = {3: 2, 4: 1, 6: 1, 7: 13}.get(which, 0)
        assert call(None, which, p(a), 1, arg, p(out)) == engine.QN_ERR_INVALID_ARG
        assert call(store.h, which, None, 1, arg, p(out)) == engine.QN_ERR_INVALID_ARG
        assert call(store.h, which, p(a), 1, arg, None) == engine.QN_ERR_INVALID_ARG
        assert call(store.h, which, p(a), 0, arg, p(out)) == engine.QN_OK                      # n == 0: nothing written
        cap = (1 << 20) if which in (3, 4, 6, 7, 8) else (1 << 16)
        assert call(store.h, which, p(a), cap + 1, arg, p(out)) == engine.QN_ERR_INVALID_ARG
    for which, arg in ((-1, 0), (9, 0), (8, 0), (8, 1), (0, 1), (1, 2), (2, 1), (3, 0), (3, 4), (3, 0x104), (3, 0x201), (4, 0), (4, 0x80000000), (4, (1 << 16) + 1), (5, 1), (6, 0), (7, 14)):
        assert call(store.h, which, p(a), 1, arg, p(out)) == engine.QN_ERR_INVALID_ARG, (which, arg)
    for which in (6, 7):
        for words in ([(1 << 20) + 1, 0], [1, 2], [1, 0, 0, 4], [1, 0, 4, 0], [0, 1, 0, 2, 1, 1], [1, 1, 0, 1, 2, 3, 3, 4]):      # m, forest, then parents / edges; n = 4
            a[:8] = 0; a[:len(words)] = words
            assert call(store.h, which, p(a), 4, 1, p(out)) == engine.QN_ERR_INVALID_ARG, (which, words)
    for n, sides in ((1, [0, 0, 0]), (6, [0, 2, 3]), (6, [1, 0, 6]), (6, [2, 3, 0]), (6, [2, 3, 2]), (6, [7, 1, 1]), (1 << 20, [1 << 10, 1 << 10, 2]), (0x10, [1 << 16, 1 << 16, 1 << 4])):
        a[:3] = sides                                                            # a zero side, a product other than n, above the cap, a product that wraps 32 bits
        assert call(store.h, 8, p(a), n, 0, p(out)) == engine.QN_ERR_INVALID_ARG, (n, sides)
    a[:8] = 0
    assert (out == 7).all()
    with pytest.raises(ValueError):
        store.debug_map_prims(store.MAP_PRIMS_WAVES, np.zeros(255, mc.LANE))
    with pytest.raises(ValueError):
        store.debug_map_prims(store.MAP_PRIMS_RANK, (np.zeros(256, np.uint8), np.zeros(2, np.uint32)))
    parent, root = store.debug_map_prims(store.MAP_PRIMS_UNITE, (4, np.zeros((0, 2), np.uint32), np.array([0, 0, 1, 3], np.uint32)), 1)      # no edge: init and flatten alone
    assert parent.tolist() == [0, 0, 1, 3] and root.tolist() == [0, 0, 0, 3]
