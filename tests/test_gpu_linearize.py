"""The device builds of what stands between a correspondence and the 6 x 6 system of a registration tick, through qn_debug_linearize on the inputs of
tests/linearize_cases.py: accumulate_point_n (csrc/qn_linearize.cuh) under the bounds of tests/linearize_checks.py against the 50-digit reference, and bit for
bit against the host build of the same text; emit_point (csrc/qn_tick.cuh) bit for bit against accumulate_point_n, one live lane per wave at every lane
position, whatever the lanes without a correspondence and the pose hold; fold7, the `first` flag, the trips and the waves bit for bit against the order restated
in Python; the cost of a trial pass bit for bit against a linearisation pass'; reduce_rows in its four instantiations bit for bit against its restated order
and against each other; reruns and refusals.  The maxima and counts are printed."""
import ctypes as C
import numpy as np
import pytest
import linearize_cases as lc
import linearize_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from qn_amd import engine
    c = engine.Context(1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device(ctx):
    """accumulate_point_n on the device, each table computed once"""
    cache = {}

    def run(rec):
        key = (rec.shape, rec.tobytes())
        if key not in cache:
            out = ctx.debug_linearize(ctx.LIN_POINT, rec)
            out.setflags(write=False)
            cache[key] = out
        return cache[key]
    return run


@pytest.fixture(scope="module")
def emit(ctx):
    """emit_point on blocks of one trip, 1024 blocks a call -> (blocks, 5, 28)"""
    def run(blocks, trips=1):
        return np.concatenate([ctx.debug_linearize(ctx.LIN_EMIT, blocks[i:i + 1024], trips) for i in range(0, len(blocks), 1024)])
    return run


@pytest.mark.parametrize("name", lc.FAMILIES)
def test_accumulate_point_n_within_the_bounds(device, name):
    chk.check_family(name, device, label="device accumulate_point_n")


def test_accumulate_point_n_equals_the_host_build_bit_for_bit(device):
    """+ - x / only, both built without contraction: every record of the families and every correspondence of the fold blocks"""
    tables = [(name, lc.family(name)) for name in lc.FAMILIES] + [("fold blocks, %d trips" % t, lc.fold_blocks(t)[1].reshape(-1, lc.POINT)) for t in (1, 2, 4)]
    total = 0
    for name, rec in tables:
        differ = (chk.bits(device(rec)) != chk.bits(chk.host(rec))).any(axis=1)
        total += len(rec)
        assert not differ.any(), (name, int(differ.sum()), np.flatnonzero(differ)[:8])
    print("device against host, accumulate_point_n: 0 of %d records differ in any bit" % total)


@pytest.mark.parametrize("name", lc.FAMILIES)
def test_emit_point_equals_accumulate_point_n_bit_for_bit(device, emit, name):
    """one trip, one live lane per wave, the other 63 without a correspondence: every wave row is the record's accumulate_point_n, the block's row four of them added
    to 0.0 in turn - the same bytes whether the other lanes hold zeros, NaN, +Inf, -Inf or 1e300 in points and normals.  Then emit_point's row under the bounds."""
    rec = lc.family(name)
    want = device(rec)
    blk = np.zeros_like(want)
    for _ in range(4):
        blk = blk + want
    blocks, at = lc.single_live(rec)
    got = emit(blocks)
    for w in range(4):
        differ = (chk.bits(got[:, w]) != chk.bits(want)).any(axis=1)
        assert not differ.any(), (name, "wave", w, int(differ.sum()), "live lanes", sorted(set((at[differ] + 16 * w) % 64))[:8])
    assert chk.same_bits(np.ascontiguousarray(got[:, 4]), blk), (name, "the block's row")
    for poison in lc.POISONS[1:]:
        assert chk.same_bits(emit(lc.single_live(rec, poison)[0]), got), (name, "lanes without a correspondence holding", poison)
    chk.check_family(name, lambda r: np.ascontiguousarray(got[:, 0]), label="device emit_point")
    print("emit_point against accumulate_point_n, %-13s: 0 of %d wave rows differ in any bit, the live lane at %d positions, 5 fillings of the other lanes" % (name, 4 * len(rec), len(set(at))))


@pytest.mark.parametrize("trips", (1, 2, 4))
def test_a_block_without_a_correspondence_gives_rows_of_zeros(emit, trips):
    """... under a pose that holds a NaN too, whatever the lanes hold"""
    got = emit(lc.dead_blocks(trips), trips)
    assert got.shape == (12, 5, lc.NPART) and chk.same_bits(got, np.zeros_like(got))


@pytest.mark.parametrize("trips", (1, 2, 4))
def test_fold7_rows_and_block_rows_equal_the_restated_order(device, emit, trips):
    """full blocks of wide-ranging contributions under the five `have` masks: the device's four wave rows and its block row are the restated fold of the lanes'
    accumulate_point_n values, bit for bit - sub-sums upwards, the three exchange steps, `first` replacing the row and later trips adding to it, the waves in
    order.  The cost of a trial pass (lin = 0) has the bits of the same block's linearisation pass, and its other 27 sums are +0.0."""
    blocks, points, have, lin, twin = lc.fold_blocks(trips)
    contrib = device(points.reshape(-1, lc.POINT)).reshape(len(blocks), trips, lc.BLOCK, lc.NPART)
    got = emit(blocks, trips)
    for i in range(len(blocks)):
        rows, blk = chk.fold_rows(contrib[i], have[i])
        assert chk.same_bits(np.ascontiguousarray(got[i, :4]), rows), (trips, i, "wave rows", np.argwhere(chk.bits(got[i, :4]) != chk.bits(rows))[:6])
        assert chk.same_bits(np.ascontiguousarray(got[i, 4]), blk), (trips, i, "block row")
    trial = np.flatnonzero(~lin)
    assert len(trial) == 20 and chk.same_bits(np.ascontiguousarray(got[trial][:, :, :27]), np.zeros((20, 5, 27)))
    assert chk.same_bits(np.ascontiguousarray(got[trial][:, :, 27]), np.ascontiguousarray(got[twin[trial]][:, :, 27])), "the cost of a trial pass goes through the same additions"
    assert (got[lin][:, 4, 27] != 0).sum() == (16 if trips == 1 else 20)      # (every mask but `none` has something to add; the masks rotate with the trips)
    print("fold7, %d trips: 0 of %d wave rows and 0 of %d block rows differ from the restated order in any bit" % (trips, 4 * len(blocks), len(blocks)))


@pytest.mark.parametrize("n", lc.ROW_COUNTS)
def test_reduce_rows_equals_the_restated_order_in_every_instantiation(ctx, n):
    rows = lc.rows_table(n)
    want = chk.reduce_rows_order(rows)
    for nt, coherent in lc.ROW_KINDS:
        got = ctx.debug_linearize(ctx.LIN_ROWS, rows, nt + coherent)
        assert chk.same_bits(got, want), (n, nt, coherent, np.flatnonzero(chk.bits(got) != chk.bits(want)))


def test_reduce_rows_a_nan_row_reaches_its_components_only(ctx):
    rows = lc.nan_table()
    for nt, coherent in lc.ROW_KINDS:
        got = ctx.debug_linearize(ctx.LIN_ROWS, rows, nt + coherent)
        assert tuple(np.flatnonzero(np.isnan(got))) == lc.NAN_COMPONENTS, (nt, coherent)
        keep = ~np.isnan(got)
        assert chk.same_bits(got[keep], chk.reduce_rows_order(lc.rows_table(513))[keep])


def test_rerun_returns_the_same_bytes(ctx, device, emit):
    rec = lc.all_records()
    assert chk.same_bits(ctx.debug_linearize(ctx.LIN_POINT, rec), device(rec)) and chk.same_bits(device(rec), np.concatenate([device(lc.family(name)) for name in lc.FAMILIES]))
    blocks = lc.fold_blocks(4)[0]
    assert chk.same_bits(emit(blocks, 4), emit(blocks, 4))
    for nt, coherent in lc.ROW_KINDS:
        assert chk.same_bits(ctx.debug_linearize(ctx.LIN_ROWS, lc.rows_table(1153), nt + coherent), ctx.debug_linearize(ctx.LIN_ROWS, lc.rows_table(1153), nt + coherent))


def test_refusals_and_the_empty_batch(ctx):
    from qn_amd import engine
    L = ctx._l
    L.qn_debug_linearize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    a = np.ones(lc.HEAD + 4 * lc.BLOCK * lc.LANE); out = np.full(5 * lc.NPART, 7.0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    good = {0: 0, 1: 1, 2: 256}
    refused = [(None, 0, p(a), 1, 0, p(out)), (ctx.h, 0, None, 1, 0, p(out)), (ctx.h, 0, p(a), 1, 0, None), (ctx.h, 3, p(a), 1, 0, p(out)), (ctx.h, -1, p(a), 1, 0, p(out)),
               (ctx.h, 0, p(a), 1, 1, p(out)), (ctx.h, 1, p(a), 1, 0, p(out)), (ctx.h, 1, p(a), 1, 5, p(out)), (ctx.h, 2, p(a), 1, 0, p(out)), (ctx.h, 2, p(a), 1, 255, p(out)),
               (ctx.h, 2, p(a), 1, 258, p(out)), (ctx.h, 2, p(a), 1, 514, p(out)), (ctx.h, 2, p(a), 1, 1024, p(out)),
               (ctx.h, 0, p(a), (1 << 20) + 1, 0, p(out)), (ctx.h, 1, p(a), (1 << 11) + 1, 1, p(out)), (ctx.h, 2, p(a), (1 << 16) + 1, 256, p(out)), (ctx.h, 2, None, 0, 256, p(out))]
    for args in refused:
        assert L.qn_debug_linearize(*args) == engine.QN_ERR_INVALID_ARG, args[1:5]
    assert (out == 7.0).all()
    for which in (3, -1):
        with pytest.raises(ValueError):
            ctx.debug_linearize(which, a)
    with pytest.raises(ValueError):
        ctx.debug_linearize(ctx.LIN_EMIT, a, 5)
    for which, arg in good.items():
        assert L.qn_debug_linearize(ctx.h, which, p(a), 0, arg, p(out)) == engine.QN_OK and (out == 7.0).all()      # n == 0: nothing written
    assert ctx.debug_linearize(ctx.LIN_POINT, np.zeros((0, lc.POINT))).shape == (0, lc.NPART)
    assert ctx.debug_linearize(ctx.LIN_EMIT, np.zeros((0, lc.HEAD + lc.BLOCK * lc.LANE)), 1).shape == (0, 5, lc.NPART)
    assert ctx.debug_linearize(ctx.LIN_ROWS, np.zeros((0, lc.NPART)), 512).shape == (0,)
    one = ctx.debug_linearize(ctx.LIN_ROWS, np.arange(28.0).reshape(1, 28), 513)
    assert np.array_equal(one, np.arange(28.0))
