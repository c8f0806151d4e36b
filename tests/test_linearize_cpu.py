"""The host build of accumulate_point_n (csrc/qn_linearize.cuh through tests/linearize_host.cpp: the text the kernels compile) against the 50-digit mpmath
reference of the dense GICP linearisation on the families of tests/linearize_cases.py, under the bounds of tests/linearize_checks.py; the dense numpy
evaluation that sets the bounds' constant; the same program under the address and undefined-behaviour sanitizers; three mutants of the text, each of which must
fail a family's check; and the restated orders of fold7 and reduce_rows on inputs where order cannot matter and on the inputs where it must.  No GPU; the
device: tests/test_gpu_linearize.py."""
import ctypes as C
import numpy as np
import pytest
import linearize_cases as lc
import linearize_checks as chk


@pytest.mark.parametrize("name", lc.FAMILIES)
def test_host_build_within_the_bounds(name):
    chk.check_family(name, chk.host, label="host accumulate_point_n")


def test_dense_evaluation_sets_the_constant():
    """the rule for C: 16 while the dense numpy f64 evaluation stays within 2 of the bounds at C = 1 on this table, otherwise the next power of two at or above eight
    times its largest ratio.  It measures 2.24 (H, a zero-normal record with cond 1, where kappa mu s^2 is smallest against the roundings of T mu_A + t): C = 32."""
    worst = np.zeros(3)
    for name in lc.FAMILIES:
        top = chk.check_family(name, chk.dense, label="dense numpy")
        worst = np.maximum(worst, top)
    rule = 16.0 if worst.max() <= 2.0 else 2.0 ** np.ceil(np.log2(8.0 * worst.max()))
    print("dense numpy: max H %.3g  b %.3g  cost %.3g over the table -> C = %g" % (tuple(worst) + (rule,)))
    assert chk.C_BOUND == rule, (worst, rule)


def test_the_families_are_what_they_say():
    for name in lc.FAMILIES:
        rec = lc.family(name)
        Rx, Tx, pa, pb, na, nb, lin = lc.split(rec)
        assert np.isfinite(rec).all() and np.array_equal(lc.f32(pa), pa) and np.array_equal(lc.f32(pb), pb)
        assert (name == "trial") == (not np.array_equal(Rx, Tx)) and lin.all() == (name != "trial")
    kappa = lambda name: chk.reference(name)[2][:, 0]
    par = lc.tags("parallel")
    assert {(o, s) for o, s in par} == {(o, s) for o in lc.OFFS for s in (1.0, -1.0)}
    exact = np.array([o <= 1e-9 for o, _ in par])
    assert (np.abs(kappa("parallel")[exact] - 1000.0) < 1e-3).all() and kappa("parallel")[~exact].min() < 999.0, "parallel normals: cond = 2 / 0.002"
    assert np.allclose(kappa("zero-normal")[np.array(lc.tags("zero-normal")) == 2], 1.0) and kappa("perpendicular").max() < 2.01 and kappa("f32-pose").max() > 990.0
    Rx = lc.split(lc.family("f32-pose"))[0][:, :, :3]
    off = np.abs(Rx @ np.swapaxes(Rx, 1, 2) - np.eye(3)).max(axis=(1, 2))
    assert np.array_equal(lc.f32(Rx), Rx) and 1e-8 < off.max() < 2e-7, "an f32 rotation is orthonormal to 6e-8 only"
    for name in ("random", "parallel", "perpendicular", "zero-normal", "f32-pose", "trial"):
        _, _, s, r, g = chk.reference(name)[2][: lc.N].T
        assert s.max() > 1e4 and s.min() < 1.1 and r.min() < 1e-5 and r.max() > 0.5
    a, b = lc.family("trial")[: lc.N], lc.family("trial")[lc.N:]
    assert np.array_equal(a[:, :36], b[:, :36]) and (a[:, 36] == 1).all() and (b[:, 36] == 0).all()
    blocks, at = lc.single_live(lc.all_records())
    assert blocks.shape == (len(lc.all_records()), lc.HEAD + lc.BLOCK * lc.LANE) and set(at) == set(range(64)) and (blocks[:, lc.HEAD::lc.LANE].sum(axis=1) == 4).all()
    for trips in (1, 2, 4):
        blocks, points, have, lin, twin = lc.fold_blocks(trips)
        assert blocks.shape == (40, lc.HEAD + trips * lc.BLOCK * lc.LANE) and np.array_equal(twin[twin], np.arange(40)) and (lin != lin[twin]).all()
        assert np.array_equal(blocks[:, :24], blocks[twin][:, :24]) and np.array_equal(blocks[:, 25:], blocks[twin][:, 25:])
        assert {tuple(h[0]) for h in have} == {tuple(lc._mask(k)) for k in range(5)}
        assert np.array_equal(points[:, :, :, 24:36].reshape(40, -1, 12), blocks[:, 25:].reshape(40, -1, 13)[:, :, 1:])
    assert np.isnan(lc.dead_blocks(2)[:, :24]).any(axis=1).sum() == 8 and not lc.dead_blocks(2)[:, lc.HEAD::lc.LANE].any()
    for n in lc.ROW_COUNTS:
        a = np.abs(lc.rows_table(n))
        assert a.shape == (n, 28) and a.min() >= 1e-8 and a.max() <= 1e8 and (lc.rows_table(n) < 0).any()


def test_sanitizer_build_runs_every_family_and_agrees():
    """address + undefined-behaviour sanitizers on the stand-alone host program, every finding fatal: every family and the fold blocks' correspondences end with
    exit status 0 (host_run checks it) and the bytes of the plain build"""
    for name in lc.FAMILIES:
        assert chk.same_bits(chk.host_run(lc.family(name), sanitize=True), chk.host(lc.family(name))), name
    pts = lc.fold_blocks(1)[1].reshape(-1, lc.POINT)
    assert chk.same_bits(chk.host_run(pts, sanitize=True), chk.host(pts))


@pytest.mark.parametrize("mutant", sorted(chk.MUTANTS))
def test_a_mutant_of_the_text_fails_its_family(mutant):
    """a transposed MS index in the cross block, G replaced by I (R R' = I assumed under an f32 rotation), 0.999 on one normal only: the check that the host
    build passes (test_host_build_within_the_bounds) fails each"""
    name = chk.MUTANTS[mutant][2]
    run = lambda rec: chk.host_run(rec, mutant=mutant)
    q = chk.ratios(name, run(lc.family(name))).max(axis=0)
    print("mutant %-26s on %-9s: max H %.3g  b %.3g  cost %.3g of the bound at C = 1" % (mutant, name, q[0], q[1], q[2]))
    with pytest.raises(AssertionError):
        chk.check_family(name, run, label=mutant, quiet=True)
    assert q.max() > 8 * chk.C_BOUND
    if mutant == "gram-is-identity":
        assert chk.ratios(name, chk.dense(lc.family(name), gram=False)).max() > 8 * chk.C_BOUND, "the dense evaluation with R R' = I misses the bound as well"
        assert chk.same_bits(run(lc.family("same-point")), chk.host(lc.family("same-point"))), "under the identity the mutant is the text"


def test_restated_orders_on_inputs_where_order_cannot_matter():
    """small integers: every partial sum is exact, so the restatements equal the plain dense sums whatever their order - they add every value once"""
    rng = np.random.default_rng(5)
    for trips in (1, 2, 4):
        x = rng.integers(-1000, 1000, size=(trips, lc.BLOCK, lc.NPART)).astype(np.float64)
        for have in (np.ones((trips, lc.BLOCK), bool), rng.random((trips, lc.BLOCK)) < 0.5, np.zeros((trips, lc.BLOCK), bool)):
            rows, blk = chk.fold_rows(x, have)
            want = np.where(have[:, :, None], x, 0.0).reshape(trips, 4, 64, lc.NPART).sum(axis=(0, 2))
            assert np.array_equal(rows, want) and np.array_equal(blk, want.sum(axis=0))
            for order in ("down", "steps", "waves", "trips"):
                assert np.array_equal(chk.fold_rows(x, have, order)[1], blk)
    for n in lc.ROW_COUNTS + (0,):
        x = rng.integers(-1000, 1000, size=(n, lc.NPART)).astype(np.float64)
        assert np.array_equal(chk.reduce_rows_order(x), x.sum(axis=0)), n


def test_the_chosen_inputs_show_the_order():
    """on the fold blocks and the row tables a permuted order gives other bits: the exact comparisons of the GPU tests see a sub-sum taken in another order"""
    for trips in (1, 2, 4):
        blocks, points, have, lin, twin = lc.fold_blocks(trips)
        contrib = chk.host(points.reshape(-1, lc.POINT)).reshape(40, trips, lc.BLOCK, lc.NPART)
        full = [i for i in range(40) if lin[i]]                      # (every mask: a permuted order must show on some block, in every component)
        for order in ("down", "steps", "waves") + (("trips",) if trips == 4 else ()):
            changed = np.zeros(lc.NPART, bool)
            for i in full:
                rows, blk = chk.fold_rows(contrib[i], have[i]); rows2, blk2 = chk.fold_rows(contrib[i], have[i], order)
                changed |= (chk.bits(blk) != chk.bits(blk2)) | (chk.bits(rows) != chk.bits(rows2)).any(axis=0)
            assert changed.all(), (trips, order, np.flatnonzero(~changed))
    for n in lc.ROW_COUNTS:
        if n >= 35:
            x = lc.rows_table(n)
            want = chk.reduce_rows_order(x)
            assert (chk.bits(chk.reduce_rows_order(x, segs=17)) != chk.bits(want)).sum() >= 14, n
            assert (chk.bits(x.sum(axis=0)) != chk.bits(want)).any(), n
        if n == 1153:
            assert (chk.bits(chk.reduce_rows_order(x, batch=16)) == chk.bits(want)).all(), "the batches continue one running sum: their size does not show"


def test_device_entry_is_exported_wrapped_and_refuses_a_null_context():
    from qn_amd import engine
    import test_capi_symbols
    assert "qn_debug_linearize" in test_capi_symbols.declared_symbols() and callable(engine.Context.debug_linearize)
    E = engine.Context
    assert (E.LIN_POINT_STRIDE, E.LIN_HEAD, E.LIN_LANE, E.LIN_BLOCK, E.LIN_NPART) == (lc.POINT, lc.HEAD, lc.LANE, lc.BLOCK, lc.NPART)
    L = engine.lib()
    L.qn_debug_linearize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    a = np.ones(lc.HEAD + lc.BLOCK * lc.LANE); out = np.full(5 * lc.NPART, 7.0)
    for which, arg in ((0, 0), (1, 1), (2, 256)):
        assert L.qn_debug_linearize(None, which, a.ctypes.data_as(C.c_void_p), 1, arg, out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_no_product_path_calls_the_debug_entry_and_the_dead_reducer_is_gone():
    import os
    import re
    names = sorted(f for f in os.listdir(chk.CSRC) if f.endswith((".hip", ".cuh", ".h", ".inc")))
    text = {f: re.sub(r"//.*", "", open(os.path.join(chk.CSRC, f)).read()) for f in names}
    assert {f for f, t in text.items() if "debug_launch_linearize" in t} == {"qn_engine.hip", "qn_linearize_debug.hip"}
    assert {f for f, t in text.items() if "qn_debug_linearize" in t} == {"qn_engine.hip"} and text["qn_engine.hip"].count("qn_debug_linearize") == 1
    assert not any("reduce_block_partials" in t for t in text.values())
    assert {f for f, t in text.items() if re.search(r"\baccumulate_point_n\s*\(", t)} == {"qn_linearize.cuh", "qn_tick.cuh", "qn_linearize_debug.hip"}
