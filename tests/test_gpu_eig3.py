"""The device builds of the two 3 x 3 symmetric eigen solvers (csrc/qn_eig3.cuh through qn_debug_eig3, one matrix per lane) against the 50-digit mpmath
reference on the families of tests/eig3_cases.py: the bounds and contracts of tests/eig3_checks.py, the same ones tests/test_eig3_cpu.py asks of the host
build.  Then a rerun (same bytes), the poisoned batch, the refusals, and the device against the host build of the same text: the `diagonal` family - where no
arithmetic happens - must agree bit for bit; elsewhere the outputs that differ in any bit are counted and printed, not asserted: the kernels' comments assume
an IEEE f64 divide and square root on the device, and nothing in the product depends on it."""
import ctypes as C
import numpy as np
import pytest
import eig3_cases as ec
import eig3_checks as chk

pytestmark = pytest.mark.gpu
SOLVERS = [chk.JACOBI, chk.SYM]
IDS = [chk.SOLVER[s] for s in SOLVERS]


@pytest.fixture(scope="module")
def ctx():
    from qn_amd import engine
    c = engine.Context(1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device(ctx):
    """(which, family) -> the device's (w, V) of every batch, computed once"""
    cache = {}

    def run(which, name):
        if (which, name) not in cache:
            cache[which, name] = tuple(ctx.debug_eig3(which, a6) for a6 in ec.family(name))
        return cache[which, name]
    return run


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ec.FINITE)
@pytest.mark.parametrize("which", SOLVERS, ids=IDS)
def test_family_within_the_bounds(device, which, name):
    batches = iter(device(which, name))
    chk.check_family(which, name, lambda a6: next(batches))


@pytest.mark.parametrize("which", SOLVERS, ids=IDS)
def test_rerun_returns_the_same_bytes(ctx, device, which):
    for name in ("random", "iso", "seams"):
        for a6, (w, V) in zip(ec.family(name), device(which, name)):
            w2, V2 = ctx.debug_eig3(which, a6)
            assert np.array_equal(_bits(w), _bits(w2)) and np.array_equal(_bits(V), _bits(V2)), name


@pytest.mark.parametrize("which", SOLVERS, ids=IDS)
def test_non_finite_rows_leave_their_neighbours_alone(ctx, which):
    chk.check_non_finite(which, lambda a6: ctx.debug_eig3(which, a6))          # (debug_eig3 raises unless the call returns QN_OK)


@pytest.mark.parametrize("which", SOLVERS, ids=IDS)
def test_device_against_the_host_build(device, which):
    total = 0
    for name in ec.FINITE:
        differ = n = 0
        for (w, V), host in zip(device(which, name), chk.host_family(name)):
            hw, hV = host[which]
            differ += int(((_bits(w) != _bits(hw)).any(axis=1) | (_bits(V) != _bits(hV)).any(axis=(1, 2))).sum()); n += len(w)
        print("%-15s %-13s %d of %d matrices differ from the host build in some bit" % (chk.SOLVER[which], name, differ, n))
        if name == "diagonal":
            assert differ == 0
        total += differ
    print("%-15s %d matrices in all differ from the host build" % (chk.SOLVER[which], total))


def test_refusals_and_the_empty_batch(ctx):
    from qn_amd import engine
    L = ctx._l
    L.qn_debug_eig3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    a = np.array([[2.0, 0.0, 0.0, 1.0, 0.0, 3.0]]); w = np.full(3, 7.0); V = np.full(9, 7.0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for args in [(None, 0, p(a), 1, p(w), p(V)), (ctx.h, 0, None, 1, p(w), p(V)), (ctx.h, 0, p(a), 1, None, p(V)), (ctx.h, 0, p(a), 1, p(w), None),
                 (ctx.h, 2, p(a), 1, p(w), p(V)), (ctx.h, -1, p(a), 1, p(w), p(V)), (ctx.h, 1, None, 0, p(w), p(V))]:
        assert L.qn_debug_eig3(*args) == engine.QN_ERR_INVALID_ARG, args[1:4]
    assert (w == 7.0).all() and (V == 7.0).all()
    for which in SOLVERS:
        assert L.qn_debug_eig3(ctx.h, which, p(a), 0, p(w), p(V)) == engine.QN_OK and (w == 7.0).all() and (V == 7.0).all()       # n == 0: nothing written
        we, Ve = ctx.debug_eig3(which, np.zeros((0, 6)))
        assert we.shape == (0, 3) and Ve.shape == (0, 3, 3)
    w1, V1 = ctx.debug_eig3(chk.JACOBI, a)
    assert np.array_equal(w1, [[2.0, 1.0, 3.0]]) and np.array_equal(V1[0], np.eye(3))
    w1, V1 = ctx.debug_eig3(chk.SYM, a)
    assert np.array_equal(w1, [[3.0, 2.0, 1.0]]) and np.array_equal(V1[0], [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
