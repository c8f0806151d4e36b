"""The device builds of the Gauss-Newton step's small dense f64 routines (csrc/qn_step_math.cuh and d_propose through qn_debug_step_math, one problem per
lane) against the 50-digit mpmath references on the families of tests/step_math_cases.py: the bounds and contracts of tests/step_math_checks.py, the same ones
tests/test_step_math_cpu.py asks of the host build.  Then a rerun (same bytes), the batches with non-finite and singular rows, the refusals, and the device
against the host build of the same text: the solves of `diagonal` (the proposal's step d and path with them; its delta and xi go through sin and cos) and
`conv` - where nothing rounds - must agree bit for bit; elsewhere the results that differ in any bit are counted and printed per routine, not asserted: the
device's sin and cos are another library's, and nothing in the product depends on the rest agreeing."""
import ctypes as C
import numpy as np
import pytest
import step_math_cases as sc
import step_math_checks as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from qn_amd import engine
    c = engine.Context(1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device(ctx):
    """run(which, records) on the device, each (routine, batch) computed once"""
    cache = {}

    def run(which, rec):
        key = (which, rec.shape, rec.tobytes())
        if key not in cache:
            out = ctx.debug_step_math(which, rec)
            out.setflags(write=False)
            cache[key] = out
        return cache[key]
    return run


@pytest.mark.parametrize("name", sc.SOLVE_FINITE)
def test_solve_family_within_the_bounds(device, name):
    chk.check_solves(name, device, label="device")


def test_so3_exp_within_the_bounds(device):
    chk.check_so3(device, label="device")


def test_m3_inverse_within_the_bounds(device):
    chk.check_inv3(device, label="device")


def test_is_converged_equals_the_restated_expression(device):
    chk.check_conv(device, label="device")


def test_rerun_returns_the_same_bytes(ctx, device):
    for name, which, rec in chk.all_batches():
        again = ctx.debug_step_math(which, rec)
        assert chk.same_bits(again, device(which, rec)), (name, chk.ROUTINE[which])


def test_non_finite_and_singular_rows_leave_their_neighbours_alone(ctx):
    chk.check_isolation(ctx.debug_step_math)                         # (debug_step_math raises unless the call returns QN_OK)


def test_device_against_the_host_build(device):
    diff = chk.count_differences(device, chk.host)
    for key in (("diagonal", "d_ldlt_solve6_fast"), ("diagonal", "d_ldlt_solve6"), ("diagonal", "d_propose d"), ("conv", "d_is_converged")):
        assert diff[key][0] == 0 and diff[key][1] > 0, (key, diff[key])


def test_refusals_and_the_empty_batch(ctx):
    from qn_amd import engine
    L = ctx._l
    L.qn_debug_step_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    a = np.ones(59); out = np.full(39, 7.0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for args in [(None, 0, p(a), 1, p(out)), (ctx.h, 0, None, 1, p(out)), (ctx.h, 0, p(a), 1, None), (ctx.h, 6, p(a), 1, p(out)), (ctx.h, -1, p(a), 1, p(out)),
                 (ctx.h, 3, None, 0, p(out)), (ctx.h, 2, p(a), (1 << 20) + 1, p(out))]:
        assert L.qn_debug_step_math(*args) == engine.QN_ERR_INVALID_ARG, args[1:4]
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        ctx.debug_step_math(6, a)
    for which, (si, so) in enumerate(sc.STRIDES):
        assert L.qn_debug_step_math(ctx.h, which, p(a), 0, p(out)) == engine.QN_OK and (out == 7.0).all()       # n == 0: nothing written
        assert ctx.debug_step_math(which, np.zeros((0, si))).shape == (0, so)
    R = ctx.debug_step_math(chk.SO3, np.zeros((1, 3)))
    assert np.array_equal(R.reshape(3, 3), np.eye(3))
    X = ctx.debug_step_math(chk.INV3, np.diag([2.0, 4.0, 0.5]).reshape(1, 9))
    assert np.array_equal(X.reshape(3, 3), np.diag([0.5, 0.25, 2.0]))
