"""The host build of the Gauss-Newton step's small dense f64 routines (csrc/qn_step_math.cuh through tests/step_math_host.cpp: the text the kernels compile)
against 50-digit mpmath references on the families of tests/step_math_cases.py: the 6 x 6 solves' backward and forward errors, the paths, the exact cases and
the composition of the proposal, d_so3_exp, m3_inverse and d_is_converged (tests/step_math_checks.py has the metrics and where every bound comes from).  The
same program built with the address and undefined-behaviour sanitizers runs every family, the non-finite ones included, and must return what the plain build
returns; the oracle's so3_exp and ldlt_solve6, which every registration comparison is pinned to, go through the same bounds.  Each family's maxima are printed.
No GPU; the device build: tests/test_gpu_step_math.py."""
import ctypes as C
import numpy as np
import pytest
import step_math_cases as sc
import step_math_checks as chk


@pytest.mark.parametrize("name", sc.SOLVE_FINITE)
def test_solve_family_within_the_bounds(name):
    top, counts = chk.check_solves(name, chk.host, label="host")
    if name in ("spd", "seams", "gicp"):
        assert counts["forward"] >= counts["n"] // 2                 # (well conditioned: the forward error is compared, not only the residual)
    if name == "graded":
        assert counts["forward"] >= 2 * sc.N and counts["refused"] == 0


def test_so3_exp_within_the_bounds():
    chk.check_so3(chk.host, label="host")


def test_m3_inverse_within_the_bounds():
    top = chk.check_inv3(chk.host, label="host")
    assert top["parallel"][2] >= 900.0 and top["spd"][2] >= 1e5      # the families reach the conditioning they are there for


def test_is_converged_equals_the_restated_expression():
    assert 20 <= chk.check_conv(chk.host, label="host") <= len(sc.conv()) - 20


def test_non_finite_and_singular_rows_leave_their_neighbours_alone():
    chk.check_isolation(chk.host_run)


def test_sanitizer_build_runs_every_family_and_agrees():
    """address + undefined-behaviour sanitizers on the stand-alone host program, every finding fatal: every batch of every family, the poisoned ones included, ends
    with exit status 0 (host_run checks it) and the results of the plain build"""
    diff = chk.count_differences(lambda w, r: chk.host_run(w, r, sanitize=True), chk.host, labels=("sanitizer", "host"))
    assert {name for name, _ in diff} == set(sc.SOLVE_FAMILIES) | {"so3", "inv3", "conv"} and all(k == 0 for k, _ in diff.values()), diff


@pytest.mark.parametrize("name", sc.SOLVE_FINITE)
def test_oracle_ldlt_solve6_within_the_bounds(name):
    """the oracle's pivoted solve under the bounds of the routine it restates, and how far the two are apart"""
    worst = dict(backward=0.0, forward=0.0); differ = n = 0
    for rec, ref in zip(sc.solve_family(name), chk.solve_reference(name)):
        x = chk.oracle(chk.PIVOTED, rec)
        assert np.isfinite(x).all()
        for metric, v in (("backward", chk.backward_error(rec, x)), ("forward", chk.forward_error(x, ref))):
            worst[metric] = max(worst[metric], chk._worst(v[~np.isnan(v)]))
        differ += int((chk.bits(x) != chk.bits(chk.host(chk.PIVOTED, rec))).any(axis=1).sum()); n += len(rec)
    print("oracle   %-9s ldlt_solve6 max: backward %.3g forward %.3g (bound %g); %d of %d differ from the host build of d_ldlt_solve6 in some bit" % (name, worst["backward"], worst["forward"], chk.K_SOLVE, differ, n))
    assert worst["backward"] <= chk.K_SOLVE and worst["forward"] <= chk.K_SOLVE, worst
    assert differ == 0, "the oracle's ldlt_solve6 and d_ldlt_solve6 are the same arithmetic"


def test_oracle_so3_exp_within_the_bounds():
    chk.check_so3(chk.oracle, label="oracle")
    om, _ = sc.so3()
    a, b = chk.oracle(chk.SO3, om), chk.host(chk.SO3, om)
    assert not ((chk.bits(a) != chk.bits(b)) & ~(np.isnan(a) & np.isnan(b))).any(), "the oracle's so3_exp and d_so3_exp are the same arithmetic"


def test_device_entry_is_exported_wrapped_and_refuses_a_null_context():
    from qn_amd import engine
    import test_capi_symbols
    assert "qn_debug_step_math" in test_capi_symbols.declared_symbols() and callable(engine.Context.debug_step_math)
    assert engine.Context.STEP_MATH_STRIDES == sc.STRIDES
    L = engine.lib()
    L.qn_debug_step_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    a = np.ones(59); out = np.full(39, 7.0)
    for which in range(6):
        assert L.qn_debug_step_math(None, which, a.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == engine.QN_ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_the_families_are_what_they_say():
    assert [len(a) for a in sc.solve_family("seams")] == list(sc.SEAMS) == [1, 63, 64, 65, 129]
    for name in sc.SOLVE_FINITE:
        for rec in sc.solve_family(name):
            A, lam, b = sc.split(rec)
            assert np.isfinite(rec).all() and np.array_equal(A, np.swapaxes(A, 1, 2)) and (len(rec) == sc.N or name in ("seams", "diagonal"))
    for c, (cond, _) in zip(sc.GRADES, chk.solve_reference("graded")):
        lg = np.log10(cond[np.isfinite(cond)])
        assert c <= 12 and len(lg) == sc.N and (np.abs(lg - c) < 1.0).all() or c == 15 and not np.isfinite(cond).any(), (c, lg.min(), lg.max())
    (cond, _), = chk.solve_reference("spd")
    assert cond.min() >= 1.0 and cond.max() <= 6e3
    gicp = dict(zip(sc.LAYOUTS, chk.solve_reference("gicp")))
    assert 1e5 <= np.median(gicp["plane"][0]) <= 1e6 and not np.isfinite(gicp["line"][0]).any() and np.isfinite(gicp["box"][0]).all() and np.isfinite(gicp["walls"][0]).all()
    line = sc.solve_family("gicp")[sc.LAYOUTS.index("line")]
    A, _, b = sc.split(line)
    assert not A[:, 0, :].any() and not A[:, :, 0].any() and not b[:, 0].any() and (np.linalg.matrix_rank(A[:, 1:, 1:]) == 5).all()
    A, _, b = sc.split(sc.solve_family("ranks")[0])
    assert all(np.linalg.matrix_rank(A[i]) <= sc.rank_of(i) for i in range(len(A))) and (A == np.round(A)).all() and not np.isfinite(chk.solve_reference("ranks")[0][0]).any()
    A, lam, _ = sc.split(sc.solve_family("lm-shift")[0])
    assert (np.linalg.matrix_rank(A) == 3).all() and len(set(np.round(np.log10(lam / np.abs(np.diagonal(A, axis1=1, axis2=2)).max(axis=1))))) == 4
    om, tags = sc.so3()
    theta, _ = chk.so3_reference()
    assert {"zero", "tiny", "seam-lo", "seam-hi", "small", "one", "pi", "2pi", "large", "axis", "random", "non-finite"} == set(tags) and theta[np.array(tags) == "large"].max() >= 9e14
    for name, (cond, _, _) in zip(sc.INV3_BATCHES, chk.inv3_reference()):
        assert np.isfinite(cond).all() == (name != "singular")


def test_the_checks_see_a_small_error():
    """the checks have teeth: the host build's results pass, and with one entry off by a part in 1e12 (the solves, well conditioned), by 64 (1 + theta) eps
    (d_so3_exp) or by a part in 1e9 (m3_inverse, condition 1e3) they miss their bounds"""
    (rec,), (ref,) = sc.solve_family("spd"), chk.solve_reference("spd")
    x = chk.host(chk.PIVOTED, rec).copy()
    assert chk._worst(chk.backward_error(rec, x)) <= chk.K_SOLVE and chk._worst(chk.forward_error(x, ref)) <= chk.K_SOLVE
    x[:, 2] *= 1.0 + 1e-12
    assert np.nanmin(chk.backward_error(rec, x)) > 0 and chk._worst(chk.backward_error(rec, x)) > chk.K_SOLVE and chk._worst(chk.forward_error(x, ref)) > 1.0
    om, _ = sc.so3()
    theta, _ = chk.so3_reference()
    R = chk.host(chk.SO3, om).copy()
    R[:, 1] += 64.0 * (1.0 + np.nan_to_num(theta)) * chk.EPS
    acc, orth, _ = chk.so3_metrics(R)
    assert np.nanmin(acc) > chk.K_SO3
    rec = sc.inv3()[sc.INV3_BATCHES.index("parallel")]
    bad = lambda w, r: chk.host(w, r) * (1.0 + 1e-9 * (np.arange(9) == 4))
    with pytest.raises(AssertionError):
        chk.check_inv3(bad, quiet=True)

    def with_fmax(which, rec):                                       # fmax in place of the ternary: a NaN ratio of the rotation is dropped
        want = chk.converged_expected(rec)
        with np.errstate(all="ignore"):
            want[:, 0] = np.fmax(want[:, 1] / rec[:, 16], want[:, 2] / rec[:, 17]) < 1.0
        return want
    with pytest.raises(AssertionError):
        chk.check_conv(with_fmax, quiet=True)
