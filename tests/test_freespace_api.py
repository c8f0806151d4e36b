"""The range-image and free-space calls (qn_kf_range_set_params / _get_params / _describe / _get, qn_kf_freespace_batch / _points): the C-ABI surface, the record
layouts, the Python wrappers, the C++ helper against the stand-ins, and the refusal of null and bad arguments before any device is touched.  No GPU needed."""
import ctypes
import math
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import engine, freespace as fs, synth
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_kf_range_set_params", "qn_kf_range_get_params", "qn_kf_range_describe", "qn_kf_range_get", "qn_kf_freespace_batch", "qn_kf_freespace_points"]


def test_header_declares_and_library_exports_the_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in SYMBOLS)


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    i = h.index("typedef struct qn_range_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "QN_RANGE_MAX_ROWS = 1024", "QN_RANGE_MAX_COLS = 8192", "32 bytes", "64 bytes", "QN_ERR_INVALID_ARG", "QN_ERR_EMPTY_CLOUD",
              "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "32767", "one host synchronisation", "SEEN THROUGH", "wrapping", "qn_amd/freespace.py", "SENSOR frame"):
        assert w in doc, w


def test_record_layouts_are_the_headers():
    assert ctypes.sizeof(engine.FreespaceDir) == 32 and ctypes.sizeof(engine.Freespace) == 64 and ctypes.sizeof(engine.RangeParams) == 56
    assert engine.Freespace.c_in_q.offset == 32 and engine.FreespaceDir.seen_through.offset == 16
    assert engine.RangeParams.el_lo.offset == 8 and engine.RangeParams.window_rows.offset == 32 and engine.RangeParams.tol_abs.offset == 40
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    m = re.search(r"typedef struct qn_freespace_dir \{ uint32_t ([^;]+); \}", h)
    assert [w.strip() for w in m.group(1).split(",")] == [f for f, _ in engine.FreespaceDir._fields_]


def test_python_wrappers_and_params_exist():
    for name in ("range_set_params", "range_params", "range_describe", "range_images", "freespace_batch", "freespace_points"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name
    d = engine.RangeParams()
    t = fs.Params()
    assert (d.n_rows, d.n_cols, d.el_lo, d.el_hi, d.min_range, d.window_rows, d.window_cols, d.tol_abs, d.tol_rel) == \
           (t.n_rows, t.n_cols, t.el_lo, t.el_hi, t.min_range, t.window_rows, t.window_cols, t.tol_abs, t.tol_rel) == (64, 1800, math.radians(-25.0), math.radians(2.2), 2.0, 1, 1, 0.3, 0.02)
    sen = synth.SpinningLidar(n_beams=32, n_cols=720)
    p = engine.RangeParams.for_sensor(sen, window_cols=2)
    assert (p.n_rows, p.n_cols, p.min_range, p.window_rows, p.window_cols) == (32, 720, 2.0, 1, 2)
    el = sen.elevations(); half = 0.5 * (el[1] - el[0])
    assert abs(p.el_lo - (el[0] - half)) < 1e-12 and abs(p.el_hi - (el[-1] + half)) < 1e-12
    assert p.twin() == fs.Params.for_sensor(sen, window_cols=2) and fs.params_ok(p.twin())
    store = object.__new__(engine.KeyframeStore)                   # the shape checks run before the library is touched: no store, no device needed
    with pytest.raises(ValueError):
        store.freespace_batch([1, 2], [3], np.zeros((2, 4, 4)))
    with pytest.raises(ValueError):
        store.freespace_batch([1, 2], [3, 4], np.zeros((1, 4, 4)))
    with pytest.raises(ValueError):
        store.freespace_points(0, 0)


def test_null_and_bad_arguments_are_refused_without_a_device():
    l = engine.lib()
    u = ctypes.c_uint32
    ids = (ctypes.c_int32 * 1)(0); st = (ctypes.c_int * 1)(); T = (ctypes.c_double * 16)(); out = (engine.Freespace * 1)(); img = (ctypes.c_float * 4)()
    cls = (ctypes.c_uint8 * 4)(); p = engine.RangeParams()
    bad = engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_range_set_params(None, ctypes.byref(p)) == bad and l.qn_kf_range_get_params(None, ctypes.byref(p)) == bad
    assert l.qn_kf_range_describe(None, ids, u(1), st) == bad and l.qn_kf_range_get(None, 0, img, img) == bad
    assert l.qn_kf_freespace_batch(None, ids, ids, T, u(1), out, st) == bad and l.qn_kf_freespace_points(None, u(0), 0, cls) == bad
    # with a non-null (never dereferenced) store: these checks come before the store is looked at
    fake = ctypes.c_void_p(8)
    assert l.qn_kf_range_set_params(fake, None) == bad and l.qn_kf_range_get_params(fake, None) == bad
    for kw in (dict(el_lo=0.3, el_hi=0.2), dict(el_lo=-math.pi / 2), dict(el_hi=math.pi / 2), dict(n_rows=0), dict(n_cols=0), dict(n_rows=1025), dict(n_cols=8193),
               dict(tol_abs=-0.1), dict(tol_rel=float("nan")), dict(min_range=float("inf")), dict(window_rows=64), dict(n_cols=4, window_cols=2), dict(window_cols=0x80000000)):
        q = engine.RangeParams(**kw)
        assert l.qn_kf_range_set_params(fake, ctypes.byref(q)) == bad, kw
        assert not fs.params_ok(q.twin()), kw
    assert l.qn_kf_range_describe(fake, None, u(1), st) == bad and l.qn_kf_range_describe(fake, ids, u(0), st) == bad and l.qn_kf_range_describe(fake, ids, u(1), None) == bad
    for args in ((None, ids, T, u(1), out, st), (ids, None, T, u(1), out, st), (ids, ids, None, u(1), out, st), (ids, ids, T, u(0), out, st), (ids, ids, T, u(1), None, st),
                 (ids, ids, T, u(1), out, None)):
        assert l.qn_kf_freespace_batch(fake, *args) == bad, args
    assert l.qn_kf_freespace_batch(fake, ids, ids, T, u(32768), out, st) == engine.QN_ERR_CAPACITY
    assert l.qn_kf_freespace_points(fake, u(0), 2, cls) == bad and l.qn_kf_freespace_points(fake, u(0), -1, cls) == bad and l.qn_kf_freespace_points(fake, u(0), 0, None) == bad


def test_the_three_kernels_have_no_scratch():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_range_bin", "k_freespace_check", "k_freespace_reduce"):
        rows = [l for l in out.splitlines() if re.search(r"\b%s\b" % k, l)]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    out = build_shim("shim_freespace.cpp", tmp_path)
    txt = subprocess.check_output([out], text=True)
    assert "refused" in txt and "qn_kf_freespace_batch" in txt and "fraction 0.25" in txt
