"""The static-map calls (qn_static_default_params, qn_kf_static_classify / _points, qn_kf_build_map_static): the C-ABI surface, the record layout, the Python
wrappers, the C++ helper against the stand-ins, and the refusal of null and bad arguments before any device is touched.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import engine, staticmap as sm
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_static_default_params", "qn_kf_static_classify", "qn_kf_static_points", "qn_kf_build_map_static"]


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
    i = h.index("typedef struct qn_static_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "8 bytes", "255", "QN_ERR_INVALID_ARG", "QN_ERR_EMPTY_CLOUD", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "one host synchronisation", "SEEN THROUGH",
              "qn_amd/staticmap.py", "SENSOR frame", "min_see_through", "agree_weight", "never removed", "map slot"):
        assert w in doc, w


def test_record_layout_and_defaults_are_the_headers():
    assert ctypes.sizeof(engine.StaticParams) == 8 and engine.StaticParams.agree_weight.offset == 4
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    m = re.search(r"typedef struct qn_static_params \{ uint32_t ([^;]+); \}", h)
    assert [w.strip() for w in m.group(1).split(",")] == [f for f, _ in engine.StaticParams._fields_]
    p = engine.StaticParams(7, 9)
    engine.lib().qn_static_default_params(ctypes.byref(p))
    d, t = engine.StaticParams(), sm.StaticParams()
    assert (p.min_see_through, p.agree_weight) == (d.min_see_through, d.agree_weight) == (t.min_see_through, t.agree_weight) == (2, 1)
    assert engine.StaticParams.from_twin(sm.StaticParams(3, 0)).twin() == sm.StaticParams(3, 0)
    engine.lib().qn_static_default_params(None)                    # (a null pointer is ignored)


def test_python_wrappers_check_their_shapes_without_a_store():
    for name in ("static_classify", "static_points", "build_map_static"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name
    store = object.__new__(engine.KeyframeStore)                   # the shape checks run before the library is touched: no store, no device needed
    P = np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(ValueError):
        store.static_classify([0, 1], P[:1])
    with pytest.raises(ValueError):
        store.static_classify([0, 1], P, witnesses=([0, 1], [1]))
    with pytest.raises(ValueError):
        store.static_classify([0, 1], P, witnesses=([0, 1, 3], [1, 0]))
    with pytest.raises(ValueError):
        store.static_classify([0, 1], P, max_k=256)
    with pytest.raises(ValueError):
        store.static_points(0)


def test_null_and_bad_arguments_are_refused_without_a_device():
    l = engine.lib()
    u = ctypes.c_uint32
    ids = (ctypes.c_int32 * 1)(0); st = (ctypes.c_int * 1)(); P = (ctypes.c_double * 16)(); off = (u * 2)(0, 0); wit = (u * 1)(0); rem = (u * 1)()
    b = (ctypes.c_uint8 * 4)(); p = engine.StaticParams(); ptr = ctypes.c_void_p(); n = u()
    bad = engine.QN_ERR_INVALID_ARG
    pp = ctypes.byref(p)
    assert l.qn_kf_static_classify(None, ids, P, u(1), off, wit, pp, rem, st) == bad
    assert l.qn_kf_static_points(None, u(0), b, b, b) == bad
    assert l.qn_kf_build_map_static(None, ctypes.c_double(0.3), ctypes.byref(ptr), ctypes.byref(n)) == bad
    # with a non-null (never dereferenced) store: these checks come before the store is looked at
    fake = ctypes.c_void_p(8)
    for args in ((None, P, u(1), off, wit, pp, rem, st), (ids, None, u(1), off, wit, pp, rem, st), (ids, P, u(0), off, wit, pp, rem, st), (ids, P, u(1), None, wit, pp, rem, st),
                 (ids, P, u(1), off, wit, None, rem, st), (ids, P, u(1), off, wit, pp, None, st), (ids, P, u(1), off, wit, pp, rem, None)):
        assert l.qn_kf_static_classify(fake, *args) == bad, args
    zero = engine.StaticParams(0, 1)
    assert l.qn_kf_static_classify(fake, ids, P, u(1), off, wit, ctypes.byref(zero), rem, st) == bad
    assert l.qn_kf_static_classify(fake, ids, P, u(1), (u * 2)(1, 0), wit, pp, rem, st) == bad            # a non-monotone wit_off
    assert l.qn_kf_static_classify(fake, ids, P, u(1), (u * 2)(0, 1), None, pp, rem, st) == bad           # witnesses listed, no list
    assert l.qn_kf_static_points(fake, u(0), None, None, None) == bad
    for leaf in (0.0, -0.3, float("nan")):
        assert l.qn_kf_build_map_static(fake, ctypes.c_double(leaf), ctypes.byref(ptr), ctypes.byref(n)) == bad
    assert l.qn_kf_build_map_static(fake, ctypes.c_double(0.3), None, ctypes.byref(n)) == bad and l.qn_kf_build_map_static(fake, ctypes.c_double(0.3), ctypes.byref(ptr), None) == bad


def test_the_three_kernels_have_no_scratch():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_static_vote", "k_static_scan", "k_static_compact"):
        rows = [l for l in out.splitlines() if re.search(r"\b%s\b" % k, l)]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_both_range_image_units_share_one_projection():
    src = {f: open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", f)).read() for f in ("qn_freespace.hip", "qn_staticmap.hip", "qn_range.cuh")}
    for f in ("qn_freespace.hip", "qn_staticmap.hip"):
        assert '#include "qn_range.cuh"' in src[f] and "bool fs_project(" not in src[f] and "fs_stage(const" not in src[f], f
    assert "bool fs_project(" in src["qn_range.cuh"] and "fs_window(" in src["qn_range.cuh"]


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    out = build_shim("shim_static_map.cpp", tmp_path)
    txt = subprocess.check_output([out], text=True)
    assert "witnesses 1 4 0 1 3 2 1 2" in txt and txt.count("refused") == 2 and "qn_kf_static_classify" in txt and "qn_kf_build_map_static" in txt
