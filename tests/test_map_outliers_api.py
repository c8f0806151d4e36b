"""The map-outlier calls (qn_outlier_default_params, qn_kf_map_outliers, qn_kf_map_outlier_points, qn_kf_map_remove_outliers): the C-ABI surface, the record
layouts, the Python wrappers and the refusal of a null store before any device is touched.  No GPU needed (the refusals that need a store:
tests/test_gpu_map_outliers.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapoutliers as mo
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_outlier_default_params", "qn_kf_map_outliers", "qn_kf_map_outlier_points", "qn_kf_map_remove_outliers"]


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
    i = h.index("typedef struct qn_outlier_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "24 bytes", "64 bytes", "2^30", "2^16", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "three host synchronisations",
              "half to even", "qn_amd/mapoutliers.py", "std_mul", "ANOTHER INDEX", "0xffffffff", "previous classification intact", "map slot", "non-finite",
              "never removed", "generation", "not measurements"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_OUTLIER_MAX_K\s+32\b", h)


def test_record_layouts_and_defaults_are_the_headers():
    P, S = engine.OutlierParams, engine.OutlierStats
    assert ctypes.sizeof(P) == 24 and (P.radius.offset, P.std_mul.offset, P.k.offset, P.reserved.offset) == (0, 8, 16, 20)
    assert ctypes.sizeof(S) == 64
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56]
    assert [f for f, _ in S._fields_] == ["n", "n_finite", "dense", "sparse", "removed", "quant_exp", "sum_q", "sum_q2", "mean_q", "std_q", "thr_q"]
    p = P(9.0, 7.0, 31); p.reserved = 5
    engine.lib().qn_outlier_default_params(ctypes.byref(p))
    assert (p.radius, p.std_mul, p.k, p.reserved) == (1.0, 2.0, 8, 0)
    engine.lib().qn_outlier_default_params(None)                      # a null pointer is ignored
    d = P()
    assert (d.radius, d.std_mul, d.k, d.reserved) == (1.0, 2.0, 8, 0) and d.twin() == mo.OutlierParams() == (1.0, 2.0, 8)
    assert P(0.5, 1.5, 17).twin() == (0.5, 1.5, 17)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.OutlierParams(); st = engine.OutlierStats(); ptr = ctypes.c_void_p(); n = ctypes.c_uint32()
    assert L.qn_kf_map_outliers(None, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    out = np.zeros(8, np.uint32)
    assert L.qn_kf_map_outlier_points(None, out.ctypes.data_as(ctypes.c_void_p), None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_remove_outliers(None, ctypes.byref(ptr), ctypes.byref(n)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_exist():
    for f in ("map_outliers", "map_remove_outliers"):
        assert callable(getattr(engine.KeyframeStore, f))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import replay
    finally:
        sys.path.pop(0)
    import inspect
    assert {"map_outliers", "outlier_radius", "outlier_k", "outlier_std"} <= set(inspect.signature(replay.run).parameters)


def test_the_selection_kernels_have_no_scratch():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_map_outliers<8>", "k_map_outliers<16>", "k_map_outliers<32>", "k_mo_flag", "k_scan_rows", "k_mo_compact", "k_slot_fold<unsigned long long, 3>",
              "k_cell_gather"):
        rows = [l for l in out.splitlines() if k in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    txt = subprocess.check_output([build_shim("shim_map_outliers.cpp", tmp_path)], text=True)
    assert txt.count("refused") == 2 and "qn_kf_map_outliers" in txt and "qn_kf_map_remove_outliers" in txt and "params 24 bytes, stats 64 bytes" in txt
