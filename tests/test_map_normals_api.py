"""The map-normals calls (qn_normal_default_params, qn_kf_map_normals, qn_kf_download_map_normals, qn_kf_map_moments): the C-ABI surface, the record layout,
the Python wrappers and the refusal of a null store before any device is touched.  No GPU needed (the refusals that need a store: tests/test_gpu_map_normals.py)."""
import ctypes
import os
import subprocess
import numpy as np
from qn_amd import engine, mapnormals as mn
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_normal_default_params", "qn_kf_map_normals", "qn_kf_download_map_normals", "qn_kf_map_moments"]


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
    i = h.index("typedef struct qn_normal_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "16 bytes", "2^21", "2^20", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "two host synchronisations", "half to even",
              "qn_amd/mapnormals.py", "min_neighbors", "lowest index", "previous results intact", "map slot", "non-finite"):
        assert w in doc, w


def test_record_layout_and_defaults_are_the_headers():
    assert ctypes.sizeof(engine.NormalParams) == 16 and engine.NormalParams.min_neighbors.offset == 8 and engine.NormalParams.reserved.offset == 12
    p = engine.NormalParams(9.0, 77); p.reserved = 5
    engine.lib().qn_normal_default_params(ctypes.byref(p))
    assert (p.radius, p.min_neighbors, p.reserved) == (0.6, 5, 0)
    engine.lib().qn_normal_default_params(None)                       # a null pointer is ignored
    d = engine.NormalParams()
    assert (d.radius, d.min_neighbors, d.reserved) == (0.6, 5, 0) and d.twin() == mn.NormalParams() == (0.6, 5)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.NormalParams(); ptr = ctypes.c_void_p(); n = ctypes.c_uint32()
    assert L.qn_kf_map_normals(None, ctypes.byref(p), None, ctypes.c_uint32(0), ctypes.byref(ptr), ctypes.byref(n)) == engine.QN_ERR_INVALID_ARG
    out = np.zeros(8, np.float32)
    assert L.qn_kf_download_map_normals(None, out.ctypes.data_as(ctypes.c_void_p), None, None) == engine.QN_ERR_INVALID_ARG
    s = np.zeros(6, np.int64)
    assert L.qn_kf_map_moments(None, s.ctypes.data_as(ctypes.c_void_p), None) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_exist():
    for f in ("map_normals", "map_moments"):
        assert callable(getattr(engine.KeyframeStore, f))


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    txt = subprocess.check_output([build_shim("shim_map_normals.cpp", tmp_path)], text=True)
    assert txt.count("refused") == 1 and "qn_kf_map_normals" in txt and "record 48 bytes" in txt
