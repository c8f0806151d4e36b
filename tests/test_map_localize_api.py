"""The map-localisation calls (qn_localize_default_params, qn_kf_map_crop, qn_kf_map_crop_get, qn_kf_map_localize, qn_kf_map_localize_c2f): the C-ABI surface,
the record layouts, the Python wrappers and the refusal of a null store before any device is touched.  No GPU needed (the refusals that need a store:
tests/test_gpu_map_crop.py, tests/test_gpu_map_localize.py)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, maplocalize as ml
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_localize_default_params", "qn_kf_map_crop", "qn_kf_map_crop_get", "qn_kf_map_localize", "qn_kf_map_localize_c2f"]


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
    i = h.index("typedef struct qn_localize_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "32 bytes", "40 bytes", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "QN_ERR_EMPTY_CLOUD", "32767", "2^32",
              "qn_amd/maplocalize.py", "float(R * R)", "left to right", "no fused multiply-add", "inclusive", "ascending map index", "no atomics", "64 centres per pass",
              "Two host synchronisations", "Four host synchronisations", "rounded to f32", "same f32 bits", "grouped by query", "qn_gicp_align_batch_guess",
              "qn_coarse_to_fine_align_batch", "max_points", "small by construction", "does NOT invalidate", "generation", "COPIES", "Non-finite records are never members",
              "0 0 0 1", "different devices", "next crop or localise call"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_LOCALIZE_SPHERE\s+0", h) and re.search(r"#define\s+QN_LOCALIZE_CYLINDER\s+1", h)
    k = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", k)                                  # the unit took no slot of its own
    for w in ("QN_KF_VERIFY_MAP ", "QN_KF_VERIFY_MAP_C2F", "QN_KF_VERIFY_FROM_MAP"):
        assert w in k, w
    v = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_verify.hip")).read()
    assert '#include "qn_maplocalize.inc"' in v and os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_maplocalize.inc"))
    e = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_engine.hip")).read()
    assert "qn_ctx_int_max_points" in e and "qn_ctx_int_device" in e


def test_record_layouts_and_defaults_are_the_headers():
    P, S = engine.LocalizeParams, engine.LocalizeStats
    assert ctypes.sizeof(P) == 32 and (P.radius.offset, P.leaf.offset, P.score_thr.offset, P.shape.offset, P.reserved.offset) == (0, 8, 16, 24, 28)
    assert ctypes.sizeof(S) == 40
    assert [f for f, _ in S._fields_] == ["n_map", "n_pairs", "n_scans", "n_crops", "passes", "reserved", "crop_points", "generation"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 32]
    p = P(9.0, 7.0, 8.0, 1); p.reserved = 5
    engine.lib().qn_localize_default_params(ctypes.byref(p))
    assert (p.radius, p.leaf, p.score_thr, p.shape, p.reserved) == (35.0, 0.3, 1.5, 0, 0)
    engine.lib().qn_localize_default_params(None)                     # a null pointer is ignored
    d = P()
    assert (d.radius, d.leaf, d.score_thr, d.shape, d.reserved) == (35.0, 0.3, 1.5, 0, 0)
    assert d.twin() == ml.LocalizeParams() == (35.0, 0.3, 1.5, 0)
    assert P(12.0, 0.2, 0.7, 1).twin() == (12.0, 0.2, 0.7, 1)
    assert (engine.QN_LOCALIZE_SPHERE, engine.QN_LOCALIZE_CYLINDER) == (ml.SPHERE, ml.CYLINDER) == (0, 1)
    assert (ml.MAX_CROPS, ml.PASS) == (32767, 64)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.LocalizeParams(); ptr = ctypes.c_void_p(); n = ctypes.c_uint32()
    c = np.zeros((1, 3)); cnt = np.zeros(1, np.uint32); q = np.zeros(1, np.int32); g = np.eye(4).reshape(1, 16).copy(); v = np.zeros(1, np.int32); s = np.zeros(1, np.int32)
    res = (engine.GicpResult * 1)(); Tt = np.zeros((1, 4, 4))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    I = engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_crop(None, P(c), ctypes.c_uint32(1), ctypes.c_double(1.0), ctypes.c_uint32(0), P(cnt)) == I
    assert L.qn_kf_map_crop_get(None, ctypes.c_uint32(0), ctypes.byref(ptr), ctypes.byref(n), None) == I
    assert L.qn_kf_map_localize(None, None, ctypes.byref(p), P(q), P(g), ctypes.c_uint32(1), res, P(v), P(s), None) == I
    assert L.qn_kf_map_localize_c2f(None, None, ctypes.byref(p), P(q), P(g), ctypes.c_uint32(1), res, P(Tt), None, P(v), P(s), None) == I


def test_python_wrappers_and_tools_exist():
    for f in ("map_crop", "map_crop_get", "map_localize", "map_localize_c2f"):
        assert callable(getattr(engine.KeyframeStore, f))
    assert list(inspect.signature(engine.KeyframeStore.map_crop).parameters)[1:] == ["centres", "radius", "shape"]
    assert list(inspect.signature(engine.KeyframeStore.map_localize).parameters)[1:] == ["ctx", "query", "guesses", "params"]
    for f in ("crop_indices", "crop", "guess_f32", "LocalizeParams"):
        assert hasattr(ml, f)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import replay
    finally:
        sys.path.pop(0)
    assert {"localize_every", "localize_radius", "localize_shift", "localize_yaw"} <= set(inspect.signature(replay.run).parameters)
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_localize_time.py"))
    assert os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_localize.hpp"))


def test_the_crop_kernels_have_no_scratch():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_ml_count", "k_scan_rows", "k_ml_compact"):
        rows = [l for l in out.splitlines() if k in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    txt = subprocess.check_output([build_shim("shim_map_localize.cpp", tmp_path)], text=True)
    assert txt.count("refused") == 3 and "qn_kf_map_crop" in txt and "qn_kf_map_localize" in txt and "qn_kf_map_localize_c2f" in txt
    assert "params 32 bytes, stats 40 bytes" in txt
