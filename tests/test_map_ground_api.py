"""The map-ground calls (qn_ground_default_params, qn_kf_map_ground, qn_kf_map_ground_points, qn_kf_map_ground_grid, qn_kf_map_keep_classes): the C-ABI surface,
the record layouts, the Python wrappers and the refusal of a null store before any device is touched.  No GPU needed (the refusals that need a store:
tests/test_gpu_map_ground.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapground as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_ground_default_params", "qn_kf_map_ground", "qn_kf_map_ground_points", "qn_kf_map_ground_grid", "qn_kf_map_keep_classes"]
KERNELS = ("k_mg_extent", "k_mg_extent_sum", "k_mg_bin", "k_mg_seed", "k_mg_relax", "k_mg_classify", "k_mg_occ_count", "k_slot_fold<unsigned int, 1>",
           "k_slot_fold<unsigned int, 2>", "k_slot_fold<unsigned int, 5>", "k_mg_keep_flag", "k_scan_rows", "k_mo_compact<HIP_vector_type<float, 4u> >")


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
    i = h.index("typedef struct qn_ground_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "40 bytes", "80 bytes", "2^30", "2^10", "2^26", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "QN_ERR_INTERNAL",
              "Host synchronisations: 2 + ceil(rounds / 8)", "half to even", "qn_amd/mapground.py", "not measurements", "previous results intact", "map slot",
              "generation", "row-major", "OVERHEAD points do not", "max(W, H) + 2", "rounds"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_GROUND_MAX_CELLS\s+\(1u << 26\)", h) and re.search(r"QN_ERR_INTERNAL\s*=\s*7\b", h)
    for k, name in enumerate(("NONE", "GROUND", "OBSTACLE", "OVERHEAD", "BELOW")):
        assert re.search(r"#define\s+QN_GROUND_%s\s+%d\b" % (name, k), h) and getattr(engine, "QN_GROUND_" + name) == getattr(mg, name) == k
    assert engine.QN_ERR_INTERNAL == 7 and engine.lib().qn_status_str(7).decode().startswith("internal error")
    assert engine.QN_GROUND_MAX_CELLS == mg.MAX_CELLS == 1 << 26
    unit = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", unit) and re.search(r"#define\s+QN_KF_INT_EXT_GROUND\s+9\b", unit)


def test_record_layouts_and_defaults_are_the_headers():
    P, S, G = engine.GroundParams, engine.GroundStats, engine.GroundGrid
    assert ctypes.sizeof(P) == 40 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 8, 16, 24, 32, 36]
    assert ctypes.sizeof(S) == 80 and [getattr(S, f).offset for f, _ in S._fields_] == list(range(0, 80, 4))
    assert [f for f, _ in S._fields_][:18] == list(mg.GroundStats._fields) and [f for f, _ in S._fields_][18:] == ["rounds", "reserved"]
    assert ctypes.sizeof(G) == 40 and [getattr(G, f).offset for f, _ in G._fields_] == [0, 8, 16, 24, 28, 32, 36]
    assert [f for f, _ in G._fields_][:6] == list(mg.GridInfo._fields)
    p = P(9.0, 7.0, 3.0, 1.0, 31); p.reserved = 5
    engine.lib().qn_ground_default_params(ctypes.byref(p))
    assert (p.cell, p.max_slope, p.ground_tol, p.clearance, p.min_points, p.reserved) == (0.5, 0.3, 0.2, 2.0, 1, 0)
    engine.lib().qn_ground_default_params(None)                       # a null pointer is ignored
    d = P()
    assert d.twin() == mg.GroundParams() == (0.5, 0.3, 0.2, 2.0, 1) and d.reserved == 0
    assert P(1.0, 0.5, 0.1, 3.0, 4).twin() == (1.0, 0.5, 0.1, 3.0, 4)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.GroundParams(); st = engine.GroundStats(); g = engine.GroundGrid(); ptr = ctypes.c_void_p(); n = ctypes.c_uint32()
    out = np.zeros(8, np.uint32)
    assert L.qn_kf_map_ground(None, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_ground_points(None, out.ctypes.data_as(ctypes.c_void_p), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_ground_grid(None, ctypes.byref(g), None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_keep_classes(None, 2, ctypes.byref(ptr), ctypes.byref(n)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_exist():
    for f in ("map_ground", "map_ground_grid", "map_keep_classes"):
        assert callable(getattr(engine.KeyframeStore, f))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import replay
    finally:
        sys.path.pop(0)
    import inspect
    assert {"occupancy_grid", "grid_cell", "max_slope", "ground_tol", "clearance", "drop_ground"} <= set(inspect.signature(replay.run).parameters)
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_ground_time.py"))


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows
    # one source: the scan in the four units that launch it (qn_mapoutliers, qn_mapground, qn_staticmap, qn_verify) and in the primitives' test entry
    # (qn_map_selftest, which launches it on caller-supplied rows), the record compaction only in the two that filter the slot - the static-map unit, which lists
    # voxels, carries none, and neither does the test entry
    assert len([l for l in out.splitlines() if "::k_scan_rows(" in l]) == 5 and len([l for l in out.splitlines() if "::k_mo_compact<" in l]) == 2


def test_no_floating_point_in_the_kernels_behind_the_quantisation():
    """only the extent and the bin kernels (before and at the quantisation) may name a floating-point type; the count tail, the fold of the slots, the scan and the rank that
    the others share live in qn_map_compact.cuh"""
    src = "".join(open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", f)).read() for f in ("qn_map_compact.cuh", "qn_mapground.hip"))
    for k in ("k_mg_seed", "k_mg_relax", "k_mg_classify", "k_mg_occ_count", "k_slot_fold", "block_count", "k_mg_keep_flag", "lane_rank", "block_rank", "scan_row",
              "k_scan_rows"):
        i = src.index(" " + k + "(")
        body = src[i:src.index("\n}\n", i)]
        assert not re.search(r"\b(float|double|float4)\b", body), k
