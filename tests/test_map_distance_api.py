"""The distance-field calls (qn_distance_default_params, qn_kf_map_distance, qn_kf_map_distance_grid, qn_kf_map_distance_slice, qn_kf_map_distance_query): the
C-ABI surface, the record layouts, the Python wrappers, the place of the device code, the refusal of a null store before any device is touched, and the shim
program.  No GPU needed (the refusals that need a store: tests/test_gpu_map_distance.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapdistance as md
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
SYMBOLS = ["qn_distance_default_params", "qn_kf_map_distance", "qn_kf_map_distance_grid", "qn_kf_map_distance_slice", "qn_kf_map_distance_query"]
KERNELS = ("k_md_x", "k_md_axis<false>", "k_md_axis<true>", "k_slot_max<unsigned int>", "k_dg_slice<unsigned short, (anonymous namespace)::op_min>", "k_md_query", "k_slot_fold<unsigned int, 3>",
           "k_slot_fold<unsigned long long, 1>")


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
    i = h.index("#define QN_DIST_FAR")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("qn_amd/mapdistance.py", "csrc/qn_mapdistance.inc", "bit for bit", "site_mask", "1 << QN_OCC_OCCUPIED", "QN_OCC_UNKNOWN", "Nothing outside the grid is a site",
              "max_dist^2", "65025", "16 bytes", "32 bytes", "2 W H D bytes", "not measurements", "sites + reached + far == W H D", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY",
              "QN_ERR_HIP", "previous field intact", "0 x 0 x 0", "next successful qn_kf_map_occupancy", "One host synchronisation", "iz_lo > iz_hi", "half to even",
              "no contraction", "1024.0", "2^20", "QN_DIST_OUTSIDE", "No atomics", "every per-axis offset <= max_dist"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_DIST_FAR\s+0xffffu", h) and re.search(r"#define\s+QN_DIST_MAX_RADIUS\s+255u", h) and re.search(r"#define\s+QN_DIST_OUTSIDE\s+0xffu", h)
    assert (engine.QN_DIST_FAR, engine.QN_DIST_MAX_RADIUS, engine.QN_DIST_OUTSIDE) == (md.FAR, md.MAX_RADIUS, md.OUTSIDE) == (0xffff, 255, 0xff)
    assert h.index("typedef struct qn_distance_params") > h.index("int  qn_kf_map_occupancy_slice")      # behind the occupancy section it builds on


def test_record_layouts_and_defaults_are_the_headers():
    P, S = engine.DistanceParams, engine.DistanceStats
    assert ctypes.sizeof(P) == 16 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8]
    assert ctypes.sizeof(S) == 32 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 24]
    assert [f for f, _ in S._fields_ if f != "reserved"] == list(md.DistanceStats._fields)
    assert [f for f, _ in P._fields_ if f != "reserved"] == list(md.DistanceParams._fields)
    p = P(3, 77); p.reserved[1] = 5
    engine.lib().qn_distance_default_params(ctypes.byref(p))
    assert (p.site_mask, p.max_dist, list(p.reserved)) == (1 << engine.QN_OCC_OCCUPIED, 16, [0, 0])
    engine.lib().qn_distance_default_params(None)                      # a null pointer is ignored
    d = P()
    assert d.twin() == md.DistanceParams() == (4, 16) and list(d.reserved) == [0, 0]
    assert P(5, 255).twin() == (5, 255)
    s = S(); s.sites, s.reached, s.far, s.max_d2, s.sum_d2 = 1, 2, 3, 4, 1 << 40
    assert s.twin() == md.DistanceStats(1, 2, 3, 4, 1 << 40)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.DistanceParams(); st = engine.DistanceStats(); g = engine.OccupancyGrid()
    out = np.zeros(8, np.uint16); cls = np.zeros(8, np.uint8); xyz = np.zeros(3)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_distance(None, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_grid(None, ctypes.byref(g), ctypes.byref(p), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_slice(None, 0, 1, pp(out)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_distance_query(None, pp(xyz), 1, pp(out), pp(cls)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_and_tools_exist():
    for f in ("map_distance", "map_distance_grid", "map_distance_slice", "map_distance_query"):
        assert callable(getattr(engine.KeyframeStore, f))
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_distance_time.py"))
    assert os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_distance.hpp"))


def test_the_device_code_hangs_on_the_occupancy_state():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert unit.index('#include "qn_mapdistance.inc"') > unit.index('#include "qn_mapoccupancy.inc"')
    internal = open(os.path.join(CSRC, "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", internal) and "DIST" not in internal      # no slot of its own
    occ = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    state = occ[occ.index("struct OccState {"):occ.index("};", occ.index("struct OccState {"))]
    assert "DistState" in state
    inc = open(os.path.join(CSRC, "qn_mapdistance.inc")).read()
    assert "atomic" not in inc and "qn_amd/mapdistance.py" in inc
    call = inc[inc.index('extern "C" int qn_kf_map_distance('):inc.index('extern "C" int qn_kf_map_distance_grid(')]
    assert len(re.findall(r"hipStreamSynchronize", call)) == 1
    assert "block_count(" in inc and "k_slot_fold<" in inc
    grid = open(os.path.join(CSRC, "qn_dense_grid.cuh")).read()      # the statistics tail and its folds are the dense grid's, shared with the route
    assert "dg_block_stats(" in inc and "dg_fold_stats(" in inc and "atomic" not in grid
    tail = grid[grid.index(" dg_block_stats("):grid.index(" dg_slice(")]
    assert "block_count(" in tail and "k_slot_fold<" in tail and "k_slot_max<" in tail and "hipStreamSynchronize" not in tail


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_no_floating_point_outside_the_query():
    """the transform, slice and statistics kernels, the fold of the largest (k_slot_max: qn_map_compact.cuh) and the two bit searches name no floating-point type;
    the query's quantisation (oc_voxel: qn_dense_grid.cuh, which the route shares) is the only place that does"""
    src = open(os.path.join(CSRC, "qn_mapdistance.inc")).read()
    compact = open(os.path.join(CSRC, "qn_map_compact.cuh")).read()
    occ = open(os.path.join(CSRC, "qn_dense_grid.cuh")).read()
    for text, k, least in ((src, "md_left", 200), (src, "md_right", 200), (src, "k_md_x", 200), (src, "k_md_axis", 200), (compact, "k_slot_max", 200), (occ, "k_dg_slice", 200),
                           (occ, "dg_block_stats", 200)):
        i = text.index(" " + k + "(")
        body = text[i:text.index("\n}\n", i)]
        assert len(body) > least and not re.search(r"\b(float|double|float4|double2)\b", body), k
    i = src.index(" k_md_query(")
    assert "oc_voxel(" in src[src.index("{\n", i):src.index("\n}\n", i)]
    i = occ.index(" oc_voxel(")
    q = occ[i:occ.index("\n}\n", i)]
    every = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cuh", ".inc", ".h")))
    assert "rint(t * 1024.0)" in q and "double" in q and every.count("rint(t * 1024.0)") == 1      # the one quantisation of a world point
    device = src[:src.index("host side")]
    assert len(re.findall(r"__global__", device)) == 3 and "k_dg_slice<uint16_t, op_min>" in src      # (the slice kernel is the dense grid's)


def test_shim_program_compiles_and_prints_its_refusals(tmp_path):
    exe = build_shim("shim_map_distance.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 5 and "mapDistance: max_dist of 1 .. 255 voxels" in txt and "distanceAt: 3 doubles per point" in txt
    assert all(s in txt for s in ("qn_kf_map_distance:", "qn_kf_map_distance_grid:")) and "params 16 bytes, stats 32 bytes" in txt
