"""The route calls (qn_route_default_params, qn_kf_map_route, qn_kf_map_route_grid, qn_kf_map_route_query, qn_kf_map_route_path): the C-ABI surface, the record
layouts, the Python wrappers, the place of the device code, the refusal of a null store before any device is touched, the text README, DESIGN.md and the header
share, and the shim program.  No GPU needed (the refusals that need a store: tests/test_gpu_map_route.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, maproute as mr
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
SYMBOLS = ["qn_route_default_params", "qn_kf_map_route", "qn_kf_map_route_grid", "qn_kf_map_route_query", "qn_kf_map_route_path"]
KERNELS = ("k_mr_init", "k_mr_goals", "k_mr_relax", "k_mr_stats", "k_mr_path", "k_mr_query", "k_slot_fold<unsigned int, 2>")
# what the header, README and DESIGN.md all say of the unit
SHARED = ("qn_amd/maproute.py", "qn_maproute.inc", "3-4-5 chamfer", "QN_ROUTE_BLOCKED", "QN_ROUTE_UNREACHED", "pass_mask", "min_d2", "planar", "interface choices")


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
    i = h.index("#define QN_ROUTE_BLOCKED")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in SHARED + ("csrc/qn_maproute.inc", "bit for bit", "1 << QN_OCC_FREE", "QN_DIST_FAR passes", "32 bytes", "64 bytes", "not measurements", "iz_lo > iz_hi", "INT32_MAX",
                       "o'_k in {0, o_k}", "No corner is cut", "undirected", "2 + |o|_1", "cost / 3 * voxel", "1 .. 2^20", "qn_kf_map_distance_query", "goals_blocked",
                       "5 * 2^27", "passable = reached + unreached", "rounds and tile_visits", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_HIP", "QN_ERR_INTERNAL",
                       "cells + 2 rounds", "previous field intact", "byte-identical", "0 x 0 x 0", "min_d2 > max_dist^2", "beyond the cap the distance is not known",
                       "ceil(rounds / QN_ROUTE_ROUNDS_PER_CHECK) + 1", "dz outermost, then dy, then dx", "-1, 0, +1", "max_len == 0", "cost / 3 + 1", "k = 0",
                       "may be NULL"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_ROUTE_BLOCKED\s+0xfffffffeu", h) and re.search(r"#define\s+QN_ROUTE_UNREACHED\s+0xffffffffu", h)
    assert re.search(r"#define\s+QN_ROUTE_MAX_POINTS\s+\(1u << 20\)", h) and re.search(r"#define\s+QN_ROUTE_ROUNDS_PER_CHECK\s+8u\s+/\* an untuned choice", h)
    assert (engine.QN_ROUTE_BLOCKED, engine.QN_ROUTE_UNREACHED, engine.QN_ROUTE_MAX_POINTS) == (mr.BLOCKED, mr.UNREACHED, mr.MAX_POINTS) == (0xfffffffe, 0xffffffff, 1 << 20)
    assert h.index("typedef struct qn_route_params") > h.index("int  qn_kf_map_distance_query")      # behind the distance section it builds on


def test_readme_design_and_the_twin_say_the_same():
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = next(l for l in readme.splitlines() if l.startswith("|") and "qn_kf_map_route" in l)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    k28 = next(l for l in design.splitlines() if l.startswith("| K28 |"))
    para = next(l for l in design.splitlines() if l.startswith("**Planning over the occupancy map"))
    twin = mr.__doc__
    for w in SHARED:
        assert w in row and w in para and (w in twin or w.startswith("QN_ROUTE_") or w == "qn_amd/maproute.py"), w      # (the twin names the constants BLOCKED and UNREACHED)
    for s in SYMBOLS:
        assert s in row, s
    for w in ("k_mr_init", "k_mr_goals", "k_mr_relax", "k_mr_stats", "k_mr_path", "k_mr_query"):
        assert w in k28, w
    for w in ("KeyframeStore.map_route", "qn_map::mapRoute", "--occ-route", "tools/gpu_map_route_time.py"):
        assert w in row, w
    assert "map_route.hpp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (row, para):                                         # the measured times, or that there are none
        assert re.search(r"\d ms", text) or "not measured" in text


def test_record_layouts_and_defaults_are_the_headers():
    P, S = engine.RouteParams, engine.RouteStats
    assert ctypes.sizeof(P) == 32 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20]
    assert ctypes.sizeof(S) == 64 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]
    assert [f for f, _ in S._fields_ if not f.startswith("reserved") and f not in ("rounds", "tile_visits")] == list(mr.RouteStats._fields)
    assert [f for f, _ in P._fields_ if f != "reserved"] == list(mr.RouteParams._fields)
    p = P(3, 77, 5, 6, 1); p.reserved[2] = 5
    engine.lib().qn_route_default_params(ctypes.byref(p))
    assert (p.pass_mask, p.min_d2, p.iz_lo, p.iz_hi, p.planar, list(p.reserved)) == (1 << engine.QN_OCC_FREE, 4, 0, 0x7fffffff, 0, [0, 0, 0])
    engine.lib().qn_route_default_params(None)                         # a null pointer is ignored
    d = P()
    assert d.twin() == mr.RouteParams() == (2, 4, 0, 0x7fffffff, 0) and list(d.reserved) == [0, 0, 0]
    assert P(5, 9, -3, 7, 1).twin() == (5, 9, -3, 7, 1)
    s = S(); s.passable, s.blocked, s.reached, s.unreached, s.goals_used, s.goals_blocked, s.max_cost, s.sum_cost, s.rounds = 1, 2, 3, 4, 5, 6, 7, 1 << 40, 9
    assert s.twin() == mr.RouteStats(1, 2, 3, 4, 5, 6, 7, 1 << 40)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.RouteParams(); st = engine.RouteStats(); g = engine.OccupancyGrid()
    out = np.zeros(8, np.uint32); ijk = np.zeros(24, np.int32); xyz = np.zeros(3)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_route(None, pp(xyz), 1, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_route_grid(None, ctypes.byref(g), ctypes.byref(p), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_route_query(None, pp(xyz), 1, pp(out)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_route_path(None, pp(xyz), 1, 8, pp(out), pp(ijk)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_and_tools_exist():
    for f in ("map_route", "map_route_grid", "map_route_query", "map_route_paths"):
        assert callable(getattr(engine.KeyframeStore, f))
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_route_time.py"))
    assert os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_route.hpp"))


def test_the_device_code_hangs_on_the_distance_state():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert unit.index('#include "qn_maproute.inc"') > unit.index('#include "qn_mapdistance.inc"') > unit.index('#include "qn_mapoccupancy.inc"')
    internal = open(os.path.join(CSRC, "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", internal) and "ROUTE" not in internal      # no slot of its own
    dist = open(os.path.join(CSRC, "qn_mapdistance.inc")).read()
    state = dist[dist.index("struct DistState {"):dist.index("};", dist.index("struct DistState {"))]
    assert "RouteState" in state and "mr_end(st->route.get())" in dist
    inc = open(os.path.join(CSRC, "qn_maproute.inc")).read()
    assert "qn_amd/maproute.py" in inc and "untuned" in inc and "ceil(rounds / QN_ROUTE_ROUNDS_PER_CHECK) + 1" in inc
    device = inc[:inc.index("host side")]
    assert len(re.findall(r"\batomic\w+\(", device)) == 1 and "atomicAdd(visits, 1u)" in device      # the one count that needs one: a diagnostic
    call = inc[inc.index('extern "C" int qn_kf_map_route('):inc.index('extern "C" int qn_kf_map_route_grid(')]
    assert len(re.findall(r"hipStreamSynchronize", call)) == 2      # one in the loop over the batches of rounds, one for the statistics
    assert "block_count(" in inc and "k_slot_fold<" in inc and "__syncthreads_or(" in inc
    assert "asm" not in device                                       # plain C++ stores only


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_no_floating_point_outside_the_quantisation():
    """the field, statistics and walk kernels name no floating-point type in their bodies; oc_voxel (qn_dense_grid.cuh), which goals, starts and query
    points share with the distance query, is the only place that computes with one"""
    src = open(os.path.join(CSRC, "qn_maproute.inc")).read()
    occ = open(os.path.join(CSRC, "qn_dense_grid.cuh")).read()
    for text, k, least in ((src, "k_mr_init", 200), (src, "k_mr_relax", 1500), (src, "k_mr_stats", 200), (occ, "dg_block_stats", 200), (occ, "dg_each_neighbour", 200)):
        i = text.index(" " + k + "(")
        body = text[i:text.index("\n}\n", i)]
        assert len(body) > least and not re.search(r"\b(float|double|float4|double2)\b", body), k
    for k in ("k_mr_goals", "k_mr_path", "k_mr_query"):
        i = src.index(" " + k + "(")
        body = src[src.index("{\n", i):src.index("\n}\n", i)]
        assert "oc_voxel(" in body and not re.search(r"\b(float|double|float4|double2)\b", body), k      # (the points and 1 / voxel are parameters)
    i = occ.index(" oc_voxel(")
    q = occ[i:occ.index("\n}\n", i)]
    assert "rint(t * 1024.0)" in q and "double" in q
    device = src[:src.index("host side")]
    assert len(re.findall(r"__global__", device)) == 6


def test_shim_program_compiles_and_prints_its_refusals(tmp_path):
    exe = build_shim("shim_map_route.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 8 and "mapRoute: 3 doubles per goal" in txt and "routePath: max_len of at least 1" in txt and "mapRoute: iz_lo <= iz_hi" in txt
    assert all(s in txt for s in ("qn_kf_map_route:", "qn_kf_map_route_grid:", "qn_kf_map_route_path:")) and "params 32 bytes, stats 64 bytes" in txt
