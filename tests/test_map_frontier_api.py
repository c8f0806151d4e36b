"""The frontier calls (qn_frontier_default_params, qn_kf_map_frontiers, qn_kf_map_frontier_grid, qn_kf_map_frontier_regions, qn_kf_map_frontier_list,
qn_kf_map_frontier_costs): the C-ABI surface, the record layouts, the Python wrappers, the place of the device code, the refusal of a null store before any
device is touched, the text README, DESIGN.md and the header share, and the shim program.  No GPU needed (the refusals that need a store:
tests/test_gpu_map_frontier.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapfrontier as mf
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
SYMBOLS = ["qn_frontier_default_params", "qn_kf_map_frontiers", "qn_kf_map_frontier_grid", "qn_kf_map_frontier_regions", "qn_kf_map_frontier_list",
           "qn_kf_map_frontier_costs"]
KERNELS = ("k_mf_mark", "k_mf_tile", "k_mf_merge", "k_mf_flatten", "k_mf_roots", "k_mf_pick", "k_mf_rows_init", "k_mf_relabel", "k_mf_rows", "k_mf_costs")
LIST_KERNELS = ("k_dg_list_flag", "k_dg_list_pick")                  # the voxel list's, of qn_dense_grid.cuh, instantiated on MfList
# what the header, README and DESIGN.md all say of the unit
SHARED = ("qn_amd/mapfrontier.py", "qn_mapfrontier.inc", "26-connect", "free_mask", "unknown_mask", "edge_unknown", "min_size", "ascending root", "interface choices")


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
    i = h.index("#define QN_FRONTIER_REJECTED")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in SHARED + ("csrc/qn_mapfrontier.inc", "bit for bit", "1 << QN_OCC_FREE", "1 << QN_OCC_UNKNOWN", "32 bytes", "48 bytes", "64 bytes", "not measurements",
                       "iz_lo > iz_hi", "INT32_MAX", "6 face neighbours", "the band does not apply to neighbours", "bounding box of the rays", "1 .. 6",
                       "(iz H + iy) W + ix", "QN_FRONTIER_REJECTED (-1)", "QN_FRONTIER_NONE (-2)", "sum / size", "too_small (components)", "rounds",
                       "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "QN_ERR_HIP", "previous result intact", "byte-identical", "0 x 0 x 0",
                       "qn_kf_map_distance and qn_kf_map_route do not touch it", "Two host synchronisations", "ascending linear index", "smallest linear index on a tie",
                       "QN_ROUTE_UNREACHED and voxel (0, 0, 0)", "without a live route field", "may be NULL"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_FRONTIER_REJECTED\s+\(-1\)", h) and re.search(r"#define\s+QN_FRONTIER_NONE\s+\(-2\)", h)
    assert (engine.QN_FRONTIER_REJECTED, engine.QN_FRONTIER_NONE) == (mf.REJECTED, mf.NONE) == (-1, -2)
    assert h.index("typedef struct qn_frontier_params") > h.index("int  qn_kf_map_route_path")      # behind the route section, the last of the chain


def test_readme_design_and_the_twin_say_the_same():
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = next(l for l in readme.splitlines() if l.startswith("|") and "qn_kf_map_frontiers" in l)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    para = next(l for l in design.splitlines() if l.startswith("**Exploration frontiers of the occupancy map"))
    twin = mf.__doc__
    for w in SHARED:
        assert w in row and w in para and (w in twin or w == "qn_amd/mapfrontier.py"), w
    for s in SYMBOLS:
        assert s in row, s
    for w in KERNELS + LIST_KERNELS:
        assert w in para, w
    for w in ("KeyframeStore.map_frontiers", "qn_map::mapFrontiers", "--occ-frontiers", "tools/gpu_map_frontier_time.py"):
        assert w in row, w
    assert "map_frontier.hpp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (row, para):                                         # the measured times, or that there are none
        assert re.search(r"\d ms", text) or "not measured" in text


def test_record_layouts_and_defaults_are_the_headers():
    P, S, I = engine.FrontierParams, engine.FrontierStats, engine.FrontierInfo
    assert ctypes.sizeof(P) == 32 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert ctypes.sizeof(S) == 48 and [getattr(S, f).offset for f, _ in S._fields_] == [4 * k for k in range(11)]
    assert ctypes.sizeof(I) == 64 == mf.INFO_DTYPE.itemsize
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [(f, mf.INFO_DTYPE.fields[f][1]) for f in mf.INFO_DTYPE.names]
    assert [f for f, _ in S._fields_ if f not in ("reserved", "rounds")] == list(mf.FrontierStats._fields)
    assert [f for f, _ in P._fields_ if f != "reserved"] == list(mf.FrontierParams._fields)
    p = P(3, 4, 0, 77, 5, 6); p.reserved[1] = 5
    engine.lib().qn_frontier_default_params(ctypes.byref(p))
    assert (p.free_mask, p.unknown_mask, p.edge_unknown, p.min_size, p.iz_lo, p.iz_hi, list(p.reserved)) == (1 << engine.QN_OCC_FREE, 1 << engine.QN_OCC_UNKNOWN, 1, 8, 0,
                                                                                                              0x7fffffff, [0, 0])
    engine.lib().qn_frontier_default_params(None)                      # a null pointer is ignored
    d = P()
    assert d.twin() == mf.FrontierParams() == (2, 1, 1, 8, 0, 0x7fffffff) and list(d.reserved) == [0, 0]
    assert P(4, 3, 0, 9, -3, 7).twin() == (4, 3, 0, 9, -3, 7)
    s = S(); s.candidates, s.frontier, s.components, s.regions, s.too_small, s.region_voxels, s.rejected_voxels, s.largest, s.unknown_faces, s.rounds = range(1, 11)
    assert s.twin() == mf.FrontierStats(*range(1, 10))


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.FrontierParams(); st = engine.FrontierStats(); g = engine.OccupancyGrid(); cnt = ctypes.c_uint32()
    out = np.zeros(8, np.uint32); ijk = np.zeros(24, np.int32); lab = np.zeros(8, np.int32); rows = np.zeros(2, mf.INFO_DTYPE)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_frontiers(None, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_grid(None, ctypes.byref(g), ctypes.byref(p), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_regions(None, pp(rows), 2, ctypes.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_list(None, pp(ijk), pp(lab), 8, ctypes.byref(cnt)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_frontier_costs(None, pp(out), pp(ijk)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_and_tools_exist():
    for f in ("map_frontiers", "map_frontier_grid", "map_frontier_regions", "map_frontier_list", "map_frontier_costs"):
        assert callable(getattr(engine.KeyframeStore, f))
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_frontier_time.py"))
    assert os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_frontier.hpp"))


def test_the_device_code_hangs_on_the_occupancy_state():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert unit.index('#include "qn_mapfrontier.inc"') > unit.index('#include "qn_maproute.inc"') > unit.index('#include "qn_mapoccupancy.inc"')
    internal = open(os.path.join(CSRC, "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", internal) and "FRONTIER" not in internal      # no slot of its own
    occ = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    state = occ[occ.index("struct OccState {"):occ.index("};", occ.index("struct OccState {"))]
    assert "FrontierState" in state and "DistState" in state and "mf_end(st->frontier.get())" in occ
    for f in ("qn_mapdistance.inc", "qn_maproute.inc"):              # neither the distance nor the route call ends the regions
        assert "mf_end" not in open(os.path.join(CSRC, f)).read()
    inc = open(os.path.join(CSRC, "qn_mapfrontier.inc")).read()
    assert "qn_amd/mapfrontier.py" in inc and "untuned" in inc and "union-find" in inc and "rounds = 1" in inc
    device = inc[:inc.index("host side")]
    assert len(re.findall(r"__global__", device)) == len(KERNELS) and "struct MfList {" in device and "dg_list_count(" in inc and "dg_list_pick(" in inc
    call = inc[inc.index('extern "C" int qn_kf_map_frontiers('):inc.index('extern "C" int qn_kf_map_frontier_grid(')]
    assert len(re.findall(r"hipStreamSynchronize", call)) == 2      # the number of regions, the statistics
    assert "block_count(" in inc and "k_slot_fold<" in inc and "block_rank(" in inc and "k_scan_rows" in inc and "__syncthreads_or(" in inc
    assert "asm" not in device and not re.search(r"\b(float|double|float4|double2)\b", device)      # plain C++ and integers only


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS + tuple(k + "<(anonymous namespace)::MfList>" for k in LIST_KERNELS):
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_shim_program_compiles_and_prints_its_refusals(tmp_path):
    exe = build_shim("shim_map_frontier.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 7 and "mapFrontiers: iz_lo <= iz_hi" in txt and "mapFrontiers: min_size of at least 1" in txt and "share a class" in txt
    assert all(s in txt for s in ("qn_kf_map_frontiers:", "qn_kf_map_frontier_regions:", "qn_kf_map_frontier_list:")) and "params 32 bytes, stats 48 bytes, info 64 bytes" in txt
