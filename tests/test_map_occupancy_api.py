"""The 3-D occupancy calls (qn_occupancy_default_params, qn_kf_map_occupancy, qn_kf_map_occupancy_grid, qn_kf_map_occupancy_list, qn_kf_map_occupancy_slice): the
C-ABI surface, the record layouts, the Python wrappers, the place of the device code, the refusal of a null store before any device is touched, and the shim
program.  No GPU needed (the refusals that need a store: tests/test_gpu_map_occupancy.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapoccupancy as mo
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
SYMBOLS = ["qn_occupancy_default_params", "qn_kf_map_occupancy", "qn_kf_map_occupancy_grid", "qn_kf_map_occupancy_list", "qn_kf_map_occupancy_slice"]
KERNELS = ("k_oc_extent", "k_oc_carve<true>", "k_oc_carve<false>", "k_oc_classify", "k_dg_list_flag<(anonymous namespace)::OcList>", "k_dg_list_pick<(anonymous namespace)::OcList>",
           "k_dg_slice<unsigned char, (anonymous namespace)::op_max>", "k_scan_rows",
           "k_slot_fold<unsigned int, 5>", "k_slot_fold<unsigned int, 3>", "k_slot_fold<unsigned long long, 2>")


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
    i = h.index("typedef struct qn_occupancy_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("qn_amd/mapoccupancy.py", "csrc/qn_mapoccupancy.inc", "bit for bit", "left to right", "no fused multiply-add", "half to even", "lowest axis", "48 bytes",
              "64 bytes", "56 bytes", "2^20", "2^15", "2^27", "2^32 records", "1024.0", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "not measurements",
              "previous result intact", "do not depend on the map slot", "ascending linear index", "Two host", "n - shell", "never carves its own end voxel",
              "dropped whole", "iz_lo > iz_hi"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_OCC_MAX_CELLS\s+\(1u << 27\)", h)
    for k, name in enumerate(("UNKNOWN", "FREE", "OCCUPIED")):
        assert re.search(r"#define\s+QN_OCC_%s\s+%d\b" % (name, k), h) and getattr(engine, "QN_OCC_" + name) == getattr(mo, name) == k
    assert engine.QN_OCC_MAX_CELLS == mo.MAX_CELLS == 1 << 27 and mo.MAX_SIDE == 1 << 15 and mo.S == 10 and mo.COORD_LIMIT == 2.0 ** 20


def test_record_layouts_and_defaults_are_the_headers():
    P, S, G = engine.OccupancyParams, engine.OccupancyStats, engine.OccupancyGrid
    assert ctypes.sizeof(P) == 48 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 8, 16, 24, 28, 32, 36]
    assert ctypes.sizeof(S) == 64 and [getattr(S, f).offset for f, _ in S._fields_] == list(range(0, 48, 4)) + [48, 56]
    assert sorted(f for f, _ in S._fields_ if f != "reserved") == sorted(mo.OccupancyStats._fields)
    assert ctypes.sizeof(G) == 56 and [getattr(G, f).offset for f, _ in G._fields_] == [0, 24, 32, 36, 40, 44]
    assert [f for f, _ in G._fields_] == list(mo.OccupancyGrid._fields)
    p = P(9.0, 7.0, 8.0, 3, 31, 5); p.reserved[2] = 5
    engine.lib().qn_occupancy_default_params(ctypes.byref(p))
    assert (p.voxel, p.min_range, p.max_range, p.shell, p.min_hits, p.hit_weight, list(p.reserved)) == (0.3, 0.5, 60.0, 1, 1, 2, [0, 0, 0])
    engine.lib().qn_occupancy_default_params(None)                    # a null pointer is ignored
    d = P()
    assert d.twin() == mo.OccupancyParams() == (0.3, 0.5, 60.0, 1, 1, 2) and list(d.reserved) == [0, 0, 0]
    assert P(1.0, 0.0, 9.0, 0, 4, 7).twin() == (1.0, 0.0, 9.0, 0, 4, 7)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.OccupancyParams(); st = engine.OccupancyStats(); g = engine.OccupancyGrid(); n = ctypes.c_uint32()
    ids = np.zeros(1, np.int32); P = np.eye(4).reshape(-1); out = np.zeros(8, np.uint8)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_occupancy(None, pp(ids), pp(P), 1, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy_grid(None, ctypes.byref(g), None, None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy_list(None, 4, ctypes.byref(n), None, None, None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy_slice(None, 0, 1, pp(out)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_and_tools_exist():
    for f in ("map_occupancy", "map_occupancy_grid", "map_occupancy_list", "map_occupancy_slice"):
        assert callable(getattr(engine.KeyframeStore, f))
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_occupancy_time.py"))
    assert os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_occupancy.hpp"))


def test_the_device_code_is_part_of_the_static_map_unit():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert '#include "qn_mapoccupancy.inc"' in unit and "OccState" in unit[unit.index("struct StaticState"):unit.index("}  // namespace")]
    internal = open(os.path.join(CSRC, "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", internal) and "OCC" not in internal      # no slot of its own
    inc = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    assert "DevBuf<uint32_t> hits, misses" in inc and "qn_amd/mapoccupancy.py" in inc
    assert len(re.findall(r"hipStreamSynchronize", inc[inc.index('extern "C" int qn_kf_map_occupancy('):inc.index('extern "C" int qn_kf_map_occupancy_grid(')])) <= 3
    calls = re.findall(r"\b(atomic[A-Z]\w*)\s*\(&(\w+)\[", inc)                              # integer atomics only: on the u32 counts and the int32 extremes
    assert {c for c, _ in calls} == {"atomicAdd", "atomicMin", "atomicMax"} and {a for _, a in calls} == {"hits", "misses", "ext"} and len(calls) == inc.count("atomic" + "Add(") + 2


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_no_floating_point_in_the_walk():
    """behind the quantisation (oc_ray, which the extent and the carve kernels share) the walk names no floating-point type: the whole of oc_walk - the setup, the
    fold of the first voxel and the loop - and the kernels behind the counts: the list's predicate and payload here, its kernels and the slice kernel in
    qn_dense_grid.cuh"""
    src = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    grid = open(os.path.join(CSRC, "qn_dense_grid.cuh")).read()
    for text, k, end in ((src, " oc_walk(", "\n}\n"), (src, " k_oc_classify(", "\n}\n"), (src, "struct OcList {", "\n};\n"), (grid, " k_dg_list_flag(", "\n}\n"),
                         (grid, " k_dg_list_pick(", "\n}\n"), (grid, " k_dg_slice(", "\n}\n")):
        i = text.index(k)
        body = text[i:text.index(end, i)]
        assert len(body) > (150 if "list_flag" in k else 200) and not re.search(r"\b(float|double|float4|double2)\b", body), k
    assert "keep(uint32_t i)" in src[src.index("struct OcList {"):] and "list.keep(i)" in grid and "list.put(i, j)" in grid and "block_rank(keep" in grid
    walk = src[src.index(" oc_walk("):]
    loop = walk[walk.index("for (uint32_t i = 0; i < carve; i++)"):walk.index("\n}\n")]
    assert "atomicAdd(&misses[lin], 1u)" in loop and "unsigned long long" in loop and not re.search(r"\b(float|double)\b", loop)
    carve = src[src.index(" k_oc_carve("):]
    assert "oc_ray(" in carve[:carve.index("\n}\n")] and "oc_walk<FOLD>(" in carve[:carve.index("\n}\n")]


def test_shim_program_compiles_and_refuses_a_null_store(tmp_path):
    exe = build_shim("shim_map_occupancy.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 4 and "mapOccupancy: 16 doubles per listed keyframe" in txt
    assert all(s in txt for s in ("qn_kf_map_occupancy:", "qn_kf_map_occupancy_grid:")) and "params 48 bytes, stats 64 bytes, grid 56 bytes" in txt
