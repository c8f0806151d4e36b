"""The view-gain calls (qn_view_default_params, qn_kf_map_view_gain, qn_kf_map_view_grid): the C-ABI surface, the record layouts, the Python wrappers, the place
of the device code, the refusal of a null store before any device is touched, the text README, DESIGN.md, the header and the twin share, and the shim program.
No GPU needed (the refusals that need a store: tests/test_gpu_map_view.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapview as mv
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
SYMBOLS = ["qn_view_default_params", "qn_kf_map_view_gain", "qn_kf_map_view_grid"]
KERNELS = ("k_mv_origin", "k_mv_cast", "k_mv_stats")
# what the header, README, DESIGN.md and the twin all say of the unit
SHARED = ("qn_amd/mapview.py", "qn_mapview.inc", "gain_mask", "stop_mask", "max_through", "band", "blocked", "escaped", "spent", "reached", "distinct", "interface choices",
          "one synchronisation") + KERNELS


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
    i = h.index("#define QN_VIEW_OK")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in SHARED + ("csrc/qn_mapview.inc", "bit for bit", "1 << QN_OCC_UNKNOWN", "1 << QN_OCC_OCCUPIED", "32 bytes", "48 bytes", "not measurements", "iz_lo > iz_hi", "INT32_MAX",
                       "2^16", "2^20", "QN_VIEW_MAX_OFFSET (2^25)", "1024ths of a voxel", "half to even", "QN_VIEW_OUTSIDE (1)", "QN_VIEW_OK (0)", "(iz H + iy) W + ix",
                       "Sum cover = sum gain", "passes", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_HIP", "previous result intact", "0 x 0 x 0",
                       "qn_kf_map_distance, qn_kf_map_route and qn_kf_map_frontiers do not", "QN_VIEW_PASS", "QN_VIEW_NO_PEEK", "may be NULL", "atomicOr"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_VIEW_OK\s+0\b", h) and re.search(r"#define\s+QN_VIEW_OUTSIDE\s+1\b", h) and re.search(r"#define\s+QN_VIEW_MAX_OFFSET\s+\(1 << 25\)", h)
    assert (engine.QN_VIEW_OK, engine.QN_VIEW_OUTSIDE, engine.QN_VIEW_MAX_OFFSET) == (mv.OK, mv.OUTSIDE, mv.MAX_OFFSET) == (0, 1, 1 << 25)
    assert h.index("typedef struct qn_view_params") > h.index("int  qn_kf_map_frontier_costs")      # behind the frontier section


def test_readme_design_and_the_twin_say_the_same():
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = next(l for l in readme.splitlines() if l.startswith("|") and "qn_kf_map_view_gain" in l)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    para = next(l for l in design.splitlines() if l.startswith("**View gain over the occupancy map"))
    twin = mv.__doc__
    for w in SHARED:
        assert w in row and w in para and (w in twin or w == "qn_amd/mapview.py"), w
    for s in SYMBOLS[1:]:
        assert s in row, s
    for w in ("KeyframeStore.map_view_gain", "qn_map::mapViewGain", "--occ-view-gain", "tools/gpu_map_view_time.py"):
        assert w in row, w
    assert "map_view.hpp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (row, para):                                         # the measured times, or that there are none
        assert re.search(r"\d ms", text) or "not measured" in text
    assert "qn_kf_map_view_gain" in open(os.path.join(ROOT, "profiles", "EXPERIMENTS.md")).read()


def test_record_layouts_and_defaults_are_the_headers():
    P, S, I = engine.ViewParams, engine.ViewStats, engine.ViewInfo
    assert ctypes.sizeof(P) == 32 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20]
    assert ctypes.sizeof(S) == 48 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert ctypes.sizeof(I) == 48 == mv.VIEW_DTYPE.itemsize
    assert [(f, getattr(I, f).offset) for f, _ in I._fields_] == [(f, mv.VIEW_DTYPE.fields[f][1]) for f in mv.VIEW_DTYPE.names]
    assert [f for f, _ in S._fields_ if f not in ("reserved", "passes")] == list(mv.ViewStats._fields)
    assert [f for f, _ in P._fields_ if f != "reserved"] == list(mv.ViewParams._fields)
    p = P(3, 4, 77, 5, 6); p.reserved[1] = 5
    engine.lib().qn_view_default_params(ctypes.byref(p))
    assert (p.gain_mask, p.stop_mask, p.max_through, p.iz_lo, p.iz_hi, list(p.reserved)) == (1 << engine.QN_OCC_UNKNOWN, 1 << engine.QN_OCC_OCCUPIED, 0, 0, 0x7fffffff, [0, 0, 0])
    engine.lib().qn_view_default_params(None)                        # a null pointer is ignored
    d = P()
    assert d.twin() == mv.ViewParams() == (1, 4, 0, 0, 0x7fffffff) and list(d.reserved) == [0, 0, 0]
    assert P(2, 5, 9, -3, 7).twin() == (2, 5, 9, -3, 7)
    s = S(); s.viewpoints, s.outside, s.rays, s.covered, s.max_cover, s.passes, s.total_gain, s.steps = 1, 2, 3, 4, 5, 6, 1 << 40, 1 << 41
    assert s.twin() == mv.ViewStats(1, 2, 3, 4, 5, 1 << 40, 1 << 41)
    r = I(); r.status, r.gain, r.blocked, r.escaped, r.spent, r.reached, r.steps = 1, 2, 3, 4, 5, 6, 1 << 33
    r.ijk[0], r.ijk[1], r.ijk[2] = -1, 8, 9
    t = r.twin()
    assert t.dtype == mv.VIEW_DTYPE and t.shape == (1,) and t["ijk"].tolist() == [[-1, 8, 9]] and int(t["steps"][0]) == 1 << 33 and int(t["reached"][0]) == 6
    assert t.tobytes() == bytes(r)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.ViewParams(); st = engine.ViewStats(); g = engine.OccupancyGrid()
    xyz = np.zeros((1, 3)); off = np.zeros((1, 3), np.int32); rows = np.zeros(1, mv.VIEW_DTYPE)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_view_gain(None, pp(xyz), 1, pp(off), 1, ctypes.byref(p), pp(rows), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_view_grid(None, ctypes.byref(g), ctypes.byref(p), None) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_tools_and_shim_exist():
    for f in ("map_view_gain", "map_view_grid"):
        assert callable(getattr(engine.KeyframeStore, f))
    for f in ("gain", "brute", "sensor_offsets", "check_params"):
        assert callable(getattr(mv, f))
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_view_time.py"))
    hpp = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_view.hpp")).read()
    assert all(w in hpp for w in ("sensorRays", "mapViewGain", "viewCover"))
    assert "--occ-view-gain" in open(os.path.join(ROOT, "tools", "replay.py")).read()


def test_the_device_code_hangs_on_the_occupancy_state():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert unit.index('#include "qn_mapview.inc"') > unit.index('#include "qn_mapfrontier.inc"') > unit.index('#include "qn_maproute.inc"') > unit.index('#include "qn_mapoccupancy.inc"')
    internal = open(os.path.join(CSRC, "qn_kf_internal.h")).read()
    assert re.search(r"#define\s+QN_KF_INT_EXT\s+10\b", internal) and "VIEW" not in internal      # no slot of its own
    occ = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    state = occ[occ.index("struct OccState {"):occ.index("};", occ.index("struct OccState {"))]
    assert "ViewState" in state and "FrontierState" in state and "mv_end(st->view.get())" in occ
    for f in ("qn_mapdistance.inc", "qn_maproute.inc", "qn_mapfrontier.inc"):      # none of the distance, route and frontier calls ends the view result
        assert "mv_end" not in open(os.path.join(CSRC, f)).read()
    grid = open(os.path.join(CSRC, "qn_dense_grid.cuh")).read()
    live = grid[grid.index("struct DgLive {"):]
    assert "ViewState* view" in live[:live.index("};")]
    inc = open(os.path.join(CSRC, "qn_mapview.inc")).read()
    assert "qn_amd/mapview.py" in inc and "untuned" in inc and "QN_VIEW_PASS" in inc and "QN_VIEW_NO_PEEK" in inc and "DgLive dg_live(qn_kf_store* s) {" in inc
    device = inc[:inc.index("host side")]
    assert len(re.findall(r"__global__", device)) == len(KERNELS) and all(k + "(" in device for k in KERNELS)
    assert "asm" not in device
    behind = device[device.index("behind the quantisation"):]        # the cast and the statistics: integers only
    assert "k_mv_cast(" in behind and "k_mv_stats(" in behind and "k_mv_origin(" not in behind and len(behind) > 4000
    assert not re.search(r"\b(float|double|float4|double2)\b", behind)
    assert "oc_walk" not in device and "unsigned long long)r1 * Db" in behind      # the walk written again, compared in 64 bits
    atomics = set(re.findall(r"\batomic[A-Z]\w*", device))
    assert atomics == {"atomicOr", "atomicAdd"}, atomics             # integer atomics only
    assert "block_count(" in device and "block_sum(" in device and "dg_block_stats(" in device and "dg_fold_stats(" in inc and "grow_beside(" in inc and "dg_band(" in inc
    call = inc[inc.index('extern "C" int qn_kf_map_view_gain('):inc.index('extern "C" int qn_kf_map_view_grid(')]
    assert len(re.findall(r"hipStreamSynchronize", call)) == 1       # whatever the number of passes
    loop = call[call.index("for (uint32_t q0 = 0;"):]
    assert "hipStreamSynchronize" not in loop[:loop.index("st_out.passes++")]


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_mv_origin(", "k_mv_cast<true>(", "k_mv_cast<false>(", "k_mv_stats("):
        rows = [l for l in out.splitlines() if "::" + k in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_shim_program_compiles_and_prints_its_refusals(tmp_path):
    exe = build_shim("shim_map_view.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 9 and "mapViewGain: iz_lo <= iz_hi" in txt and "share a class" in txt and "sensorRays: max_range / voxel beyond the offset limit" in txt
    assert "beyond QN_VIEW_MAX_OFFSET" in txt and txt.count("qn_kf_map_view_gain:") == 1 and txt.count("qn_kf_map_view_grid:") == 1
    assert "params 32 bytes, info 48 bytes, stats 48 bytes" in txt
