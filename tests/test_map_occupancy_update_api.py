"""qn_kf_map_occupancy_update: the C-ABI surface, the record layout on both sides, the header's contract, the Python wrapper's argument checks, the place of the
device code, the shim, and tools/replay.py --occ-incremental on the oracle backend.  No GPU needed (the call itself: tests/test_gpu_map_occupancy_update.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import engine, mapoccupancy as mo
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ("k_oc_extent_entry", "k_oc_uncarve<true>", "k_oc_uncarve<false>", "k_oc_regrid", "k_oc_carve<true>", "k_oc_carve<false>")


def test_the_record_is_64_bytes_on_both_sides(tmp_path):
    U = engine.OccupancyUpdate
    assert ctypes.sizeof(U) == 64 and [getattr(U, f).offset for f, _ in U._fields_] == [0, 4, 8, 12, 16, 20, 24, 36, 48, 56]
    assert [f for f, _ in U._fields_] == list(mo.OccupancyUpdate._fields)
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    body = h[h.index("typedef struct qn_occupancy_update {"):h.index("} qn_occupancy_update;")]
    assert re.findall(r"\b([a-z_]+)(?:\[3\])?[,;]", body) == [f for f, _ in U._fields_] and "/* 64 bytes */" in h[h.index("} qn_occupancy_update;"):][:200]
    exe = build_shim("shim_map_occupancy_update.cpp", tmp_path)
    txt = subprocess.check_output([exe], text=True)
    assert txt.count("refused") == 2 and "updateOccupancy: 16 doubles per listed keyframe" in txt and "qn_kf_map_occupancy_update:" in txt and "update 64 bytes" in txt
    shim = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map", "map_occupancy.hpp")).read()
    assert shim.index("inline MapOccupancy mapOccupancy(") < shim.index("inline MapOccupancy updateOccupancy(")


def test_the_header_documents_the_call_and_the_library_exports_it():
    import test_capi_symbols
    assert "qn_kf_map_occupancy_update" in test_capi_symbols.declared_symbols()
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    i = h.index("typedef struct qn_occupancy_update")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("csrc/qn_mapoccupancy_update.inc", "qn_amd/mapoccupancy.py", "byte for byte", "multiset", "memcmp", "sign of a zero", "rebuilt = 1", "min_hits or hit_weight",
              "union", "previous result", "64 bytes", "2^20", "2^15", "2^27", "2^32 records", "QN_ERR_CAPACITY", "no live result and no ledger", "dirty_lo", "NEW grid",
              "drops it", "also shrinks", "tools/gpu_map_occupancy_update_time.py"):
        assert w in doc, w
    from qn_amd import build
    build.build()
    assert hasattr(ctypes.CDLL(build.LIB), "qn_kf_map_occupancy_update")


def test_a_null_store_and_null_outputs_are_refused_before_any_device_call():
    L = engine.lib()
    p = engine.OccupancyParams(); st = engine.OccupancyStats(); up = engine.OccupancyUpdate()
    ids = np.zeros(1, np.int32); P = np.eye(4).reshape(-1)
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.qn_kf_map_occupancy_update(None, pp(ids), pp(P), 1, ctypes.byref(p), ctypes.byref(st), ctypes.byref(up)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_occupancy_update(None, pp(ids), pp(P), 1, ctypes.byref(p), None, None) == engine.QN_ERR_INVALID_ARG


def test_the_wrapper_checks_its_arguments_as_map_occupancy_does():
    class Refuses:                                                   # the wrapper must fail on its own checks, before it reaches the library
        def __getattr__(self, name):
            raise AssertionError("the library was reached: " + name)
    s = engine.KeyframeStore.__new__(engine.KeyframeStore)
    s._l = Refuses(); s.h = None
    for call in (engine.KeyframeStore.map_occupancy, engine.KeyframeStore.map_occupancy_update):
        with pytest.raises(ValueError):
            call(s, [0, 1], [np.eye(4)])                             # two ids, one pose
        with pytest.raises(ValueError):
            call(s, [0], np.zeros(15))
        with pytest.raises((ValueError, TypeError)):
            call(s, ["a"], [np.eye(4)])
        with pytest.raises(AttributeError):
            call(s, [0], [np.eye(4)], params=(0.3, 0.5))             # neither an OccupancyParams nor the twin's
    import inspect
    assert list(inspect.signature(engine.KeyframeStore.map_occupancy_update).parameters) == list(inspect.signature(engine.KeyframeStore.map_occupancy).parameters)


def test_the_device_code_sits_behind_the_occupancy_unit():
    unit = open(os.path.join(CSRC, "qn_staticmap.hip")).read()
    assert unit.index('#include "qn_mapoccupancy.inc"') < unit.index('#include "qn_mapoccupancy_update.inc"') < unit.index('#include "qn_mapdistance.inc"')
    inc = open(os.path.join(CSRC, "qn_mapoccupancy_update.inc")).read()
    assert {c for c in re.findall(r"\b(atomic[A-Z]\w*)\s*\(", inc)} == {"atomicAdd", "atomicMin", "atomicMax"} and "oc_walk<FOLD, true>(" in inc
    call = inc[inc.index('extern "C" int qn_kf_map_occupancy_update('):]
    assert "oc_check_list(" in call and "QN_OCC_NO_FOLD" in call and "dg_blocks(" in call and "sv_each_chunk(" in inc
    regrid = inc[inc.index(" k_oc_regrid("):]
    regrid = regrid[:regrid.index("\n}\n")]
    assert not re.search(r"\b(float|double|atomic\w+)\b", regrid) and "oc_ijk(" in regrid
    base = open(os.path.join(CSRC, "qn_mapoccupancy.inc")).read()
    assert "st->ledger.reset()" in base[base.index('extern "C" int qn_kf_map_occupancy('):base.index('extern "C" int qn_kf_map_occupancy_grid(')]
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_occupancy_update_time.py"))


def test_the_kernels_have_no_scratch_and_no_spills():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        rows = [l for l in out.splitlines() if "::" + k + "(" in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_replay_keeps_the_volume_live_on_the_oracle_backend(tmp_path):
    import test_replay_map_occupancy_update as t
    n = 5
    once, live = t.run_both(tmp_path, "oracle", n)
    o = live["occupancy"]
    assert o["updates"] == n and o["entries_listed"] == n * (n + 1) // 2 and n <= o["entries_walked"] < o["entries_listed"] and o["occupied"] > 1000
