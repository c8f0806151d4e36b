"""The two-way overlap calls (qn_kf_overlap_batch, qn_kf_verify_overlap, qn_kf_overlap_points): the C-ABI surface, the record layout, the Python wrappers, the
C++ helper against the stand-ins, the replay's options, and the refusal of null and bad arguments before any device is touched.  No GPU needed."""
import ctypes
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import engine
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_kf_overlap_batch", "qn_kf_verify_overlap", "qn_kf_overlap_points"]


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
    i = h.index("typedef struct qn_overlap_dir")
    doc = h[h.rindex("/*", 0, i):i]
    for w in ("bit for bit", "24 bytes", "48 bytes", "QN_ERR_INVALID_ARG", "QN_ERR_EMPTY_CLOUD", "QN_ERR_NOT_READY", "two host synchronisations", "lowest index",
              "QN_VERIFY_FINAL", "QN_VERIFY_DST", "qn_amd/overlap.py"):
        assert w in doc, w


def test_record_layout_is_the_headers():
    assert ctypes.sizeof(engine.OverlapDir) == 24 and ctypes.sizeof(engine.Overlap) == 48
    assert engine.OverlapDir.sum_d2.offset == 16 and engine.Overlap.b_to_a.offset == 24


def test_python_wrappers_exist_and_check_their_arguments():
    for name in ("overlap_batch", "verify_overlap", "overlap_points"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name
    store = object.__new__(engine.KeyframeStore)                   # the shape checks run before the library is touched: no store, no device needed
    with pytest.raises(ValueError):
        store.overlap_batch([(1, 2, 3)], 0.3)
    with pytest.raises(ValueError):
        store.verify_overlap(0.3)
    with pytest.raises(ValueError):
        store.overlap_points(0, 0)


def test_null_and_bad_arguments_are_refused_without_a_device():
    l = engine.lib()
    u = ctypes.c_uint32
    ptr = (ctypes.c_void_p * 1)(); n = (u * 1)(1); out = (engine.Overlap * 1)(); st = (ctypes.c_int * 1)(); idx = (u * 1)(0)
    d2 = (ctypes.c_float * 1)(); ix = (ctypes.c_int32 * 1)()
    bad = engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_overlap_batch(None, ptr, n, ptr, n, u(1), ctypes.c_double(0.3), out, st) == bad
    assert l.qn_kf_verify_overlap(None, idx, u(1), ctypes.c_double(0.3), out, st) == bad
    assert l.qn_kf_verify_overlap(None, None, u(1), ctypes.c_double(0.3), out, st) == bad
    assert l.qn_kf_overlap_points(None, u(0), 0, d2, ix) == bad
    # with a non-null (never dereferenced) store: every other check comes before the store is looked at
    fake = ctypes.c_void_p(8)
    for args in ((None, n, ptr, n, u(1), 0.3, out, st), (ptr, None, ptr, n, u(1), 0.3, out, st), (ptr, n, None, n, u(1), 0.3, out, st), (ptr, n, ptr, None, u(1), 0.3, out, st),
                 (ptr, n, ptr, n, u(0), 0.3, out, st), (ptr, n, ptr, n, u(1), 0.3, None, st), (ptr, n, ptr, n, u(1), 0.3, out, None),
                 (ptr, n, ptr, n, u(1), 0.0, out, st), (ptr, n, ptr, n, u(1), -1.0, out, st), (ptr, n, ptr, n, u(1), float("nan"), out, st),
                 (ptr, n, ptr, n, u(1), float("inf"), out, st)):
        a = list(args); a[5] = ctypes.c_double(a[5])
        assert l.qn_kf_overlap_batch(fake, *a) == bad, args
    for args in ((idx, u(0), 0.3, out, st), (idx, u(1), 0.3, None, st), (idx, u(1), 0.3, out, None), (idx, u(1), 0.0, out, st), (idx, u(1), float("nan"), out, st)):
        a = list(args); a[2] = ctypes.c_double(a[2])
        assert l.qn_kf_verify_overlap(fake, *a) == bad, args
    assert l.qn_kf_overlap_points(fake, u(0), 2, d2, ix) == bad
    assert l.qn_kf_overlap_points(fake, u(0), -1, d2, ix) == bad
    assert l.qn_kf_overlap_points(fake, u(0), 0, None, None) == bad


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    out = build_shim("shim_overlap.cpp", tmp_path)
    txt = subprocess.check_output([out], text=True)
    assert "refused" in txt and "qn_kf_verify_overlap" in txt


def test_replay_gates_loops_on_the_overlap_with_the_oracle_backend():
    """off (the default) is today's run, on every path; with a threshold of 0 the relative run closes what it closes today and every attempt carries both
    overlaps; with a threshold no pair reaches, nothing closes.  (uniform stream, 40 keyframes, seed 11: today's run closes (20, 0) and rejects two pairs.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    a = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle")
    b = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle", min_overlap=None, overlap_radius=None)
    assert a["loop_list"] == b["loop_list"] and a["attempts"] == b["attempts"] and "overlaps" not in a
    assert all(np.array_equal(p, q) for p, q in zip(a["poses"], b["poses"]))
    kw = dict(n_kf=40, seed=11, verbose=False, backend="oracle", detector="scancontext", verify="relative")
    off = replay.run(**kw)
    assert [(q, c) for q, c, _ in off["loop_list"]] == [(20, 0)] and off["attempts"] == 3
    z = replay.run(min_overlap=0.0, overlap_radius=0.6, **kw)
    assert z["loop_list"] == off["loop_list"] and all(np.array_equal(p, q) for p, q in zip(z["poses"], off["poses"]))
    assert [(o["query"], o["cand"], o["valid"], o["accepted"]) for o in z["overlaps"]] == [(20, 0, True, True), (30, 9, False, False), (35, 12, False, False)]
    for o in z["overlaps"]:
        assert 0.0 < o["overlap_ab"] <= 1.0 and 0.0 < o["overlap_ba"] <= 1.0 and 0.0 < o["rmse_ab"] <= 0.6 and 0.0 < o["rmse_ba"] <= 0.6
    none = replay.run(min_overlap=0.99, overlap_radius=0.6, **kw)
    assert none["loop_list"] == [] and none["overlaps"][0]["valid"] and not none["overlaps"][0]["accepted"]
    for bad in (dict(min_overlap=0.5, overlap_radius=0.0), dict(min_overlap=0.5), dict(min_overlap=0.5, overlap_radius=float("nan"))):
        with pytest.raises(ValueError):
            replay.run(n_kf=4, verbose=False, backend="oracle", detector="scancontext", verify="relative", **bad)
    with pytest.raises(ValueError):
        replay.run(n_kf=4, verbose=False, backend="oracle", min_overlap=0.5, overlap_radius=0.3)          # the reference-style check keeps no pair clouds
