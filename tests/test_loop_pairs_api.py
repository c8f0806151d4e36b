"""Many queries in one drift-free verification (qn_kf_verify_loop_pairs / _c2f) and the debug clouds of a verified pair (qn_kf_verify_cloud): the C-ABI
surface and its constants, the Python wrappers, the C++ helpers compiling against the stand-ins, and the replay's loop_every = 1 being today's loop.
No GPU needed."""
import ctypes
import os
import re
import sys
import numpy as np
from qn_amd import engine
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_kf_verify_loop_pairs", "qn_kf_verify_loop_pairs_c2f", "qn_kf_verify_cloud"]


def test_header_declares_and_library_exports_the_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in SYMBOLS)


def test_header_defines_the_cloud_constants():
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    want = dict(QN_VERIFY_SRC=0, QN_VERIFY_DST=1, QN_VERIFY_COARSE=2, QN_VERIFY_FINAL=3)
    for name, v in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == v, name
        assert getattr(engine, name) == v, name


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    for fn, words in (("int  qn_kf_verify_loop_pairs(", ("bit for bit", "QN_ERR_INVALID_ARG", "first appearance", "repeated (query, cand) pair")),
                      ("int  qn_kf_verify_loop_pairs_c2f(", ("bit for bit", "QN_ERR_INVALID_ARG", "repeated (query, cand) pair")),
                      ("int  qn_kf_verify_cloud(", ("QN_ERR_NOT_READY", "qn_gicp_transformed_source", "valid until"))):
        i = h.index(fn)
        doc = h[h.rindex("/*", 0, i):i]
        for w in words:
            assert w in doc, (fn, w)


def test_python_wrappers_exist():
    for name in ("verify_loop_pairs", "verify_loop_pairs_c2f", "verify_cloud"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name


def test_helpers_compile_against_the_standins(tmp_path):
    out = build_shim("shim_loop_pairs.cpp", tmp_path)
    assert os.path.exists(out)


def test_replay_loop_every_one_is_todays_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    a = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle")
    b = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle", loop_every=1)
    assert a["loop_list"] == b["loop_list"] and a["attempts"] == b["attempts"]
    assert all(np.array_equal(p, q) for p, q in zip(a["poses"], b["poses"]))
