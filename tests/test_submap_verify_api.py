"""Resident local submaps and the drift-free submap-to-submap verification (qn_kf_submap_*, qn_kf_verify_loop_pairs_submap[_c2f]): the C-ABI surface, the
window rule against a three-line restatement, the Python wrappers' own argument checks, the C++ helpers compiling against the stand-ins, and the replay's
existing option combinations being untouched by the new one.  No GPU needed."""
import ctypes
import os
import subprocess
import sys
import numpy as np
import pytest
from qn_amd import engine
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_kf_submap_describe", "qn_kf_submap_cloud", "qn_kf_submap_features", "qn_kf_submap_release", "qn_kf_verify_loop_pairs_submap",
           "qn_kf_verify_loop_pairs_submap_c2f"]


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
    for fn, words in (("int  qn_kf_submap_describe(", ("bit for bit", "QN_ERR_INVALID_ARG", "QN_ERR_CAPACITY", "QN_ERR_EMPTY_CLOUD", "i < n - 1", "144 B", "16 B")),
                      ("int  qn_kf_verify_loop_pairs_submap(", ("bit for bit", "QN_ERR_INVALID_ARG", "qn_gicp_align_batch_guess", "repeated (query, cand) pair")),
                      ("int  qn_kf_verify_loop_pairs_submap_c2f(", ("bit for bit", "QN_ERR_INVALID_ARG", "qn_coarse_to_fine_align_batch", "qn_kf_verify_cloud"))):
        i = h.index(fn)
        doc = h[h.rindex("/*", 0, i):i]
        for w in words:
            assert w in doc, (fn, w)


def test_local_submap_ids_is_the_clipped_window():
    for n in (1, 2, 7, 30):
        for r in (0, 1, 5, 40):
            for c in range(n):
                want = []
                for i in range(c - r, c + r + 1):
                    if 0 <= i < n:
                        want.append(i)
                got = engine.local_submap_ids(c, r, n)
                assert got == want and c in got, (c, r, n)
                if c + r < n - 1:           # away from the newest keyframe it is the reference's candidate window
                    assert got == engine.loop_submap_ids(n - 1, c, r, False, False, n)[1], (c, r, n)
    # at the newest keyframe the reference's rule drops the centre itself; this one keeps it
    assert engine.local_submap_ids(9, 2, 10) == [7, 8, 9] and engine.loop_submap_ids(9, 9, 2, False, True, 10)[1] == [7, 8]


def test_python_wrappers_exist_and_check_their_lists():
    for name in ("submap_describe", "submap_cloud", "submap_features", "submap_release", "verify_loop_pairs_submap", "verify_loop_pairs_submap_c2f",
                 "verify_loop_candidates_submap", "verify_loop_candidates_submap_c2f"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name
    # the length checks run before the library is touched: no store, no device needed
    store = object.__new__(engine.KeyframeStore)
    with pytest.raises(ValueError):
        store.verify_loop_pairs_submap(None, [1, 2], [0])
    with pytest.raises(ValueError):
        store.verify_loop_pairs_submap(None, [1, 2], [0, 3], [0.0])
    with pytest.raises(ValueError):
        store.verify_loop_pairs_submap_c2f(None, [1], [0, 3])


def test_null_arguments_are_refused_without_a_device():
    l = engine.lib()
    one = (ctypes.c_int32 * 1)(0); st = (ctypes.c_int * 1)(); P = (ctypes.c_double * 16)()
    assert l.qn_kf_submap_describe(None, None, one, ctypes.c_uint32(1), P, ctypes.c_uint32(1), ctypes.c_uint32(1), ctypes.c_double(0.3), 1, st) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_submap_cloud(None, ctypes.c_int32(0), None, None) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_submap_features(None, ctypes.c_int32(0), None) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_submap_release(None, None, ctypes.c_uint32(0)) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_verify_loop_pairs_submap(None, None, one, one, None, ctypes.c_uint32(1), ctypes.c_double(1.5), None, None, None) == engine.QN_ERR_INVALID_ARG
    assert l.qn_kf_verify_loop_pairs_submap_c2f(None, None, one, one, ctypes.c_uint32(1), ctypes.c_double(1.5), None, None, None, None, None) == engine.QN_ERR_INVALID_ARG


def test_helpers_compile_against_the_standins(tmp_path):
    out = build_shim("shim_submap_verify.cpp", tmp_path)
    assert os.path.exists(out)


def test_replay_refuses_submap_matching_without_relative_verification():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    with pytest.raises(ValueError):
        replay.run(n_kf=4, verbose=False, backend="oracle", submap_matching=True)


def test_replay_without_the_option_is_todays_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay
    a = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle")
    b = replay.run(n_kf=30, seed=11, verbose=False, backend="oracle", submap_matching=False)
    assert a["loop_list"] == b["loop_list"] and a["attempts"] == b["attempts"]
    assert all(np.array_equal(p, q) for p, q in zip(a["poses"], b["poses"]))
