"""Resident Quatro descriptors per keyframe and the drift-free coarse-to-fine check (qn_kf_quatro_describe / _cloud / _features,
qn_kf_verify_loop_candidates_c2f): the C-ABI surface, the Python wrappers, and the C++ helper compiling against the stand-ins.  No GPU needed."""
import ctypes
import os
from qn_amd import engine
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_kf_quatro_describe", "qn_kf_quatro_cloud", "qn_kf_quatro_features", "qn_kf_verify_loop_candidates_c2f"]


def test_header_declares_and_library_exports_the_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in SYMBOLS)


def test_python_wrappers_exist():
    for name in ("quatro_describe", "quatro_cloud", "quatro_features", "verify_loop_candidates_c2f"):
        assert callable(getattr(engine.KeyframeStore, name, None)), name


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "qn_engine.h")).read()
    i = h.index("int  qn_kf_verify_loop_candidates_c2f(")
    doc = h[h.rindex("/*", 0, i):i]
    for words in ("bit for bit", "QN_ERR_INVALID_ARG", "radii", "inv(P_c) P_query", "loop_closure.cpp:129"):
        assert words in doc, words


def test_helper_compiles_against_the_standins(tmp_path):
    out = build_shim("shim_kf_quatro.cpp", tmp_path)
    assert os.path.exists(out)
