"""The map-cluster calls (qn_cluster_default_params, qn_kf_map_clusters, qn_kf_map_cluster_points, qn_kf_map_cluster_list, qn_kf_map_drop_rejected_clusters):
the C-ABI surface, the record layouts, the Python wrappers and the refusal of a null store before any device is touched.  No GPU needed (the refusals that
need a store: tests/test_gpu_map_clusters.py)."""
import ctypes
import os
import re
import subprocess
import sys
import numpy as np
from qn_amd import engine, mapclusters as mc
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["qn_cluster_default_params", "qn_kf_map_clusters", "qn_kf_map_cluster_points", "qn_kf_map_cluster_list", "qn_kf_map_drop_rejected_clusters"]


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
    i = h.index("typedef struct qn_cluster_params")
    doc = h[h.rindex("/* ----", 0, i):i]
    for w in ("bit for bit", "24 bytes", "56 bytes", "2^31", "2^10", "QN_ERR_INVALID_ARG", "QN_ERR_NOT_READY", "QN_ERR_CAPACITY", "four host synchronisations",
              "half to even", "qn_amd/mapclusters.py", "class_mask", "DIFFERENT map indices", "0xffffffff", "previous results intact", "map slot", "non-finite",
              "smallest map index", "generation", "not measurements", "-0 < +0", "ascending order of root", "inclusive"):
        assert w in doc, w
    assert re.search(r"#define\s+QN_CLUSTER_REJECTED\s+\(-1\)", h) and re.search(r"#define\s+QN_CLUSTER_NONE\s+\(-2\)", h)
    k = open(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_kf_internal.h")).read()
    assert "qn_kf_int_ground_classes" in k and os.path.exists(os.path.join(ROOT, "fast-lio-sam-qn_amd", "csrc", "qn_mapclusters.inc"))


def test_record_layouts_and_defaults_are_the_headers():
    P, S, I = engine.ClusterParams, engine.ClusterStats, engine.ClusterInfo
    assert ctypes.sizeof(P) == 24 and (P.tolerance.offset, P.min_size.offset, P.max_size.offset, P.class_mask.offset, P.reserved.offset) == (0, 8, 12, 16, 20)
    assert ctypes.sizeof(S) == 56
    assert [f for f, _ in S._fields_] == ["n", "n_finite", "members", "components", "clusters", "too_small", "too_large", "clustered_points", "rejected_points",
                                          "largest", "quant_exp", "reserved", "edges"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48]
    assert ctypes.sizeof(I) == 56 and (I.root.offset, I.size.offset, I.lo.offset, I.hi.offset, I.sum_q.offset) == (0, 4, 8, 20, 32)
    D = mc.INFO_DTYPE
    assert D.itemsize == 56 and [D.fields[f][1] for f in ("root", "size", "lo", "hi", "sum_q")] == [0, 4, 8, 20, 32]
    p = P(9.0, 7, 8, 3); p.reserved = 5
    engine.lib().qn_cluster_default_params(ctypes.byref(p))
    assert (p.tolerance, p.min_size, p.max_size, p.class_mask, p.reserved) == (0.5, 10, 0xffffffff, 0, 0)
    engine.lib().qn_cluster_default_params(None)                      # a null pointer is ignored
    d = P()
    assert (d.tolerance, d.min_size, d.max_size, d.class_mask, d.reserved) == (0.5, 10, 0xffffffff, 0, 0)
    assert d.twin() == mc.ClusterParams() == (0.5, 10, 0xffffffff, 0)
    assert P(0.25, 3, 17, 12).twin() == (0.25, 3, 17, 12)
    assert (engine.QN_CLUSTER_REJECTED, engine.QN_CLUSTER_NONE) == (mc.REJECTED, mc.NONE) == (-1, -2)


def test_a_null_store_is_refused_before_any_device_call():
    L = engine.lib()
    p = engine.ClusterParams(); st = engine.ClusterStats(); ptr = ctypes.c_void_p(); n = ctypes.c_uint32()
    assert L.qn_kf_map_clusters(None, ctypes.byref(p), ctypes.byref(st)) == engine.QN_ERR_INVALID_ARG
    out = np.zeros(8, np.uint32)
    assert L.qn_kf_map_cluster_points(None, None, out.ctypes.data_as(ctypes.c_void_p), None) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_cluster_list(None, None, ctypes.c_uint32(0), ctypes.byref(n)) == engine.QN_ERR_INVALID_ARG
    assert L.qn_kf_map_drop_rejected_clusters(None, ctypes.byref(ptr), ctypes.byref(n)) == engine.QN_ERR_INVALID_ARG


def test_python_wrappers_exist():
    for f in ("map_clusters", "map_drop_rejected_clusters"):
        assert callable(getattr(engine.KeyframeStore, f))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import replay
    finally:
        sys.path.pop(0)
    import inspect
    assert {"map_clusters", "cluster_tol", "cluster_min", "cluster_max", "drop_small_clusters"} <= set(inspect.signature(replay.run).parameters)
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_map_clusters_time.py"))


def test_the_cluster_kernels_have_no_scratch():
    from qn_amd import build
    build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scratch_report.py"), "--all"], capture_output=True, text=True, check=True).stdout
    for k in ("k_mc_member", "k_mc_pick", "k_mc_init", "k_mc_hook", "k_mc_flatten", "k_mc_number", "k_mc_root_label", "k_mc_finish", "k_mc_info_init", "k_mc_info(",
              "k_mc_info_fin", "k_slot_fold<unsigned int, 10>", "k_slot_fold<unsigned long long, 1>"):
        rows = [l for l in out.splitlines() if k in l]
        assert rows, k
        assert all(int(l.split()[0]) == 0 and " spill   0 " in l for l in rows), rows


def test_helper_compiles_against_the_standins_and_refuses_a_null_store(tmp_path):
    txt = subprocess.check_output([build_shim("shim_map_clusters.cpp", tmp_path)], text=True)
    assert txt.count("refused") == 2 and "qn_kf_map_clusters" in txt and "qn_kf_map_drop_rejected_clusters" in txt
    assert "params 24 bytes, info 56 bytes, stats 56 bytes" in txt
