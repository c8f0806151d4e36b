"""Many loop-closure submaps in one pass (qn_kf_assemble_batch / qn_kf_download_batch): the C-ABI surface, the keyframe lists of
LoopClosure::setSrcAndDstCloud (qn_amd.engine.loop_submap_ids and shim/qn_map/loop_submaps.hpp) against a line-by-line restatement of
loop_closure.cpp:58-108, and the C++ helper compiling against the stand-in Eigen header.  No GPU needed."""
import ctypes
import itertools
import os
import subprocess
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_BIN = os.path.join(ROOT, "tests", "shim_loop_submaps")
BATCH_SYMBOLS = ["qn_kf_assemble_batch", "qn_kf_download_batch"]


def _int(v):
    """static_cast<int> of a size_t (two's complement): keyframes.size() - 1 of an empty vector is -1"""
    v %= 2 ** 64
    v %= 2 ** 32
    return v - 2 ** 32 if v >= 2 ** 31 else v


def reference_lists(keyframes_size, src_idx, dst_idx, submap_range, enable_quatro, enable_submap_matching):
    """loop_closure.cpp:58-108 statement by statement: which keyframes are accumulated into src_accum and dst_accum, in order"""
    src_accum, dst_accum = [], []
    if enable_submap_matching:
        i = src_idx - submap_range
        while i < src_idx + submap_range + 1:
            if i >= 0 and i < _int(keyframes_size - 1):
                src_accum.append(i)
            i += 1
        i = dst_idx - submap_range
        while i < dst_idx + submap_range + 1:
            if i >= 0 and i < _int(keyframes_size - 1):
                dst_accum.append(i)
            i += 1
    else:
        src_accum = [src_idx]
        if enable_quatro:
            dst_accum = [dst_idx]
        else:
            i = dst_idx - submap_range
            while i < dst_idx + submap_range + 1:
                if i >= 0 and i < _int(keyframes_size - 1):
                    dst_accum.append(i)
                i += 1
    return src_accum, dst_accum


FLAGS = list(itertools.product([False, True], [False, True]))          # (enable_quatro, enable_submap_matching)


def _cases():
    """(n_keyframes, src_idx, dst_idx, submap_range) edge cases: query at 0, candidate next to the newest keyframe, fewer keyframes than the range"""
    yield 40, 0, 0, 10                      # query at index 0
    yield 40, 0, 25, 10
    yield 40, 39, 35, 10                    # the newest keyframe as query; candidate within range of it
    yield 40, 39, 38, 10
    yield 40, 39, 30, 10
    yield 5, 4, 1, 10                       # fewer keyframes than the range
    yield 1, 0, 0, 10                       # one keyframe: every submap is empty
    yield 3, 2, 0, 0                        # range 0
    yield 21, 20, 10, 10
    for n in (2, 7, 12):
        for r in (0, 1, 3, 10):
            for src in (0, n // 2, n - 1):
                for dst in (0, 1, n - 2, n - 1):
                    yield n, src, max(dst, 0), r


def test_header_declares_and_library_exports_the_batch_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in BATCH_SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in BATCH_SYMBOLS)


def test_loop_submap_ids_restates_set_src_and_dst_cloud():
    from qn_amd import engine
    for (n, src, dst, r), (quatro, submap) in itertools.product(list(_cases()), FLAGS):
        want = reference_lists(n, src, dst, r, quatro, submap)
        got = engine.loop_submap_ids(src, dst, r, quatro, submap, n)
        assert (list(got[0]), list(got[1])) == want, (n, src, dst, r, quatro, submap, got, want)


def test_newest_keyframe_never_enters_a_submap_but_single_keyframe_cases_keep_it():
    from qn_amd import engine
    s, d = engine.loop_submap_ids(39, 38, 10, False, True, 40)
    assert 39 not in s and 39 not in d and s == list(range(29, 39)) and d == list(range(28, 39))
    assert engine.loop_submap_ids(39, 38, 10, True, False, 40) == ([39], [38])          # the reference default: scan to scan
    assert engine.loop_submap_ids(39, 38, 10, False, False, 40) == ([39], list(range(28, 39)))
    assert engine.loop_submap_ids(0, 0, 10, False, True, 1) == ([], [])


def build_loop_program():
    assert build_shim("shim_loop_submaps.cpp", os.path.dirname(LOOP_BIN)) == LOOP_BIN
    return LOOP_BIN


def test_loop_submaps_helper_compiles_and_links():
    assert os.path.exists(build_loop_program())


def test_cpp_loop_submap_ids_restates_set_src_and_dst_cloud(tmp_path):
    """the header's loopSubmapIds (no library call) against the same restatement"""
    prog = tmp_path / "ids.cpp"
    prog.write_text("#include <cstdio>\n#include <cstdlib>\n#include <qn_map/loop_submaps.hpp>\n"
                    "int main(int c, char** v) { int a[6]; for (int k = 0; k < 6; k++) a[k] = std::atoi(v[k + 1]);\n"
                    "  const qn_map::SubmapIds r = qn_map::loopSubmapIds(a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5]);\n"
                    "  for (int i : r.src) std::printf(\"%d \", i); std::printf(\"|\"); for (int i : r.dst) std::printf(\" %d\", i); std::printf(\"\\n\"); return 0; }\n")
    exe = build_shim(str(prog), tmp_path, link=False)
    cases = list(_cases())[:12]
    for (n, src, dst, r), (quatro, submap) in itertools.product(cases, FLAGS):
        out = subprocess.check_output([exe, str(src), str(dst), str(r), str(int(quatro)), str(int(submap)), str(n)], text=True)
        a, b = out.split("|")
        assert ([int(x) for x in a.split()], [int(x) for x in b.split()]) == reference_lists(n, src, dst, r, quatro, submap), (n, src, dst, r, quatro, submap, out)
