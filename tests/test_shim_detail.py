"""shim/qn_map/detail.hpp, the one place the qn_map headers take their refusal text, their status check and their parameter defaults from: every header in two
translation units of one program (inline-clean, guarded, -Wall as the other shim programs), one entry point per header called with a null store, and the text of
each exception byte for byte.  No GPU needed.

The text is "[qn_map] <call>: <status> <the store's last error>".  For a null store the last error reads "null store"; map_localize.hpp leaves it out for a null
store (it always has: its helper was written that way before it moved to detail.hpp), and CorrectedMap's constructor has no store to ask yet."""
import os
import re
import subprocess
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "fast-lio-sam-qn_amd", "shim", "qn_map")
# header -> the library call its entry point makes first (the label its refusal carries)
CALLS = [("corrected_map.hpp", "qn_kf_store_create"), ("freespace.hpp", "qn_kf_range_describe"), ("loop_submaps.hpp", "qn_kf_assemble_batch"),
         ("map_clusters.hpp", "qn_kf_map_clusters"), ("map_distance.hpp", "qn_kf_map_distance"), ("map_frontier.hpp", "qn_kf_map_frontiers"),
         ("map_frontier.hpp", "qn_kf_map_frontier_regions"), ("map_ground.hpp", "qn_kf_map_ground"), ("map_localize.hpp", "qn_kf_map_crop"),
         ("map_normals.hpp", "qn_kf_map_normals"), ("map_occupancy.hpp", "qn_kf_map_occupancy"), ("map_outliers.hpp", "qn_kf_map_outliers"),
         ("map_route.hpp", "qn_kf_map_route"), ("map_view.hpp", "qn_kf_map_view_grid"), ("scan_context.hpp", "qn_kf_sc_query"),
         ("static_map.hpp", "qn_kf_build_map_static"), ("second unit", "qn_kf_map_distance_grid")]


def test_every_header_is_in_both_units_and_every_refusal_reads_as_before(tmp_path):
    from qn_amd import engine
    headers = sorted(f for f in os.listdir(SHIM) if f.endswith(".hpp"))
    listed = re.findall(r"#include <qn_map/(\w+\.hpp)>", open(os.path.join(ROOT, "tests", "shim_detail_headers.h")).read())
    assert sorted(listed) == headers and {h for h, _ in CALLS} == set(headers) - {"detail.hpp"} | {"second unit"}
    for unit in ("shim_detail.cpp", "shim_detail_second.cpp"):
        assert '#include "shim_detail_headers.h"' in open(os.path.join(ROOT, "tests", unit)).read()
    exe = build_shim("shim_detail.cpp", tmp_path, "shim_detail_second.cpp")
    txt = subprocess.check_output([exe], text=True)
    L = engine.lib()
    L.qn_kf_last_error.restype = engine.C.c_char_p; L.qn_kf_last_error.argtypes = [engine.C.c_void_p]
    status = lambda rc: L.qn_status_str(rc).decode()
    null_store = L.qn_kf_last_error(None).decode()
    want = []
    for header, call in CALLS:
        if header == "corrected_map.hpp":
            tail = status(engine.QN_ERR_NO_DEVICE)
        elif header == "map_localize.hpp":
            tail = status(engine.QN_ERR_INVALID_ARG)
        else:
            tail = status(engine.QN_ERR_INVALID_ARG) + " " + null_store
        want.append("%s: [qn_map] %s: %s" % (header, call, tail))
    assert txt.splitlines() == want, txt


def test_the_headers_hold_no_second_copy_of_the_helpers():
    for f in sorted(os.listdir(SHIM)):
        src = open(os.path.join(SHIM, f)).read()
        if f == "detail.hpp":
            assert src.count("inline ") == 3 and "Eigen" not in src.split("#pragma once")[1] and "pcl" not in src.split("#pragma once")[1]
            continue
        assert 'throw std::runtime_error(std::string("[qn_map]' not in src and "if (params) p = *params" not in src, f
        assert "inline std::string why(" not in src and '#include "detail.hpp"' in src, f
