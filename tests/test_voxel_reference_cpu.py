"""The two references of the voxel-grid pipeline held to each other on every case of tests/voxel_cases.py, on the CPU: the C++ oracle
(oracle.voxel_grid / voxel_guard, xyz) and the numpy restatement (voxel_grid_xyzi, tests/test_kf_map_api.py).  Bit for bit: the same tripped flag,
the same point count, the same 12 xyz bytes of every record; the numpy transform against the oracle's.  A RuntimeWarning (an invalid cast, an
overflow outside the places where the guard rule names infinity as a value) is an error here.  This is what shows, without a GPU, that the
references agree on every input tests/test_gpu_voxel_edges.py compares the engine with; every case also asserts the branch it was built for."""
import warnings
import numpy as np
import pytest

import voxel_cases as vc
from test_kf_map_api import voxel_grid_xyzi


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def references(oracle, case, l):
    """one submap through both references -> dict(cat, fin, xyz (oracle), tripped, xyzi (restatement: the map's expected records))"""
    cat = case.concat(l)
    fin = cat[np.isfinite(cat[:, :3]).all(1)]
    xyz = oracle.voxel_grid(fin[:, :3], case.leaf) if len(fin) else np.zeros((0, 3), np.float32)
    tripped = oracle.voxel_guard(fin[:, :3], case.leaf) if len(fin) else False
    xyzi, overflowed = voxel_grid_xyzi(cat, case.leaf)
    return dict(cat=cat, fin=fin, xyz=xyz, tripped=tripped, xyzi=xyzi, overflowed=overflowed)


def test_the_table_covers_what_it_says():
    names = vc.NAMES
    assert len(names) == len(set(names)) >= 60, len(names)
    for family in ("sizes", "radix-switch", "leaf-bits", "single-point", "groups", "leaf-borders", "far", "guard"):
        assert any(n.startswith(family) for n in names), family


@pytest.mark.parametrize("name", vc.NAMES)
def test_oracle_and_restatement_agree(oracle, name):
    with warnings.catch_warnings(), np.errstate(invalid="raise"):
        warnings.simplefilter("error", RuntimeWarning)
        case = vc.get(name)
        d = vc.check(case)
        for s, l in enumerate(case.lists):
            parts = [oracle.transform_pcd(case.kfs[i], case.poses[i]) for i in l]
            r = references(oracle, case, l)
            finite = lambda a: a[np.isfinite(a).all(1)]
            if parts:                                                              # the numpy transform is the oracle's (non-finite results: the same rows)
                ref_cat = np.concatenate(parts)
                assert np.array_equal(np.isfinite(ref_cat).all(1), np.isfinite(r["cat"][:, :3]).all(1)), (name, s)
                assert same_bits(finite(ref_cat), r["fin"][:, :3]), (name, s)
            assert r["tripped"] == r["overflowed"] == bool(d["sub"][s]["tripped"]), (name, s, r["tripped"], r["overflowed"], d["sub"][s]["tripped"])
            if r["tripped"]:                                                       # the oracle: the finite points; the restatement: the whole concatenation
                assert same_bits(r["xyz"], r["fin"][:, :3]) and len(r["xyzi"]) == len(r["cat"]), (name, s)
                assert same_bits(finite(r["xyzi"][:, :3]), r["xyz"]), (name, s)
            else:
                assert len(r["xyz"]) == len(r["xyzi"]), (name, s, len(r["xyz"]), len(r["xyzi"]))
                assert same_bits(r["xyzi"][:, :3], r["xyz"]), (name, s)
                assert len(r["xyz"]) <= len(r["fin"]) and (len(r["xyz"]) > 0) == (len(r["fin"]) > 0), (name, s)
