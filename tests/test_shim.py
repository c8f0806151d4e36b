"""The header-only drop-in shim (nano_gicp/nano_gicp.hpp) compiles against stand-in pcl/Eigen headers,
links against the C-ABI library and - on a GPU - reproduces LoopClosure::icpAlignment
(fast_lio_sam_qn/src/loop_closure.cpp:110-136) with the oracle's answer."""
import os
import subprocess
import numpy as np
import pytest
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "shim_icp_alignment")
BIN2 = os.path.join(ROOT, "tests", "shim_coarse_to_fine")


def build_shim_program():
    for name, out in (("shim_icp_alignment.cpp", BIN), ("shim_coarse_to_fine.cpp", BIN2)):
        assert build_shim(name, os.path.dirname(out)) == out
    return BIN


def test_shim_compiles_and_links():
    assert os.path.exists(build_shim_program()) and os.path.exists(BIN2)


@pytest.mark.gpu
def test_shims_reproduce_coarse_to_fine(tmp_path, oracle):
    """nano_gicp + quatro shims driven exactly like LoopClosure::coarseToFineAlignment (loop_closure.cpp:138-159)."""
    from qn_amd import synth
    if not os.path.exists(BIN2):
        build_shim_program()
    src, tgt, T = synth.make_pair(320, 6000, extent=42.0, mode="quatro")
    a, b = tmp_path / "src.bin", tmp_path / "dst.bin"
    src.tofile(a); tgt.tofile(b)
    out = subprocess.check_output([BIN2, str(a), str(b)]).decode().split()
    valid, conv, score = int(out[0]), int(out[1]), float(out[2])
    Tm = np.array([float(x) for x in out[3:19]]).reshape(4, 4)
    o = oracle.coarse_to_fine_alignment(src, tgt)
    assert bool(valid) == o["valid"] and bool(conv) == o["converged"]
    assert abs(score - o["score"]) <= 1e-6 * o["score"]
    dt, dr = synth.pose_error(Tm, o["T"])
    assert dt <= 1e-4 and dr <= 1e-4
    # quatro_matcher<>::optimizedMatching(35, 200, 0.95) on its own FPFH sets == the oracle matcher on the same descriptors
    from qn_amd import engine
    ctx = engine.Context(8192)
    fs, ft = engine.fpfh(ctx, src), engine.fpfh(ctx, tgt)
    ctx.close()
    _, corres = oracle.quatro_match(src, tgt, fs, ft)
    assert int(out[19]) == len(corres) and int(out[20]) == int((31 * corres[:, 0].astype(np.int64) + corres[:, 1]).sum())


@pytest.mark.gpu
def test_shim_reproduces_icp_alignment(tmp_path, oracle):
    from qn_amd import synth
    if not os.path.exists(BIN):
        build_shim_program()
    src, tgt, T = synth.make_pair(70, 5000, extent=45.0)
    a, b = tmp_path / "src.bin", tmp_path / "dst.bin"
    src.tofile(a); tgt.tofile(b)
    out = subprocess.check_output([BIN, str(a), str(b)]).decode().split()
    valid, conv, score = int(out[0]), int(out[1]), float(out[2])
    Tm = np.array([float(x) for x in out[3:19]]).reshape(4, 4)
    ro = oracle.icp_alignment(src, tgt)
    assert bool(valid) == ro["valid"] and bool(conv) == ro["converged"]
    assert abs(score - ro["score"]) <= 1e-6 * ro["score"]
    dt, dr = synth.pose_error(Tm, ro["T"])
    assert dt <= 1e-4 and dr <= 1e-4
    n_out, x0, inten = int(out[19]), float(out[20]), float(out[21])
    assert n_out == len(src) and inten == 42.0                     # output cloud: source fields kept, xyz transformed
    assert abs(x0 - ro["raw"]["Tf"][0] @ np.r_[src[0], 1.0]) < 1e-3


@pytest.mark.gpu
def test_shim_target_first_regrow(tmp_path, oracle):
    """Target set first, then a source large enough to make the shim regrow its context: the target and its covariances
    must survive (they were silently lost and align() read as hasConverged() == false)."""
    from qn_amd import synth
    if not os.path.exists(BIN):
        build_shim_program()
    src, tgt, T = synth.make_pair(71, 14000, extent=45.0)
    tgt = np.ascontiguousarray(tgt[::4])
    a, b = tmp_path / "src.bin", tmp_path / "dst.bin"
    src.tofile(a); tgt.tofile(b)
    out = subprocess.check_output([BIN, str(a), str(b), "t"]).decode().split()
    valid, conv, score = int(out[0]), int(out[1]), float(out[2])
    Tm = np.array([float(x) for x in out[3:19]]).reshape(4, 4)
    ro = oracle.icp_alignment(src, tgt)
    assert bool(conv) == ro["converged"] and bool(valid) == ro["valid"]
    assert abs(score - ro["score"]) <= 1e-6 * ro["score"]
    dt, dr = synth.pose_error(Tm, ro["T"])
    assert dt <= 1e-4 and dr <= 1e-4
