"""The corrected global map (qn_kf_add_xyzi / qn_kf_build_map / qn_kf_download_map): the C-ABI surface, the numpy restatement of
pcl::VoxelGrid with intensity that the GPU tests compare against (checked here against the oracle's xyz), and the C++ helper
(shim/qn_map/corrected_map.hpp) compiling against the stand-in pcl/Eigen headers.  No GPU needed."""
import ctypes
import os
import numpy as np
from shim_build import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_BIN = os.path.join(ROOT, "tests", "shim_corrected_map")
MAP_SYMBOLS = ["qn_kf_add_xyzi", "qn_kf_build_map", "qn_kf_download_map"]
INT32_MAX = 2 ** 31 - 1


def voxel_guard(mn, mx, leaf):
    """The overflow guard from the box of the finite points (f32 mn, mx) -> (tripped, minb, div), minb / div as Python ints (None when tripped).
    The one rule of the engine (voxel_dims, qn_cloud.hip) and the oracle (voxel_guard, oracle/cloud_oracle.cpp), inv = 1 / float32(leaf), all f32: tripped when
      (1) on any axis floor(min * inv) or floor(max * inv) is outside [-2^31, 2^31)      (deviation from PCL, which converts unchecked)
      (2) on any axis (max - min) * inv is not below 2^63, infinite or NaN included      (deviation from PCL, which converts unchecked)
      (3) pd = product of int64((max - min) * inv) + 1 > INT32_MAX                       (PCL's own guard)
      (4) cells = product of floor(max * inv) - floor(min * inv) + 1 > INT32_MAX         (deviation from PCL, whose index wraps)
    Compared in floating point before any conversion; the integers are Python's, which do not overflow.  An f32 product or difference that
    overflows to infinity is IEEE arithmetic, not an error: it trips (1) or (2)."""
    mn = np.asarray(mn, np.float32); mx = np.asarray(mx, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):                # inf and inf * 0 = NaN are values the rule names
        inv = np.float32(1.0) / np.float32(leaf)
        lo, hi, ext = np.floor(mn * inv), np.floor(mx * inv), (mx - mn) * inv
    two31, two63 = np.float32(2.0 ** 31), np.float32(2.0 ** 63)
    if not ((lo >= -two31) & (lo < two31) & (hi >= -two31) & (hi < two31)).all() or not (ext < two63).all():
        return True, None, None
    minb = [int(v) for v in lo]; div = [int(h) - int(l) + 1 for l, h in zip(lo, hi)]
    pdf = [int(e) + 1 for e in ext]
    if pdf[0] * pdf[1] * pdf[2] > INT32_MAX or div[0] * div[1] * div[2] > INT32_MAX:
        return True, None, None
    return False, minb, div


def voxel_grid_xyzi(p4, leaf):
    """pcl::VoxelGrid (downsample_all_data_) on an (n, 4) float32 x y z intensity cloud, as the engine fixes it -> ((m, 4) float32, overflowed).
    Leaf index floor(p * inv) - min_b in f32; output in ascending leaf index; inside a leaf, f32 sums in ascending input order, / (float)count.
    Non-finite xyz is dropped (a non-dense cloud); a NaN intensity on a finite point poisons its leaf's intensity.  The overflow guard
    (voxel_guard) returns the input unfiltered, non-finite points included."""
    p4 = np.ascontiguousarray(p4, dtype=np.float32)
    q = p4[np.isfinite(p4[:, :3]).all(1)]
    if len(q) == 0:
        return np.zeros((0, 4), np.float32), False
    inv = np.float32(1.0) / np.float32(leaf)
    tripped, minb, div = voxel_guard(q[:, :3].min(0), q[:, :3].max(0), leaf)
    if tripped:
        return p4.copy(), True
    minb = np.array(minb, np.int64); div = np.array(div, np.int64)
    ijk = (np.floor(q[:, :3] * inv) - minb.astype(np.float32)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * (div[0] * div[1])
    order = np.argsort(idx, kind="stable")
    s, pts = idx[order], q[order]
    heads = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    counts = np.diff(np.r_[heads, len(s)])
    # the r-th point of every leaf with more than r points, r = 0, 1, ...: each leaf's sum is added strictly in order
    byc = np.argsort(-counts, kind="stable")
    hc, cc = heads[byc], counts[byc]
    acc = np.zeros((len(heads), 4), np.float32)
    for r in range(int(cc[0])):
        k = int(np.searchsorted(-cc, -r, side="left"))            # leaves with count > r come first
        acc[:k] += pts[hc[:k] + r]
    out = np.empty_like(acc)
    out[byc] = acc / cc.astype(np.float32)[:, None]
    return out, False


def transform_xyzi(p4, T):
    """transformPcd (utilities.hpp:164-175) in the engine's f64 arithmetic and order; intensity carried."""
    p = np.asarray(p4, np.float32); x, y, z = (p[:, d].astype(np.float64) for d in range(3))
    out = np.empty((len(p), 4), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    out[:, 3] = p[:, 3] if p.shape[1] > 3 else 0.0
    return out


def build_map_program():
    assert build_shim("shim_corrected_map.cpp", os.path.dirname(MAP_BIN)) == MAP_BIN
    return MAP_BIN


def test_header_declares_and_library_exports_the_map_api():
    from qn_amd import build
    import test_capi_symbols
    declared = test_capi_symbols.declared_symbols()
    assert all(s in declared for s in MAP_SYMBOLS), declared
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, s) for s in MAP_SYMBOLS)


def test_restatement_matches_the_oracle_voxel_grid(oracle):
    rng = np.random.default_rng(5)
    kfs = [np.c_[rng.uniform(-25, 25, (20000, 2)), rng.uniform(-2, 6, 20000)].astype(np.float32) for _ in range(15)]
    poses = []
    for k in range(15):
        T = np.eye(4); a = 0.3 * k; T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; T[:3, 3] = [3.0 * k, 1.5 * k, 0.1 * k]
        poses.append(T)
    ids = list(range(15)) + [3]
    cat = np.concatenate([transform_xyzi(kfs[i], poses[i]) for i in ids])
    cat[:, 3] = rng.uniform(0, 255, len(cat)).astype(np.float32)
    ours, of = voxel_grid_xyzi(cat, 0.3)
    ref = oracle.assemble_submap(kfs, poses, ids, 0.3)
    assert not of and len(ours) > 10000
    assert np.array_equal(ours[:, :3].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(cat[:, :3].view(np.uint32), np.concatenate([oracle.transform_pcd(kfs[i], poses[i]) for i in ids]).view(np.uint32))


def test_restatement_intensity_sequential_sum():
    pts = np.array([[0.01, 0, 0, 1.0], [0.02, 0, 0, 1e8], [5, 5, 5, 3.0], [0.03, 0, 0, -1e8], [np.nan, 0, 0, 7.0], [5.1, 5, 5, np.nan]], np.float32)
    out, of = voxel_grid_xyzi(pts, 1.0)
    assert not of and len(out) == 2
    assert out[0, 3] == np.float32((np.float32(1.0) + np.float32(1e8)) + np.float32(-1e8)) / np.float32(3)    # in-order f32: 0, not 1/3
    assert np.isnan(out[1, 3]) and np.isfinite(out[1, :3]).all()


def test_restatement_overflow_guard_passes_everything_through():
    pts = np.array([[0, 0, 0, 1], [1e4, 1e4, 1e4, 2], [np.inf, 0, 0, 3]], np.float32)
    out, of = voxel_grid_xyzi(pts, 1e-3)
    assert of and np.array_equal(out.view(np.uint32), pts.view(np.uint32))


def test_corrected_map_helper_compiles_and_links():
    assert os.path.exists(build_map_program())
