#!/usr/bin/env python
"""Replay harness (SURVEY.md 8f rank 4 / BASELINE configs[4]): the loop-closure side of FastLioSamQn on a synthetic
keyframe stream, with the registration engine on the GPU and the pose graph on the host.

What is reproduced from the reference (fast_lio_sam_qn/src/fast_lio_sam_qn.cpp):
  * keyframes every `keyframe_thr` metres of odometry (FQ:124, config.yaml:7), each with its sensor-frame cloud (PosePcd, PP:7-19);
  * prior + odometry BetweenFactors with the reference's variances (FQ:112-116, 132-143);
  * loopTimerFunc (FQ:203-252): candidate = closest keyframe within `loop_detection_radius` and older than
    `loop_detection_timediff_threshold` (LC:34-56) -> setSrcAndDstCloud (LC:58-108) -> coarseToFineAlignment /
    icpAlignment (LC:110-159) -> if valid: BetweenFactor(latest, closest, (T_reg * pose_latest).between(pose_closest)), variance = score
    on all 6 dof (FQ:220-238) -> re-optimise, rewrite all corrected poses (FQ:180-188).
What is NOT the reference: GTSAM/iSAM2 is not installed here, so the pose graph is a small batch SE(3) Gauss-Newton in numpy
(same factors, same noise models) - the optimiser stays on the host either way, as the north-star prescribes.
The registration engine is the product under test: keyframe clouds resident in HBM (qn_kf_store), cloud assembly + voxel grid
on the device, Nano-GICP and (--quatro) Quatro + Nano-GICP on the device through the `_device` entry points: a loop attempt moves no
point cloud across PCIe.  `backend="oracle"` runs the same loop with the CPU oracle's assembly and registrations instead (test
infrastructure: tests/test_replay.py compares the two); `save_dir` writes the corrected trajectory the way saveFlagCallback does
(FQ:344-373): poses_kitti.txt (3x4 row-major, default stream precision) and poses_tum.txt ("#timestamp x y z qx qy qz qw", 8 decimals);
with `save_map_leaf` the GPU backend also writes the corrected global map there as map.pcd (FQ:398-411: every keyframe with its corrected
pose, voxel grid at save_voxel_resolution, on the device through qn_kf_build_map); with `static_map` also map_static.pcd beside it, the same map without the
records other keyframes saw through (qn_kf_static_classify / qn_kf_build_map_static).  `moving_boxes` puts boxes into the spinning sensor's scene that stand
somewhere else in every keyframe - the ghost trails the static map is there to remove.
The reference's extra iSAM2::update() calls after a loop (FQ:160-165) are iSAM2 relinearisation sweeps; the batch Gauss-Newton stand-in
iterates to convergence instead.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "fast-lio-sam-qn_amd"))
import ctypes as C
import numpy as np


# ------------------------------------------------------------------ SE(3) helpers (host pose graph)
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(xi):
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 1e-9:
        R = np.eye(3) + W; V = np.eye(3) + 0.5 * W
    else:
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = V @ v
    return T


def log_se3(T):
    R, t = T[:3, :3], T[:3, 3]
    c = np.clip((np.trace(R) - 1) / 2, -1, 1); th = np.arccos(c)
    if th < 1e-9:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
        Vi = np.eye(3) - 0.5 * hat(w)
    else:
        w = th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        W = hat(w)
        Vi = np.eye(3) - 0.5 * W + (1 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))) * W @ W
    return np.r_[w, Vi @ t]


def inv(T):
    Ti = np.eye(4); Ti[:3, :3] = T[:3, :3].T; Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return Ti


class PoseGraph:
    """prior + between factors, Gauss-Newton with right perturbations X <- X exp(dx); numeric Jacobians (graphs here are small)."""

    def __init__(self):
        self.poses = []; self.factors = []           # (i, j, Z, sqrt_info[6]) ; j = -1 for a prior on i

    def add_pose(self, T):
        self.poses.append(T.copy()); return len(self.poses) - 1

    def add_prior(self, i, Z, var):
        self.factors.append((i, -1, Z.copy(), 1.0 / np.sqrt(var)))

    def add_between(self, i, j, Z, var):
        self.factors.append((i, j, Z.copy(), 1.0 / np.sqrt(var)))

    def _res(self, f, Xi, Xj):
        i, j, Z, s = f
        E = inv(Z) @ (Xi if j < 0 else inv(Xi) @ Xj)
        return s * log_se3(E)

    def optimize(self, iters=25):
        n = len(self.poses)
        for _ in range(iters):
            H = np.zeros((6 * n, 6 * n)); g = np.zeros(6 * n)
            for f in self.factors:
                i, j = f[0], f[1]
                Xi = self.poses[i]; Xj = self.poses[j] if j >= 0 else None
                r0 = self._res(f, Xi, Xj)
                eps = 1e-6; Ji = np.zeros((6, 6)); Jj = np.zeros((6, 6))
                for k in range(6):
                    d = np.zeros(6); d[k] = eps
                    Ji[:, k] = (self._res(f, Xi @ exp_se3(d), Xj) - r0) / eps
                    if j >= 0:
                        Jj[:, k] = (self._res(f, Xi, Xj @ exp_se3(d)) - r0) / eps
                si = slice(6 * i, 6 * i + 6)
                H[si, si] += Ji.T @ Ji; g[si] += Ji.T @ r0
                if j >= 0:
                    sj = slice(6 * j, 6 * j + 6)
                    H[sj, sj] += Jj.T @ Jj; g[sj] += Jj.T @ r0; H[si, sj] += Ji.T @ Jj; H[sj, si] += Jj.T @ Ji
            dx = np.linalg.solve(H + 1e-9 * np.eye(6 * n), -g)
            for i in range(n):
                self.poses[i] = self.poses[i] @ exp_se3(dx[6 * i:6 * i + 6])
            if np.abs(dx).max() < 1e-6:
                break


# ------------------------------------------------------------------ synthetic keyframe stream
def make_stream(n_kf, seed, scan_range=28.0, drift_yaw=0.004, drift_xy=0.03, pts_per_scan=9000, yaw_bias=0.006):
    from qn_amd import synth
    rng = np.random.default_rng(seed)
    scene = synth.Scene(rng, 120.0)
    world = scene.sample(rng, 700000, (-60, 60, -60, 60))
    s = np.linspace(0, 2 * np.pi, n_kf, endpoint=False)           # figure-8: passes the centre twice -> loops
    xy = np.c_[30 * np.sin(s), 22 * np.sin(2 * s)]
    head = np.arctan2(np.gradient(xy[:, 1]), np.gradient(xy[:, 0]))
    gt = []
    for k in range(n_kf):
        T = np.eye(4); T[:3, :3] = synth._rot_zyx(head[k], 0, 0); T[:3, 3] = [xy[k, 0], xy[k, 1], 1.8]
        gt.append(T)
    scans = []
    for k in range(n_kf):
        d = np.linalg.norm(world[:, :2] - xy[k], axis=1)
        sel = np.flatnonzero(d < scan_range)
        sel = rng.choice(sel, min(len(sel), pts_per_scan * 3), replace=False)
        p = world[sel] + rng.normal(0, 0.02, (len(sel), 3))
        local = (p - gt[k][:3, 3]) @ gt[k][:3, :3]                  # sensor frame (PosePcd::pcd_, PP:39)
        local = synth.voxel_centroids(local, 0.2)
        if len(local) > pts_per_scan:
            local = local[np.sort(rng.choice(len(local), pts_per_scan, replace=False))]
        scans.append(local.astype(np.float32))
    odom = [gt[0].copy()]
    for k in range(1, n_kf):
        rel = inv(gt[k - 1]) @ gt[k]
        noise = exp_se3(np.r_[0, 0, rng.normal(0, drift_yaw) + yaw_bias, rng.normal(0, drift_xy, 2), 0])   # biased yaw drift
        odom.append(odom[-1] @ rel @ noise)
    return scans, gt, odom, np.arange(n_kf) * 1.0


def make_lidar_stream(n_kf, seed, lidar=None, drift_yaw=0.004, drift_xy=0.03, yaw_bias=0.006):
    """The figure-8 of make_stream seen by a spinning LiDAR: the scene's primitives, the sensor, one noise seed per keyframe and the
    ground-truth / odometry poses.  The keyframe clouds are ray-cast from the ground-truth poses (sensor frame): on the GPU straight into
    the keyframe store (KeyframeStore.add_lidar_scans), for the oracle by the numpy twin synth.lidar_scan - the same bits."""
    from qn_amd import synth
    lidar = synth.SpinningLidar(n_beams=32, n_cols=360) if lidar is None else lidar      # few columns: the oracle casts with numpy
    rng = np.random.default_rng(seed)
    scene = synth.Scene(rng, 120.0)
    s = np.linspace(0, 2 * np.pi, n_kf, endpoint=False)
    xy = np.c_[30 * np.sin(s), 22 * np.sin(2 * s)]
    head = np.arctan2(np.gradient(xy[:, 1]), np.gradient(xy[:, 0]))
    gt = []
    for k in range(n_kf):
        T = np.eye(4); T[:3, :3] = synth._rot_zyx(head[k], 0, 0); T[:3, 3] = [xy[k, 0], xy[k, 1], 1.8]
        gt.append(T)
    seeds = rng.integers(0, 2 ** 32, n_kf).astype(np.uint32)
    odom = [gt[0].copy()]
    for k in range(1, n_kf):
        rel = inv(gt[k - 1]) @ gt[k]
        noise = exp_se3(np.r_[0, 0, rng.normal(0, drift_yaw) + yaw_bias, rng.normal(0, drift_xy, 2), 0])
        odom.append(odom[-1] @ rel @ noise)
    return scene.primitives(), lidar, seeds, gt, odom, np.arange(n_kf) * 1.0


MOVING_BOX_SIZE = (4.0, 2.0, 1.5)                                  # length (x), width (y), height [m]


def moving_box_lane(j):
    """the line y = const box j drives along"""
    return 6.0 + 9.0 * j


def moving_box_prims(n_boxes, k):
    """the n_boxes PRIM_BOX primitives of keyframe k: box j drives along its lane, 2.5 m further in x per keyframe (wrapping over -35 .. 35)"""
    from qn_amd import synth
    return np.array([(synth.PRIM_BOX, (-35.0 + (2.5 * k + 23.0 * j) % 70.0, moving_box_lane(j)) + MOVING_BOX_SIZE + (0.0,)) for j in range(n_boxes)], dtype=synth.PRIM_DTYPE)


def rot_to_quat(R):
    """(qx, qy, qz, qw) of a rotation matrix (what tf::Matrix3x3::getRotation yields in poseEigToPoseStamped, utilities.hpp)"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2; q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2; q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2; q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2; q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    return np.array(q)


def write_kitti_tum(save_dir, poses, stamps):
    """saveFlagCallback's pose files (fast_lio_sam_qn.cpp:344-373): KITTI = the 3x4 [R|t] row by row with the stream's default
    formatting (6 significant digits), TUM = header line + `stamp x y z qx qy qz qw`, fixed, 8 decimals."""
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "poses_kitti.txt"), "w") as fk, open(os.path.join(save_dir, "poses_tum.txt"), "w") as ft:
        ft.write("#timestamp x y z qx qy qz qw\n")
        for T, st in zip(poses, stamps):
            fk.write(" ".join("%g" % T[r, c] for r in range(3) for c in range(4)) + "\n")
            q = rot_to_quat(T[:3, :3])
            ft.write("%.8f %.8f %.8f %.8f %.8f %.8f %.8f %.8f\n" % (st, T[0, 3], T[1, 3], T[2, 3], q[0], q[1], q[2], q[3]))


def write_pcd_xyzi(path, pts):
    """PCD v0.7 ASCII, FIELDS x y z intensity (what pcl::io::savePCDFileASCII writes for a PointXYZI cloud)."""
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(pts), len(pts)))
        for p in pts:
            f.write("%.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], p[3]))


def write_grid(save_dir, stem, info, occupancy):
    """stem.pgm and stem.yaml in map_server's conventions (qn_amd/mapground.to_pgm / map_yaml)"""
    from qn_amd import mapground
    with open(os.path.join(save_dir, stem + ".pgm"), "wb") as f:
        f.write(mapground.to_pgm(occupancy))
    with open(os.path.join(save_dir, stem + ".yaml"), "w") as f:
        f.write(mapground.map_yaml(info, stem + ".pgm"))


def write_pcd_voxels(path, centres, hits, misses):
    """PCD v0.7 ASCII, FIELDS x y z hits misses: the centres of voxels of the 3-D occupancy map with their counts"""
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z hits misses\nSIZE 4 4 4 4 4\nTYPE F F F U U\nCOUNT 1 1 1 1 1\n"
                "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(centres), len(centres)))
        for c, h, m in zip(centres, hits, misses):
            f.write("%.9g %.9g %.9g %d %d\n" % (np.float32(c[0]), np.float32(c[1]), np.float32(c[2]), h, m))


def write_occupancy(save_dir, result, slice_z=None):
    """the 3-D occupancy map `result` (the dict of qn_amd/mapoccupancy.classify, or the GPU's arrays in the same form) as occupied.pcd - the centres of the
    occupied voxels with their hits and misses - and, with slice_z = (z_lo, z_hi) in metres, occupancy_slice.pgm / .yaml: the layers those heights fall in,
    flattened (mapground.to_pgm / map_yaml: here free means that a ray passed); with result["d2_slice"] (the distance field's slice2d) and
    result["robot_radius"] in metres also occupancy_inflated.pgm / .yaml, the slice with every column occupied whose clearance over those layers is at most the
    radius: d2 <= floor((radius / voxel)^2) (mapdistance.inflate) -> the layers (iz_lo, iz_hi) or None"""
    from qn_amd import mapdistance, mapground, mapoccupancy
    g = mapoccupancy.OccupancyGrid(*result["grid"])
    ijk, hits, misses = mapoccupancy.voxel_list(result, 1 << mapoccupancy.OCCUPIED)
    write_pcd_voxels(os.path.join(save_dir, "occupied.pcd"), mapoccupancy.centres(ijk, g), hits, misses)
    if slice_z is None:
        return None
    lo, hi = mapoccupancy.layer_of(slice_z[0], g), mapoccupancy.layer_of(slice_z[1], g)
    occ = result["slice"](lo, hi) if "slice" in result else mapoccupancy.slice2d(result["classes"], lo, hi)
    write_grid(save_dir, "occupancy_slice", mapground.GridInfo(g.origin[0], g.origin[1], g.voxel, g.width, g.height, 0), occ)
    if "d2_slice" in result:                                                                      # the slice inflated by the robot's radius
        r2 = int(np.floor((float(result["robot_radius"]) / float(g.voxel)) ** 2))
        d2 = result["d2_slice"](lo, hi)
        write_grid(save_dir, "occupancy_inflated", mapground.GridInfo(g.origin[0], g.origin[1], g.voxel, g.width, g.height, 0), mapdistance.inflate(occ, d2, r2))
    return lo, hi


def write_pcd_xyzi_normal(path, pts, normals, curvature):
    """PCD v0.7 ASCII, FIELDS x y z intensity normal_x normal_y normal_z curvature (a PointXYZINormal cloud); a point without a normal carries nan"""
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4 4\n"
                "TYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(pts), len(pts)))
        for p, n, c in zip(pts, normals, curvature):
            f.write("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], p[3], n[0], n[1], n[2], c))


def write_pcd_labelled(path, pts, label, normals=None, curvature=None):
    """PCD v0.7 ASCII, FIELDS x y z intensity [normal_x normal_y normal_z curvature] label: the integer cluster number of every point (-1: in a rejected
    clump, -2: not clustered at all)"""
    nf = 4 if normals is None else 8
    names = "x y z intensity" + ("" if normals is None else " normal_x normal_y normal_z curvature") + " label"
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s I\nCOUNT %s\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
                "POINTS %d\nDATA ascii\n" % (names, " ".join(["4"] * (nf + 1)), " ".join(["F"] * nf), " ".join(["1"] * (nf + 1)), len(pts), len(pts)))
        for i, p in enumerate(pts):
            v = [p[0], p[1], p[2], p[3]] + ([] if normals is None else [normals[i][0], normals[i][1], normals[i][2], curvature[i]])
            f.write(" ".join("%.9g" % x for x in v) + " %d\n" % label[i])


def write_clusters_csv(path, clusters):
    """one row per cluster of KeyframeStore.map_clusters: id, size, the box and the centroid (f32 / f64 values printed so that they read back exactly)"""
    with open(path, "w") as f:
        f.write("id,size,min_x,min_y,min_z,max_x,max_y,max_z,centroid_x,centroid_y,centroid_z\n")
        for j in range(len(clusters["size"])):
            f.write("%d,%d,%s,%s,%s\n" % (j, clusters["size"][j], ",".join("%.9g" % v for v in clusters["lo"][j]), ",".join("%.9g" % v for v in clusters["hi"][j]),
                                          ",".join("%.17g" % v for v in clusters["centroid"][j])))


def ate(poses, gt):
    return float(np.sqrt(np.mean([np.sum((a[:3, 3] - b[:3, 3]) ** 2) for a, b in zip(poses, gt)])))


def _oracle_relative(orc, scans, poses, k, c, yaw, submap_range, voxel, max_corr_dist, score_thr):
    """verify_loop_candidates for one candidate on the CPU oracle: the same clouds and guess from the twins"""
    from qn_amd import scancontext, engine
    sub = engine.loop_submap_ids(k, c, submap_range, False, False, len(poses))[1]
    src = orc.assemble_submap(scans, {k: np.eye(4)}, [k], voxel)
    dst = orc.assemble_submap(scans, {i: scancontext.relative_pose(poses[c], poses[i]) for i in sub}, sub, voxel)
    g = orc.GicpOracle(k=15, max_iter=32, max_corr_dist=max_corr_dist, trans_eps=0.01)
    g.set_source(src); g.compute_covariances(0); g.set_target(dst); g.compute_covariances(1)
    r = g.align(scancontext.seed_from_yaw(yaw).astype(np.float64))
    return dict(valid=bool(r["converged"] and r["fitness"] < score_thr), converged=r["converged"], score=r["fitness"], T=r["Tf"].astype(np.float64), _src=src, _dst=dst)


def _oracle_scan_c2f(orc, scans, q, c, voxel, max_corr_dist, score_thr):
    """verify_loop_pairs_c2f for one pair on the CPU oracle: scan to scan, each in its own sensor frame"""
    src, dst = orc.voxel_grid(scans[q], voxel), orc.voxel_grid(scans[c], voxel)
    r = dict(orc.coarse_to_fine_alignment(src, dst, max_corr_dist=max_corr_dist, score_thr=score_thr))
    r["_src"] = src; r["_dst"] = dst
    return r


def _overlap_figures(rec):
    from qn_amd import overlap
    return dict(overlap_ab=overlap.overlap_fraction(rec["a_to_b"]), overlap_ba=overlap.overlap_fraction(rec["b_to_a"]),
                rmse_ab=overlap.inlier_rmse(rec["a_to_b"]), rmse_ba=overlap.inlier_rmse(rec["b_to_a"]))


def _oracle_overlap(r, radius):
    """the twin on the oracle's own clouds: the source through the pair's T (f64, rounded to f32) against the target"""
    from qn_amd import overlap
    src = np.asarray(r["_src"], np.float64)[:, :3]; T = np.asarray(r["T"], np.float64)
    final = (src @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return _overlap_figures(overlap.overlap(final, np.asarray(r["_dst"], np.float32)[:, :3], radius))


def _oracle_submap_relative(orc, scans, poses, q, c, yaw, submap_range, voxel, max_corr_dist, score_thr, use_quatro):
    """verify_loop_pairs_submap[_c2f] for one pair on the CPU oracle: both local submaps assembled from the twins, each in its centre's sensor frame"""
    from qn_amd import scancontext, engine
    def local(x):
        sub = engine.local_submap_ids(x, submap_range, len(poses))
        return orc.assemble_submap(scans, {i: scancontext.relative_pose(poses[x], poses[i]) for i in sub}, sub, voxel)
    src, dst = local(q), local(c)
    if use_quatro:
        r = dict(orc.coarse_to_fine_alignment(src, dst, max_corr_dist=max_corr_dist, score_thr=score_thr))
        r["_src"] = src; r["_dst"] = dst
        return r
    g = orc.GicpOracle(k=15, max_iter=32, max_corr_dist=max_corr_dist, trans_eps=0.01)
    g.set_source(src); g.compute_covariances(0); g.set_target(dst); g.compute_covariances(1)
    r = g.align(scancontext.seed_from_yaw(yaw).astype(np.float64))
    return dict(valid=bool(r["converged"] and r["fitness"] < score_thr), converged=r["converged"], score=r["fitness"], T=r["Tf"].astype(np.float64), _src=src, _dst=dst)


def run(n_kf=70, seed=7, use_quatro=False, radius=12.0, tdiff=15.0, voxel=0.3, submap_range=5, score_thr=1.5, verbose=True, backend="gpu", save_dir=None,
        save_map_leaf=None, sensor="uniform", detector="radius", sc_max_dist=0.3, yaw_bias=0.006, verify="reference", sc_top_k=1, loop_every=1, catch_up=False,
        submap_matching=False, min_overlap=None, overlap_radius=None, max_see_through=None, range_params=None, static_map=False, static_radius=15.0,
        static_max_k=8, moving_boxes=0, save_map_normals=False, normal_radius=0.6, normal_min_neighbors=5, map_outliers=False,
        outlier_radius=1.0, outlier_k=8, outlier_std=2.0, occupancy_grid=False, grid_cell=0.5, max_slope=0.3, ground_tol=0.2, clearance=2.0,
        drop_ground=False, map_clusters=False, cluster_tol=0.5, cluster_min=10, cluster_max=0xffffffff, drop_small_clusters=False,
        localize_every=0, localize_radius=35.0, localize_shift=0.5, localize_yaw=3.0, occupancy_3d=False, occ_voxel=0.3, occ_min_range=0.5,
        occ_max_range=60.0, occ_shell=1, occ_slice=None, occ_distance=False, occ_dist_max=16, occ_unknown_obstacle=False, robot_radius=None, occ_route=None,
        route_from=None, route_min_d2=4, route_planar=False, occ_frontiers=False, frontier_min_size=8, occ_view_gain=False, view_range=20.0, view_beams=16, view_azimuth=300,
        occ_incremental=False):
    """sensor = "uniform": keyframe clouds sampled uniformly by area inside a disc (make_stream); "spinning": ray-cast spinning-LiDAR
    scans from the ground-truth poses of the same figure-8 (make_lidar_stream).  detector = "radius": the candidate is the closest older
    keyframe within `radius` of the corrected position (LC:34-56); "scancontext": the older keyframe nearest by Scan Context distance, kept
    when that is below sc_max_dist - on the GPU from the resident keyframes (KeyframeStore.sc_describe / sc_query), for the oracle backend by
    the numpy twin qn_amd.scancontext.  yaw_bias: the odometry's heading drift per keyframe [rad].
    verify = "reference": the candidate's registration as loop_closure.cpp does it (both clouds in the world frame of the corrected poses, GICP from
    identity).  "relative" (with detector="scancontext"): the query's top sc_top_k candidates with D < sc_max_dist in ONE drift-free verification
    (KeyframeStore.verify_loop_candidates: the query scan in its sensor frame against each candidate's window in the candidate's sensor frame, seeded
    with its Scan Context heading); the valid one with the lowest score gives the loop factor Z = inv(T), variance = score.  The oracle backend
    rebuilds the same clouds and guesses from the twins (scancontext.relative_pose / seed_from_yaw) and registers them with the CPU oracle.
    "relative" with use_quatro (the reference's default check, scan to scan): every keyframe is described on arrival (KeyframeStore.quatro_describe:
    its voxel grid in its sensor frame and its FPFH, kept resident) and the candidates go through ONE verify_loop_candidates_c2f (Quatro -> transformPcd
    -> Nano-GICP from the resident features, no pose involved); the oracle backend runs oracle.coarse_to_fine_alignment on oracle.voxel_grid of the
    sensor-frame scans.
    loop_every = N > 1 (verify="relative", detector="scancontext"): the loop timer fires after every N-th keyframe instead of after each one (loop_update_hz,
    fast_lio_sam_qn.cpp:203-252); every keyframe is described on arrival.  Without catch_up a tick checks only the newest keyframe, as the reference's
    timer does (keyframes_.back()); with catch_up it checks every keyframe added since the last tick: one sc_query for all of them, then ONE
    verify_loop_pairs (verify_loop_pairs_c2f with use_quatro) for all their pairs; each query's best valid candidate becomes a factor (Z = inv(T),
    variance = score), then one optimisation.  The oracle backend runs the same pairs through the twins and the CPU oracle.  loop_every = 1 is the loop above.
    submap_matching (verify="relative"; the reference's enable_submap_matching, made drift-free): both sides of a pair are local submaps, the keyframes within
    submap_range of the query / the candidate, each submap in its centre's own sensor frame and placed with the RAW ODOMETRY poses, so no pose-graph update
    ever invalidates one.  At a tick the keyframes involved are described (KeyframeStore.submap_describe, with FPFH rows when use_quatro) unless their entry
    is still current - a window is final once submap_range later keyframes exist - and the pairs go through ONE verify_loop_pairs_submap
    (verify_loop_pairs_submap_c2f with use_quatro).  The oracle backend assembles the same windows (orc.assemble_submap, scancontext.relative_pose).
    min_overlap = F with overlap_radius = R (verify="relative"; default None: off, the run is what it is without them): after every verification the two-way
    overlap of each pair is measured (KeyframeStore.verify_overlap on the pairs' resident clouds; the oracle backend runs the twin qn_amd.overlap on its own
    clouds), printed per attempt, and a pair counts as valid only if the registration says so AND both directions' overlap are >= F.  A single query's
    candidates then go through the many-pair verify calls (the same records), which keep what verify_overlap needs.  out["overlaps"]: one dict per pair.
    max_see_through = F (verify="relative"; default None: off, the run is what it is without it): every keyframe's range images are made on arrival
    (KeyframeStore.range_describe; range_params, a freespace.Params, defaults to the simulated sensor's image, or to a 32 x 360 image over +-60 degrees for
    the uniform clouds), after every verification each pair's T goes through the free-space check (KeyframeStore.freespace_batch, one pass for all pairs; the
    oracle backend runs the twin qn_amd.freespace on the raw scans), printed per attempt, and a pair counts as valid only if it was valid so far AND neither
    direction's share of observed points that the other scan saw through exceeds F.  out["see_through"]: one dict per pair.
    static_map (the GPU backend, with save_dir and save_map_leaf; default False: the run is what it is without it): after the run every keyframe's range images
    are made (unless max_see_through made them on arrival), every record of every keyframe is checked against the images of its static_max_k nearest keyframes
    within static_radius under the corrected poses (KeyframeStore.static_classify), and map_static.pcd - map.pcd without the records voted out - is written
    beside map.pcd (KeyframeStore.build_map_static).  out["static_removed"]: the records removed, out["static_map_points"] / out["map_points"]: the maps' sizes.
    save_map_normals (the GPU backend, with save_dir and save_map_leaf; default False): map.pcd (and map_static.pcd) carry normal_x normal_y normal_z curvature
    beside x y z intensity - every map point's surface normal from its neighbours within normal_radius (at least normal_min_neighbors of them, else nan), turned
    towards the nearest corrected keyframe position, on the device from the resident map (KeyframeStore.map_normals).  out["map_normals_valid"]: the points of
    map.pcd that have one.
    map_outliers (the GPU backend, with save_dir and save_map_leaf; default False): the map (and the static map) is filtered on the device before it is
    written and before its normals are made: every point with fewer than outlier_k neighbours within outlier_radius, or whose mean distance to its outlier_k
    nearest exceeds the map's mean by more than outlier_std standard deviations, is removed (KeyframeStore.map_outliers / map_remove_outliers).
    out["map_outliers_removed"] (and out["static_outliers_removed"]): the points removed; out["map_points"] / out["static_map_points"]: what was written.
    occupancy_grid (with save_dir and save_map_leaf; default False): the ground of the map as it is written - after the outlier filter when given - is
    segmented and the map flattened into map.pgm and map.yaml, the 2-D occupancy grid a planner or map_server loads (columns of grid_cell m; ground slopes up
    to max_slope rise over run; a point within ground_tol of the ground envelope is ground, one up to clearance above it occupies its column, one higher does
    not: qn_amd/mapground.py), and with static_map map_static.pgm / map_static.yaml beside map_static.pcd.  On the GPU backend by KeyframeStore.map_ground /
    map_ground_grid; on the oracle backend, which has no map of its own, the map is the oracle's voxel grid over every keyframe (map.pcd, intensity 0) and the
    grid the numpy twin's.  out["grid"]: width, height, occupied, free, unknown, n_ground.  drop_ground (with occupancy_grid): map.pcd is written without its
    GROUND class (KeyframeStore.map_keep_classes), the grid still comes from the whole map.
    map_clusters (the GPU backend, with save_dir and save_map_leaf; default False): the points of the map are clustered into objects on the device
    (KeyframeStore.map_clusters: joined within cluster_tol, a clump of cluster_min .. cluster_max points is a cluster) - with occupancy_grid what stands on the
    ground (the OBSTACLE and OVERHEAD classes, after the ground call), otherwise every finite point.  map.pcd gains an integer field label (the cluster's
    number, -1 in a rejected clump, -2 not clustered) and clusters.csv lists id, size, box and centroid (with static_map: map_static.pcd and
    clusters_static.csv too).  drop_small_clusters: the rejected clumps leave the map (KeyframeStore.map_drop_rejected_clusters).  The filters run in the order
    outliers, ground, clusters, drop_ground, normals; with drop_small_clusters and drop_ground both, the ground that leaves is that of the map without the
    clumps, segmented again.  out["clusters"] (and out["static_clusters"]): clusters, components, too_small, too_large, clustered_points, rejected_points.
    localize_every = N > 0 (the GPU backend, with save_dir; default 0: off): once the corrected map stands (the map map.pcd is written from, filters included;
    without save_map_leaf a map at `voxel`), every N-th keyframe is localised in it on the device (KeyframeStore.map_localize, map_localize_c2f with use_quatro)
    from its corrected pose displaced by localize_shift metres and localize_yaw degrees, against the crop of localize_radius around that guess (a radius below
    the scans' reach leaves far scan points without a partner and raises the score).  localized_tum.txt: one row per chosen keyframe, the pose found.
    out["localized"]: per chosen keyframe id, valid, status, score and the translation [m] / rotation [rad] error of guess and result against the corrected pose
    the map was built with (guess_t_err, guess_r_err, t_err, r_err).
    occupancy_3d (with save_dir; default False): the rays of every keyframe - from its corrected sensor position to each of its records within occ_min_range ..
    occ_max_range - are walked through a grid of occ_voxel metres (qn_amd/mapoccupancy.py: a hit where a ray ends, a miss in the voxels it crossed but the last
    occ_shell), on the GPU backend by KeyframeStore.map_occupancy, on the oracle backend by the numpy twin.  occupied.pcd: the centres of the occupied voxels,
    FIELDS x y z hits misses.  occ_slice = (z_lo, z_hi) in metres: also occupancy_slice.pgm / .yaml, the layers of those heights flattened to the grid a planner
    loads (occupied where any voxel is, else free where a ray passed, else unknown).  out["occupancy"]: rays, total_misses, width, height, depth, occupied, free,
    unknown, and slice_layers with occ_slice.
    occ_incremental (with occupancy_3d; default False): the volume is kept live through the run instead of being built once at the end - after every loop-timer
    tick it is brought to the current estimate of every keyframe's pose (KeyframeStore.map_occupancy_update on the GPU backend, mapoccupancy.update on the oracle
    backend: the keyframes whose pose did not change are kept, the others walked out and in again), and once more with the final poses.  The files written and
    out["occupancy"] are those of the one-shot run; out["occupancy"] also has updates, the number of calls, entries_listed, the sum of their list lengths, and
    entries_walked, the entries they added plus those they removed.
    occ_distance (with occupancy_3d; default False): the exact Euclidean distance field of that volume (qn_amd/mapdistance.py: per voxel the squared distance in
    voxels to the nearest occupied voxel - with occ_unknown_obstacle to the nearest occupied or unknown one - up to occ_dist_max voxels), on the GPU backend by
    KeyframeStore.map_distance, on the oracle backend by the numpy twin.  out["distance"]: sites, reached, far, max_d2, sum_d2, site_mask, max_dist.
    robot_radius = M metres (with occ_distance and occ_slice): also occupancy_inflated.pgm / .yaml, the slice with every column occupied whose clearance over
    the slice's layers is at most M: d2 <= floor((M / occ_voxel)^2).
    occ_route = (GX, GY, GZ) in metres (with occupancy_3d and occ_distance; default None): the cost-to-go field to that goal through the free voxels whose d2 is at
    least route_min_d2 (qn_amd/maproute.py: the 3-4-5 chamfer cost of the shortest path, no corner cut), on the GPU backend by KeyframeStore.map_route, on the
    oracle backend by the numpy twin, and the path down it from route_from = (X, Y, Z) (default: the last corrected keyframe position).  route_planar: the field
    of columns instead, every voxel of a column over the band passable - the band being the layers of occ_slice, or without it the goal's layer.
    out["route"]: passable, blocked, reached, unreached, goals_used, goals_blocked, max_cost, sum_cost, the parameters used, path_len and path_cost (None when
    the start is outside, blocked or cut off).  route.csv: "x y z cost" per voxel of the path, the voxel's centre in metres and its cost, start first.
    occ_frontiers (with occupancy_3d; default False): the exploration frontiers of that volume - the free voxels with an unknown face neighbour, the space outside
    the grid unknown too, grouped into 26-connected regions of at least frontier_min_size voxels (qn_amd/mapfrontier.py), over the layers of occ_slice when
    given, else over all - on the GPU backend by KeyframeStore.map_frontiers, on the oracle backend by the numpy twin.  It needs neither occ_distance nor
    occ_route.  out["frontiers"]: candidates, frontier, components, regions, too_small, region_voxels, rejected_voxels, largest, unknown_faces and the parameters
    used.  frontiers.csv: one row per region, "region size faces cx cy cz lo_x lo_y lo_z hi_x hi_y hi_z" - its number, voxels, unknown faces, centroid in metres
    and box of grid indices; with occ_route the row also carries "reach ex ey ez", the cost in metres of reaching the region down the route field (inf when no
    voxel of it is reached) and the centre of the voxel where it is entered (nan then).
    occ_view_gain (with occupancy_3d and occ_frontiers; default False): next-best-view gain, one viewpoint per frontier region - with occ_route the centre of the
    region's cheapest voxel under the route field (its root voxel when no voxel of it is reached), else the centre of its root voxel.  From each viewpoint the rays
    of a spinning sensor of view_beams beams between -15 and 15 degrees, view_azimuth steps a turn and view_range metres (mapview.sensor_offsets) are cast through
    the volume until an occupied voxel, and the distinct unknown voxels they pass through are counted (qn_amd/mapview.py) - on the GPU backend by
    KeyframeStore.map_view_gain, on the oracle backend by the numpy twin.  out["view_gain"]: viewpoints, outside, rays, covered, max_cover, total_gain, steps and
    the sensor.  view_gain.csv: one row per region, "region x y z gain blocked escaped spent reached" - the viewpoint in metres, its gain and its rays by their
    end.  frontiers.csv stays as it is.
    moving_boxes = N (sensor="spinning" only; default 0: every run is what it was): N extra boxes in the scene that stand somewhere else in every keyframe
    (moving_box_prims), so every keyframe is cast by a call of its own."""
    if detector not in ("radius", "scancontext"):
        raise ValueError("detector must be 'radius' or 'scancontext', not %r" % (detector,))
    if verify not in ("reference", "relative"):
        raise ValueError("verify must be 'reference' or 'relative', not %r" % (verify,))
    if verify == "relative" and detector != "scancontext":
        raise ValueError("verify='relative' needs detector='scancontext' (it is seeded with the Scan Context heading)")
    if int(loop_every) < 1:
        raise ValueError("loop_every must be >= 1, not %r" % (loop_every,))
    if (loop_every > 1 or catch_up) and (verify != "relative" or detector != "scancontext"):
        raise ValueError("loop_every > 1 / catch_up need verify='relative' and detector='scancontext'")
    if submap_matching and verify != "relative":
        raise ValueError("submap_matching needs verify='relative' (the reference's world-frame submap matching is verify='reference' without it)")
    gate = min_overlap is not None
    if gate and verify != "relative":
        raise ValueError("min_overlap needs verify='relative' (the verify calls that keep their pairs' clouds)")
    if gate and not (overlap_radius is not None and np.isfinite(overlap_radius) and overlap_radius > 0):
        raise ValueError("min_overlap needs overlap_radius > 0, not %r" % (overlap_radius,))
    fgate = max_see_through is not None
    if fgate and verify != "relative":
        raise ValueError("max_see_through needs verify='relative' (a transform between two sensor frames)")
    if fgate and not (np.isfinite(max_see_through) and max_see_through >= 0):
        raise ValueError("max_see_through must be a fraction >= 0, not %r" % (max_see_through,))
    if int(moving_boxes) != moving_boxes or moving_boxes < 0:
        raise ValueError("moving_boxes must be a whole number >= 0, not %r" % (moving_boxes,))
    if moving_boxes and sensor != "spinning":
        raise ValueError("moving_boxes needs sensor='spinning' (the boxes are primitives of the ray-cast scene)")
    if static_map and backend != "gpu":
        raise ValueError("static_map needs backend='gpu' (the oracle backend writes no map)")
    if static_map and (save_dir is None or save_map_leaf is None):
        raise ValueError("static_map needs save_dir and save_map_leaf (map_static.pcd is written beside map.pcd)")
    if static_map and not (np.isfinite(save_map_leaf) and save_map_leaf > 0):
        raise ValueError("static_map needs save_map_leaf > 0, not %r" % (save_map_leaf,))
    if static_map and not (np.isfinite(static_radius) and static_radius >= 0 and int(static_max_k) == static_max_k and 0 <= static_max_k <= 255):
        raise ValueError("static_map needs static_radius >= 0 and 0 <= static_max_k <= 255, not %r / %r" % (static_radius, static_max_k))
    if save_map_normals and backend != "gpu":
        raise ValueError("save_map_normals needs backend='gpu' (the oracle backend writes no map)")
    if save_map_normals and (save_dir is None or save_map_leaf is None):
        raise ValueError("save_map_normals needs save_dir and save_map_leaf (the normals are fields of map.pcd)")
    if save_map_normals and not (np.isfinite(normal_radius) and normal_radius > 0 and int(normal_min_neighbors) == normal_min_neighbors and normal_min_neighbors >= 3):
        raise ValueError("save_map_normals needs normal_radius > 0 and normal_min_neighbors >= 3, not %r / %r" % (normal_radius, normal_min_neighbors))
    if map_outliers and backend != "gpu":
        raise ValueError("map_outliers needs backend='gpu' (the oracle backend writes no map)")
    if map_outliers and (save_dir is None or save_map_leaf is None):
        raise ValueError("map_outliers needs save_dir and save_map_leaf (it filters the map that map.pcd is written from)")
    if map_outliers and not (np.isfinite(outlier_radius) and outlier_radius > 0 and np.isfinite(outlier_std) and outlier_std >= 0 and int(outlier_k) == outlier_k
                             and 1 <= outlier_k <= 32):
        raise ValueError("map_outliers needs outlier_radius > 0, outlier_std >= 0 and 1 <= outlier_k <= 32, not %r / %r / %r" % (outlier_radius, outlier_std, outlier_k))
    if occupancy_grid and (save_dir is None or save_map_leaf is None):
        raise ValueError("occupancy_grid needs save_dir and save_map_leaf (the grid is made from the map that map.pcd is written from)")
    if drop_ground and not occupancy_grid:
        raise ValueError("drop_ground needs occupancy_grid (the ground comes from its segmentation)")
    if occupancy_grid:
        from qn_amd import mapground
        mapground.units((grid_cell, max_slope, ground_tol, clearance, 1))                         # (raises ValueError on a parameter outside its range)
    if occ_slice is not None and not occupancy_3d:
        raise ValueError("occ_slice needs occupancy_3d (the slice is cut from its volume)")
    if occupancy_3d and save_dir is None:
        raise ValueError("occupancy_3d needs save_dir (occupied.pcd is written there)")
    if occupancy_3d:
        from qn_amd import mapoccupancy
        occ_params = mapoccupancy.OccupancyParams(occ_voxel, occ_min_range, occ_max_range, occ_shell)
        mapoccupancy.check_params(occ_params)                                                     # (raises ValueError on a parameter outside its range)
        if occ_slice is not None and not (len(occ_slice) == 2 and np.isfinite(occ_slice).all() and occ_slice[0] <= occ_slice[1]):
            raise ValueError("occ_slice must be two finite heights z_lo <= z_hi, not %r" % (occ_slice,))
    if occ_incremental and not occupancy_3d:
        raise ValueError("occ_incremental needs occupancy_3d (it keeps that volume live)")
    if (occ_distance or robot_radius is not None or occ_unknown_obstacle) and not (occupancy_3d and occ_distance):
        raise ValueError("occ_distance needs occupancy_3d, and occ_unknown_obstacle and robot_radius need occ_distance (the field is computed from its volume)")
    if occ_distance:
        from qn_amd import mapdistance
        dist_params = mapdistance.DistanceParams((1 << mapoccupancy.OCCUPIED) | ((1 << mapoccupancy.UNKNOWN) if occ_unknown_obstacle else 0), occ_dist_max)
        mapdistance.check_params(dist_params)                                                     # (raises ValueError on a parameter outside its range)
        if robot_radius is not None and not (np.isfinite(robot_radius) and robot_radius >= 0.0):
            raise ValueError("robot_radius must be finite and >= 0, not %r" % (robot_radius,))
    if (occ_route is None) and (route_from is not None or route_planar or route_min_d2 != 4):
        raise ValueError("route_from, route_min_d2 and route_planar need occ_route")
    if occ_route is not None:
        if not (occupancy_3d and occ_distance):
            raise ValueError("occ_route needs occupancy_3d and occ_distance (the field is computed from the volume and its distance field)")
        from qn_amd import maproute
        for name, v in (("occ_route", occ_route), ("route_from", route_from)):
            if v is not None and not (len(v) == 3 and np.isfinite(np.asarray(v, np.float64)).all()):
                raise ValueError("%s must be three finite coordinates, not %r" % (name, v))
        maproute.check_params(maproute.RouteParams(1 << mapoccupancy.FREE, route_min_d2, 0, 0, int(bool(route_planar))), occ_dist_max)
    if (occ_frontiers or frontier_min_size != 8) and not (occupancy_3d and occ_frontiers):
        raise ValueError("occ_frontiers needs occupancy_3d, and frontier_min_size needs occ_frontiers (the regions are found in its volume)")
    if occ_frontiers:
        from qn_amd import mapfrontier
        mapfrontier.check_params(mapfrontier.FrontierParams(min_size=frontier_min_size))          # (raises ValueError on a parameter outside its range)
    if (occ_view_gain or view_range != 20.0 or view_beams != 16 or view_azimuth != 300) and not (occupancy_3d and occ_frontiers and occ_view_gain):
        raise ValueError("occ_view_gain needs occupancy_3d and occ_frontiers, and view_range, view_beams and view_azimuth need occ_view_gain (a viewpoint per region)")
    if occ_view_gain:
        from qn_amd import mapview
        if not (isinstance(view_beams, (int, np.integer)) and isinstance(view_azimuth, (int, np.integer)) and view_beams >= 1 and view_azimuth >= 1 and
                view_beams * view_azimuth <= mapview.MAX_RAYS):
            raise ValueError("view_beams and view_azimuth must be integers >= 1 with at most 2^20 rays in all")
        if not (np.isfinite(view_range) and view_range > 0):
            raise ValueError("view_range must be finite and > 0")
        view_offsets = mapview.sensor_offsets(occ_voxel, view_range, view_beams, view_azimuth, -15.0, 15.0)      # (raises ValueError beyond the offset limit)
    if drop_small_clusters and not map_clusters:
        raise ValueError("drop_small_clusters needs map_clusters (the clumps come from its components)")
    if map_clusters and backend != "gpu":
        raise ValueError("map_clusters needs backend='gpu' (the oracle backend writes no map of its own)")
    if map_clusters and (save_dir is None or save_map_leaf is None):
        raise ValueError("map_clusters needs save_dir and save_map_leaf (the labels are a field of map.pcd)")
    if map_clusters:
        from qn_amd import mapclusters
        mapclusters.check_params(mapclusters.ClusterParams(cluster_tol, cluster_min, cluster_max, 0))      # (raises ValueError on a parameter outside its range)
    if int(localize_every) != localize_every or localize_every < 0:
        raise ValueError("localize_every must be a whole number >= 0, not %r" % (localize_every,))
    if localize_every and backend != "gpu":
        raise ValueError("localize_every needs backend='gpu' (the map it localises in is the store's)")
    if localize_every and save_dir is None:
        raise ValueError("localize_every needs save_dir (localized_tum.txt is written there)")
    if localize_every and not (np.isfinite(localize_radius) and localize_radius > 0 and np.isfinite(localize_shift) and np.isfinite(localize_yaw)):
        raise ValueError("localize_every needs localize_radius > 0 and a finite shift and yaw, not %r / %r / %r" % (localize_radius, localize_shift, localize_yaw))
    overlaps = []; see_through = []; fs_images = {}

    def apply_freespace(rs, pairs):
        """check every pair's T against the two keyframes' range images, print, and clear `valid` where either direction is seen through too much"""
        if not fgate:
            return rs
        from qn_amd import freespace
        live = [j for j, r in enumerate(rs) if np.all(np.isfinite(np.asarray(r["T"], np.float64)))]
        recs = {}
        if live and backend == "gpu":
            out = store.freespace_batch([ids[pairs[j][0]] for j in live], [ids[pairs[j][1]] for j in live], [rs[j]["T"] for j in live])
            recs = dict(zip(live, out))
        elif live:
            for j in live:
                q, c = pairs[j]
                for x in (q, c):
                    if x not in fs_images:
                        fs_images[x] = freespace.range_images(scans[x], fs_params)
                recs[j] = freespace.freespace(scans[q], scans[c], rs[j]["T"], fs_params, q_images=fs_images[q], c_images=fs_images[c])
        for j, (r, (q, c)) in enumerate(zip(rs, pairs)):
            f = dict(query=q, cand=c, valid=bool(r["valid"]), score=r["score"], q_in_c=None, c_in_q=None, observed=(0, 0))
            if j in recs:
                a, b = recs[j]["q_in_c"], recs[j]["c_in_q"]
                f.update(q_in_c=freespace.see_through_fraction(a), c_in_q=freespace.see_through_fraction(b), observed=(a["observed"], b["observed"]))
            keep = bool(r["valid"]) and j in recs and f["q_in_c"] <= max_see_through and f["c_in_q"] <= max_see_through
            f["accepted"] = keep
            see_through.append(f)
            if verbose and j in recs:
                print("see-through (%d, %d): query in candidate %.4f of %d, candidate in query %.4f of %d; so far %s, loop %s"
                      % (q, c, f["q_in_c"], f["observed"][0], f["c_in_q"], f["observed"][1], "valid" if r["valid"] else "invalid", "kept" if keep else "dropped"))
            r["valid"] = keep
        return rs

    def apply_gate(rs, pairs):
        """measure every pair of the verification that just ran, print, and clear `valid` where either overlap is below min_overlap"""
        if not gate:
            return rs
        if backend == "gpu":
            figs = [dict(_overlap_figures(o), status=o["status"]) for o in store.verify_overlap(overlap_radius, n_pairs=len(rs))]
        else:
            figs = [dict(_oracle_overlap(r, overlap_radius), status=0) for r in rs]
        for r, f, (q, c) in zip(rs, figs, pairs):
            keep = bool(r["valid"]) and f["status"] == 0 and f["overlap_ab"] >= min_overlap and f["overlap_ba"] >= min_overlap
            f.update(query=q, cand=c, valid=bool(r["valid"]), accepted=keep, score=r["score"])
            overlaps.append(f)
            if verbose:
                print("overlap (%d, %d): src->dst %.3f (rmse %.3f m), dst->src %.3f (rmse %.3f m); registration %s, loop %s"
                      % (q, c, f["overlap_ab"], f["rmse_ab"], f["overlap_ba"], f["rmse_ba"], "valid" if r["valid"] else "invalid", "kept" if keep else "dropped"))
            r["valid"] = keep
        return rs
    if sensor == "uniform":
        scans, gt, odom, stamps = make_stream(n_kf, seed, yaw_bias=yaw_bias)
    elif sensor == "spinning":
        prims, lidar, seeds, gt, odom, stamps = make_lidar_stream(n_kf, seed, yaw_bias=yaw_bias)
        scans = None
    else:
        raise ValueError("sensor must be 'uniform' or 'spinning', not %r" % (sensor,))
    if backend == "gpu":
        from qn_amd import engine
        store = engine.KeyframeStore()
        ctx = engine.Context(400000)
        g = engine.NanoGICP(ctx)                                    # LoopClosure ctor, loop_closure.cpp:9-16, SURVEY App. C values
        g.setCorrespondenceRandomness(15); g.setMaximumIterations(32); g.setMaxCorrespondenceDistance(1.5 * radius); g.setTransformationEpsilon(0.01)
        quatro = engine.Quatro(ctx) if use_quatro else None
        loop_candidates = engine.loop_candidates
        if scans is None and moving_boxes:                          # the boxes stand elsewhere in every keyframe: one call per keyframe
            cast_ids = [int(store.add_lidar_scans(np.concatenate([prims, moving_box_prims(moving_boxes, k)]), lidar, [gt[k]], [seeds[k]])[0]) for k in range(n_kf)]
        elif scans is None:                                         # one call casts every keyframe into the store
            cast_ids = list(store.add_lidar_scans(prims, lidar, gt, seeds))
    else:
        from oracle import oracle as orc                           # the checker's side of the comparison (tests only)
        loop_candidates = orc.loop_candidates
        if scans is None:
            from qn_amd import synth
            scans = [synth.lidar_scan(np.concatenate([prims, moving_box_prims(moving_boxes, k)]) if moving_boxes else prims, lidar, T, int(sd))[:, :3]
                     for k, (T, sd) in enumerate(zip(gt, seeds))]
    if fgate or static_map:
        from qn_amd import freespace
        fs_params = range_params if range_params is not None else (freespace.Params.for_sensor(lidar) if sensor == "spinning" else
                                                                   freespace.Params(n_rows=32, n_cols=360, el_lo=-np.pi / 3, el_hi=np.pi / 3, min_range=1.0))
        if backend == "gpu":
            store.range_set_params(fs_params)
    pg = PoseGraph(); ids = []; corrected = []; sc_descs = {}
    prior_var = np.array([1e-4, 1e-4, 1e-4, 1e-2, 1e-2, 1e-2]); odom_var = prior_var.copy()   # FQ:112-114, 132-133 (rot, then trans)
    loops = []; t_reg = []; loop_T = []; last_tick = -1
    sub_hi = {}                                                                             # keyframe -> the last keyframe of its described window

    def describe_submaps(kfs, k):
        """the local submaps of `kfs` with the k + 1 keyframes that exist, from raw odometry; entries whose window has not grown are kept"""
        todo = [x for x in dict.fromkeys(kfs) if sub_hi.get(x) != min(x + submap_range, k)]
        if todo:
            st = store.submap_describe(ctx, [ids[x] for x in todo], odom[:k + 1], submap_range, voxel, with_features=use_quatro)
            sub_hi.update({x: min(x + submap_range, k) for x, v in zip(todo, st) if v != engine.QN_ERR_CAPACITY})
    occ_live = dict(updates=0, entries_listed=0, entries_walked=0, ledger=None, result=None, stats=None)

    def occ_update():
        """the live volume brought to the keyframes that exist, at their current estimate"""
        n = len(corrected)
        if backend == "gpu":
            occ_live["stats"], up = store.map_occupancy_update(ids[:n], corrected, engine.OccupancyParams(*occ_params))
            walked = up["entries_added"] + up["entries_removed"]
        else:
            occ_live["result"], up, occ_live["ledger"] = mapoccupancy.update(occ_live["ledger"], dict(enumerate(scans)), range(n), corrected, occ_params)
            walked = up.entries_added + up.entries_removed
        occ_live["updates"] += 1; occ_live["entries_listed"] += n; occ_live["entries_walked"] += walked
    for k in range(n_kf):
        if occ_incremental and k and (k % loop_every == 0 if loop_every > 1 or catch_up else True):
            occ_update()                                                                     # the tick of keyframe k - 1 is over: the volume follows what it left
        if backend == "gpu":
            ids.append(store.add(scans[k]) if scans is not None else cast_ids[k])
            if fgate:                                                                        # the keyframe's range images, once, on arrival
                store.range_describe([ids[k]])
        pose = odom[k] if k == 0 else corrected[-1] @ (inv(odom[k - 1]) @ odom[k])           # realtime pose = last corrected * delta odom (FQ:93-103)
        pg.add_pose(pose); corrected.append(pose)
        if k == 0:
            pg.add_prior(0, pose, prior_var)
        else:
            pg.add_between(k - 1, k, inv(odom[k - 1]) @ odom[k], odom_var)
        if loop_every > 1 or catch_up:                                                      # ---- a timer that fires every loop_every keyframes
            from qn_amd import scancontext
            if backend == "gpu":                                                             # every keyframe is described on arrival
                store.sc_describe([ids[k]])
                if use_quatro and not submap_matching:
                    store.quatro_describe(ctx, [ids[k]], voxel)
            else:
                sc_descs[k] = scancontext.descriptor(scans[k])
            if (k + 1) % loop_every:
                continue
            queries = list(range(last_tick + 1, k + 1)) if catch_up else [k]
            last_tick = k
            if backend == "gpu":
                found = [(c_ids[c_d < sc_max_dist], c_sh[c_d < sc_max_dist]) for c_ids, c_d, c_sh in store.sc_query([ids[q] for q in queries], stamps, tdiff, sc_top_k)]
            else:
                found = []
                for q in queries:
                    best = scancontext.query(sc_descs, q, stamps, tdiff, sc_top_k)
                    found.append(([b[0] for b in best if b[1] < sc_max_dist], [b[2] for b in best if b[1] < sc_max_dist]))
            pq, pc, py = [], [], []
            for q, (cs, shs) in zip(queries, found):
                for x, sh in zip(cs, shs):
                    pq.append(q); pc.append(int(x)); py.append(scancontext.yaw_of_shift(int(sh), scancontext.Params().n_sectors))
            if not pq:
                continue
            t0 = time.perf_counter()
            if submap_matching and backend == "gpu":
                describe_submaps(pq + pc, k)
                rs = (store.verify_loop_pairs_submap_c2f(ctx, [ids[q] for q in pq], [ids[x] for x in pc], score_thr) if use_quatro else
                      store.verify_loop_pairs_submap(ctx, [ids[q] for q in pq], [ids[x] for x in pc], py, score_thr))
            elif submap_matching:
                rs = [_oracle_submap_relative(orc, scans, odom[:k + 1], q, x, y, submap_range, voxel, 1.5 * radius, score_thr, use_quatro) for q, x, y in zip(pq, pc, py)]
            elif use_quatro and backend == "gpu":
                rs = store.verify_loop_pairs_c2f(ctx, [ids[q] for q in pq], [ids[x] for x in pc], score_thr)
            elif use_quatro:
                rs = [_oracle_scan_c2f(orc, scans, q, x, voxel, 1.5 * radius, score_thr) for q, x in zip(pq, pc)]
            elif backend == "gpu":
                rs = store.verify_loop_pairs(ctx, [ids[q] for q in pq], [ids[x] for x in pc], py, corrected[:k + 1], submap_range, voxel, score_thr)
            else:
                rs = [_oracle_relative(orc, scans, corrected[:k + 1], q, x, y, submap_range, voxel, 1.5 * radius, score_thr) for q, x, y in zip(pq, pc, py)]
            t_reg.append(time.perf_counter() - t0)
            rs = apply_freespace(apply_gate(rs, list(zip(pq, pc))), list(zip(pq, pc)))
            added = False
            for q in queries:
                ok = [(rs[j]["score"], j) for j in range(len(pq)) if pq[j] == q and rs[j]["valid"]]
                if not ok:
                    continue
                score, j = min(ok)
                pg.add_between(q, pc[j], inv(rs[j]["T"]), np.full(6, max(score, 1e-6)))      # T ~ inv(P_c) P_q
                loops.append((q, pc[j], score)); loop_T.append(rs[j]["T"]); added = True
            if added:
                pg.optimize()
                corrected = [p.copy() for p in pg.poses]
            continue
        # ---- loopTimerFunc
        if detector == "radius":
            pos = np.array([c[:3, 3] for c in corrected])
            cand = loop_candidates(pos, stamps[:k + 1], k, radius, tdiff, max_k=1)
        elif backend == "gpu":                                                               # store ids are keyframe indices here
            store.sc_describe([ids[k]])
            if verify == "relative" and use_quatro and not submap_matching:                  # the keyframe's Quatro features, once, on arrival
                store.quatro_describe(ctx, [ids[k]], voxel)
            c_ids, c_d, c_sh = store.sc_query([ids[k]], stamps, tdiff, sc_top_k if verify == "relative" else 1)[0]
            cand, shifts = c_ids[c_d < sc_max_dist], c_sh[c_d < sc_max_dist]
        else:
            from qn_amd import scancontext
            sc_descs[k] = scancontext.descriptor(scans[k])
            best = scancontext.query(sc_descs, k, stamps, tdiff, sc_top_k if verify == "relative" else 1)
            cand = [b[0] for b in best if b[1] < sc_max_dist]; shifts = [b[2] for b in best if b[1] < sc_max_dist]
        if len(cand) == 0:
            continue
        if verify == "relative":
            from qn_amd import scancontext
            cand = [int(x) for x in cand]; yaws = [scancontext.yaw_of_shift(int(x), scancontext.Params().n_sectors) for x in shifts]
            t0 = time.perf_counter()
            if submap_matching and backend == "gpu":
                describe_submaps([k] + cand, k)
                rs = (store.verify_loop_candidates_submap_c2f(ctx, ids[k], [ids[x] for x in cand], score_thr) if use_quatro else
                      store.verify_loop_candidates_submap(ctx, ids[k], [ids[x] for x in cand], yaws, score_thr))
            elif submap_matching:
                rs = [_oracle_submap_relative(orc, scans, odom[:k + 1], k, x, y, submap_range, voxel, 1.5 * radius, score_thr, use_quatro) for x, y in zip(cand, yaws)]
            elif use_quatro and backend == "gpu":
                rs = (store.verify_loop_pairs_c2f(ctx, [ids[k]] * len(cand), [ids[x] for x in cand], score_thr) if gate else
                      store.verify_loop_candidates_c2f(ctx, ids[k], [ids[x] for x in cand], score_thr))
            elif use_quatro:
                rs = [_oracle_scan_c2f(orc, scans, k, x, voxel, 1.5 * radius, score_thr) for x in cand]
            elif backend == "gpu":
                rs = (store.verify_loop_pairs(ctx, [ids[k]] * len(cand), [ids[x] for x in cand], yaws, corrected[:k + 1], submap_range, voxel, score_thr) if gate else
                      store.verify_loop_candidates(ctx, ids[k], [ids[x] for x in cand], yaws, corrected[:k + 1], submap_range, voxel, score_thr))
            else:
                rs = [_oracle_relative(orc, scans, corrected[:k + 1], k, x, y, submap_range, voxel, 1.5 * radius, score_thr) for x, y in zip(cand, yaws)]
            t_reg.append(time.perf_counter() - t0)
            rs = apply_freespace(apply_gate(rs, [(k, x) for x in cand]), [(k, x) for x in cand])
            ok = [(r["score"], j) for j, r in enumerate(rs) if r["valid"]]
            if not ok:
                continue
            score, j = min(ok)
            c = cand[j]
            pg.add_between(k, c, inv(rs[j]["T"]), np.full(6, max(score, 1e-6)))               # T ~ inv(P_c) P_k: the between factor (k -> c) is its inverse
            loops.append((k, c, score)); loop_T.append(rs[j]["T"])
            pg.optimize()
            corrected = [p.copy() for p in pg.poses]
            continue
        c = int(cand[0])
        t0 = time.perf_counter()
        if use_quatro:
            sub = [c]                                                                        # LC:89-92: scan to scan
        else:
            lo, hi = max(0, c - submap_range), min(k - 1, c + submap_range)                  # LC:98-104: scan to submap
            sub = list(range(lo, hi + 1))
        if backend == "gpu":
            ps, ns = store.assemble([ids[k]], [corrected[k]], voxel, 0)
            pd, nd = store.assemble([ids[i] for i in sub], [corrected[i] for i in sub], voxel, 1)
            if use_quatro:                                                                   # both clouds stay on the device (qn_coarse_to_fine_alignment_device)
                r = engine.coarse_to_fine_alignment_device(ctx, ps, ns, pd, nd, 16, quatro=quatro, max_corr_dist=1.5 * radius, score_thr=score_thr)
                valid, score, Treg = r["valid"], r["score"], r["T"]
            else:
                res = engine.GicpResult(); v = C.c_int()
                ctx.check(ctx._l.qn_icp_alignment_device(ctx.h, C.c_void_p(ps), C.c_uint32(ns), C.c_void_p(pd), C.c_uint32(nd), C.c_uint32(16),
                                                         C.c_double(score_thr), C.byref(res), C.byref(v)))
                valid, score, Treg = bool(v.value), res.fitness, np.array(res.T, dtype=np.float64).reshape(4, 4)
        else:
            src = orc.assemble_submap(scans, corrected, [k], voxel); dst = orc.assemble_submap(scans, corrected, sub, voxel)
            if use_quatro:
                r = orc.coarse_to_fine_alignment(src, dst, max_corr_dist=1.5 * radius, score_thr=score_thr)
            else:
                r = orc.icp_alignment(src, dst, max_corr_dist=1.5 * radius, score_thr=score_thr)
            valid, score, Treg = r["valid"], r["score"], r["T"]
        t_reg.append(time.perf_counter() - t0)
        if not valid:
            continue
        pose_from = Treg @ corrected[k]; pose_to = corrected[c]                              # FQ:224-225
        pg.add_between(k, c, inv(pose_from) @ pose_to, np.full(6, max(score, 1e-6)))        # FQ:226-233
        loops.append((k, c, score)); loop_T.append(Treg)
        pg.optimize()
        corrected = [p.copy() for p in pg.poses]                                             # FQ:180-188
    out = dict(sensor=sensor, detector=detector, n_keyframes=n_kf, loops=len(loops), attempts=len(t_reg), ate_odometry=ate(odom, gt), ate_corrected=ate(corrected, gt),
               ms_per_attempt=1e3 * float(np.mean(t_reg)) if t_reg else None, quatro=use_quatro, verify=verify, loop_list=loops, poses=corrected,
               loop_T=loop_T, gt=gt, loop_every=loop_every, catch_up=catch_up, submap_matching=submap_matching)
    if gate:
        out["overlaps"] = overlaps
    if fgate:
        out["see_through"] = see_through
    def localize_stage():
        """every localize_every-th keyframe localised in the map slot as it stands from its displaced corrected pose; fills out["localized"], writes localized_tum.txt"""
        from qn_amd import engine, synth
        pick = list(range(0, len(ids), int(localize_every)))
        a = np.radians(localize_yaw); D = np.eye(4)
        D[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; D[:3, 3] = (0.6 * localize_shift, 0.8 * localize_shift, 0.0)
        guesses = [corrected[k] @ D for k in pick]
        call = store.map_localize_c2f if use_quatro else store.map_localize
        rs, lst = call(ctx, [ids[k] for k in pick], guesses, engine.LocalizeParams(localize_radius, voxel, score_thr, 0))
        out["localized"] = []
        for k, G, r in zip(pick, guesses, rs):
            gt_err, gr_err = synth.pose_error(G, corrected[k]); t_err, r_err = synth.pose_error(r["T"], corrected[k])
            out["localized"].append(dict(id=k, valid=r["valid"], status=r["status"], score=r["score"], guess_t_err=gt_err, guess_r_err=gr_err, t_err=t_err,
                                         r_err=r_err, T=r["T"]))
        out["localize_stats"] = lst
        with open(os.path.join(save_dir, "localized_tum.txt"), "w") as ft:
            ft.write("#timestamp x y z qx qy qz qw\n")
            for k, r in zip(pick, rs):
                q = rot_to_quat(r["T"][:3, :3])
                ft.write("%.8f %.8f %.8f %.8f %.8f %.8f %.8f %.8f\n" % (stamps[k], r["T"][0, 3], r["T"][1, 3], r["T"][2, 3], q[0], q[1], q[2], q[3]))
    if save_dir:
        write_kitti_tum(save_dir, corrected, stamps)
        if occupancy_3d:
            if occ_incremental:
                occ_update()                                                                 # once more, with the final poses
            if backend == "gpu":
                from qn_amd import engine
                st = occ_live["stats"] if occ_incremental else store.map_occupancy(ids, corrected, engine.OccupancyParams(*occ_params))
                info, hits, misses, cls = store.map_occupancy_grid()
                res = dict(hits=hits, misses=misses, classes=cls, grid=mapoccupancy.OccupancyGrid(*(info[f] for f in mapoccupancy.OccupancyGrid._fields)),
                           slice=store.map_occupancy_slice)
            else:
                res = dict(occ_live["result"]) if occ_incremental else mapoccupancy.classify(scans, corrected, occ_params)
                st = res["stats"]._asdict()
            if occ_distance:
                if backend == "gpu":
                    dst = store.map_distance(engine.DistanceParams(*dist_params))
                    d2_slice = store.map_distance_slice
                else:
                    field = mapdistance.transform(res["classes"], dist_params)
                    dst = field["stats"]._asdict()
                    d2_slice = lambda lo, hi: mapdistance.slice2d(field["d2"], lo, hi)
                out["distance"] = dict({k: int(dst[k]) for k in mapdistance.DistanceStats._fields}, site_mask=int(dist_params.site_mask), max_dist=int(dist_params.max_dist))
                if robot_radius is not None:
                    res["d2_slice"] = d2_slice; res["robot_radius"] = float(robot_radius)
            layers = write_occupancy(save_dir, res, occ_slice)
            if occ_route is not None:
                g = res["grid"]
                lo, hi = 0, maproute.INT32_MAX
                if route_planar:
                    lo, hi = layers if layers is not None else (mapoccupancy.layer_of(occ_route[2], g),) * 2
                rp = maproute.RouteParams(1 << mapoccupancy.FREE, int(route_min_d2), int(lo), int(hi), int(bool(route_planar)))
                start = np.asarray(corrected[-1][:3, 3] if route_from is None else route_from, np.float64).reshape(1, 3)
                if backend == "gpu":
                    rst = store.map_route([occ_route], engine.RouteParams(*rp))
                    at = int(store.map_route_query(start)[0])
                    n, ijk = store.map_route_paths(start, at // 3 + 1 if at < maproute.BLOCKED else 1)
                    cost = store.map_route_query(maproute.centres(g, ijk[0, :int(n[0])], rp)) if n[0] else np.zeros(0, np.uint32)
                else:
                    rf = maproute.field(res["classes"], field["d2"], g, [occ_route], rp)
                    rst = rf["stats"]._asdict()
                    at = int(maproute.query(rf["cost"], g, start, rp)[0])
                    n, ijk = maproute.paths(rf["cost"], g, start, at // 3 + 1 if at < maproute.BLOCKED else 1, rp)
                    v = ijk[0, :int(n[0])]
                    cost = rf["cost"][v[:, 2], v[:, 1], v[:, 0]]
                xyz = maproute.centres(g, ijk[0, :int(n[0])], rp)
                with open(os.path.join(save_dir, "route.csv"), "w") as fr:
                    fr.write("x y z cost\n")
                    for q, c in zip(xyz, cost):
                        fr.write("%.6f %.6f %.6f %d\n" % (q[0], q[1], q[2], int(c)))
                out["route"] = dict({k: int(rst[k]) for k in maproute.RouteStats._fields}, **rp._asdict(), path_len=int(n[0]), path_cost=at if at < maproute.BLOCKED else None)
            if occ_frontiers:
                g = res["grid"]
                flo, fhi = layers if layers is not None else (0, mapfrontier.INT32_MAX)
                fp = mapfrontier.FrontierParams(min_size=int(frontier_min_size), iz_lo=int(flo), iz_hi=int(fhi))
                reach = None
                if backend == "gpu":
                    fst = store.map_frontiers(engine.FrontierParams(*fp))
                    finfo = store.map_frontier_regions()
                    if occ_route is not None:
                        reach = store.map_frontier_costs()
                else:
                    fr = mapfrontier.frontier(res["classes"], fp)
                    fst, finfo = fr["stats"]._asdict(), fr["info"]
                    if occ_route is not None:
                        reach = mapfrontier.costs(fr["labels"], len(finfo), rf["cost"])
                centroid = mapoccupancy.centres(mapfrontier.centroid(finfo), g)
                with open(os.path.join(save_dir, "frontiers.csv"), "w") as ff:
                    ff.write("region size faces cx cy cz lo_x lo_y lo_z hi_x hi_y hi_z" + (" reach ex ey ez" if reach is not None else "") + "\n")
                    if reach is not None:
                        metres = maproute.metres(reach[0], g.voxel)
                        entry = np.where((reach[0] < maproute.BLOCKED)[:, None], mapoccupancy.centres(reach[1], g), np.nan)
                    for k, r in enumerate(finfo):
                        row = "%d %d %d %.6f %.6f %.6f %d %d %d %d %d %d" % ((k, int(r["size"]), int(r["faces"])) + tuple(centroid[k]) + tuple(int(v) for v in r["lo"]) +
                                                                            tuple(int(v) for v in r["hi"]))
                        if reach is not None:
                            row += " %.6f %.6f %.6f %.6f" % ((float(metres[k]),) + tuple(entry[k]))
                        ff.write(row + "\n")
                out["frontiers"] = dict({k: int(fst[k]) for k in mapfrontier.FrontierStats._fields}, **fp._asdict())
                if occ_view_gain and len(finfo):
                    root = finfo["root"].astype(np.int64)
                    at = np.stack([root % g.width, (root // g.width) % g.height, root // (g.width * g.height)], axis=1)
                    if reach is not None:
                        at = np.where((reach[0] < maproute.BLOCKED)[:, None], reach[1], at)
                    vps = mapoccupancy.centres(at, g)
                    if backend == "gpu":
                        vinfo, vst = store.map_view_gain(vps, view_offsets)
                    else:
                        vr = mapview.gain(res["classes"], g, vps, view_offsets)
                        vinfo, vst = vr["info"], vr["stats"]._asdict()
                    with open(os.path.join(save_dir, "view_gain.csv"), "w") as fv:
                        fv.write("region x y z gain blocked escaped spent reached\n")
                        for k, r in enumerate(vinfo):
                            fv.write("%d %.6f %.6f %.6f %d %d %d %d %d\n" % ((k,) + tuple(vps[k]) + tuple(int(r[f]) for f in ("gain", "blocked", "escaped", "spent", "reached"))))
                    out["view_gain"] = dict({k: int(vst[k]) for k in mapview.ViewStats._fields}, range=float(view_range), beams=int(view_beams), azimuth=int(view_azimuth))
            out["occupancy"] = {k: int(st[k]) for k in ("n_rays", "total_misses", "width", "height", "depth", "occupied", "free", "unknown")}
            if layers is not None:
                out["occupancy"]["slice_layers"] = [int(layers[0]), int(layers[1])]
            if occ_incremental:
                out["occupancy"].update({k: occ_live[k] for k in ("updates", "entries_listed", "entries_walked")})
        if localize_every and save_map_leaf is None:
            store.build_map(ids, corrected, voxel)
            localize_stage()
        if save_map_leaf is not None and backend == "gpu":
            def write_map(name, n, label=None):
                """the map slot as a .pcd, with the normals of its points when asked and their cluster labels when given -> the points that have a normal"""
                if not save_map_normals:
                    if label is None:
                        write_pcd_xyzi(os.path.join(save_dir, name), store.download_map(n))
                    else:
                        write_pcd_labelled(os.path.join(save_dir, name), store.download_map(n), label)
                    return None
                from qn_amd import engine
                nr = store.map_normals(engine.NormalParams(normal_radius, int(normal_min_neighbors)), np.array([T[:3, 3] for T in corrected]))
                if label is None:
                    write_pcd_xyzi_normal(os.path.join(save_dir, name), store.download_map(n), nr["normals"], nr["curvature"])
                else:
                    write_pcd_labelled(os.path.join(save_dir, name), store.download_map(n), label, nr["normals"], nr["curvature"])
                return int(np.isfinite(nr["curvature"]).sum())
            def filter_map(n):
                """the outliers of the map slot removed in place -> (the points left, the points removed)"""
                if not map_outliers:
                    return n, None
                from qn_amd import engine
                st = store.map_outliers(engine.OutlierParams(outlier_radius, outlier_std, int(outlier_k)))[0]
                return store.map_remove_outliers()[1], int(st["removed"])
            def ground_stage(stem, n):
                """the occupancy grid of the map slot written as stem.pgm / stem.yaml, then the clusters of what stands on the ground (of every finite point
                without a grid) as stem's clusters .csv; then the rejected clumps and the GROUND class leave the slot when asked -> (the points left, their
                cluster labels or None)"""
                from qn_amd import engine, mapground
                cls = label = None
                if occupancy_grid:
                    st, cls, _ = store.map_ground(engine.GroundParams(grid_cell, max_slope, ground_tol, clearance, 1))
                    info, _, occ = store.map_ground_grid()
                    write_grid(save_dir, stem, mapground.GridInfo(*(info[f] for f in mapground.GridInfo._fields)), occ)
                    out["grid" if stem == "map" else "static_grid"] = {k: int(st[k]) for k in ("width", "height", "occupied", "free", "unknown", "n_ground")}
                if map_clusters:
                    mask = ((1 << mapground.OBSTACLE) | (1 << mapground.OVERHEAD)) if occupancy_grid else 0
                    st, label, _, _, cl = store.map_clusters(engine.ClusterParams(cluster_tol, int(cluster_min), int(cluster_max), mask))
                    write_clusters_csv(os.path.join(save_dir, "clusters.csv" if stem == "map" else "clusters_static.csv"), cl)
                    out["clusters" if stem == "map" else "static_clusters"] = {k: int(st[k]) for k in ("clusters", "components", "too_small", "too_large",
                                                                                                     "clustered_points", "rejected_points")}
                    if drop_small_clusters:
                        n = store.map_drop_rejected_clusters()[1]
                        label = label[label != engine.QN_CLUSTER_REJECTED]
                        if drop_ground:                                                      # the slot has changed: the ground of what is left
                            cls = store.map_ground(engine.GroundParams(grid_cell, max_slope, ground_tol, clearance, 1))[1]
                if drop_ground:
                    n = store.map_keep_classes(0b11101)[1]
                    label = None if label is None else label[cls != mapground.GROUND]
                return n, label
            n, removed = filter_map(store.build_map(ids, corrected, save_map_leaf))
            n, label = ground_stage("map", n)
            valid = write_map("map.pcd", n, label)
            if localize_every:
                localize_stage()
            if map_outliers:
                out["map_points"] = n; out["map_outliers_removed"] = removed
            if map_clusters:
                out["map_points"] = n
            if save_map_normals:
                out["map_points"] = n; out["map_normals_valid"] = valid
            if static_map:
                out["map_points"] = n
                if not fgate:                                                                # (with the gate on, every keyframe was described on arrival)
                    store.range_describe(ids)
                st = store.static_classify(ids, corrected, radius=static_radius, max_k=static_max_k)
                n, removed = filter_map(store.build_map_static(save_map_leaf))
                n, label = ground_stage("map_static", n)
                write_map("map_static.pcd", n, label)
                if map_outliers:
                    out["static_outliers_removed"] = removed
                out["static_removed"] = int(st["removed"].sum()); out["static_map_points"] = n
        elif occupancy_grid:                                                                 # the oracle backend: the oracle's voxel grid, the twin's grid
            from qn_amd import mapground
            xyz = np.asarray(orc.assemble_submap(scans, corrected, list(range(len(scans))), save_map_leaf), np.float32)[:, :3]
            pts = np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], axis=1)
            r = mapground.classify(pts, (grid_cell, max_slope, ground_tol, clearance, 1))
            write_grid(save_dir, "map", r["info"], r["occupancy"])
            out["grid"] = {k: int(getattr(r["stats"], k)) for k in ("width", "height", "occupied", "free", "unknown", "n_ground")}
            write_pcd_xyzi(os.path.join(save_dir, "map.pcd"), mapground.keep(pts, r["classes"], 0b11101) if drop_ground else pts)
    if verbose:
        print({k: v for k, v in out.items() if k not in ("poses", "loop_list", "loop_T", "gt", "overlaps", "see_through", "localized")})
        for r in out.get("localized", []):
            print("localized keyframe %d: valid %s, score %.4f, guess %.3f m / %.2f deg -> %.4f m / %.3f deg" %
                  (r["id"], r["valid"], r["score"], r["guess_t_err"], np.degrees(r["guess_r_err"]), r["t_err"], np.degrees(r["r_err"])))
    if backend == "gpu":
        ctx.close(); store.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=70)
    ap.add_argument("--quatro", action="store_true")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sensor", choices=["uniform", "spinning"], default="uniform", help="keyframe clouds: uniform surface samples, or ray-cast spinning-LiDAR scans")
    ap.add_argument("--save-dir", default=None, help="write poses_kitti.txt / poses_tum.txt (FQ:344-373) here")
    ap.add_argument("--save-map-leaf", type=float, default=None, help="with --save-dir: also write map.pcd, the corrected map at this leaf (0.3 = save_voxel_resolution)")
    ap.add_argument("--detector", choices=["radius", "scancontext"], default="radius", help="loop candidates: radius search on corrected poses, or Scan Context")
    ap.add_argument("--yaw-bias", type=float, default=0.006, help="odometry heading drift per keyframe [rad]")
    ap.add_argument("--verify", choices=["reference", "relative"], default="reference",
                    help="candidate registration: the reference's world-frame submaps from identity, or (with --detector scancontext) drift-free relative submaps seeded with the Scan Context heading "
                         "(with --quatro: the keyframes' resident Quatro features, scan to scan)")
    ap.add_argument("--sc-top-k", type=int, default=1, help="with --verify relative: Scan Context candidates verified per query, in one batched registration")
    ap.add_argument("--loop-every", type=int, default=1, help="with --verify relative: the loop timer fires after every N-th keyframe (loop_update_hz)")
    ap.add_argument("--catch-up", action="store_true", help="with --loop-every: a tick checks every keyframe added since the last one, in one batched verification")
    ap.add_argument("--submap-matching", action="store_true",
                    help="with --verify relative: submap against submap from resident local submaps (the reference's enable_submap_matching, drift-free); with --quatro coarse to fine")
    ap.add_argument("--min-overlap", type=float, default=None,
                    help="with --verify relative and --overlap-radius: add a loop only if it is valid and both directions' overlap (aligned source <-> target) reach this fraction")
    ap.add_argument("--overlap-radius", type=float, default=None, help="with --min-overlap: the radius [m] within which a point counts as having a partner")
    ap.add_argument("--max-see-through", type=float, default=None,
                    help="with --verify relative: add a loop only if neither scan sees through more than this share of the other's observed points under the verified transform")
    ap.add_argument("--static-map", action="store_true",
                    help="with --save-dir and --save-map-leaf: also write map_static.pcd, the map without the records other keyframes saw through")
    ap.add_argument("--save-map-normals", action="store_true",
                    help="with --save-dir and --save-map-leaf: map.pcd also carries normal_x normal_y normal_z curvature, estimated on the GPU from the resident map")
    ap.add_argument("--normal-radius", type=float, default=0.6, help="with --save-map-normals: the neighbourhood radius [m]")
    ap.add_argument("--map-outliers", action="store_true",
                    help="with --save-dir and --save-map-leaf: isolated noise points are removed from the map on the GPU before it (and its normals) are written")
    ap.add_argument("--outlier-radius", type=float, default=1.0, help="with --map-outliers: the neighbourhood radius [m]")
    ap.add_argument("--outlier-k", type=int, default=8, help="with --map-outliers: the nearest neighbours the mean distance is taken over (fewer within the radius: removed)")
    ap.add_argument("--outlier-std", type=float, default=2.0, help="with --map-outliers: removed above the mean of the mean distances plus this many standard deviations")
    ap.add_argument("--occupancy-grid", action="store_true",
                    help="with --save-dir and --save-map-leaf: also write map.pgm and map.yaml, the map's 2-D occupancy grid (ground segmented, obstacles projected)")
    ap.add_argument("--grid-cell", type=float, default=0.5, help="with --occupancy-grid: the grid's cell edge [m]")
    ap.add_argument("--max-slope", type=float, default=0.3, help="with --occupancy-grid: the steepest ground, rise over run")
    ap.add_argument("--ground-tol", type=float, default=0.2, help="with --occupancy-grid: a point within this of the ground envelope is ground [m]")
    ap.add_argument("--clearance", type=float, default=2.0, help="with --occupancy-grid: a point higher than this above the ground does not occupy its cell [m]")
    ap.add_argument("--drop-ground", action="store_true", help="with --occupancy-grid: map.pcd is written without the ground points")
    ap.add_argument("--map-clusters", action="store_true",
                    help="with --save-dir and --save-map-leaf: the map's points are clustered into objects on the GPU (with --occupancy-grid: what stands on the ground); "
                         "map.pcd gains an integer label field and clusters.csv lists id, size, box and centroid")
    ap.add_argument("--cluster-tol", type=float, default=0.5, help="with --map-clusters: points this close are joined [m]")
    ap.add_argument("--cluster-min", type=int, default=10, help="with --map-clusters: the fewest points of a cluster")
    ap.add_argument("--cluster-max", type=int, default=0xffffffff, help="with --map-clusters: the most points of a cluster")
    ap.add_argument("--drop-small-clusters", action="store_true", help="with --map-clusters: the clumps that are no cluster leave the map")
    ap.add_argument("--localize-every", type=int, default=0,
                    help="with --save-dir: once the map stands, every N-th keyframe is localised in it on the device from its displaced corrected pose (with --quatro coarse to "
                         "fine); writes localized_tum.txt")
    ap.add_argument("--localize-radius", type=float, default=35.0, help="with --localize-every: the radius of the map crop around the guess [m]")
    ap.add_argument("--localize-shift", type=float, default=0.5, help="with --localize-every: the guess is this far from the corrected pose [m]")
    ap.add_argument("--localize-yaw", type=float, default=3.0, help="with --localize-every: and turned by this much [deg]")
    ap.add_argument("--occupancy-3d", action="store_true",
                    help="with --save-dir: also write occupied.pcd, the occupied voxels of the 3-D occupancy map carved by every keyframe's rays (x y z hits misses)")
    ap.add_argument("--occ-incremental", action="store_true",
                    help="with --occupancy-3d: keep the volume live through the run - updated in place at every loop-timer tick and once more with the final "
                         "poses - instead of building it once at the end; the files are the same")
    ap.add_argument("--occ-voxel", type=float, default=0.3, help="with --occupancy-3d: the voxel edge [m]")
    ap.add_argument("--occ-min-range", type=float, default=0.5, help="with --occupancy-3d: records closer than this are no rays [m]")
    ap.add_argument("--occ-max-range", type=float, default=60.0, help="with --occupancy-3d: records farther than this are no rays [m]")
    ap.add_argument("--occ-shell", type=int, default=1, help="with --occupancy-3d: the voxels before a ray's end that it does not carve")
    ap.add_argument("--occ-slice", type=float, nargs=2, default=None, metavar=("ZLO", "ZHI"),
                    help="with --occupancy-3d: also write occupancy_slice.pgm / .yaml, the layers between these heights [m] flattened")
    ap.add_argument("--occ-distance", action="store_true",
                    help="with --occupancy-3d: also compute the volume's Euclidean distance field (per voxel the distance to the nearest occupied voxel)")
    ap.add_argument("--occ-dist-max", type=int, default=16, help="with --occ-distance: the largest distance the field resolves [voxels, 1 .. 255]")
    ap.add_argument("--occ-unknown-obstacle", action="store_true", help="with --occ-distance: unknown voxels are obstacles too")
    ap.add_argument("--robot-radius", type=float, default=None, metavar="M",
                    help="with --occ-distance and --occ-slice: also write occupancy_inflated.pgm / .yaml, the slice inflated by this radius [m]")
    ap.add_argument("--occ-route", type=float, nargs=3, default=None, metavar=("GX", "GY", "GZ"),
                    help="with --occupancy-3d --occ-distance: the cost-to-go field to this goal [m] through free space and the path to it, written to route.csv")
    ap.add_argument("--route-from", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="with --occ-route: the path's start [m] (default: the last keyframe's position)")
    ap.add_argument("--route-min-d2", type=int, default=4, help="with --occ-route: the smallest squared distance to an obstacle, in voxels, a passable voxel has")
    ap.add_argument("--route-planar", action="store_true", help="with --occ-route: plan in the plane of columns over the layers of --occ-slice (or the goal's layer)")
    ap.add_argument("--occ-frontiers", action="store_true",
                    help="with --occupancy-3d: also find the exploration frontiers, the free voxels beside unknown space grouped into regions, written to frontiers.csv "
                         "(over the layers of --occ-slice when given; with --occ-route each region's reach cost and entry voxel too)")
    ap.add_argument("--frontier-min-size", type=int, default=8, help="with --occ-frontiers: the smallest component, in voxels, that is a region")
    ap.add_argument("--occ-view-gain", action="store_true",
                    help="with --occ-frontiers: also the next-best-view gain of one viewpoint per region (with --occ-route where the region is entered, else its root voxel): "
                         "the distinct unknown voxels a spinning sensor's rays would pass through, written to view_gain.csv")
    ap.add_argument("--view-range", type=float, default=20.0, help="with --occ-view-gain: the sensor's range [m]")
    ap.add_argument("--view-beams", type=int, default=16, help="with --occ-view-gain: the sensor's beams, between -15 and 15 degrees")
    ap.add_argument("--view-azimuth", type=int, default=300, help="with --occ-view-gain: the sensor's steps a turn")
    ap.add_argument("--moving-boxes", type=int, default=0, help="with --sensor spinning: this many boxes that stand somewhere else in every keyframe")
    ap.add_argument("--backend", choices=["gpu", "oracle"], default="gpu", help="the engine on the GPU, or the CPU oracle")
    a = ap.parse_args()
    if a.save_map_normals and (a.save_dir is None or a.save_map_leaf is None):
        ap.error("--save-map-normals needs --save-dir and --save-map-leaf")
    if a.map_outliers and (a.save_dir is None or a.save_map_leaf is None):
        ap.error("--map-outliers needs --save-dir and --save-map-leaf")
    if a.occupancy_grid and (a.save_dir is None or a.save_map_leaf is None):
        ap.error("--occupancy-grid needs --save-dir and --save-map-leaf")
    if a.drop_ground and not a.occupancy_grid:
        ap.error("--drop-ground needs --occupancy-grid")
    if a.map_clusters and (a.save_dir is None or a.save_map_leaf is None):
        ap.error("--map-clusters needs --save-dir and --save-map-leaf")
    if a.drop_small_clusters and not a.map_clusters:
        ap.error("--drop-small-clusters needs --map-clusters")
    if a.occupancy_3d and a.save_dir is None:
        ap.error("--occupancy-3d needs --save-dir")
    if a.occ_slice is not None and not a.occupancy_3d:
        ap.error("--occ-slice needs --occupancy-3d")
    if a.occ_incremental and not a.occupancy_3d:
        ap.error("--occ-incremental needs --occupancy-3d")
    if a.occ_distance and not a.occupancy_3d:
        ap.error("--occ-distance needs --occupancy-3d")
    if (a.occ_unknown_obstacle or a.robot_radius is not None) and not a.occ_distance:
        ap.error("--occ-unknown-obstacle and --robot-radius need --occ-distance")
    if a.occ_route is not None and not (a.occupancy_3d and a.occ_distance):
        ap.error("--occ-route needs --occupancy-3d and --occ-distance")
    if a.occ_route is None and (a.route_from is not None or a.route_planar or a.route_min_d2 != 4):
        ap.error("--route-from, --route-min-d2 and --route-planar need --occ-route")
    if a.occ_frontiers and not a.occupancy_3d:
        ap.error("--occ-frontiers needs --occupancy-3d")
    if a.frontier_min_size != 8 and not a.occ_frontiers:
        ap.error("--frontier-min-size needs --occ-frontiers")
    if a.occ_view_gain and not (a.occupancy_3d and a.occ_frontiers):
        ap.error("--occ-view-gain needs --occupancy-3d and --occ-frontiers")
    if (a.view_range != 20.0 or a.view_beams != 16 or a.view_azimuth != 300) and not a.occ_view_gain:
        ap.error("--view-range, --view-beams and --view-azimuth need --occ-view-gain")
    run(a.keyframes, a.seed, a.quatro, save_dir=a.save_dir, save_map_leaf=a.save_map_leaf, sensor=a.sensor, detector=a.detector, yaw_bias=a.yaw_bias,
        verify=a.verify, sc_top_k=a.sc_top_k, backend=a.backend, loop_every=a.loop_every, catch_up=a.catch_up, submap_matching=a.submap_matching,
        min_overlap=a.min_overlap, overlap_radius=a.overlap_radius, max_see_through=a.max_see_through, static_map=a.static_map, moving_boxes=a.moving_boxes,
        save_map_normals=a.save_map_normals, normal_radius=a.normal_radius, map_outliers=a.map_outliers, outlier_radius=a.outlier_radius, outlier_k=a.outlier_k,
        outlier_std=a.outlier_std, occupancy_grid=a.occupancy_grid, grid_cell=a.grid_cell, max_slope=a.max_slope, ground_tol=a.ground_tol,
        clearance=a.clearance, drop_ground=a.drop_ground, map_clusters=a.map_clusters, cluster_tol=a.cluster_tol, cluster_min=a.cluster_min,
        cluster_max=a.cluster_max, drop_small_clusters=a.drop_small_clusters, localize_every=a.localize_every, localize_radius=a.localize_radius,
        localize_shift=a.localize_shift, localize_yaw=a.localize_yaw, occupancy_3d=a.occupancy_3d, occ_voxel=a.occ_voxel, occ_min_range=a.occ_min_range,
        occ_max_range=a.occ_max_range, occ_shell=a.occ_shell, occ_slice=a.occ_slice, occ_distance=a.occ_distance, occ_dist_max=a.occ_dist_max,
        occ_unknown_obstacle=a.occ_unknown_obstacle, robot_radius=a.robot_radius, occ_route=a.occ_route, route_from=a.route_from, route_min_d2=a.route_min_d2,
        route_planar=a.route_planar, occ_frontiers=a.occ_frontiers, frontier_min_size=a.frontier_min_size, occ_view_gain=a.occ_view_gain, view_range=a.view_range,
        view_beams=a.view_beams, view_azimuth=a.view_azimuth, occ_incremental=a.occ_incremental)
