"""Deterministic synthetic scan-pair generator (SURVEY.md §8d, row "G").

No KITTI data exists in the container, so every config of BASELINE.json is run on a
seeded "street scene": ground plane, building walls, poles and boxes, sampled on
surfaces, voxel-snapped to centroids at 0.3 m (what the reference's `voxelizePcd`
does before registration: fast_lio_sam_qn/include/utilities.hpp:38-51, called at
src/loop_closure.cpp:107) and resampled to exactly N points.

  source = scene sampled in window W_s                      (world frame)
  target = T_gt * (scene sampled independently in W_t + N(0, sigma))

so a registration of source onto target should recover T_gt.  seed = 20241220 + pair_id.
Pure numpy (PCG64) - identical output here and on the GPU box (same image).
"""
import numpy as np

BASE_SEED = 20241220


def _rot_zyx(yaw, pitch, roll):
    cy, sy = np.cos(yaw), np.sin(yaw)
    cp, sp = np.cos(pitch), np.sin(pitch)
    cr, sr = np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


class Scene:
    """Piecewise-planar/cylindrical world; `sample(rng, m, window)` draws m surface points."""

    def __init__(self, rng, extent=120.0):
        self.extent = float(extent)
        h = extent / 2.0
        s = extent / 120.0  # object sizes scale with the scene so small test scenes stay busy
        nwalls, npoles, nboxes = 10, 40, 30
        # walls: (x0, y0, dx, dy, height) vertical rectangles, axis aligned
        self.walls = []
        for i in range(nwalls):
            L = rng.uniform(25, 45) * s
            H = rng.uniform(8, 16) * min(1.0, max(s, 0.35))
            cx, cy = rng.uniform(-h * 0.85, h * 0.85, 2)
            if i % 2 == 0:
                self.walls.append((cx - L / 2, cy, L, 0.0, H))
            else:
                self.walls.append((cx, cy - L / 2, 0.0, L, H))
        self.poles = [(rng.uniform(-h * 0.9, h * 0.9), rng.uniform(-h * 0.9, h * 0.9),
                       0.15, 6.0 * min(1.0, max(s, 0.35))) for _ in range(npoles)]
        self.boxes = []
        for _ in range(nboxes):
            cx, cy = rng.uniform(-h * 0.9, h * 0.9, 2)
            sx, sy = (2.0, 4.0) if rng.random() < 0.5 else (4.0, 2.0)
            self.boxes.append((cx, cy, sx * max(s, 0.5), sy * max(s, 0.5), 1.5))

    def sample(self, rng, m, window):
        """window = (xmin, xmax, ymin, ymax): points outside are rejected (re-drawn)."""
        out = []
        need = m
        while need > 0:
            p = self._draw(rng, int(need * 1.6) + 64)
            keep = (p[:, 0] >= window[0]) & (p[:, 0] <= window[1]) & \
                   (p[:, 1] >= window[2]) & (p[:, 1] <= window[3])
            p = p[keep][:need]
            out.append(p)
            need -= len(p)
        return np.concatenate(out, 0)

    def primitives(self):
        """The surfaces `_draw` samples as analytic primitives (PRIM_DTYPE: kind + six f64 parameters), for the ray-caster: ground, then
        walls, poles and boxes in their list order.  Draws nothing from any RNG: the scene is fully built by the constructor."""
        h = self.extent / 2.0
        rows = [(PRIM_GROUND, (-h, -h, h, h, 0.0, 0.0))]
        rows += [(PRIM_WALL, tuple(w) + (0.0,)) for w in self.walls]
        rows += [(PRIM_POLE, tuple(p) + (0.0, 0.0)) for p in self.poles]
        rows += [(PRIM_BOX, tuple(b) + (0.0,)) for b in self.boxes]
        return np.array(rows, dtype=PRIM_DTYPE)

    def _draw(self, rng, m):
        h = self.extent / 2.0
        kind = rng.random(m)
        pts = np.empty((m, 3))
        # ground 40 %
        g = kind < 0.40
        ng = int(g.sum())
        pts[g] = np.stack([rng.uniform(-h, h, ng), rng.uniform(-h, h, ng), np.zeros(ng)], 1)
        # walls 35 %
        w = (kind >= 0.40) & (kind < 0.75)
        nw = int(w.sum())
        wi = rng.integers(0, len(self.walls), nw)
        W = np.array(self.walls)[wi]
        u = rng.random(nw)
        pts[w] = np.stack([W[:, 0] + u * W[:, 2], W[:, 1] + u * W[:, 3], rng.random(nw) * W[:, 4]], 1)
        # poles 5 %
        p = (kind >= 0.75) & (kind < 0.80)
        npz = int(p.sum())
        pi = rng.integers(0, len(self.poles), npz)
        P = np.array(self.poles)[pi]
        a = rng.uniform(0, 2 * np.pi, npz)
        pts[p] = np.stack([P[:, 0] + P[:, 2] * np.cos(a), P[:, 1] + P[:, 2] * np.sin(a),
                           rng.random(npz) * P[:, 3]], 1)
        # boxes 20 % (4 sides + top, area weighted roughly)
        b = kind >= 0.80
        nb = int(b.sum())
        bi = rng.integers(0, len(self.boxes), nb)
        B = np.array(self.boxes)[bi]
        face = rng.integers(0, 5, nb)
        u, v = rng.random(nb), rng.random(nb)
        x = np.where(face == 0, B[:, 0] - B[:, 2] / 2,
            np.where(face == 1, B[:, 0] + B[:, 2] / 2, B[:, 0] + (u - 0.5) * B[:, 2]))
        y = np.where(face == 2, B[:, 1] - B[:, 3] / 2,
            np.where(face == 3, B[:, 1] + B[:, 3] / 2,
            np.where(face == 4, B[:, 1] + (v - 0.5) * B[:, 3], B[:, 1] + (u - 0.5) * B[:, 3])))
        # for faces 0/1 x is fixed and y varies with u
        y = np.where((face == 0) | (face == 1), B[:, 1] + (u - 0.5) * B[:, 3], y)
        z = np.where(face == 4, B[:, 4], v * B[:, 4])
        pts[b] = np.stack([x, y, z], 1)
        return pts


def voxel_centroids(p, leaf):
    """pcl::VoxelGrid semantics: one centroid per occupied leaf, output ordered by leaf index."""
    q = np.floor(p / leaf).astype(np.int64)
    q -= q.min(0)
    dims = q.max(0) + 1
    key = q[:, 0] + dims[0] * (q[:, 1] + dims[1] * q[:, 2])
    order = np.argsort(key, kind="stable")
    key_s = key[order]
    first = np.flatnonzero(np.r_[True, key_s[1:] != key_s[:-1]])
    cnt = np.diff(np.r_[first, len(key_s)])
    sums = np.add.reduceat(p[order], first, axis=0)
    return sums / cnt[:, None]


def random_gt(rng, mode="gicp"):
    """T_gt distribution of SURVEY §8d: small for GICP-only pairs, large yaw/xy for Quatro pairs."""
    d = np.pi / 180.0
    if mode == "gicp":
        yaw = rng.uniform(-10, 10) * d
        pitch, roll = rng.uniform(-1, 1, 2) * d
        t = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-0.2, 0.2)])
    elif mode == "quatro":
        yaw = rng.uniform(-180, 180) * d
        pitch, roll = rng.uniform(-2, 2, 2) * d
        t = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-0.2, 0.2)])
    elif mode == "identity":
        yaw = pitch = roll = 0.0
        t = np.zeros(3)
    else:
        raise ValueError(mode)
    T = np.eye(4)
    T[:3, :3] = _rot_zyx(yaw, pitch, roll)
    T[:3, 3] = t
    return T


def make_pair(pair_id, n_src, n_tgt=None, *, extent=120.0, leaf=0.3, sigma=0.02,
              shift=None, mode="gicp"):
    """Returns (src[n_src,3] f32, tgt[n_tgt,3] f32, T_gt[4,4] f64).

    `shift` [m]: the target's scene window is the source's shifted along x (default extent/24,
    i.e. 5 m on the 120 m scene: ~96 % overlap, which keeps the PCL fitness score - the mean
    squared NN distance over ALL source points - under the reference's 1.5 m^2 accept
    threshold, loop_closure.cpp:129 + config.yaml:21, for a correct registration)."""
    n_tgt = n_src if n_tgt is None else n_tgt
    rng = np.random.Generator(np.random.PCG64(BASE_SEED + int(pair_id)))
    scene = Scene(rng, extent)
    T = random_gt(rng, mode)
    h = extent / 2.0
    shift = extent / 24.0 if shift is None else float(shift)
    win_s = (-h, h - shift, -h, h)
    win_t = (-h + shift, h, -h, h)

    def cloud(n, win, transform, noise):
        over = 3.0
        for _ in range(8):
            raw = scene.sample(rng, int(n * over) + 256, win)
            if noise > 0:
                raw = raw + rng.normal(0.0, noise, raw.shape)
            if transform is not None:
                raw = raw @ transform[:3, :3].T + transform[:3, 3]
            c = voxel_centroids(raw, leaf)
            if len(c) >= n:
                sel = rng.permutation(len(c))[:n]
                sel.sort()
                return c[sel].astype(np.float32)
            over *= 1.8
        raise RuntimeError("scene too small for %d points at leaf %.2f" % (n, leaf))

    src = cloud(n_src, win_s, None, 0.0)
    tgt = cloud(n_tgt, win_t, T, sigma)
    return src, tgt, T


def lever_arm_pair(seed, n=3000, offset=300.0, rot_sigma=0.1, scene=True, noise=0.05):
    """A small pair 300 m from the origin with a wrong initial rotation: the lever arm makes the cost strongly non-quadratic in the
    rotation, so Levenberg-Marquardt REJECTS trial steps (inner tries 2..9) - pairs near the origin never do.  scene = True: a street-scene
    pair (surface points: well-conditioned plane normals); False: uniform points in a cube (near-isotropic neighbourhoods: the plane normal
    of A.1.3 is ill-conditioned there, see SURVEY App. B-4 - for probing, not for strict parity).  -> (src, tgt, guess[4,4] f64)"""
    rng = np.random.Generator(np.random.PCG64(77000 + int(seed)))
    if scene:
        src, tgt, _ = make_pair(600 + int(seed), n, extent=30.0)
        off = np.array([offset, 0.0, 0.0])
        src = (src.astype(np.float64) + off).astype(np.float32); tgt = (tgt.astype(np.float64) + off).astype(np.float32)
    w = rng.normal(0, rot_sigma, 3); th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    if not scene:
        src = (rng.uniform(-3, 3, (n, 3)) + [offset, 0, 0]).astype(np.float32)
        tgt = (src + rng.normal(0, noise, (n, 3))).astype(np.float32)
    guess = np.eye(4); guess[:3, :3] = R; guess[:3, 3] = rng.uniform(-1, 1, 3)
    return src, tgt, guess


def pose_error(T_a, T_b):
    """(translation error [m], rotation error [rad]) between two 4x4 transforms."""
    D = np.linalg.inv(T_a) @ T_b
    c = (np.trace(D[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip(c, -1.0, 1.0)))


# ---------------------------------------------------------------------------------------------------------------------------------
# Spinning-LiDAR scans of the same scene (the ray-caster csrc/qn_sim.hip and its numpy twin `lidar_scan`, bit for bit).
# Primitives (PRIM_DTYPE = C struct qn_sim_prim): kind + six f64 parameters
#   PRIM_GROUND (x0, y0, x1, y1, -, -)  plane z = 0 over [x0, x1] x [y0, y1]
#   PRIM_WALL   (x0, y0, dx, dy, H, -)  zero-thickness vertical rectangle: dy == 0 -> plane y = y0 over x in [x0, x0 + dx], else plane x = x0
#                                       over y in [y0, y0 + dy]; z in [0, H]
#   PRIM_POLE   (cx, cy, r, H, -, -)    side surface of a vertical cylinder, z in [0, H]
#   PRIM_BOX    (cx, cy, sx, sy, H, -)  four sides (x = cx -+ sx/2, y = cy -+ sy/2) and the top z = H of a box standing on the ground
PRIM_GROUND, PRIM_WALL, PRIM_POLE, PRIM_BOX = 0, 1, 2, 3
PRIM_DTYPE = np.dtype([("kind", np.uint32), ("p", np.float64, (6,))], align=True)
SIM_SQRT3 = 1.7320508075688772                       # the noise is sigma * sqrt(3) * (u0 + u1 + u2 + u3 - 2): unit variance, no log / cos
SIM_INTENSITY = ((0.1, 0.3), (0.3, 0.5), (0.5, 0.4), (0.2, 0.6))   # per kind: intensity = base + gain * |n . d|
_U32 = np.uint32


class SpinningLidar:
    """A spinning multi-beam LiDAR: n_beams elevations spaced linearly over [el_min, el_max] degrees (HDL-64E-like), n_cols azimuths
    2 pi c / n_cols, blind radius min_range, detection range max_range, range noise sigma [m].  Defaults: 64 lines, blind 2 m and
    det_range 100 m of the reference's KITTI config; `height` is the mount height above the ground [m]."""

    height = 1.73

    def __init__(self, n_beams=64, el_min=-24.8, el_max=2.0, n_cols=1800, min_range=2.0, max_range=100.0, sigma=0.02):
        self.n_beams, self.n_cols = int(n_beams), int(n_cols)
        self.el_min, self.el_max = float(el_min), float(el_max)
        self.min_range, self.max_range, self.sigma = float(min_range), float(max_range), float(sigma)

    def elevations(self):
        return np.deg2rad(np.linspace(self.el_min, self.el_max, self.n_beams))

    def tables(self):
        """(cos el, sin el, cos az, sin az), f64: every transcendental the ray-caster needs, computed here on the host."""
        el = self.elevations()
        az = 2.0 * np.pi * np.arange(self.n_cols) / self.n_cols
        return np.cos(el), np.sin(el), np.cos(az), np.sin(az)

    @property
    def rays(self):
        return self.n_beams * self.n_cols


def _mix32(x):
    """32-bit integer finaliser (xor-shift / multiply); x: uint32 array, wraps like the device's uint32_t."""
    x = x ^ (x >> _U32(16)); x = x * _U32(0x7FEB352D)
    x = x ^ (x >> _U32(15)); x = x * _U32(0x846CA68B)
    return x ^ (x >> _U32(16))


def sim_uniforms(seed, beam, col):
    """The four uniforms of ray (beam, col) of a scan with this seed: u_i = mix32(base + i) / 2^32 with
    base = mix32(mix32(mix32(seed) ^ beam) ^ col) - counter-based, so any ray's noise is computed on its own."""
    base = _mix32(_mix32(_mix32(np.full(np.shape(beam), seed, _U32)) ^ beam.astype(_U32)) ^ col.astype(_U32))
    return [_mix32(base + _U32(i)).astype(np.float64) * 2.0 ** -32 for i in range(4)]


def lidar_scan(prims, sensor, pose, seed):
    """Numpy twin of the ray-caster (csrc/qn_sim.hip): the specification the kernel matches bit for bit.  One ray per (beam, col),
    from the pose's translation along d = R u, u = (cos el cos az, cos el sin az, sin el); primitives in index order, a hit kept only
    when strictly nearer (ties: lowest index); range noise along the ray; the noisy range t' gated to [min_range, max_range].
    -> (n, 4) float32 records x y z intensity, the point t' u in the SENSOR frame (PosePcd::pcd_), in (beam, col) order.
    All arithmetic f64 without fused multiply-adds, rounded to f32 once at the end."""
    prims = np.asarray(prims, dtype=PRIM_DTYPE).reshape(-1)
    ce, se, ca, sa = sensor.tables()
    nb, nc = len(ce), len(ca)
    T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    ux = (ce[:, None] * ca[None, :]).ravel(); uy = (ce[:, None] * sa[None, :]).ravel(); uz = np.repeat(se, nc)
    dx = T[0, 0] * ux + T[0, 1] * uy + T[0, 2] * uz
    dy = T[1, 0] * ux + T[1, 1] * uy + T[1, 2] * uz
    dz = T[2, 0] * ux + T[2, 1] * uy + T[2, 2] * uz
    ox, oy, oz = T[0, 3], T[1, 3], T[2, 3]
    n = nb * nc
    best = np.full(n, np.inf); kind = np.zeros(n, np.int64); cn = np.zeros(n)

    def hit(k, t, ok, c):
        m = ok & (t > 0.0) & (t < best)
        best[m] = t[m]; kind[m] = k; cn[m] = c[m]

    def inside(v, lo, hi):
        return (v >= lo) & (v <= hi)

    with np.errstate(all="ignore"):
        for pr in prims:
            k = int(pr["kind"]); p = pr["p"]
            if k == PRIM_GROUND:
                t = (0.0 - oz) / dz
                hit(k, t, (dz != 0.0) & inside(ox + t * dx, p[0], p[2]) & inside(oy + t * dy, p[1], p[3]), np.abs(dz))
            elif k == PRIM_WALL:
                if p[3] == 0.0:
                    t = (p[1] - oy) / dy
                    hit(k, t, (dy != 0.0) & inside(ox + t * dx, p[0], p[0] + p[2]) & inside(oz + t * dz, 0.0, p[4]), np.abs(dy))
                else:
                    t = (p[0] - ox) / dx
                    hit(k, t, (dx != 0.0) & inside(oy + t * dy, p[1], p[1] + p[3]) & inside(oz + t * dz, 0.0, p[4]), np.abs(dx))
            elif k == PRIM_POLE:
                px, py, r = ox - p[0], oy - p[1], p[2]
                a = dx * dx + dy * dy
                b = px * dx + py * dy
                c = px * px + py * py - r * r
                disc = b * b - a * c
                ok = (a > 0.0) & (disc >= 0.0)
                s = np.sqrt(np.where(ok, disc, 0.0))
                for t in ((-b - s) / a, (-b + s) / a):
                    hit(k, t, ok & inside(oz + t * dz, 0.0, p[3]), np.abs((px + t * dx) * dx + (py + t * dy) * dy) / r)
            elif k == PRIM_BOX:
                xlo, xhi = p[0] - 0.5 * p[2], p[0] + 0.5 * p[2]
                ylo, yhi = p[1] - 0.5 * p[3], p[1] + 0.5 * p[3]
                H = p[4]
                for xf in (xlo, xhi):
                    t = (xf - ox) / dx
                    hit(k, t, (dx != 0.0) & inside(oy + t * dy, ylo, yhi) & inside(oz + t * dz, 0.0, H), np.abs(dx))
                for yf in (ylo, yhi):
                    t = (yf - oy) / dy
                    hit(k, t, (dy != 0.0) & inside(ox + t * dx, xlo, xhi) & inside(oz + t * dz, 0.0, H), np.abs(dy))
                t = (H - oz) / dz
                hit(k, t, (dz != 0.0) & inside(ox + t * dx, xlo, xhi) & inside(oy + t * dy, ylo, yhi), np.abs(dz))
            else:
                raise ValueError("unknown primitive kind %d" % k)
    beam, col = np.divmod(np.arange(n, dtype=np.int64), nc)
    u0, u1, u2, u3 = sim_uniforms(int(seed) & 0xFFFFFFFF, beam, col)
    tp = best + sensor.sigma * SIM_SQRT3 * ((((u0 + u1) + u2) + u3) - 2.0)
    keep = np.flatnonzero(np.isfinite(best) & (tp >= sensor.min_range) & (tp <= sensor.max_range))
    base = np.array([g[0] for g in SIM_INTENSITY]); gain = np.array([g[1] for g in SIM_INTENSITY])
    out = np.empty((len(keep), 4), np.float32)
    t = tp[keep]
    out[:, 0] = t * ux[keep]; out[:, 1] = t * uy[keep]; out[:, 2] = t * uz[keep]
    out[:, 3] = base[kind[keep]] + gain[kind[keep]] * cn[keep]
    return out


def sensor_pose(x, y, yaw, z=SpinningLidar.height):
    T = np.eye(4); T[:3, :3] = _rot_zyx(yaw, 0.0, 0.0); T[:3, 3] = [x, y, z]
    return T


def _free_spot(scene, x, y, clearance=1.5):
    """True when (x, y) is at least `clearance` from every wall, pole and box footprint (a sensor there sees the street)."""
    for x0, y0, dx, dy, _ in scene.walls:
        if x0 - clearance <= x <= x0 + dx + clearance and y0 - clearance <= y <= y0 + dy + clearance:
            return False
    for cx, cy, r, _ in scene.poles:
        if (x - cx) ** 2 + (y - cy) ** 2 <= (r + clearance) ** 2:
            return False
    for cx, cy, sx, sy, _ in scene.boxes:
        if abs(x - cx) <= sx / 2 + clearance and abs(y - cy) <= sy / 2 + clearance:
            return False
    return True


def make_lidar_pair(pair_id, *, separation=5.0, mode="gicp", leaf=0.3, sensor=None):
    """Returns (src[n_src,3] f32, tgt[n_tgt,3] f32, T_gt[4,4] f64) with make_pair's meaning, from two spinning-LiDAR scans (the numpy
    twin) of a 120 m street scene taken at poses `separation` metres apart along the first pose's heading:
      source = scan A in the world frame, voxel centroids at `leaf`
      target = T_gt * (scan B in the world frame), voxel centroids at `leaf`
    N is whatever the two scans give (no resampling).  seed = 20241220 + 500000 + pair_id."""
    sensor = SpinningLidar() if sensor is None else sensor
    rng = np.random.Generator(np.random.PCG64(BASE_SEED + 500000 + int(pair_id)))
    scene = Scene(rng, 120.0)
    T = random_gt(rng, mode)
    for _ in range(200):
        x, y = rng.uniform(-25.0, 25.0, 2); yaw = rng.uniform(-np.pi, np.pi)
        xb, yb = x + separation * np.cos(yaw), y + separation * np.sin(yaw)
        if _free_spot(scene, x, y) and _free_spot(scene, xb, yb):
            break
    else:
        raise RuntimeError("no free sensor spot in pair %d" % pair_id)
    seeds = rng.integers(0, 2 ** 32, 2)
    prims = scene.primitives()

    def world(x, y, seed):
        P = sensor_pose(x, y, yaw)
        s = lidar_scan(prims, sensor, P, int(seed))[:, :3].astype(np.float64)
        return s @ P[:3, :3].T + P[:3, 3]

    src = voxel_centroids(world(x, y, seeds[0]), leaf).astype(np.float32)
    wb = world(xb, yb, seeds[1])
    tgt = voxel_centroids(wb @ T[:3, :3].T + T[:3, 3], leaf).astype(np.float32)
    return src, tgt, T
