"""The case table of the Scan Context family (csrc/qn_sc.hip: k_sc_bin, k_sc_finish, k_sc_ringkey, k_sc_dist, k_sc_select, k_sc_gather and the host
loops of qn_kf_sc_describe / qn_kf_sc_query): deterministic inputs, each built to put records ON an edge of the binning arithmetic or to cross a seam of
a launch, with the expected bins, values, distances, shifts and result order stated BY CONSTRUCTION wherever the geometry gives them - never read back
from the engine, and from the twin only where a distance has no closed form (then the tie classes and their order are still by construction).
tests/test_sc_edges_cpu.py holds the twin (qn_amd/scancontext.py) to a scalar restatement of the header's definition and to these expectations;
tests/test_gpu_sc_edges.py holds the engine to the twin and to them.  Pure numpy, no GPU, no random draws.

Seams and the constant each belongs to (restated from csrc/qn_sc.hip; whoever changes one there changes it here):
  SC_BIN_BLOCK 256, SC_BIN_TILE 256 * 16        threads / records per block of k_sc_bin ("#define SC_BIN_BLOCK 256", "#define SC_BIN_TILE (SC_BIN_BLOCK * 16)")
  SC_DIST_ITERS 4                               candidates per wave of a k_sc_dist block ("#define SC_DIST_ITERS 4"); waves = clamp(65536 / stage, 1, 4),
                                                stage = align16(8 Ns + 4 Nr Ns), per_block = waves * SC_DIST_ITERS (qn_kf_sc_query: "const uint32_t stage", "waves")
  SC_SEL_BLOCK 256, SC_SEL_MAX 1024             threads / staged entries of k_sc_select; 8 key digits then 4 id digits of 8 bits
  SC_SCRATCH_BYTES 256 << 20, SC_MAX_ROWS 65535 queries per chunk: qc = min(nq, SC_SCRATCH_BYTES / per_q, 65535) (qn_kf_sc_query: "const size_t per_q", "qc")
  SC_DESCRIBE_CHUNK 8192                        keyframes per describe launch ("#define SC_DESCRIBE_CHUNK 8192u")
  SC_MIN_CAP 64                                 sc_reserve: cap = max(n, 2 cap, 64)

Sensitivity (each single mutation of the twin makes the named case fail in tests/test_sc_edges_cpu.py):
  ring test >= -> >              knife "pythagoras" (the on-edge records (12, 16), (-16, 12), ... fall one ring)
  cross test >= -> >             knife "diagonal-8" ... (the records (23, 23), (46, 46), (51, 51): both products round to the same f64, the cross is 0.0)
  hp > hb -> hp >= hb            knife "half-plane" ((5, -1e-45) must land in sector 59) and every upper-half record of "pythagoras"
  r2 < e[nr] -> <=               knife "pythagoras" ((48, -64), r2 == 6400, must be dropped)
  argmin takes the last minimum  distance shape (8, 128): roll 5 of a period-64 descriptor has its minima at shifts 5 and 69
  order key (D, -id)             selection "ties": the 255th .. 257th entries are ids 254, 255, 256 of one tie class
  tdiff test not strict          selection "strict-tdiff": keyframe 697 sits exactly tdiff before the query
On the GPU the whole-cloud descriptor of a knife cloud cannot show the first four (an on-edge record shares both candidate bins with its neighbours, all at
one height), so tests/test_gpu_sc_edges.py also describes every knife record as a keyframe of its own (single_records): the descriptor of a one-record
keyframe IS the record's bin, and k_sc_bin with any of those four comparisons changed puts the records named above into another bin or keeps a dropped one."""
import math
from fractions import Fraction
import numpy as np
from qn_amd import scancontext as sc

SC_BIN_BLOCK, SC_BIN_TILE = 256, 256 * 16
SC_DIST_ITERS = 4
SC_SEL_BLOCK, SC_SEL_MAX = 256, 1024
SC_SCRATCH_BYTES, SC_MAX_ROWS = 256 << 20, 65535
SC_DESCRIBE_CHUNK = 8192
SC_MIN_CAP = 64

DEFAULT = sc.Params()
F32 = np.float32


def stage_bytes(nr, ns):
    return (8 * ns + 4 * nr * ns + 15) & ~15


def waves(nr, ns):
    return max(1, min(4, (64 << 10) // stage_bytes(nr, ns)))


def per_block(nr, ns):
    return waves(nr, ns) * SC_DIST_ITERS


def per_query_bytes(N, P, K):
    M = P if P > 0 else N
    return M * 12 + ((N * 8 + P * 4 + 4) if P > 0 else 0) + K * 4 + 4


def query_chunk(nq, N, P, K):
    return max(1, min(nq, SC_SCRATCH_BYTES // per_query_bytes(N, P, K), SC_MAX_ROWS))


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def away(v):
    """the f32 neighbour of v with the larger magnitude"""
    return np.nextafter(F32(v), F32(np.copysign(np.inf, v)))


def inward(v):
    """the f32 neighbour of v with the smaller magnitude"""
    return np.nextafter(F32(v), F32(0.0) * F32(np.copysign(1.0, v)))


def centre(ring, sector, p=DEFAULT):
    """(x, y) of the centre of a bin in f64: half a ring and half a sector (>= 0.5 degree here) from every edge, f32 rounding moves it 1e-7"""
    r = (ring + 0.5) * p.max_radius / p.n_rings
    a = 2.0 * math.pi * (sector + 0.5) / p.n_sectors
    return r * math.cos(a), r * math.sin(a)


def cloud_of(values, p=DEFAULT):
    """one record at the centre of every bin whose value is not 0, at z = value - lidar_height (exact for the small dyadic values used here): the
    descriptor of the cloud is `values`"""
    values = np.asarray(values, np.float64)
    out = []
    for i, j in zip(*np.nonzero(values)):
        x, y = centre(int(i), int(j), p)
        out.append([x, y, values[i, j] - p.lidar_height])
    return np.array(out, F32).reshape(-1, 3)


def keys_of(values):
    """(ring key, column norms) of a descriptor given as an array of f32-representable values, restated here from the definition with Python floats in
    its order (independent of the twin's keys()): rk[i] = (sum over j in order) / Ns, cn[j] = sqrt(sum over i in order of d[i][j]^2)"""
    d = [[float(v) for v in row] for row in np.asarray(values, F32)]
    nr, ns = len(d), len(d[0])
    rk, cn = [], []
    for i in range(nr):
        acc = 0.0
        for j in range(ns):
            acc = acc + d[i][j]
        rk.append(acc / ns)
    for j in range(ns):
        acc = 0.0
        for i in range(nr):
            acc = acc + d[i][j] * d[i][j]
        cn.append(math.sqrt(acc))
    return np.array(rk), np.array(cn)


# ---- the definition's binning with exact rationals (one rounding where the definition rounds once)
def table_values(p):
    """the host tables, restated: edges squared, cos, sin as Python floats"""
    nr, ns, R = int(p.n_rings), int(p.n_sectors), float(p.max_radius)
    e = [(float(i) * R / nr) * (float(i) * R / nr) for i in range(nr)] + [R * R]
    return e, [math.cos(2.0 * math.pi * j / ns) for j in range(ns)], [math.sin(2.0 * math.pi * j / ns) for j in range(ns)]


def exact_bins(x, y, p, tabs=None):
    """-> (ring, sector, keep) of a finite f32 (x, y): r2 is the exact x^2 + y^2 rounded ONCE to f64 (each square of an f32 is exact in f64, so the
    definition's x*x + y*y rounds once too); each product of the cross test is the exact product rounded once, the difference of two f64 has the sign
    of their exact difference"""
    e, c, s = tabs or table_values(p)
    fx, fy = Fraction(float(x)), Fraction(float(y))
    r2 = float(fx * fx + fy * fy)
    keep = not (fx == 0 and fy == 0) and r2 < e[-1]
    ring = sum(1 for i in range(1, p.n_rings) if r2 >= e[i])
    hp = 0 if (fy > 0 or (fy == 0 and fx > 0)) else 1
    sector = 0
    for j in range(1, p.n_sectors):
        hb = 0 if (s[j] > 0.0 or (s[j] == 0.0 and c[j] > 0.0)) else 1
        cross = Fraction(float(Fraction(c[j]) * fy)) - Fraction(float(Fraction(s[j]) * fx))
        sector += 1 if (hp > hb or (hp == hb and cross >= 0)) else 0
    return ring, sector, keep


class Knife:
    """a cloud on the edges of the binning: `bins` = (ring, sector, keep) of every record from exact_bins, `pinned` = [(record, ring or None, sector or
    None, keep)] stated from the geometry alone, `desc` = {(ring, sector): value} stated from the geometry where the case is about values (else None)"""

    def __init__(self, name, params, cloud, pinned=(), desc=None):
        self.name, self.params, self.cloud, self.pinned, self.desc = name, params, np.asarray(cloud, F32).reshape(-1, 3), list(pinned), desc
        self._bins = None

    @property
    def bins(self):
        if self._bins is None:
            tabs = table_values(self.params)
            self._bins = [exact_bins(x, y, self.params, tabs) for x, y, _ in self.cloud.tolist()]
        return self._bins


def single_records(k):
    """-> [(cloud of one record, {(ring, sector): value} or {} when the record is dropped)] for every record of a knife cloud, from its exact bins: what a
    one-record keyframe's descriptor must be"""
    out = []
    for (ring, sector, keep), rec in zip(k.bins, k.cloud):
        v = F32(np.float64(rec[2]) + k.params.lidar_height)
        out.append((rec.reshape(1, 3).copy(), {(ring, sector): v} if keep else {}))
    return out


def with_neighbours(x, y, z=1.0):
    """the record, then |x| one f32 down and up, then |y| one f32 down and up"""
    x, y = F32(x), F32(y)
    return [[x, y, z], [inward(x), y, z], [away(x), y, z], [x, inward(y), z], [x, away(y), z]]


# Pythagorean triples scaled onto the ring edges r = 4 i of the default parameters: the coordinates are exact in f32, r2 is exact in f64
TRIPLES = [(12, 16, 5), (-16, 12, 5), (-12, -16, 5), (16, -12, 5), (24, -32, 10), (-20, 48, 13), (-60, -32, 17), (48, -64, 20), (-64, -48, 20), (64, 48, 20)]


def knife_pythagoras():
    rows, pinned = [], []
    for x, y, i in TRIPLES:
        # at r = 4 i exactly: ring i (the edge belongs to the upper ring), i == 20 is r2 == max_radius^2: dropped.  One f32 inward: ring i - 1.
        for k, rec in enumerate(with_neighbours(x, y)):
            on_or_out = k in (0, 2, 4)
            ring = i if on_or_out else i - 1
            pinned.append((len(rows), ring if ring < 20 else None, None, ring < 20))
            rows.append(rec)
    # atan2(16, 12) = 53.13 deg = 8.86 sectors of 6 deg; (-16, 12): 143.13 deg = 23.86; (48, -64): 306.87 deg = 51.14 (inward neighbours: the same sector)
    pinned += [(0, 5, 8, True), (5, 5, 23, True), (35, None, None, False), (36, 19, 51, True), (38, 19, 51, True)]
    return Knife("pythagoras", DEFAULT, rows, pinned)


ODD = sc.Params(n_rings=7, n_sectors=13, max_radius=25.0, lidar_height=2.0)


def knife_odd_ring_width():
    """ring edges i * 25 / 7, not representable: records at the f32 nearest to the edge along four directions and two f32 steps to either side; and the
    triples of r == 25 exactly (dropped; one f32 inward: ring 6)"""
    rows, pinned = [], []
    for i in range(1, 7):
        r = i * 25.0 / 7.0
        for cx, cy in ((1.0, 0.0), (0.6, 0.8), (-5.0 / 13.0, 12.0 / 13.0), (-8.0 / 17.0, -15.0 / 17.0), (0.28, -0.96)):
            x, y = F32(r * cx), F32(r * cy)
            rows.append([x, y, 1.0])
            for step in (1, 2):
                xi, xo, yi, yo = x, x, y, y
                for _ in range(step):
                    xi, xo, yi, yo = inward(xi), away(xo), inward(yi), away(yo)
                rows += [[xi, y, 1.0], [xo, y, 1.0], [x, yi, 1.0], [x, yo, 1.0]] if cy else [[xi, y, 1.0], [xo, y, 1.0]]
    for x, y in ((15, 20), (7, -24), (-20, 15), (-24, -7)):
        for k, rec in enumerate(with_neighbours(x, y)):
            pinned.append((len(rows), None if k in (0, 2, 4) else 6, None, k not in (0, 2, 4)))
            rows.append(rec)
    return Knife("odd-ring-width", ODD, rows, pinned)


DIAGONAL_NS = (8, 16, 24, 40, 120, 360)


def knife_diagonal(ns):
    """(+-r, +-r) for Ns a multiple of 8: the boundary direction b_{Ns/8} is (cos, sin)(pi / 4) as the C library rounds them - here cos is one f64 step
    above sin, so (r, r) is at or past the boundary (for r = 23, 46, 51 both products round to the same f64 and the cross is exactly 0).  The expectation
    comes from exact_bins on the table values, whatever they are."""
    p = sc.Params(n_rings=4, n_sectors=ns, max_radius=80.0, lidar_height=2.0)
    rows = []
    for r in (1.0, 3.0, 5.0, 23.0, 46.0, 51.0, F32(0.1), F32(33.3), F32(1e-3)):
        for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
            rows += with_neighbours(sx * r, sy * r)
    return Knife("diagonal-%d" % ns, p, rows)


def knife_half_plane():
    """y = +0, -0 and the f32 subnormals +-1e-45 on both sides of the x axis.  sin(pi) from the C library is +1.22e-16, so boundary 30 of 60 counts as
    the UPPER half plane and lies a hair before the -x axis: (-5, +1e-45) is past it - sector 30, not 29 - and so are (-5, +-0) and (-5, -1e-45).
    (5, -1e-45) is in the lower half plane and past every boundary: sector 59.  This pins the definition as it stands."""
    tiny = F32(1e-45)
    rows, pinned = [], []
    for x in (-5.0, F32(-79.99), F32(-1e-3)):
        for y in (F32(0.0), F32(-0.0), tiny, -tiny):
            pinned.append((len(rows), None, 30, True)); rows.append([x, y, 1.0])
    for x in (5.0, F32(79.99), F32(1e-3)):
        for y, sec in ((F32(0.0), 0), (F32(-0.0), 0), (tiny, 0), (-tiny, 59)):
            pinned.append((len(rows), None, sec, True)); rows.append([x, y, 1.0])
    return Knife("half-plane", DEFAULT, rows, pinned)


def knife_values():
    """value edges, each in a bin of its own (centres), the descriptor stated from the arithmetic:
      (4, 10)  z = -3 and -2.5: the maximum -0.5 is negative and stays, beside the empty bin (4, 11) = 0
      (5, 0)   z = -lidar_height: value 0, the same as an empty bin
      (6, k)   z + 2 at the f32 rounding edges: the f32 step at 2 is 2^-22, so z = 2^-23 is a tie and goes to the even 2.0, one f32 above it goes up to
               2 + 2^-22, one below stays 2.0; z = 3 * 2^-23 is a tie between 2 + 2^-22 (odd) and 2 + 2^-21 (even): even; its lower neighbour goes to
               2 + 2^-22, its upper to 2 + 2^-21"""
    h, t = 2.0 ** -23, 2.0 ** -22
    zs = [F32(h), up(h), down(h), F32(3 * h), down(3 * h), up(3 * h)]
    vals = [2.0, 2.0 + t, 2.0, 2.0 + 2 * t, 2.0 + t, 2.0 + 2 * t]
    rows = [[*centre(4, 10), -3.0], [*centre(4, 10), -2.5], [*centre(5, 0), -2.0]] + [[*centre(6, k), z] for k, z in enumerate(zs)]
    desc = {(4, 10): -0.5, (5, 0): 0.0}
    desc.update({(6, k): v for k, v in enumerate(vals)})
    pinned = [(0, 4, 10, True), (1, 4, 10, True), (2, 5, 0, True)] + [(3 + k, 6, k, True) for k in range(6)]
    return Knife("values", DEFAULT, rows, pinned, desc)


def knives():
    return [knife_pythagoras(), knife_odd_ring_width(), knife_half_plane(), knife_values()] + [knife_diagonal(ns) for ns in DIAGONAL_NS]


# ---- tile seams of k_sc_bin
TILE_COUNTS = [1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193]
FLOOR_BIN, DECIDING_BIN = (2, 3), (7, 41)


def tile_keyframes():
    """-> [(cloud, {(ring, sector): value})]: n records in the floor bin at z = -1.25 (value 0.75), one of them (the middle one) at z = -1 (value 1.0, the
    bin's maximum), and ONE record that alone sets another bin to 5.5: the last record (variant 0) or the first record of the last tile (variant 1)"""
    fx, fy = centre(*FLOOR_BIN)
    dx, dy = centre(*DECIDING_BIN)
    out = []
    for variant in (0, 1):
        for n in TILE_COUNTS:
            a = np.empty((n, 3), F32)
            a[:] = [fx, fy, -1.25]
            pos = n - 1 if variant == 0 else ((n - 1) // SC_BIN_TILE) * SC_BIN_TILE
            mid = (n - 1) // 2
            want = {DECIDING_BIN: 5.5}
            if mid != pos:
                a[mid, 2] = -1.0
                want[FLOOR_BIN] = 1.0
            elif n > 1:
                want[FLOOR_BIN] = 0.75
            a[pos] = [dx, dy, 3.5]
            out.append((a, want))
    return out


def dense(want, p=DEFAULT):
    d = np.zeros((p.n_rings, p.n_sectors), F32)
    for (i, j), v in want.items():
        d[i, j] = v
    return d


# ---- distance cases: periodic descriptors against themselves rolled
def periodic(nr, ns, period):
    """(nr, ns) values with column period `period` (<= 64, nr >= 7): column jj of a period spells jj in binary over the rings (i mod 7), entries 1 + bit,
    row i scaled by 1 + i mod 3.  Two columns of a period are proportional only if equal (entries 1 or 2 before the row scale, and no jj < 64 has seven
    bits set), so against itself rolled by k every shift s != k mod period pairs every column with a non-parallel one: D_s > 0 by Cauchy-Schwarz with a
    margin far above rounding, while s = k mod period pairs equal columns: every term is 1 - ss / sqrt(ss ss) = 0 exactly."""
    assert period <= 64 and nr >= 7 and ns % period == 0
    v = np.zeros((nr, ns))
    for i in range(nr):
        for j in range(ns):
            v[i, j] = (1 + (((j % period) >> (i % 7)) & 1)) * (1 + i % 3)
    return v


def other(nr, ns, m):
    """a descriptor unrelated to periodic(): no period, every ninth column empty"""
    v = np.zeros((nr, ns))
    for i in range(nr):
        for j in range(ns):
            if (j + m) % 9:
                v[i, j] = (1 + (((j * 3 + m * 5) >> (i % 7)) & 1)) * (1 + (i + m) % 3) * 0.5
    return v


# shape -> (period, rolls of the odd keyframes in order).  waves: (20, 60) 4, (30, 128) 4 at stage == 16384 (65536 bytes of LDS), (50, 100) 3, (64, 100) 2,
# (64, 128) 1, (8, 128) and (8, 120) 4.  Equal minima: (8, 128) roll 5 -> shifts 5 and 69, the same lane; (8, 120) rolls 2 and 10 -> 2 / 62 and 10 / 70,
# different lanes; (30, 128) roll 63 -> 63 and 127, the last lane twice.
DIST_SHAPES = {(20, 60): (30, [7, 29, 30, 31, 59, 1, 45, 15, 3]), (30, 128): (64, [63, 5, 64, 127, 1, 65, 100, 32, 9]), (50, 100): (50, [49, 50, 51, 99, 1, 25, 75]),
               (64, 100): (25, [24, 26, 99, 1, 50]), (64, 128): (32, [31, 33, 127, 65]), (8, 128): (64, [5, 63, 64, 69, 1, 127, 70, 33, 2]),
               (8, 120): (60, [2, 10, 59, 60, 61, 119, 1, 30, 62])}


class DistWorld:
    """one store of a shape: keyframe 0 is the query (periodic, not rolled); odd ids are the query's descriptor rolled by rolls[...] (D == 0.0, shift ==
    roll mod period by construction); even ids are other().  stamps[c] = -c: every other keyframe is older than the query 0 by more than tdiff = 0.5."""

    def __init__(self, nr, ns):
        self.nr, self.ns = nr, ns
        self.period, rolls = DIST_SHAPES[(nr, ns)]
        self.params = sc.Params(n_rings=nr, n_sectors=ns, max_radius=80.0, lidar_height=2.0)
        self.per_block = per_block(nr, ns)
        self.count = self.per_block + 2                              # exhaustive at N = per_block - 1, per_block, per_block + 1; then one more for the prefilter
        base = periodic(nr, ns, self.period)
        self.values, self.rolled = [base], {}
        for m in range(1, self.count):
            if m % 2:
                k = rolls[(m // 2) % len(rolls)]
                self.values.append(np.roll(base, k, axis=1)); self.rolled[m] = k
            else:
                self.values.append(other(nr, ns, m))
        self.clouds = [cloud_of(v, self.params) for v in self.values]
        self.stamps = -np.arange(self.count, dtype=np.float64)
        self.tdiff = 0.5

    def zero_class(self, ids):
        """the candidates among `ids` at exactly 0, in result order, with their shifts"""
        return [(c, 0.0, self.rolled[c] % self.period) for c in sorted(ids) if c in self.rolled]


# ---- selection cases (default shape): one store, the candidate set of each query chosen by the stamps passed with it
Q_BINS = {(3, 5): 2.0, (8, 5): 1.0, (6, 20): 3.0, (10, 44): 1.5}                  # the query's cloud
A2_BINS = {(3, 5): 2.5, (8, 5): 1.0, (6, 20): 3.0, (10, 44): 1.5}                 # one value off: D_A > 0, ring-key distance (0.5 / 60)^2
A_BINS = {(3, 5): 2.5, (8, 5): 1.0, (6, 20): 6.0, (10, 44): 1.5}                  # A2 with column 20 doubled: the SAME D bit for bit (a power of two scales dot and
#                                                                                   sqrt(ss ss) alike at every shift), ring-key distance larger by (3 / 60)^2
B_BINS = {(3, 5): 2.0, (8, 5): 3.0, (6, 20): 3.0, (10, 44): 5.5}                  # farther in both: cos of column 5 is 0.868 (A: 0.9966), ring-key (2^2 + 4^2) / 60^2
FAR_BINS = {(15, 0): 1.0}                                                         # ring 15 is in no other cloud: every dot is 0, D == 1.0 at every shift, shift 0


class SelectWorld:
    """Keyframes of four records (not one to three: column 5 needs two rings for an angle other than 0 between two clouds, and columns 20 and 44 carry the
    scaled column and the ring-key difference); they are as cheap to add.  ids 0 .. 699, the tie world (query 699):
         A   0 .. 319 without 100, 101      318 keyframes at one D
         A2  400 .. 449                     the same D, nearer by ring key: the prefilter lists them BEFORE A, so D ties arrive out of id order
         Q   690, 691                       the query's own cloud: D == 0.0
         B   everything else below 699
       ids 700 .. 999: empty keyframes; 1000: FAR (the query of the empties)
       ids 1001 .. 1040: `ulps` - A with the value of bin (3, 5) raised by m = 1 .. 40 f32 steps, m scrambled over the ids (query 1041 = Q's cloud): D and
         the ring-key distance grow with m, by 1e-7 relative per step: keys that differ in their low bytes only
       ids 1042 .. 1074: `decades` - Q with bin (3, 5) at 2 + 2^e, e = -22 .. 10, scrambled (query 1075 = Q's cloud): ring-key distances (2^e / 60)^2
         from 1.6e-17 to 2.9e2"""
    N_TIES = 700

    def __init__(self):
        p = DEFAULT
        cl = {k: cloud_of(dense(b), p) for k, b in (("Q", Q_BINS), ("A", A_BINS), ("A2", A2_BINS), ("B", B_BINS), ("FAR", FAR_BINS))}
        self.kind = []
        for i in range(self.N_TIES):
            if i in (690, 691, 699):
                self.kind.append("Q")
            elif i < 320 and i not in (100, 101):
                self.kind.append("A")
            elif 400 <= i < 450:
                self.kind.append("A2")
            else:
                self.kind.append("B")
        self.clouds = [cl[k] for k in self.kind]
        self.a_ids = [i for i in range(self.N_TIES) if self.kind[i] == "A"]
        self.a2_ids = list(range(400, 450))
        self.empties = list(range(700, 1000))
        self.clouds += [np.zeros((0, 3), F32)] * 300 + [cl["FAR"]]
        self.q_empty = 1000
        self.ulp_ids, self.ulp_of = [], {}
        base = F32(2.5)
        for k in range(40):
            m = (k * 17) % 40 + 1                                    # 17 is coprime to 40: every m once
            v = base
            for _ in range(m):
                v = up(v)
            b = dict(A_BINS); b[(3, 5)] = v
            d = dense(b, p)
            c = cloud_of(d, p)
            c[0, 2] = F32(np.float64(v) - 2.0)                       # bin (3, 5) is the first non-zero bin: its z so that z + 2 is v exactly (v - 2 is exact)
            self.ulp_of[len(self.clouds)] = m; self.ulp_ids.append(len(self.clouds)); self.clouds.append(c)
        self.q_ulp = len(self.clouds); self.clouds.append(cl["Q"])
        self.dec_ids, self.dec_of = [], {}
        for k in range(33):
            e = (k * 5) % 33 - 22
            b = dict(Q_BINS); b[(3, 5)] = 2.0 + 2.0 ** e
            c = cloud_of(dense(b, p), p)
            c[0, 2] = F32(2.0 ** e)
            self.dec_of[len(self.clouds)] = e; self.dec_ids.append(len(self.clouds)); self.clouds.append(c)
        self.q_dec = len(self.clouds); self.clouds.append(cl["Q"])
        self.count = len(self.clouds)

    def stamps_for(self, q, cands):
        """stamps that admit exactly `cands` for query q under tdiff = 1"""
        st = np.full(self.count, 1000.0)
        st[list(cands)] = 0.0
        st[q] = 100.0
        return st

    def tie_stamps(self):
        """the tie world's stamps: seconds 0 .. 698 and the query at 699 - under tdiff = 2.0 keyframe 697 is exactly tdiff older (not admissible: the
        test is strict), 698 is younger than that, 0 .. 696 are admissible; everything past 699 is newer than the query"""
        st = np.arange(self.count, dtype=np.float64)
        return st

    def tie_prefix(self, top_k, prefilter=0):
        """the head of query 699's result by construction -> ids in order (the D == 0 pair, then the A / A2 tie class by id)"""
        if prefilter:
            listed = ([690, 691] + self.a2_ids + self.a_ids)[:prefilter]              # ring-key rank: rk distance 0, then A2, then A; ties by id
        else:
            listed = [690, 691] + self.a_ids + self.a2_ids
        zero = [c for c in listed if self.kind[c] == "Q"]
        tie = sorted(c for c in listed if self.kind[c] in ("A", "A2"))
        return (zero + tie)[:top_k]


# ---- chunk seams: tiny indexed keyframes
def tiny_bin(i, rings=20):
    """keyframe i's single record: ring i mod rings, sector (i / rings) mod 60, value 1 + (i / (60 rings)) / 2 - distinct over i < 8 * 60 * rings"""
    return i % rings, (i // rings) % 60, 1.0 + 0.5 * (i // (rings * 60))


def tiny_cloud(i, rings=20):
    r, s, v = tiny_bin(i, rings)
    x, y = centre(r, s)
    return np.array([[x, y, v - 2.0]], F32)


def tiny_pair(q, c, rings=20):
    """(D, shift) of tiny keyframe q against c: one column each.  The same ring: the one shift that aligns the columns gives 1 - v v' / sqrt(v^2 v'^2) = 0,
    every other shift has no common column (D_s = 1).  Different rings: the aligning shift gives 1 - 0, the others 1: D = 1 at the lowest shift, 0."""
    rq, sq, _ = tiny_bin(q, rings)
    rc, s_c, _ = tiny_bin(c, rings)
    return (0.0, (s_c - sq) % 60) if rq == rc else (1.0, 0)


def tiny_query(q, cands, top_k, rings=20):
    """the result rows of query q over the admissible ids `cands` by construction"""
    rows = sorted((tiny_pair(q, c, rings)[0], c) for c in cands)[:top_k]
    return [(c, D, tiny_pair(q, c, rings)[1]) for D, c in rows]


DESCRIBE_COUNT = SC_DESCRIBE_CHUNK + 5
GROWTH_STEPS = (10, 65, 200)                                         # sc_reserve: capacity 64, then 128, then 256
ROWCAP_KEYFRAMES, ROWCAP_RINGS, ROWCAP_NQ = 8, 3, SC_MAX_ROWS + 3
SCRATCH_N, SCRATCH_P, SCRATCH_K = 200, 1024, 3


def rowcap_queries():
    return (np.arange(ROWCAP_NQ, dtype=np.int64) * 5 + 3) % ROWCAP_KEYFRAMES


def scratch_queries():
    """-> (query ids, qc): qc + 7 queries among keyframes 100 .. 199 of the growth store"""
    qc = SC_SCRATCH_BYTES // per_query_bytes(SCRATCH_N, SCRATCH_P, SCRATCH_K)
    nq = qc + 7
    return 100 + (np.arange(nq, dtype=np.int64) * 37) % 100, qc


def tiny_rows(queries, n_keyframes, top_k, rings=20):
    """stamps[i] = i, tdiff = 0.5: the candidates of q are the ids below q.  -> (ids [nq, top_k], D, shift, n) with the padding -1 / NaN / -1, the rows of
    each distinct query computed once"""
    memo = {}
    nq = len(queries)
    ids = np.full((nq, top_k), -1, np.int32); D = np.full((nq, top_k), np.nan); sh = np.full((nq, top_k), -1, np.int32); n = np.zeros(nq, np.uint32)
    for q in sorted(set(int(v) for v in queries)):
        memo[q] = tiny_query(q, range(min(q, n_keyframes)), top_k, rings)
    for q, rows in memo.items():
        at = np.flatnonzero(np.asarray(queries) == q)
        n[at] = len(rows)
        for r, (c, d, s) in enumerate(rows):
            ids[at, r] = c; D[at, r] = d; sh[at, r] = s
    return ids, D, sh, n
