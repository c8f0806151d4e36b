"""Inputs for the direct tests of the neighbour search's building blocks (tests/test_search_cpu.py, tests/test_gpu_search.py): five small clouds that reach every
path of csrc/qn_device.cuh's searches at a fixed cell edge (the knob `cell`: 1 m, and 0.45 m where the f32 cell arithmetic has to round), their queries, and the
sink sequences.  Deterministic; built once per process."""
import functools
import numpy as np
import search_checks as chk

F = np.float32
CLOUDS = ("seams", "lattice", "slabs", "shifted", "edges")
CELLS = {"seams": 1.0, "lattice": 1.0, "slabs": 1.0, "shifted": 1.0, "edges": 0.45}      # the knob `cell` each cloud's grid is built under


def _ulps(v, ks=(-2, -1, 0, 1, 2)):
    v = F(v)
    out = []
    for k in ks:
        x = v
        for _ in range(abs(k)):
            x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
        out.append(x)
    return out


def _seams(origin):
    """(a) 17 x 9 x 9 cells: the tile seams at x-cell 8 and 16 and at y / z-cell 4 and 8 lie inside; emptied rows, part-rows, exact duplicates, points on and
    one or two ulps beside cell, tile and grid faces"""
    rng = np.random.default_rng(11)
    o = np.asarray(origin, dtype=np.float64)
    p = rng.uniform([0, 0, 0], [16.9, 8.9, 8.9], size=(3300, 3))
    cy, cz, cx = np.floor(p[:, 1]).astype(int), np.floor(p[:, 2]).astype(int), np.floor(p[:, 0]).astype(int)
    keep = np.ones(len(p), dtype=bool)
    keep &= ~((cy == 2) & (cz == 3))                                   # emptied rows
    keep &= ~((cy == 4) & (cz == 4))
    keep &= ~((cy == 8) & (cz == 7))
    keep &= ~((cy == 5) & (cz == 1) & (cx < 6))                        # part-rows
    keep &= ~((cy == 3) & (cz == 6) & (cx > 9))
    keep &= ~((cy == 7) & (cz == 8) & (cx != 8))
    p = p[keep]
    face = []
    for x in (1.0, 8.0, 16.0):                                         # points on cell, tile and (almost) grid faces and beside them
        for y in (0.5, 4.0, 8.0):
            for z in (2.5, 4.0, 8.0):
                for dx in _ulps(F(o[0] + x)):
                    face.append((float(dx) - o[0], y, z))
    p = np.concatenate([p, np.array(face), [[0, 0, 0], [16.5, 8.5, 8.5]]])
    pts = (p + o).astype(np.float32)
    pts = np.concatenate([pts, pts[5:45], pts[5:15]])                 # exact duplicates (some three times)
    return pts[rng.permutation(len(pts))]


def _lattice():
    """(b) a 0.5 m lattice, 16 x 12 x 10 nodes"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(12), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(12)
    return (g * 0.5).astype(np.float32)[rng.permutation(len(g))]


def _slabs():
    """(c) 40 x 16 x 16 cells, sparse: two slabs 30 cells apart"""
    rng = np.random.default_rng(13)
    a = rng.uniform([0, 0, 0], [4, 15.9, 15.9], size=(700, 3))
    b = rng.uniform([34, 0, 0], [39.9, 15.9, 15.9], size=(900, 3))
    return np.concatenate([a, b, [[0, 0, 0], [39.5, 15.5, 15.5]]]).astype(np.float32)[rng.permutation(1602)]


def _edges():
    """(e) 17 x 9 x 9 cells of 0.45 m from a negative origin: (v - o) * inv_cell rounds, and points one to four ulps BELOW a tile face land in the tile above it -
    outside that tile's f32 box, by less than the grid's eps.  The case tile_box_d2's shrink exists for"""
    rng = np.random.default_rng(15)
    c, o = 0.45, -3.7
    p = rng.uniform([0, 0, 0], [16.9 * c, 8.9 * c, 8.9 * c], size=(1500, 3)) + o
    knife = []
    of, cf = F(o), F(c)
    for a, faces in enumerate(((8, 16), (4, 8), (4, 8))):
        for k in faces:
            for v in _ulps(of + F(k) * cf, ks=(-4, -3, -2, -1, 0, 1)):
                for _ in range(4):
                    q = rng.uniform([0, 0, 0], [16.9 * c, 8.9 * c, 8.9 * c]) + o
                    q[a] = float(v)
                    knife.append(q)
    pts = np.concatenate([p, np.array(knife), [[o, o, o], [o + 16.5 * c, o + 8.5 * c, o + 8.5 * c]]]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


SHIFT = (8000.0, -6000.0, 50.0)


@functools.lru_cache(maxsize=None)
def cloud(name):
    pts = {"seams": lambda: _seams((0.1, 0.2, 0.3)), "lattice": _lattice, "slabs": _slabs, "shifted": lambda: _seams(SHIFT), "edges": _edges}[name]()
    assert len(pts) <= 4000
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def grid(name):
    return chk.Grid(cloud(name), CELLS[name])


@functools.lru_cache(maxsize=None)
def queries(name):
    """inside the grid; on cell, tile and grid faces and one ulp either side; up to 30 cells outside through faces, edges and corners; (slabs) in the gap, more
    than 6 cells from every point"""
    g = grid(name); pts = cloud(name); CELL = CELLS[name]
    rng = np.random.default_rng(21 + CLOUDS.index(name))
    o = g.o.astype(np.float64); ext = g.dims * CELL
    q = [o + rng.uniform(0, 1, size=(500, 3)) * ext]
    q.append(pts[rng.choice(len(pts), 60, replace=False)].astype(np.float64))                       # on a point
    if name in ("seams", "shifted"):
        u, cnt = np.unique(pts, axis=0, return_counts=True)
        q.append(u[cnt > 1][:25].astype(np.float64))                  # on a point that is there twice or three times: the runner-up is at distance 0
    if name == "edges":
        c = g.cells(pts)
        lo = g.o[None, :] + (g.tile_of(c) * np.array([8, 4, 4])).astype(np.float32) * g.cell
        q.append(pts[(pts < lo).any(axis=1)].astype(np.float64))      # on every point the cell arithmetic put above the tile face it lies below
    if name == "lattice":
        half = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) * 0.5
        for off in ((0.25, 0, 0), (0, 0.25, 0), (0.25, 0.25, 0), (0.25, 0, 0.25), (0.25, 0.25, 0.25)):      # half a step off: 2, 4 or 8 equidistant nodes
            q.append(half + np.array(off) + 2.0)
    face = []
    for a in range(3):                                                 # faces, one and two ulps either side
        for f in (0, 1, 4, 8, 16, int(g.dims[a])):
            if f > g.dims[a]:
                continue
            for v in _ulps(F(o[a] + f * CELL)):
                for _ in range(3):
                    p = o + rng.uniform(0, 1, 3) * ext
                    p[a] = float(v)
                    face.append(p)
    q.append(np.array(face))
    out = []
    for sx in (-1, 0, 1):                                              # outside through faces, edges and corners
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                for dist in (0.3, 2.0, 9.0, 30.0):
                    p = o + rng.uniform(0.1, 0.9, 3) * ext
                    for a, s in enumerate((sx, sy, sz)):
                        if s:
                            p[a] = o[a] - dist * CELL if s < 0 else o[a] + ext[a] + dist * CELL
                    out.append(p)
    q.append(np.array(out))
    if name == "slabs":
        q.append(o + rng.uniform([11, 0, 0], [27, 16, 16], size=(150, 3)))
    q = np.concatenate(q).astype(np.float32)
    assert len(q) <= 2000
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def truth(name):
    """brute force, once per cloud: chk.brute_force's (key, i1, D1, D2) for queries(name)"""
    t = chk.brute_force(queries(name), cloud(name))
    for a in t:
        a.setflags(write=False)
    return t


FAR_M = (1, 2, 3, 5, 8, 16)


@functools.lru_cache(maxsize=None)
def far16_waves(name):
    """wave_search_far16: waves of 16 slots with 1, 2, 3, 5, 8 and 16 members at random slots, tight (within a twentieth of a cell of each other) and spread
    (anywhere among the cloud's queries) -> slots (W x 16, 3) f32, radius (W x 16) f32, member (W x 16) bool, and the brute force of the slots"""
    rng = np.random.default_rng(41 + CLOUDS.index(name))
    q = queries(name); c = CELLS[name]
    slots, rad, mem = [], [], []
    for m in FAR_M:
        for tight in (True, False):
            for _ in range(5):
                s = q[rng.choice(len(q), 16)].astype(np.float64)
                if tight:
                    s = s[:1] + rng.uniform(-0.05, 0.05, size=(16, 3)) * c
                on = np.zeros(16, dtype=bool); on[rng.choice(16, m, replace=False)] = True
                slots.append(s); mem.append(on)
                rad.append(rng.choice(np.array([0.3, 1.0, 3.0, 7.0], dtype=np.float32) * F(c), size=16))
    slots = np.concatenate(slots).astype(np.float32); rad = np.concatenate(rad); mem = np.concatenate(mem)
    return slots, rad, mem, chk.brute_force(slots, cloud(name))


def first_radii(name, seed):
    """a first radius per query: a fraction of a cell to a few cells"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.3, 1.0, 1.0, 2.5, 5.0], dtype=np.float32) * F(CELLS[name]), size=len(queries(name)))


# ------------------------------------------------------------------ stream_box
@functools.lru_cache(maxsize=None)
def boxes(name):
    """inclusive cell boxes: single cells, boxes across the tile seams, thin and fat, the whole grid"""
    g = grid(name); rng = np.random.default_rng(31 + CLOUDS.index(name))
    nx, ny, nz = (int(v) for v in g.dims)
    out = [(0, nx - 1, 0, ny - 1, 0, nz - 1), (0, 0, 0, 0, 0, 0), (nx - 1, nx - 1, ny - 1, ny - 1, nz - 1, nz - 1), (7, 8, 3, 4, 3, 4), (0, nx - 1, 3, 3, 4, 4),
           (min(8, nx - 1), min(8, nx - 1), 0, ny - 1, 0, nz - 1), (min(15, nx - 1), nx - 1, 0, min(7, ny - 1), min(3, nz - 1), min(8, nz - 1))]
    for _ in range(40):
        a = [sorted(rng.integers(0, n, 2)) for n in (nx, ny, nz)]
        out.append((int(a[0][0]), int(a[0][1]), int(a[1][0]), int(a[1][1]), int(a[2][0]), int(a[2][1])))
    lim = (nx - 1, nx - 1, ny - 1, ny - 1, nz - 1, nz - 1)           # (the lattice's grid is smaller than the seams the fixed boxes name)
    return tuple(tuple(min(v, m) for v, m in zip(b, lim)) for b in out)


# ------------------------------------------------------------------ Best1 sequences
def best1_waves(seed, L, unequal=True):
    """(waves, L, 64, 3) uint32 (on, d2 bits, idx) and (waves, 64) finish `on`: few distinct d2 (ties everywhere: equal d2 with different indices), d2 = +0, and -
    for the sink without UNIQUE - the same (d2, idx) shown again"""
    rng = np.random.default_rng(seed)
    waves = 24
    vals = np.array([0.0, 0.25, 0.25, 1.0, 1.5, 2.0, 7.0, 1e-30, 3e38], dtype=np.float32)
    rec = np.zeros((waves, L, 64, 3), dtype=np.uint32)
    for w in range(waves):
        d2 = rng.choice(vals, size=(L, 64)) if w % 3 else rng.uniform(0, 4, size=(L, 64)).astype(np.float32)
        idx = rng.integers(0, 12 if w % 2 else 4000, size=(L, 64))
        on = rng.uniform(size=(L, 64)) < (0.8 if w % 4 else 0.3)
        if unequal:
            on &= np.arange(L)[:, None] < rng.integers(0, L + 1, size=64)[None, :]
        rec[w, :, :, 0] = on; rec[w, :, :, 1] = chk.bits(d2); rec[w, :, :, 2] = idx
    fin = (rng.uniform(size=(waves, 64)) < 0.7).astype(np.uint32)
    fin[0] = 1; fin[1] = 0
    return rec, fin


def cluster_waves(name, S):
    """build_clusters / stream_clusters: waves of 64 / S queries (S = 4: each in the lanes l, l + 16, l + 32, l + 48) -> q (W, 64, 3), r (W, 64), todo (W, 64).
    Neighbours with a one-cell radius (few clusters, one table: the REUSE walk reuses it), queries from anywhere (many clusters, more than 64 segments), radii of
    7 cells (boxes of more than 384 segments where the grid is 15 rows high: tile mode), one open lane, one query 64 times"""
    rng = np.random.default_rng(51 + CLOUDS.index(name) + 10 * S)
    qs = queries(name); c = F(CELLS[name]); nq = 64 // S
    Q, R, T = [], [], []
    for kind in ("near", "near", "any", "any", "wide", "wide", "lone", "same"):
        if kind in ("near", "wide"):
            a = qs[rng.integers(len(qs))]
            q = qs[np.argsort(((qs - a) ** 2).sum(axis=1))[:nq]]
        else:
            q = qs[rng.choice(len(qs), nq)]
        if kind == "same":
            q = np.repeat(q[:1], nq, axis=0)
        r = np.full(nq, c * F(7.0 if kind == "wide" else 1.0), dtype=np.float32) if kind != "any" else rng.choice(np.array([0.3, 1.0, 2.5], dtype=np.float32) * c, nq)
        t = rng.uniform(size=nq) < 0.85
        if kind == "lone":
            t[:] = False; t[rng.integers(nq)] = True
        Q.append(np.tile(q, (S, 1))); R.append(np.tile(r, S)); T.append(np.tile(t, S))
    return np.array(Q, dtype=np.float32), np.array(R, dtype=np.float32), np.array(T)


def ball_queries(name):
    """the ball walks: queries with radii of 0.4, 1.2, 2.6 and 4.2 cells - boxes of a few, of up to QN_SEG_CAP = 80 and of more than 80 segments - a quarter of them
    not `on`, between ones that are -> q (n, 3), r (n,), on (n,)"""
    rng = np.random.default_rng(61 + CLOUDS.index(name))
    qs = queries(name)
    q = qs[rng.choice(len(qs), 120)]
    r = rng.choice(np.array([0.4, 1.2, 2.6, 4.2], dtype=np.float32) * F(CELLS[name]), 120)
    return q, r, rng.uniform(size=120) < 0.75


KMAXES = (16, 20, 24, 32)                                           # BestK<KMAX> as the product instantiates it (k_knn_cov<16 | 20 | 24 | 32, LIST, 4>)


def ks_of(kmax):
    return sorted({1, 2, kmax - 1, kmax, 15})                         # 15: the reference's k_correspondences


def bestk_waves(seed, L):
    """(3, L, 64, 3) uint32 (on, d2 bits, idx) and (3, 64) finish `on` (one per query, the same in its four sub-slots).  Every index once per wave (each point
    is shown once); few distinct d2 in wave 0 (ties by index), descending d2 in wave 1 (every key passes the stale filter: the queues fill), random in wave 2;
    lanes stop after 0, 1, 15, 16, 17 or 33 keys, so that one lane's full queue flushes a wave whose other queues hold less"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((3, L, 64, 3), dtype=np.uint32)
    vals = np.array([0.0, 0.25, 0.25, 1.0, 1.5, 2.0, 7.0], dtype=np.float32)
    for w in range(3):
        if w == 0:
            d2 = rng.choice(vals, size=(L, 64))
        elif w == 1:
            d2 = (100.0 - np.arange(L)[:, None] - rng.uniform(0, 0.9, size=(L, 64))).astype(np.float32)
        else:
            d2 = rng.uniform(0, 4, size=(L, 64)).astype(np.float32)
        stop = rng.choice(np.array([0, 1, 15, 16, 17, 33]), size=64)
        stop[rng.integers(0, 64)] = 33
        on = (np.arange(L)[:, None] < stop[None, :]) & (rng.uniform(size=(L, 64)) < 0.95)
        rec[w, :, :, 0] = on; rec[w, :, :, 1] = chk.bits(d2); rec[w, :, :, 2] = rng.permutation(L * 64).reshape(L, 64) if L else 0
    fin = np.tile((rng.uniform(size=(3, 16)) < 0.7).astype(np.uint32), (1, 4))
    fin[0] = 1
    return rec, fin


def bestk_steps(rec_wave):
    """one wave of bestk_waves as chk.bestk_wave_serial takes it: [L][64] of (on, key)"""
    return [[(bool(r[0]), (int(r[1]) << 32) | int(r[2])) for r in row] for row in rec_wave]


@functools.lru_cache(maxsize=None)
def truth_k(name):
    t = chk.brute_force_k(queries(name), cloud(name))
    t.setflags(write=False)
    return t


def make_unique(rec):
    """the same sequences with every (wave, lane-group) index distinct: what the UNIQUE contract promises (a point is shown once per query, whichever sub-slot)"""
    r = rec.copy()
    waves, L = r.shape[:2]
    r[:, :, :, 2] = (np.arange(L)[None, :, None] * 64 + np.arange(64)[None, None, :]) ^ (np.arange(waves)[:, None, None] & 1)
    return r
