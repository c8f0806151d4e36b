"""The k-NN tables a registration actually used (qn_gicp_get_lane_knn / qn_gicp_get_lane_covariances), read back after the registration and compared bit for
bit with the oracle's KD-tree (calculateSource/TargetCovariances, loop_closure.cpp:121,123).  The developer entry qn_gicp_knn runs the classic selection once more
into private buffers; this file reads the tables of the batched lanes (k_lanes<KnnHistK>, several groups of 16 queries per wave with knn_trips, wave-stride list
passes, borrowed sources, the target on the swapped scratch set) and of the classic chain (the pipelined target in the second buffer), at every KMAX / HCAP
boundary, through both scoring paths (knob knn_mm), on the inputs where the matrix-core screen is weakest.  The batched path keeps no distances: indices only;
the f32 distances are compared where a path produces them (qn_gicp_knn).  Oracle tables are cached per cloud and k: the CPU KD-tree is the slow side."""
import hashlib
import numpy as np
import pytest
from qn_amd import synth

pytestmark = pytest.mark.gpu

KS = (1, 5, 15, 16, 17, 20, 24, 25, 27, 32)          # every KMAX (16 / 20 / 24 / 32) and HCAP (32 / 48) boundary, both BestK tails, k = 1
_KNN, _COV = {}, {}


def _key(cloud, k):
    return hashlib.sha1(np.ascontiguousarray(cloud, dtype=np.float32).tobytes()).hexdigest(), k      # (by content: a name could be reused)


def ref_knn(oracle, name, cloud, k):
    if _key(cloud, k) not in _KNN:
        o = oracle.GicpOracle(); o.set_source(cloud)
        _KNN[_key(cloud, k)] = o.knn(0, cloud, k)
    return _KNN[_key(cloud, k)]


def ref_cov(oracle, name, cloud, k):
    """the oracle's covariances and the rows where the plane normal is unique (as test_small_k: the raw scatter's two smallest eigenvalues differ by 1e-6 of the
    largest) and every neighbour exists"""
    if _key(cloud, k) not in _COV:
        o = oracle.GicpOracle(k=k); o.set_source(cloud); o.compute_covariances(0)
        idx, _ = ref_knn(oracle, name, cloud, k)
        nb = cloud[np.maximum(idx, 0)].astype(np.float64); nb -= nb.mean(1, keepdims=True)
        ws = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", nb, nb) / k)
        unique = ((ws[:, 1] - ws[:, 0]) > 1e-6 * np.maximum(ws[:, 2], 1e-300)) & (idx >= 0).all(1)
        _COV[_key(cloud, k)] = (o.covariances(0), unique)
    return _COV[_key(cloud, k)]


def check_table(engine, ctx, lane, which, oracle, name, cloud, k, cov=False):
    idx = engine.lane_knn(ctx, lane, which)
    oi, _ = ref_knn(oracle, name, cloud, k)
    assert idx.shape == oi.shape, (name, lane, which, k, idx.shape, oi.shape)
    bad = np.nonzero((idx != oi).any(1))[0]
    assert bad.size == 0, ("table differs from the oracle's", name, "lane", lane, "which", which, "k", k, "rows", bad.size, bad[:4].tolist(),
                           idx[bad[0]].tolist(), oi[bad[0]].tolist())
    if cov:
        Co, unique = ref_cov(oracle, name, cloud, k)
        Cg = engine.lane_covariances(ctx, lane, which, len(cloud))
        diff = np.abs(Cg - Co).reshape(len(cloud), -1).max(1)
        assert (diff[unique] < 1e-9).all(), ("covariances", name, lane, which, k, int((diff[unique] >= 1e-9).sum()))


def not_ready(engine, ctx, lane, which):
    with pytest.raises(engine.EngineError) as ei:
        engine.lane_knn(ctx, lane, which)
    return ei.value.status == engine.QN_ERR_NOT_READY


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ clouds
def _ulps(a, rng, u=2):
    """every coordinate moved by up to u ulps (0 stays 0: its bit pattern minus 1 would be a NaN)"""
    a = f32(a)
    return np.where(a == 0, a, (a.view(np.int32) + rng.integers(-u, u + 1, a.shape).astype(np.int32)).view(np.float32))


def _lattice(seed, off=(31.0, -17.125, 2.0)):
    """the ulp-perturbed lattice of test_gpu_knn_mm.py: squared distances that differ in their last bits or not at all, many of them on a histogram bin edge (a
    power of two times 1 + j/8).  (No coordinate is 0: its bit pattern minus 2 would be a NaN.)"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(70, dtype=np.float64) * 0.25, np.arange(70, dtype=np.float64) * 0.25)
    lat = np.stack([gx.ravel() + off[0], gy.ravel() + off[1], np.full(4900, off[2])], 1)
    return _ulps(lat, rng)


def _micro_clumps(seed):
    """millimetre clumps as ulp-perturbed micro-lattices (4 x 4 x 3 points, 2^-10 m apart, centres on a 2^-4 m grid) in a 60 m scene: k nearest within
    millimetres, their squared distances small integers times 2^-20 - on bin edges and tied - while the wave's candidate box spans metres"""
    rng = np.random.default_rng(seed)
    base, _, _ = synth.make_pair(58 + seed, 6000, extent=60.0)
    centres = np.round(base[rng.choice(len(base), 60, replace=False)].astype(np.float64) * 16.0) / 16.0
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 2.0 ** -10
    clumps = (centres[:, None, :] + g[None]).reshape(-1, 3)
    return f32(np.concatenate([base, _ulps(clumps, rng, 1)]))


def _clumps(seed):
    """millimetre clumps of 40 points in a 60 m scene (the screening margin exceeds tau itself)"""
    rng = np.random.default_rng(seed)
    base, _, _ = synth.make_pair(48 + seed, 6000, extent=60.0)
    centres = base[rng.choice(len(base), 60, replace=False)]
    clumps = (centres[:, None, :] + rng.normal(0, 1e-3, (60, 40, 3))).reshape(-1, 3)
    return f32(np.concatenate([base, clumps]))


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(2024)
    C = {}
    C["street9k_s"], C["street9k_t"], _ = synth.make_pair(61, 9000, 7500, extent=50.0)
    C["street20k_s"], C["street20k_t"], _ = synth.make_pair(62, 20000, 14000, extent=70.0)
    C["street3k_s"], C["street3k_t"], _ = synth.make_pair(63, 3000, 4100, extent=30.0)
    C["sparse_s"], C["sparse_t"], _ = synth.make_pair(64, 12000, 11000, extent=120.0)
    C["tiny_s"] = f32(C["street3k_s"][:12] + 0.0)                                               # fewer points than every k >= 15: -1 columns
    iso, _, _ = synth.make_pair(65, 6000, extent=60.0)                                          # isolated points scattered through the volume
    C["isolated_s"] = f32(np.concatenate([iso, rng.uniform([-100, -100, -8], [100, 100, 30], (40, 3))])[rng.permutation(6040)])
    base, _, _ = synth.make_pair(66, 4000, extent=40.0)                                          # exact duplicates: ties go to the lowest index
    rep = np.repeat(np.arange(4000), rng.integers(1, 4, 4000) * (rng.random(4000) < 0.4) + 1)
    C["dups_s"] = f32(base[rep][rng.permutation(len(rep))])
    scene = synth.Scene(np.random.default_rng(5), 120.0)
    prims = scene.primitives(); sen = synth.SpinningLidar(n_beams=16, n_cols=1024)             # raw spinning-LiDAR scans: rings of nearly collinear points
    C["lidar_s"] = f32(synth.lidar_scan(prims, sen, synth.sensor_pose(3.0, -2.0, 0.4), 7)[:, :3])
    C["lidar_t"] = f32(synth.lidar_scan(prims, sen, synth.sensor_pose(5.5, -1.0, 0.5), 8)[:, :3])
    C["lattice_lane_t"] = _lattice(15, (-8.0, -9.125, 1.5))                                          # shells of tied distances on histogram bin edges, at every k
    for n, c in C.items():
        C[n] = f32(c)
        assert np.isfinite(C[n]).all(), n
    return C


# the eight lanes: distinct source buffers (a shared source buffer would be borrowed, tested below)
LANES = [("street9k_s", "street9k_t"), ("tiny_s", "street3k_t"), ("isolated_s", "street9k_t"), ("dups_s", "street3k_t"),
         ("lidar_s", "lidar_t"), ("street20k_s", "street20k_t"), ("street3k_s", "lattice_lane_t"), ("sparse_s", "street20k_t")]
MAXP = 24000


def configure(engine, ctx, k, iters=3):
    g = engine.NanoGICP(ctx)
    g.setCorrespondenceRandomness(k); g.setMaximumIterations(iters); g.setMaxCorrespondenceDistance(52.5); g.setTransformationEpsilon(0.01); g.bind()
    return g


def run_batch(engine, ctx, pairs, k, iters=3):
    configure(engine, ctx, k, iters)
    return engine.gicp_align_batch(ctx, [(s, len(s), t, len(t), 12, 0) for s, t in pairs])


def last_run_lanes(n_pairs, B):
    """lane l -> the pair it carried last: the lanes of the final run hold its pairs, the lanes beyond it the pairs of the run before"""
    out = {}
    for base in range(0, n_pairs, B):
        for l in range(min(B, n_pairs - base)):
            out[l] = base + l
    return out


# ------------------------------------------------------------------------------------------------ batched lanes, every table
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("trips", [1, 2, 3, 4])
def test_batched_lane_tables(oracle, clouds, B, trips):
    """every lane's source and target table after gicp_align_batch, k at every KMAX / HCAP boundary, knn_trips groups of 16 per wave.  B = 3 carries the eight pairs in
    three runs: lanes 0, 1 hold the pairs of the last run, lane 2 still the one of the run before."""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("batch_lanes", B); ctx.debug_set("knn_trips", trips)
    pairs = [(clouds[s], clouds[t]) for s, t in LANES]
    for k in KS:                                  # (consecutive runs differ in k: a row a pass failed to write is never the right row of the run before)
        run_batch(engine, ctx, pairs, k)
        for l, p in last_run_lanes(len(pairs), B).items():
            s, t = LANES[p]
            check_table(engine, ctx, l, 0, oracle, s, clouds[s], k, cov=trips == 3)
            check_table(engine, ctx, l, 1, oracle, t, clouds[t], k, cov=trips == 3)
    ctx.close()


@pytest.mark.parametrize("cell", [0.25, 3.0])
def test_batched_lane_tables_cell_edges(oracle, clouds, cell):
    """the `cell` knob (whole context): 0.25 m cells make queries retry with several clusters per wave, 3 m cells put thousands of candidates into a round"""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("batch_lanes", 8); ctx.debug_set("cell", cell)
    pairs = [(clouds[s], clouds[t]) for s, t in LANES]
    for k in (20, 27):
        run_batch(engine, ctx, pairs, k)
        for l, (s, t) in enumerate(LANES):
            check_table(engine, ctx, l, 0, oracle, s, clouds[s], k)
            check_table(engine, ctx, l, 1, oracle, t, clouds[t], k)
    ctx.close()


# ------------------------------------------------------------------------------------------------ the matrix-core screen's hard inputs, k > 24, both scoring paths
@pytest.fixture(scope="module")
def hard():
    src, tgt, _ = synth.make_pair(47, 20000, 16000, extent=60.0)
    H = {}
    for name, off in (("far8k", (8000.0, -3000.0, 150.0)), ("far65k", (-65000.0, 40000.0, 0.0))):      # f32 coordinates with 1 mm / 4 mm resolution
        H[name + "_s"] = f32(src.astype(np.float64) + np.array(off))
        H[name + "_t"] = f32(tgt.astype(np.float64) + np.array(off))
    H["clumps_s"], H["clumps_t"] = _clumps(0), _clumps(1)
    H["lattice_s"], H["lattice_t"] = _lattice(11), _lattice(12)
    H["farlat_s"], H["farlat_t"] = _lattice(13, (8000.0, -3000.0, 150.0)), _lattice(14, (8000.0, -3000.0, 150.0))      # the lattice 8 km out: 1 mm ulps
    H["microclumps_s"], H["microclumps_t"] = _micro_clumps(0), _micro_clumps(1)
    for n, c in H.items():
        assert np.isfinite(c).all(), n
    return H


HARD = [("far8k_s", "far8k_t"), ("far65k_s", "far65k_t"), ("clumps_s", "clumps_t"), ("lattice_s", "lattice_t"), ("farlat_s", "farlat_t"),
        ("microclumps_s", "microclumps_t")]


def _failures(checks):
    """runs every check, returns the labels of those that failed (each hard case is reported, not just the first)"""
    bad = []
    for label, fn in checks:
        try:
            fn()
        except AssertionError:
            bad.append(label)
    return bad


@pytest.mark.parametrize("mm", [1, 0])
def test_hard_inputs_classic(oracle, hard, mm):
    """classic path: the table calculateSourceCovariances used (lane 0 of a context without lanes) and the developer read-back's indices and f32 distances"""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("knn_mm", mm)
    bad = []
    for k in (20, 27):
        g = configure(engine, ctx, k)
        for name in [n for pair in HARD for n in pair]:
            g.setInputSource(hard[name]); assert g.calculateSourceCovariances()
            oi, od = ref_knn(oracle, name, hard[name], k)
            bad += _failures([(("table", name, k), lambda: check_table(engine, ctx, 0, 0, oracle, name, hard[name], k))])
            idx, d2 = g.knn(0, k)
            if not (np.array_equal(idx, oi) and np.array_equal(d2, od)):
                bad.append(("knn", name, k))
    ctx.close()
    assert not bad, bad


@pytest.mark.parametrize("mm", [1, 0])
def test_hard_inputs_batched(oracle, hard, mm):
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("batch_lanes", len(HARD)); ctx.debug_set("knn_mm", mm)
    bad = []
    for k in (20, 27):
        run_batch(engine, ctx, [(hard[s], hard[t]) for s, t in HARD], k, iters=2)
        for l, (s, t) in enumerate(HARD):
            bad += _failures([((name, k), lambda l=l, w=w, name=name: check_table(engine, ctx, l, w, oracle, name, hard[name], k)) for w, name in ((0, s), (1, t))])
    ctx.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ shared sources
def test_shared_source_lanes(oracle, clouds):
    """the candidates of one query (batch_share_source): the lending lane's source table is the oracle's, the borrowing lanes report NOT_READY for the source (their
    own buffers were never written) and carry correct target tables"""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("batch_lanes", 4)
    S = clouds["street20k_s"]
    names = [("street20k_s", "street20k_t"), ("street20k_s", "street9k_t"), ("street20k_s", "lidar_t"), ("dups_s", "sparse_t")]
    for k in (20, 27):
        run_batch(engine, ctx, [(S if s == "street20k_s" else clouds[s], clouds[t]) for s, t in names], k)
        check_table(engine, ctx, 0, 0, oracle, "street20k_s", S, k, cov=True)
        for l in (1, 2):
            assert not_ready(engine, ctx, l, 0), l
            with pytest.raises(engine.EngineError):
                engine.lane_covariances(ctx, l, 0, len(S))
        check_table(engine, ctx, 3, 0, oracle, "dups_s", clouds["dups_s"], k)
        for l, (_, t) in enumerate(names):
            check_table(engine, ctx, l, 1, oracle, t, clouds[t], k, cov=True)
    ctx.close()


# ------------------------------------------------------------------------------------------------ classic chain
@pytest.mark.parametrize("pipeline", [1, 0])
def test_classic_chain(oracle, clouds, pipeline):
    """setInputSource -> calculateSourceCovariances -> setInputTarget -> calculateTargetCovariances -> align (loop_closure.cpp:120-124): the target's table is the
    oracle's; the source's survives only where the target went to the second buffer (pair pipeline), otherwise it reads NOT_READY"""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("pair_pipeline", pipeline)
    src, tgt = clouds["street20k_s"], clouds["street20k_t"]
    for k in (20, 27):
        g = configure(engine, ctx, k)
        g.setInputSource(src); assert g.calculateSourceCovariances()
        g.setInputTarget(tgt); assert g.calculateTargetCovariances()
        g.align()
        check_table(engine, ctx, 0, 1, oracle, "street20k_t", tgt, k, cov=True)
        if pipeline:
            check_table(engine, ctx, 0, 0, oracle, "street20k_s", src, k, cov=True)
        else:
            assert not_ready(engine, ctx, 0, 0)
    with pytest.raises(engine.EngineError) as ei:
        engine.lane_knn(ctx, 1, 0)                                 # a context without lanes has lane 0 only
    assert ei.value.status == engine.QN_ERR_NOT_READY
    ctx.close()


# ------------------------------------------------------------------------------------------------ read-back discipline
def test_no_stale_table_classic(oracle, clouds):
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    src, tgt, new = clouds["street9k_s"], clouds["street9k_t"], clouds["lidar_s"]
    g = configure(engine, ctx, 20)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances(); g.align()
    check_table(engine, ctx, 0, 0, oracle, "street9k_s", src, 20)
    g.setInputSource(new)                                          # a new cloud: its table does not exist yet
    assert not_ready(engine, ctx, 0, 0)
    check_table(engine, ctx, 0, 1, oracle, "street9k_t", tgt, 20)
    g.calculateSourceCovariances()
    check_table(engine, ctx, 0, 0, oracle, "lidar_s", new, 20)
    g.setCorrespondenceRandomness(27)                              # a k change: both tables are of the old k
    assert not_ready(engine, ctx, 0, 0) and not_ready(engine, ctx, 0, 1)
    g.calculateSourceCovariances(); g.calculateTargetCovariances()
    check_table(engine, ctx, 0, 0, oracle, "lidar_s", new, 27)
    check_table(engine, ctx, 0, 1, oracle, "street9k_t", tgt, 27)
    g.knn(0, 7)                                                    # the developer read-back at another k re-forms the covariances from its private table
    assert not_ready(engine, ctx, 0, 0)
    check_table(engine, ctx, 0, 1, oracle, "street9k_t", tgt, 27)
    ctx.close()


def test_no_stale_table_batched(oracle, clouds):
    """several runs of one batch call reuse the lanes; a k change on the owner; a lane whose source the next call borrows"""
    from qn_amd import engine
    ctx = engine.Context(MAXP)
    ctx.debug_set("batch_lanes", 3)
    c = clouds
    # six distinct pairs: two runs, every lane ends with the second run's pair
    names = LANES[:6]
    run_batch(engine, ctx, [(c[s], c[t]) for s, t in names], 20)
    for l in range(3):
        s, t = names[3 + l]
        check_table(engine, ctx, l, 0, oracle, s, c[s], 20); check_table(engine, ctx, l, 1, oracle, t, c[t], 20)
    configure(engine, ctx, 25)
    for l in range(3):
        assert not_ready(engine, ctx, l, 0) and not_ready(engine, ctx, l, 1), l
    # run 2: lane 0 keeps its source buffer of run 1 (not rebuilt), lane 1 borrows lane 0's, lane 2 has a source of its own
    A, D = c["street9k_s"], c["dups_s"]
    names = [("street9k_s", "street3k_t"), ("lidar_s", "lidar_t"), ("isolated_s", "street9k_t"),
             ("street9k_s", "sparse_t"), ("street9k_s", "street20k_t"), ("dups_s", "street3k_t")]
    run_batch(engine, ctx, [(A if s == "street9k_s" else D if s == "dups_s" else c[s], c[t]) for s, t in names], 25)
    check_table(engine, ctx, 0, 0, oracle, "street9k_s", A, 25)
    assert not_ready(engine, ctx, 1, 0)                            # (its own buffer still holds lidar_s's table from run 1: never handed out)
    check_table(engine, ctx, 2, 0, oracle, "dups_s", D, 25)
    for l in range(3):
        t = names[3 + l][1]
        check_table(engine, ctx, l, 1, oracle, t, c[t], 25)
    ctx.close()


# ------------------------------------------------------------------------------------------------ full size: matrix cores against VALU scoring, through 8 lanes
def test_full_size_lanes_match_valu_scoring():
    """eight 40k-100k-point lanes at k = 20 and 27: the tables of knn_mm 1 and knn_mm 0 (every histogram pass on the VALU) are the same, and 64 rows of each lane's
    source are the brute-force ones"""
    from qn_amd import engine
    pairs = []
    for i, n in enumerate((100000, 80000, 60000, 40000)):
        s, t, _ = synth.make_pair(70 + i, n, n - 7000 * i)
        pairs += [(s, t), (t.copy(), s.copy())]
    ctx = engine.Context(100000)
    ctx.debug_set("batch_lanes", 8)
    rng = np.random.default_rng(0)
    for k in (20, 27):
        out = []
        for mm in (1, 0):
            ctx.debug_set("knn_mm", mm)
            run_batch(engine, ctx, pairs, k, iters=2)
            out.append([(engine.lane_knn(ctx, l, 0), engine.lane_knn(ctx, l, 1)) for l in range(8)])
        for l in range(8):
            for w in (0, 1):
                assert np.array_equal(out[0][l][w], out[1][l][w]), (k, l, w)
            src = pairs[l][0]
            for i in rng.choice(len(src), 8, replace=False):
                d = (src - src[i]) ** 2
                order = np.lexsort((np.arange(len(src)), (d[:, 0] + d[:, 1]) + d[:, 2]))[:k]
                assert np.array_equal(out[0][l][0][i], order.astype(np.int32)), (k, l, i)
    ctx.close()


# ------------------------------------------------------------------------------------------------ capacity
def test_capacity_beyond_the_26_bit_screen_field_is_refused():
    """max_points > 2^26 would overflow the screen's 26-bit position field: QN_ERR_CAPACITY, and nothing is allocated (a context at 2^26 itself would take tens of GB)"""
    import torch
    from qn_amd import engine
    free0, _ = torch.cuda.mem_get_info(0)
    with pytest.raises(engine.EngineError) as ei:
        engine.Context((1 << 26) + 1)
    assert ei.value.status == engine.QN_ERR_CAPACITY
    free1, _ = torch.cuda.mem_get_info(0)
    assert free0 - free1 < (256 << 20), (free0, free1)
