"""ctypes binding of include/qn_engine.h.  Mirrors the reference's operator surface:
`NanoGICP` has the member functions LoopClosure calls on nano_gicp::NanoGICP
(fast_lio_sam_qn/src/loop_closure.cpp:9-16, 120-133), argument meaning and failure
behaviour included (no exceptions for a failed registration: hasConverged() == False)."""
import ctypes as C
import math
import os
import numpy as np
from . import build as _build

QN_OK, QN_ERR_INVALID_ARG, QN_ERR_EMPTY_CLOUD, QN_ERR_CAPACITY, QN_ERR_NOT_READY, QN_ERR_HIP, QN_ERR_NO_DEVICE, QN_ERR_INTERNAL = range(8)
QN_SOURCE, QN_TARGET = 0, 1
QN_VERIFY_SRC, QN_VERIFY_DST, QN_VERIFY_COARSE, QN_VERIFY_FINAL = 0, 1, 2, 3
FLOAT_MAX = 3.4028234663852886e38
KERNEL_FAMILIES = ["grid_build", "knn_cov", "nn_search", "nn_fallback", "accumulate", "solve", "fitness", "transform",
                   "fpfh_normals", "fpfh_spfh", "fpfh_fpfh", "feat_match", "gn_tick_fused", "knn_select", "match_tail", "far_refresh", "align_persist"]


class GicpParams(C.Structure):
    _fields_ = [("k_correspondences", C.c_int32), ("max_iterations", C.c_int32), ("max_corr_dist", C.c_double),
                ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double), ("optimizer", C.c_int32),
                ("lm_max_iterations", C.c_int32), ("lm_init_lambda_factor", C.c_double), ("force_iterations", C.c_int32),
                ("ransac_iterations", C.c_int32), ("ransac_outlier_threshold", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double)]


class GicpResult(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("T64", C.c_double * 16), ("H", C.c_double * 36), ("fitness", C.c_double),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("lm_failed", C.c_int32), ("reserved", C.c_int32)]


class IterTrace(C.Structure):
    _fields_ = [("y0", C.c_double), ("lambda_", C.c_double), ("rho", C.c_double), ("max_dR", C.c_double),
                ("max_dt", C.c_double), ("inner", C.c_int32), ("accepted", C.c_int32)]


class KernelStat(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("launches", C.c_int64)]


class EngineError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("qn_engine status %d (%s)" % (status, msg))
        self.status = status


_lib = None
DEBUG_KNOBS_FROM_ENV = False     # harness opt-in for the QN_DEBUG_KNOBS environment variable (Context.__init__)


def lib():
    """Loads the in-tree libqn_engine.so.  Fails loudly when it is missing or unloadable."""
    global _lib
    if _lib is None:
        path = _build.LIB
        if not os.path.exists(path):
            raise ImportError("libqn_engine.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        _lib = C.CDLL(path)
        _lib.qn_status_str.restype = C.c_char_p
        _lib.qn_last_error.restype = C.c_char_p
        _lib.qn_last_error.argtypes = [C.c_void_p]
        _lib.qn_ctx_stream.restype = C.c_void_p
        _lib.qn_ctx_stream.argtypes = [C.c_void_p]
        _lib.qn_ctx_destroy.argtypes = [C.c_void_p]
        _lib.hipMemcpy.restype = C.c_int                 # the HIP runtime's, through the library that links it: the device read-backs of KeyframeStore
        _lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    def __init__(self, max_points, device=0):
        self._l = lib()
        h = C.c_void_p()
        st = self._l.qn_ctx_create(C.c_int(device), C.c_uint32(max_points), C.byref(h))
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode())
        self.h = h
        self.max_points = max_points
        # developer tuning (qn_debug_set) for every context of the process - a whole test file or bench run under a knob.  Opt-in only:
        # a harness sets engine.DEBUG_KNOBS_FROM_ENV = True (tests/conftest.py, bench.py, tools/); a production host never reads the variable.
        knobs = os.environ.get("QN_DEBUG_KNOBS") if DEBUG_KNOBS_FROM_ENV else None
        if knobs:
            import json, sys
            try:
                for k, v in json.loads(knobs).items():
                    self.debug_set(k, float(v))
            except Exception:
                self.close()
                raise
            print("qn_amd: QN_DEBUG_KNOBS applied to a context: %s" % knobs, file=sys.stderr)

    def close(self):
        if getattr(self, "h", None):
            self._l.qn_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode() + ": " + self._l.qn_last_error(self.h).decode())

    @property
    def stream(self):
        return self._l.qn_ctx_stream(self.h)

    def synchronize(self):
        self.check(self._l.qn_ctx_synchronize(self.h))

    def debug_set(self, key, value):
        self.check(self._l.qn_debug_set(self.h, key.encode(), C.c_double(value)))

    def debug_get(self, key):
        v = C.c_double()
        self.check(self._l.qn_debug_get(self.h, key.encode(), C.byref(v)))
        return v.value

    def debug_eig3(self, which, a6):
        """qn_debug_eig3: the device build of a 3 x 3 symmetric eigen solver (0: qn_eig3_jacobi, 1: sym_eig3) on the rows (xx, xy, xz, yy, yz, zz) of a6
        -> w (n, 3), V (n, 3, 3) with the eigenvector of w[:, k] in V[:, :, k].  Test infrastructure."""
        a = np.ascontiguousarray(a6, dtype=np.float64).reshape(-1, 6)
        n = len(a)
        if n == 0:
            a = np.zeros((1, 6))                                      # (an empty array may have no address; the call refuses null pointers)
        w = np.zeros((max(n, 1), 3)); V = np.zeros((max(n, 1), 3, 3))
        self._l.qn_debug_eig3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self.check(self._l.qn_debug_eig3(self.h, C.c_int(which), _p(a), C.c_uint32(n), _p(w), _p(V)))
        return w[:n], V[:n]

    STEP_MATH_STRIDES = ((43, 7), (43, 6), (59, 39), (3, 9), (9, 9), (18, 3))          # (in, out) f64 per record of qn_debug_step_math, by `which`

    def debug_step_math(self, which, records):
        """qn_debug_step_math: the device build of one of the Gauss-Newton step's small dense routines (0 d_ldlt_solve6_fast, 1 d_ldlt_solve6, 2 d_propose,
        3 d_so3_exp, 4 m3_inverse, 5 d_is_converged) on the rows of `records` (n, stride_in) -> (n, stride_out) f64; the record layouts are at the declaration
        in include/qn_engine.h.  Test infrastructure."""
        if not 0 <= which < len(self.STEP_MATH_STRIDES):
            raise ValueError("debug_step_math: which = %r" % (which,))
        si, so = self.STEP_MATH_STRIDES[which]
        a = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, si)
        n = len(a)
        if n == 0:
            a = np.zeros((1, si))                                     # (an empty array may have no address; the call refuses null pointers)
        out = np.zeros((max(n, 1), so))
        self._l.qn_debug_step_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        self.check(self._l.qn_debug_step_math(self.h, C.c_int(which), _p(a), C.c_uint32(n), _p(out)))
        return out[:n]

    LIN_POINT, LIN_EMIT, LIN_ROWS = 0, 1, 2                          # qn_debug_linearize's `which`
    LIN_POINT_STRIDE, LIN_HEAD, LIN_LANE, LIN_BLOCK, LIN_NPART = 37, 25, 13, 256, 28

    def debug_linearize(self, which, data, arg=0):
        """qn_debug_linearize (the record layouts: include/qn_engine.h).  LIN_POINT: accumulate_point_n on the rows of data (n, 37) -> (n, 28).  LIN_EMIT:
        emit_point on blocks of 256 lanes, data (blocks, 25 + arg x 256 x 13), arg = trips -> (blocks, 5, 28): the four wave rows, then the block's row.
        LIN_ROWS: reduce_rows<NT, COHERENT> with arg = NT + COHERENT on data (rows, 28) -> (28,).  Test infrastructure."""
        if which == self.LIN_POINT:
            si, shape = self.LIN_POINT_STRIDE, lambda n: (n, self.LIN_NPART)
        elif which == self.LIN_EMIT:
            if arg not in (1, 2, 3, 4):
                raise ValueError("debug_linearize: %r trips" % (arg,))
            si, shape = self.LIN_HEAD + arg * self.LIN_BLOCK * self.LIN_LANE, lambda n: (n, 5, self.LIN_NPART)
        elif which == self.LIN_ROWS:
            si, shape = self.LIN_NPART, lambda n: (min(n, 1) * self.LIN_NPART,)
        else:
            raise ValueError("debug_linearize: which = %r" % (which,))
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, si)
        n = len(a)
        if n == 0:
            a = np.zeros((1, si))                                     # (an empty array may have no address; the call refuses null pointers)
        out = np.zeros(max(int(np.prod(shape(n))), 1))
        self._l.qn_debug_linearize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        self.check(self._l.qn_debug_linearize(self.h, C.c_int(which), _p(a), C.c_uint32(n), C.c_uint32(arg), _p(out)))
        return out[:int(np.prod(shape(n)))].reshape(shape(n))

    DS_DUMP, DS_BEST1, DS_BOUNDS, DS_DIVMOD, DS_STREAM_BOX, DS_WAVE_SEARCH1, DS_WAVE_SEARCH_SINGLE, DS_WAVE_SEARCH_FAR16, DS_BESTK, DS_WAVE_SEARCH_K, DS_LANE_BALL_KNN, DS_STREAM_CLUSTERS, DS_BALL_CELLS = range(13)      # qn_debug_search's `which`

    def debug_search(self, which, grid, words, n, arg, n_out):
        """qn_debug_search (the record layouts: include/qn_engine.h): `words` = the packed uint32 input (floats as their bits), n and arg as the header says,
        n_out = the uint32 words the call writes -> that many uint32.  Test infrastructure."""
        a = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        if a.size == 0:
            a = np.zeros(1, dtype=np.uint32)                          # (an empty array may have no address; the call refuses null pointers)
        out = np.zeros(max(int(n_out), 1), dtype=np.uint32)
        self._l.qn_debug_search.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        self.check(self._l.qn_debug_search(self.h, C.c_int(which), C.c_int(grid), _p(a), C.c_uint32(n), C.c_uint32(arg), _p(out)))
        return out[:int(n_out)]

    def grid_info(self, which):
        out = np.zeros(8)
        self.check(self._l.qn_debug_get_grid(self.h, C.c_int(which), _p(out)))
        return dict(origin=out[:3], cell=out[3], dims=out[4:7].astype(int), eps=out[7])

    # profiling hooks
    def prof_enable(self, on=True):
        self.check(self._l.qn_prof_enable(self.h, C.c_int(1 if on else 0)))

    def prof_reset(self):
        self.check(self._l.qn_prof_reset(self.h))

    def prof_stats(self):
        out = {}
        for i, name in enumerate(KERNEL_FAMILIES):
            ks = KernelStat()
            self.check(self._l.qn_prof_get(self.h, C.c_int(i), C.byref(ks)))
            out[name] = (ks.total_ms, ks.launches)
        return out


def _cloud_arg(xyz):
    """(pointer-holder, n, stride_bytes) for an (n,3) or (n,4)/(n,8) float32 array."""
    a = np.ascontiguousarray(xyz, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be (n, >=3) float32")
    return a, a.shape[0], a.shape[1] * 4


class NanoGICP:
    """nano_gicp::NanoGICP<PointType, PointType> as LoopClosure uses it."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._l = ctx._l
        self.p = GicpParams()
        self._l.qn_gicp_default_params(C.byref(self.p))
        self._res = None
        self._n = [0, 0]
        self._push()

    def _push(self):
        self.ctx.check(self._l.qn_gicp_set_params(self.ctx.h, C.byref(self.p)))

    def bind(self):
        """Make this object's parameters the context's again (several NanoGICP objects may share one context; the context holds ONE set)."""
        self._push()

    # --- the 8 setters of loop_closure.cpp:9-16
    def setNumThreads(self, n):                      # CPU thread count: meaningless on the GPU, accepted
        self.num_threads = n

    def setCorrespondenceRandomness(self, k):
        self.p.k_correspondences = k; self._push()

    def setMaximumIterations(self, n):
        self.p.max_iterations = n; self._push()

    def setRANSACIterations(self, n):
        self.p.ransac_iterations = n; self._push()

    def setMaxCorrespondenceDistance(self, d):
        self.p.max_corr_dist = d; self._push()

    def setTransformationEpsilon(self, e):
        self.p.transformation_epsilon = e; self._push()

    def setEuclideanFitnessEpsilon(self, e):
        self.p.euclidean_fitness_epsilon = e; self._push()

    def setRANSACOutlierRejectionThreshold(self, t):
        self.p.ransac_outlier_threshold = t; self._push()

    # extras the reference leaves at defaults
    def setRotationEpsilon(self, e):
        self.p.rotation_epsilon = e; self._push()

    def setLMMaxIterations(self, n):                 # LM trial steps per outer iteration before "lm not converged!!" (>= 1; default 10)
        self.p.lm_max_iterations = n; self._push()

    def setLMInitLambdaFactor(self, f):              # lambda = f * max |diag H| at the first linearisation (default 1e-9)
        self.p.lm_init_lambda_factor = f; self._push()

    def setOptimizer(self, name):
        self.p.optimizer = 0 if name == "lm" else 1; self._push()

    def setForceIterations(self, n):
        self.p.force_iterations = n; self._push()

    # --- clouds
    def setInputSource(self, xyz):
        a, n, stride = _cloud_arg(xyz); self._n[0] = n
        st = self._l.qn_gicp_set_source(self.ctx.h, _p(a), C.c_uint32(n), C.c_uint32(stride))
        if st != QN_ERR_EMPTY_CLOUD:
            self.ctx.check(st)

    def setInputTarget(self, xyz):
        a, n, stride = _cloud_arg(xyz); self._n[1] = n
        st = self._l.qn_gicp_set_target(self.ctx.h, _p(a), C.c_uint32(n), C.c_uint32(stride))
        if st != QN_ERR_EMPTY_CLOUD:
            self.ctx.check(st)

    def setInputSourceDevice(self, ptr, n, stride):
        self._n[0] = n
        self.ctx.check(self._l.qn_gicp_set_source_device(self.ctx.h, C.c_void_p(ptr), C.c_uint32(n), C.c_uint32(stride)))

    def setInputTargetDevice(self, ptr, n, stride):
        self._n[1] = n
        self.ctx.check(self._l.qn_gicp_set_target_device(self.ctx.h, C.c_void_p(ptr), C.c_uint32(n), C.c_uint32(stride)))

    def calculateSourceCovariances(self):
        return self._l.qn_gicp_compute_covariances(self.ctx.h, C.c_int(QN_SOURCE)) == QN_OK

    def calculateTargetCovariances(self):
        return self._l.qn_gicp_compute_covariances(self.ctx.h, C.c_int(QN_TARGET)) == QN_OK

    def align(self, guess=None):
        """Returns the transformed source cloud like align(output) fills `output`; on an unusable
        input (empty cloud) the engine, like the reference, reports hasConverged() == False."""
        res = GicpResult()
        g = None if guess is None else np.ascontiguousarray(guess, dtype=np.float32)
        st = self._l.qn_gicp_align(self.ctx.h, None if g is None else _p(g), C.byref(res))
        if st in (QN_ERR_EMPTY_CLOUD, QN_ERR_NOT_READY):
            self._res = None
            return None
        self.ctx.check(st)
        self._res = res
        return res

    def alignedCloud(self):
        out = np.zeros((self._n[0], 4), dtype=np.float32)
        self.ctx.check(self._l.qn_gicp_transformed_source(self.ctx.h, _p(out), C.c_uint32(16)))
        return out[:, :3]

    def getFitnessScore(self, max_range=1.7976931348623157e308):
        if self._res is None:
            return 1.7976931348623157e308
        if max_range >= 1.7976931348623157e308:
            return self._res.fitness
        s = C.c_double()
        self.ctx.check(self._l.qn_gicp_fitness(self.ctx.h, C.c_double(max_range), C.byref(s)))
        return s.value

    def hasConverged(self):
        return bool(self._res.converged) if self._res is not None else False

    def getFinalTransformation(self):
        return np.array(self._res.T, dtype=np.float32).reshape(4, 4) if self._res is not None else np.eye(4, dtype=np.float32)

    # --- parity read-backs
    def result_dict(self):
        r = self._res
        return dict(T=np.array(r.T64).reshape(4, 4), Tf=np.array(r.T, dtype=np.float32).reshape(4, 4), H=np.array(r.H).reshape(6, 6),
                    fitness=r.fitness, iterations=r.iterations, converged=bool(r.converged), lm_failed=bool(r.lm_failed),
                    trace=self.trace())

    def trace(self):
        buf = (IterTrace * 1024)(); n = C.c_uint32()
        self.ctx.check(self._l.qn_gicp_get_trace(self.ctx.h, buf, C.c_uint32(1024), C.byref(n)))
        return np.array([[t.y0, t.lambda_, t.rho, t.max_dR, t.max_dt, t.inner, t.accepted] for t in buf[:n.value]]).reshape(-1, 7)

    def covariances(self, which):
        out = np.zeros((self._n[which], 3, 3))
        self.ctx.check(self._l.qn_gicp_get_covariances(self.ctx.h, C.c_int(which), _p(out)))
        return out

    def knn(self, which, k):
        idx = np.zeros((self._n[which], k), dtype=np.int32); d2 = np.zeros((self._n[which], k), dtype=np.float32)
        self.ctx.check(self._l.qn_gicp_knn(self.ctx.h, C.c_int(which), C.c_int(k), _p(idx), _p(d2)))
        return idx, d2

    def linearize(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64)
        H = np.zeros((6, 6)); b = np.zeros(6); e = C.c_double()
        corr = np.zeros(self._n[0], dtype=np.int32); sqd = np.zeros(self._n[0], dtype=np.float32)
        self.ctx.check(self._l.qn_gicp_linearize(self.ctx.h, _p(T), _p(H), _p(b), C.byref(e), _p(corr), _p(sqd)))
        return H, b, e.value, corr, sqd

    def compute_error(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64); e = C.c_double()
        self.ctx.check(self._l.qn_gicp_compute_error(self.ctx.h, _p(T), C.byref(e)))
        return e.value


class _ParamsScope:
    """The helpers below register at the reference's effective config on a context the caller handed in: the context's own NanoGICP
    parameters are read first (qn_gicp_get_params) and put back afterwards, so a caller's configured object keeps working."""

    def __init__(self, ctx):
        self.ctx = ctx; self.saved = GicpParams()
        ctx.check(ctx._l.qn_gicp_get_params(ctx.h, C.byref(self.saved)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.check(self.ctx._l.qn_gicp_set_params(self.ctx.h, C.byref(self.saved)))
        return False


def _reference_gicp(ctx, k, max_iter, max_corr_dist, trans_eps):
    p = GicpParams(); ctx._l.qn_gicp_default_params(C.byref(p))
    p.k_correspondences, p.max_iterations, p.max_corr_dist, p.transformation_epsilon = k, max_iter, max_corr_dist, trans_eps
    ctx.check(ctx._l.qn_gicp_set_params(ctx.h, C.byref(p)))


def icp_alignment(ctx, src, dst, *, k=15, max_iter=32, max_corr_dist=52.5, trans_eps=0.01, score_thr=1.5):
    """LoopClosure::icpAlignment (loop_closure.cpp:110-136) at the reference's effective config."""
    a, ns, stride = _cloud_arg(src); b, nt, _ = _cloud_arg(dst)
    res = GicpResult(); valid = C.c_int()
    with _ParamsScope(ctx):
        _reference_gicp(ctx, k, max_iter, max_corr_dist, trans_eps)
        st = ctx._l.qn_icp_alignment(ctx.h, _p(a), C.c_uint32(ns), _p(b), C.c_uint32(nt), C.c_uint32(stride),
                                     C.c_double(score_thr), C.byref(res), C.byref(valid))
    if st == QN_ERR_EMPTY_CLOUD:
        return dict(valid=False, converged=False, score=1.7976931348623157e308, T=np.eye(4), iterations=0)
    ctx.check(st)
    return dict(valid=bool(valid.value), converged=bool(res.converged), score=res.fitness,
                T=np.array(res.T, dtype=np.float32).reshape(4, 4).astype(np.float64), iterations=res.iterations)


def fpfh(ctx, xyz):
    """qn_fpfh: n x 33 FPFH descriptors (NaN rows where PCL yields none), radii from the context's Quatro parameters."""
    a, n, stride = _cloud_arg(xyz)
    out = np.zeros((n, 33), dtype=np.float32)
    ctx.check(ctx._l.qn_fpfh(ctx.h, _p(a), C.c_uint32(n), C.c_uint32(stride), _p(out)))
    return out


def match_optimized(ctx, src, dst, fs, ft, thr_dist=35.0, num_max_corres=200, tuple_scale=0.95):
    """qn_match_optimized: Matcher::optimizedMatching on two clouds and their descriptors -> (m, 2) int32 pairs (src idx, dst idx)."""
    a, ns, stride = _cloud_arg(src); b, nt, _ = _cloud_arg(dst)
    fs = np.ascontiguousarray(fs, dtype=np.float32); ft = np.ascontiguousarray(ft, dtype=np.float32)
    pairs = np.zeros((num_max_corres, 2), dtype=np.int32); n = C.c_uint32()
    ctx.check(ctx._l.qn_match_optimized(ctx.h, _p(a), C.c_uint32(ns), _p(b), C.c_uint32(nt), C.c_uint32(stride), _p(fs), _p(ft),
                                        C.c_float(thr_dist), C.c_int(num_max_corres), C.c_float(tuple_scale), _p(pairs), C.c_uint32(num_max_corres), C.byref(n)))
    return pairs[:min(n.value, num_max_corres)].copy()


# ---------------------------------------------------------------------------------------- Quatro
class QuatroParams(C.Structure):
    _fields_ = [("fpfh_normal_radius", C.c_double), ("fpfh_radius", C.c_double), ("noise_bound", C.c_double),
                ("rot_gnc_factor", C.c_double), ("rot_cost_diff_thr", C.c_double), ("rot_max_iter", C.c_int32),
                ("estimate_scale", C.c_int32), ("use_optimized_matching", C.c_int32), ("distance_threshold", C.c_double),
                ("max_num_corres", C.c_int32), ("rng_seed", C.c_uint32), ("tuple_scale", C.c_double)]


def quatro_default_params():
    p = QuatroParams(); lib().qn_quatro_default_params(C.byref(p)); return p


class Quatro:
    """quatro<PointType> as LoopClosure uses it: the 10-argument constructor in the reference's order
    (fast_lio_sam_qn/src/loop_closure.cpp:18-27) and align(src, dst) -> (4x4 f64, is_converged) (:144)."""

    def __init__(self, ctx, fpfh_normal_radius=0.9, fpfh_radius=1.5, noise_bound=0.3, rot_gnc_factor=1.4, rot_cost_diff_thr=1e-4,
                 rot_max_iter=50, estimate_scale=False, use_optimized_matching=True, distance_threshold=35.0, max_num_corres=200,
                 rng_seed=1):
        self.ctx = ctx; self._l = ctx._l
        p = quatro_default_params()
        p.fpfh_normal_radius, p.fpfh_radius, p.noise_bound = fpfh_normal_radius, fpfh_radius, noise_bound
        p.rot_gnc_factor, p.rot_cost_diff_thr, p.rot_max_iter = rot_gnc_factor, rot_cost_diff_thr, rot_max_iter
        p.estimate_scale, p.use_optimized_matching = int(estimate_scale), int(use_optimized_matching)
        p.distance_threshold, p.max_num_corres, p.rng_seed = distance_threshold, max_num_corres, rng_seed
        self.p = p
        ctx.check(self._l.qn_quatro_set_params(ctx.h, C.byref(p)))
        self._n = [0, 0]

    def align(self, src, dst, debug=False):
        a, ns, stride = _cloud_arg(src); b, nt, _ = _cloud_arg(dst); self._n = [ns, nt]
        T = np.zeros((4, 4)); valid = C.c_int()
        if not debug:
            st = self._l.qn_quatro_align(self.ctx.h, _p(a), C.c_uint32(ns), _p(b), C.c_uint32(nt), C.c_uint32(stride), _p(T), C.byref(valid))
            if st != QN_ERR_EMPTY_CLOUD:
                self.ctx.check(st)
            return T, bool(valid.value)
        cap = min(ns, nt) + 8
        mutual = np.zeros((cap, 2), np.int32); corres = np.zeros((cap, 2), np.int32); clique = np.zeros(cap, np.int32)
        nm, nc, nq, it = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        self.ctx.check(self._l.qn_quatro_align_debug(self.ctx.h, _p(a), C.c_uint32(ns), _p(b), C.c_uint32(nt), C.c_uint32(stride), _p(T), C.byref(valid),
                                                     _p(mutual), C.byref(nm), _p(corres), C.byref(nc), C.c_uint32(cap), _p(clique), C.byref(nq), C.byref(it)))
        return dict(T=T, valid=bool(valid.value), mutual=mutual[:nm.value].copy(), corres=corres[:nc.value].copy(),
                    clique=clique[:nq.value].copy(), rot_iterations=it.value)

    def align_device(self, src_ptr, ns, dst_ptr, nt, stride):
        """qn_quatro_align_device: both clouds are HIP device pointers (n points, `stride` bytes apart)."""
        self._n = [ns, nt]
        T = np.zeros((4, 4)); valid = C.c_int()
        self.ctx.check(self._l.qn_quatro_align_device(self.ctx.h, C.c_void_p(src_ptr), C.c_uint32(ns), C.c_void_p(dst_ptr), C.c_uint32(nt), C.c_uint32(stride), _p(T), C.byref(valid)))
        return T, bool(valid.value)

    def scale(self):
        """TEASER++'s scale estimate of the latest align (1 unless estimate_scale)"""
        v = C.c_double()
        self.ctx.check(self._l.qn_quatro_get_scale(self.ctx.h, C.byref(v)))
        return v.value

    def features(self, which):
        n = self._n[which]
        nrm = np.zeros((n, 3), np.float32); sp = np.zeros((n, 33), np.float32); fp = np.zeros((n, 33), np.float32)
        self.ctx.check(self._l.qn_quatro_get_features(self.ctx.h, C.c_int(which), _p(nrm), _p(sp), _p(fp)))
        return nrm, sp, fp


def quatro_solve(src, dst, corres, params=None):
    """Host-side Matcher tail + TEASER++/Quatro solve on given correspondences (no GPU involved)."""
    p = params or quatro_default_params()
    a, _, stride = _cloud_arg(src); b, _, _ = _cloud_arg(dst)
    corres = np.ascontiguousarray(corres, dtype=np.int32)
    T = np.zeros((4, 4)); valid = C.c_int(); clique = np.zeros(max(len(corres), 1), np.int32); nq = C.c_uint32()
    scale = C.c_double(1.0); it = C.c_int32()
    st = lib().qn_quatro_solve_iter(_p(a), _p(b), C.c_uint32(stride), _p(corres), C.c_uint32(len(corres)), C.byref(p), _p(T), C.byref(valid), _p(clique), C.byref(nq), C.byref(scale), C.byref(it))
    if st != QN_OK:
        raise EngineError(st, lib().qn_status_str(st).decode())
    return dict(T=T, valid=bool(valid.value), clique=clique[:nq.value].copy(), scale=scale.value, rot_iterations=it.value)


def coarse_to_fine_alignment(ctx, src, dst, *, quatro=None, k=15, max_iter=32, max_corr_dist=52.5, trans_eps=0.01, score_thr=1.5):
    """LoopClosure::coarseToFineAlignment (loop_closure.cpp:138-159) at the reference's effective config."""
    quatro = quatro or Quatro(ctx)
    a, ns, stride = _cloud_arg(src); b, nt, _ = _cloud_arg(dst)
    res = GicpResult(); valid = C.c_int(); T = np.zeros((4, 4)); Tq = np.zeros((4, 4))
    with _ParamsScope(ctx):
        _reference_gicp(ctx, k, max_iter, max_corr_dist, trans_eps)
        st = ctx._l.qn_coarse_to_fine_alignment(ctx.h, _p(a), C.c_uint32(ns), _p(b), C.c_uint32(nt), C.c_uint32(stride), C.c_double(score_thr),
                                                C.byref(res), _p(T), _p(Tq), C.byref(valid))
    if st == QN_ERR_EMPTY_CLOUD:
        return dict(valid=False, converged=False, score=1.7976931348623157e308, T=np.eye(4), T_quatro=np.eye(4))
    ctx.check(st)
    return dict(valid=bool(valid.value), converged=bool(res.converged), score=res.fitness, T=T, T_quatro=Tq, iterations=res.iterations,
                T_gicp=np.array(res.T, dtype=np.float32).reshape(4, 4).astype(np.float64))


def coarse_to_fine_alignment_device(ctx, src_ptr, ns, dst_ptr, nt, stride, *, quatro=None, k=15, max_iter=32, max_corr_dist=52.5, trans_eps=0.01, score_thr=1.5):
    """qn_coarse_to_fine_alignment_device: the same with both clouds resident on the GPU (e.g. KeyframeStore.assemble outputs)."""
    quatro = quatro or Quatro(ctx)
    res = GicpResult(); valid = C.c_int(); T = np.zeros((4, 4)); Tq = np.zeros((4, 4))
    with _ParamsScope(ctx):
        _reference_gicp(ctx, k, max_iter, max_corr_dist, trans_eps)
        ctx.check(ctx._l.qn_coarse_to_fine_alignment_device(ctx.h, C.c_void_p(src_ptr), C.c_uint32(ns), C.c_void_p(dst_ptr), C.c_uint32(nt), C.c_uint32(stride),
                                                           C.c_double(score_thr), C.byref(res), _p(T), _p(Tq), C.byref(valid)))
    return dict(valid=bool(valid.value), converged=bool(res.converged), score=res.fitness, T=T, T_quatro=Tq, iterations=res.iterations,
                T_gicp=np.array(res.T, dtype=np.float32).reshape(4, 4).astype(np.float64))


# ---------------------------------------------------------------------------------------- batch
class PairDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("ns", C.c_uint32), ("dst", C.c_void_p), ("nt", C.c_uint32), ("stride_bytes", C.c_uint32), ("on_device", C.c_int32)]


def icp_alignment_batch(contexts, pairs, score_thr=1.5):
    """pairs: list of (src_ptr_or_array, ns, dst_ptr_or_array, nt, stride_bytes, on_device).  Arrays are host float32
    clouds; ints are device pointers.  Every context must already carry its NanoGICP parameters.
    Returns (results[GicpResult], valid[int], status[int])."""
    n = len(pairs)
    descs = (PairDesc * n)(); keep = []
    for i, (s, ns, d, nt, stride, dev) in enumerate(pairs):
        if not dev:
            s = np.ascontiguousarray(s, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32); keep += [s, d]
            descs[i] = PairDesc(s.ctypes.data, ns, d.ctypes.data, nt, stride, 0)
        else:
            descs[i] = PairDesc(s, ns, d, nt, stride, 1)
    results = (GicpResult * n)(); valid = (C.c_int * n)(); status = (C.c_int * n)()
    hs = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    st = lib().qn_icp_alignment_batch(hs, C.c_uint32(len(contexts)), descs, C.c_uint32(n), C.c_double(score_thr), results, valid, status)
    if st != QN_OK:
        raise EngineError(st, lib().qn_status_str(st).decode())
    return results, list(valid), list(status)


def gicp_align_batch(ctx, pairs, score_thr=1.5, guesses=None):
    """qn_gicp_align_batch: the same batch on ONE context, the pair as a grid dimension of every kernel launch (`batch_lanes` pairs in lockstep).
    pairs / return value as icp_alignment_batch.  guesses (n x 4 x 4, rounded to f32) given: qn_gicp_align_batch_guess, pair i starts from guesses[i]."""
    n = len(pairs)
    descs = (PairDesc * n)(); keep = []
    for i, (s, ns, d, nt, stride, dev) in enumerate(pairs):
        if not dev:
            s = np.ascontiguousarray(s, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32); keep += [s, d]
            descs[i] = PairDesc(s.ctypes.data, ns, d.ctypes.data, nt, stride, 0)
        else:
            descs[i] = PairDesc(s, ns, d, nt, stride, 1)
    results = (GicpResult * n)(); valid = (C.c_int * n)(); status = (C.c_int * n)()
    if guesses is None:
        st = lib().qn_gicp_align_batch(ctx.h, descs, C.c_uint32(n), C.c_double(score_thr), results, valid, status)
    else:
        g = np.ascontiguousarray(np.asarray(guesses, dtype=np.float64).astype(np.float32).reshape(-1, 16))
        if len(g) != n:
            raise ValueError("gicp_align_batch: %d pairs but %d guesses" % (n, len(g)))
        st = lib().qn_gicp_align_batch_guess(ctx.h, descs, _p(g), C.c_uint32(n), C.c_double(score_thr), results, valid, status)
    if st != QN_OK:
        raise EngineError(st, lib().qn_status_str(st).decode() + ": " + lib().qn_last_error(ctx.h).decode())
    return results, list(valid), list(status)


def coarse_to_fine_align_batch(contexts, pairs, score_thr=1.5):
    """qn_coarse_to_fine_align_batch: n independent coarseToFineAlignment calls (loop_closure.cpp:138-159) over the contexts' lanes.  pairs as icp_alignment_batch; every
    context must carry its NanoGICP and Quatro parameters.  -> list of dict(valid, converged, score, iterations, T (= T_gicp * T_quatro), T_quatro, T_gicp (f32 record as f64), status)"""
    n = len(pairs)
    descs = (PairDesc * max(n, 1))(); keep = []
    for i, (s, ns, d, nt, stride, dev) in enumerate(pairs):
        if not dev:
            s = np.ascontiguousarray(s, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32); keep += [s, d]
            descs[i] = PairDesc(s.ctypes.data, ns, d.ctypes.data, nt, stride, 0)
        else:
            descs[i] = PairDesc(s, ns, d, nt, stride, 1)
    results = (GicpResult * max(n, 1))(); valid = (C.c_int * max(n, 1))(); status = (C.c_int * max(n, 1))()
    Tt = np.zeros((max(n, 1), 4, 4)); Tq = np.zeros((max(n, 1), 4, 4))
    hs = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    st = lib().qn_coarse_to_fine_align_batch(hs, C.c_uint32(len(contexts)), descs, C.c_uint32(n), C.c_double(score_thr), results, _p(Tt), _p(Tq), valid, status)
    if st != QN_OK:
        raise EngineError(st, lib().qn_status_str(st).decode())
    return [dict(valid=bool(valid[i]), converged=bool(results[i].converged), score=results[i].fitness, iterations=results[i].iterations, T=Tt[i].copy(), T_quatro=Tq[i].copy(),
                 T_gicp=np.array(results[i].T, dtype=np.float32).reshape(4, 4).astype(np.float64), status=int(status[i])) for i in range(n)]


def lane_trace(ctx, lane):
    """qn_gicp_get_lane_trace: the iteration trace (y0, lambda, rho, max_dR, max_dt, inner, accepted) of lane `lane` of the latest qn_gicp_align_batch run"""
    buf = (IterTrace * 1024)(); n = C.c_uint32()
    ctx.check(lib().qn_gicp_get_lane_trace(ctx.h, C.c_uint32(lane), buf, C.c_uint32(1024), C.byref(n)))
    return np.array([[t.y0, t.lambda_, t.rho, t.max_dR, t.max_dt, t.inner, t.accepted] for t in buf[:n.value]]).reshape(-1, 7)


def lane_knn(ctx, lane, which):
    """qn_gicp_get_lane_knn: the k-NN index table (n x k int32, original point order, -1 = missing) cloud `which` of lane `lane` was last given its covariances from -
    the table the registration used.  EngineError QN_ERR_NOT_READY once it is gone (cloud set anew, k changed, buffer reused for the other cloud, a borrowed source)"""
    n = C.c_uint32(); k = C.c_int()
    ctx.check(lib().qn_gicp_get_lane_knn(ctx.h, C.c_uint32(lane), C.c_int(which), None, C.byref(n), C.byref(k)))
    idx = np.zeros((n.value, k.value), dtype=np.int32)
    ctx.check(lib().qn_gicp_get_lane_knn(ctx.h, C.c_uint32(lane), C.c_int(which), _p(idx), C.byref(n), C.byref(k)))
    return idx


def lane_covariances(ctx, lane, which, n):
    """qn_gicp_get_lane_covariances: the covariances cloud `which` (n points) of lane `lane` holds, n x 3 x 3"""
    out = np.zeros((ctx.max_points, 3, 3))
    ctx.check(lib().qn_gicp_get_lane_covariances(ctx.h, C.c_uint32(lane), C.c_int(which), _p(out)))
    return out[:n].copy()


class PairRecord(C.Structure):
    _fields_ = [("pair_id", C.c_int32), ("status", C.c_int32), ("valid", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("reserved", C.c_int32), ("fitness", C.c_double), ("T", C.c_float * 16)]


class MultiGpu:
    """qn_multi_*: candidate pairs sharded pair i -> GPU i mod N inside one process, one RCCL all-gather of the result records."""

    def __init__(self, n_gpus, max_points, in_flight=4, device_ids=None):
        self._l = lib(); h = C.c_void_p()
        self._l.qn_multi_last_error.restype = C.c_char_p; self._l.qn_multi_last_error.argtypes = [C.c_void_p]
        self._l.qn_multi_destroy.argtypes = [C.c_void_p]
        ids = None if device_ids is None else (C.c_int * n_gpus)(*device_ids)
        st = self._l.qn_multi_init(C.c_int(n_gpus), ids, C.c_uint32(max_points), C.c_int(in_flight), C.byref(h))
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode() + ": " + self._l.qn_multi_last_error(None).decode())
        self.h = h; self.n_gpus = n_gpus

    def close(self):
        if getattr(self, "h", None):
            self._l.qn_multi_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode() + ": " + self._l.qn_multi_last_error(self.h).decode())

    def set_params(self, p):
        self._check(self._l.qn_multi_set_params(self.h, C.byref(p)))

    def debug_set(self, key, value):
        self._check(self._l.qn_multi_debug_set(self.h, key.encode(), C.c_double(value)))

    def set_quatro_params(self, qp):
        """enable_quatro_ (loop_closure.h:54): a QuatroParams = every pair becomes a coarseToFineAlignment; None = Nano-GICP only"""
        self._check(self._l.qn_multi_set_quatro_params(self.h, C.byref(qp) if qp is not None else None))

    def timing(self):
        """(per-GPU ms [n_gpus], gather ms) of the latest align_best"""
        per = (C.c_double * self.n_gpus)(); gms = C.c_double()
        self._check(self._l.qn_multi_get_timing(self.h, per, C.byref(gms)))
        return list(per), gms.value

    def gpu_count(self):
        return int(self._l.qn_multi_gpu_count(self.h))

    def rccl_ranks(self):
        """ranks of the communicator as RCCL reports them (ncclCommCount), -1 on failure"""
        return int(self._l.qn_multi_rccl_ranks(self.h))

    def verify_gather(self):
        """after align_best: every GPU's receive buffer holds the table GPU 0 received"""
        self._check(self._l.qn_multi_verify_gather(self.h))

    def align_best(self, pairs, score_thr=1.5):
        """pairs as for icp_alignment_batch.  -> (records[n], best or None)"""
        n = len(pairs)
        descs = (PairDesc * max(n, 1))(); keep = []
        for i, (s, ns, d, nt, stride, dev) in enumerate(pairs):
            if not dev:
                s = np.ascontiguousarray(s, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32); keep += [s, d]
                descs[i] = PairDesc(s.ctypes.data, ns, d.ctypes.data, nt, stride, 0)
            else:
                descs[i] = PairDesc(s, ns, d, nt, stride, 1)
        recs = (PairRecord * max(n, 1))(); best = PairRecord(); found = C.c_int()
        self._check(self._l.qn_multi_align_best(self.h, descs, C.c_uint32(n), C.c_double(score_thr), recs, C.byref(best), C.byref(found)))
        return list(recs[:n]), (best if found.value else None)


# ---------------------------------------------------------------------------------------- keyframe store / cloud assembly
# The records below and KeyframeStore's wrappers share one set of idioms; the next unit's wrapper starts from them, not from a copy of the previous unit's:
# a parameter record is a _Twinned Structure that names its twin once; a params= argument goes through _record; a result record becomes a dict through _as_dict.
def _open_fields(cls):
    """the (name, ctypes type) of a record's fields, in field order, without those whose names start with reserved or pad"""
    return [(f, t) for f, t in cls._fields_ if not f.startswith(("reserved", "pad"))]


def _as_dict(rec):
    """a record as a dict of its open fields: numbers as Python numbers, arrays as tuples of them, nested records as dicts"""
    def py(v):
        return _as_dict(v) if isinstance(v, C.Structure) else tuple(py(x) for x in v) if isinstance(v, C.Array) else v
    return {f: py(getattr(rec, f)) for f, _ in _open_fields(type(rec))}


class _Twinned:
    """mixin of a record with a numpy twin: TWIN = (the module of qn_amd, the name in it) says where the twin lives, once; the fields go across by name"""
    TWIN = None

    @classmethod
    def _twin_type(cls):
        import importlib
        return getattr(importlib.import_module("." + cls.TWIN[0], __package__), cls.TWIN[1])

    def twin(self):
        """-> the twin with these values: a namedtuple twin's own fields (a stats twin has fewer than the record), else every open field"""
        T = self._twin_type()
        return T(**{f: getattr(self, f) for f in getattr(T, "_fields", [f for f, _ in _open_fields(type(self))])})

    @classmethod
    def from_twin(cls, p):
        """-> the record of any object with the open fields as attributes, each coerced by the field's type: float() for a double, int() for an integer"""
        return cls(**{f: (float if t is C.c_double else int)(getattr(p, f)) for f, t in _open_fields(cls)})


def _record(cls, params):
    """every params= argument: None -> the defaults, a cls -> that object, anything else (the twin) -> cls.from_twin(params)"""
    if params is None:
        return cls()
    return params if isinstance(params, cls) else cls.from_twin(params)


class SimSensor(C.Structure):
    """qn_sim_sensor"""
    _fields_ = [("n_beams", C.c_uint32), ("n_cols", C.c_uint32), ("cos_el", C.c_void_p), ("sin_el", C.c_void_p), ("cos_az", C.c_void_p),
                ("sin_az", C.c_void_p), ("min_range", C.c_double), ("max_range", C.c_double), ("sigma", C.c_double)]


class ScParams(C.Structure):
    """qn_sc_params: Scan Context descriptor shape and the ring-key prefilter (defaults = the original's, exhaustive search)"""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("max_radius", C.c_double), ("lidar_height", C.c_double),
                ("ringkey_prefilter", C.c_uint32), ("pad_", C.c_uint32)]

    def __init__(self, n_rings=20, n_sectors=60, max_radius=80.0, lidar_height=2.0, ringkey_prefilter=0):
        super().__init__(n_rings, n_sectors, max_radius, lidar_height, ringkey_prefilter, 0)


class OverlapDir(C.Structure):
    """qn_overlap_dir (24 bytes): one direction of a pair's overlap record"""
    _fields_ = [("n", C.c_uint32), ("n_finite", C.c_uint32), ("inliers", C.c_uint32), ("reserved", C.c_uint32), ("sum_d2", C.c_double)]


class Overlap(C.Structure):
    """qn_overlap (48 bytes)"""
    _fields_ = [("a_to_b", OverlapDir), ("b_to_a", OverlapDir)]


class RangeParams(_Twinned, C.Structure):
    """qn_range_params (56 bytes): the range-image shape, field of view, blind radius, and the free-space check's window and tolerances"""
    TWIN = ("freespace", "Params")
    _fields_ = [("n_rows", C.c_uint32), ("n_cols", C.c_uint32), ("el_lo", C.c_double), ("el_hi", C.c_double), ("min_range", C.c_double),
                ("window_rows", C.c_uint32), ("window_cols", C.c_uint32), ("tol_abs", C.c_double), ("tol_rel", C.c_double)]

    def __init__(self, n_rows=64, n_cols=1800, el_lo=-0.4363323129985824, el_hi=0.038397243543875255, min_range=2.0, window_rows=1, window_cols=1,
                 tol_abs=0.3, tol_rel=0.02):
        super().__init__(n_rows, n_cols, el_lo, el_hi, min_range, window_rows, window_cols, tol_abs, tol_rel)

    @classmethod
    def for_sensor(cls, sensor, **kw):
        """The image of a synth.SpinningLidar: a row per beam, a column per azimuth step, the edges half a beam spacing outside el_min / el_max
        (freespace.Params.for_sensor)"""
        from . import freespace
        return cls.from_twin(freespace.Params.for_sensor(sensor, **kw))


class FreespaceDir(C.Structure):
    """qn_freespace_dir (32 bytes): one direction of a pair's free-space record"""
    _fields_ = [(f, C.c_uint32) for f in ("n", "n_finite", "in_fov", "observed", "seen_through", "occluded", "agree", "reserved")]


class Freespace(C.Structure):
    """qn_freespace (64 bytes)"""
    _fields_ = [("q_in_c", FreespaceDir), ("c_in_q", FreespaceDir)]


class StaticParams(_Twinned, C.Structure):
    """qn_static_params (8 bytes): the rule of the static map - a record is removed iff seen_through >= min_see_through and seen_through > agree_weight * agree"""
    TWIN = ("staticmap", "StaticParams")
    _fields_ = [("min_see_through", C.c_uint32), ("agree_weight", C.c_uint32)]

    def __init__(self, min_see_through=2, agree_weight=1):
        super().__init__(min_see_through, agree_weight)


class NormalParams(_Twinned, C.Structure):
    """qn_normal_params (16 bytes): the neighbourhood radius of the map normals and the fewest neighbours (the point included) that make one"""
    TWIN = ("mapnormals", "NormalParams")
    _fields_ = [("radius", C.c_double), ("min_neighbors", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, radius=0.6, min_neighbors=5):
        super().__init__(radius, min_neighbors, 0)


class OutlierParams(_Twinned, C.Structure):
    """qn_outlier_params (24 bytes): the neighbourhood radius, PCL's std_mul and the k nearest neighbours of the map's outlier filter"""
    TWIN = ("mapoutliers", "OutlierParams")
    _fields_ = [("radius", C.c_double), ("std_mul", C.c_double), ("k", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, radius=1.0, std_mul=2.0, k=8):
        super().__init__(radius, std_mul, k, 0)


class OutlierStats(C.Structure):
    """qn_outlier_stats (64 bytes); mean_q, std_q and thr_q in units of 2^-quant_exp m"""
    _fields_ = [(f, C.c_uint32) for f in ("n", "n_finite", "dense", "sparse", "removed")] + [("quant_exp", C.c_int32), ("sum_q", C.c_uint64), ("sum_q2", C.c_uint64),
                                                                                              ("mean_q", C.c_double), ("std_q", C.c_double), ("thr_q", C.c_double)]


class GroundParams(_Twinned, C.Structure):
    """qn_ground_params (40 bytes): the grid edge, the largest ground slope (rise over run), the ground tolerance, the clearance below which a point occupies
    its column, and the points a column needs to seed the ground.  The defaults are interface choices, not measurements."""
    TWIN = ("mapground", "GroundParams")
    _fields_ = [("cell", C.c_double), ("max_slope", C.c_double), ("ground_tol", C.c_double), ("clearance", C.c_double), ("min_points", C.c_uint32),
                ("reserved", C.c_uint32)]

    def __init__(self, cell=0.5, max_slope=0.3, ground_tol=0.2, clearance=2.0, min_points=1):
        super().__init__(cell, max_slope, ground_tol, clearance, min_points, 0)


class GroundStats(C.Structure):
    """qn_ground_stats (80 bytes); rounds is the only field the twin does not share"""
    _fields_ = ([(f, C.c_uint32) for f in ("n", "n_finite", "n_none", "n_ground", "n_obstacle", "n_overhead", "n_below", "width", "height", "seeded", "occupied",
                                           "free", "unknown")] +
                [(f, C.c_int32) for f in ("quant_exp", "step_s", "step_d", "tol_q", "clear_q")] + [("rounds", C.c_uint32), ("reserved", C.c_uint32)])


class GroundGrid(C.Structure):
    """qn_ground_grid (40 bytes): the corner of column (0, 0), the edge, the size and the height unit 2^-quant_exp m of the occupancy grid"""
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("cell", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32), ("quant_exp", C.c_int32),
                ("reserved", C.c_uint32)]


QN_GROUND_NONE, QN_GROUND_GROUND, QN_GROUND_OBSTACLE, QN_GROUND_OVERHEAD, QN_GROUND_BELOW = range(5)
QN_GROUND_MAX_CELLS = 1 << 26


class OccupancyParams(_Twinned, C.Structure):
    """qn_occupancy_params (48 bytes): the voxel edge, the ranges between which a record is a ray, the voxels before a ray's end that are not carved, the hits a
    voxel needs to be occupied and the weight of a hit against a miss.  The defaults are interface choices, not measurements."""
    TWIN = ("mapoccupancy", "OccupancyParams")
    _fields_ = [("voxel", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("shell", C.c_uint32), ("min_hits", C.c_uint32),
                ("hit_weight", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, voxel=0.3, min_range=0.5, max_range=60.0, shell=1, min_hits=1, hit_weight=2):
        super().__init__(voxel, min_range, max_range, shell, min_hits, hit_weight)


class OccupancyStats(C.Structure):
    """qn_occupancy_stats (64 bytes): every field is an integer the twin shares"""
    _fields_ = ([(f, C.c_uint32) for f in ("n_records", "n_rays", "n_nonfinite", "n_near", "n_far", "width", "height", "depth", "occupied", "free", "unknown",
                                           "reserved")] + [("total_hits", C.c_uint64), ("total_misses", C.c_uint64)])


class OccupancyGrid(C.Structure):
    """qn_occupancy_grid (56 bytes): the corner of voxel (0, 0, 0), the edge, the size and the voxel coordinates of that corner"""
    _fields_ = [("origin", C.c_double * 3), ("voxel", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32), ("minc", C.c_int32 * 3)]


class OccupancyUpdate(C.Structure):
    """qn_occupancy_update (64 bytes): what qn_kf_map_occupancy_update did - the entries kept, added and removed, whether it started from nothing, whether the
    counts were moved to another box, the records the walks read, the box of the new grid outside which no count changed, the rays added and removed"""
    _fields_ = ([(f, C.c_uint32) for f in ("entries_kept", "entries_added", "entries_removed", "rebuilt", "regridded", "records_walked")] +
                [("dirty_lo", C.c_int32 * 3), ("dirty_hi", C.c_int32 * 3), ("rays_added", C.c_uint64), ("rays_removed", C.c_uint64)])


QN_OCC_UNKNOWN, QN_OCC_FREE, QN_OCC_OCCUPIED = range(3)
QN_OCC_MAX_CELLS = 1 << 27


class DistanceParams(_Twinned, C.Structure):
    """qn_distance_params (16 bytes): the classes that count as sites (bit 1 << class) and the largest distance, in voxels, the field resolves.  The defaults
    are interface choices, not measurements."""
    TWIN = ("mapdistance", "DistanceParams")
    _fields_ = [("site_mask", C.c_uint32), ("max_dist", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, site_mask=1 << QN_OCC_OCCUPIED, max_dist=16):
        super().__init__(site_mask, max_dist)


class DistanceStats(_Twinned, C.Structure):
    """qn_distance_stats (32 bytes): every field is an integer the twin shares"""
    TWIN = ("mapdistance", "DistanceStats")
    _fields_ = [("sites", C.c_uint32), ("reached", C.c_uint32), ("far", C.c_uint32), ("max_d2", C.c_uint32), ("sum_d2", C.c_uint64), ("reserved", C.c_uint32 * 2)]


QN_DIST_FAR = 0xffff
QN_DIST_MAX_RADIUS = 255
QN_DIST_OUTSIDE = 0xff


class RouteParams(_Twinned, C.Structure):
    """qn_route_params (32 bytes): the classes that are passable (bit 1 << class), the smallest d2 a passable voxel has (0: no test), the band of layers, and
    whether the field is the plane of columns.  The defaults are interface choices, not measurements."""
    TWIN = ("maproute", "RouteParams")
    _fields_ = [("pass_mask", C.c_uint32), ("min_d2", C.c_uint32), ("iz_lo", C.c_int32), ("iz_hi", C.c_int32), ("planar", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, pass_mask=1 << QN_OCC_FREE, min_d2=4, iz_lo=0, iz_hi=0x7fffffff, planar=0):
        super().__init__(pass_mask, min_d2, iz_lo, iz_hi, planar)


class RouteStats(_Twinned, C.Structure):
    """qn_route_stats (64 bytes): every field but rounds and tile_visits - diagnostics of the GPU schedule - is an integer the twin shares"""
    TWIN = ("maproute", "RouteStats")
    _fields_ = [("passable", C.c_uint32), ("blocked", C.c_uint32), ("reached", C.c_uint32), ("unreached", C.c_uint32), ("goals_used", C.c_uint32),
                ("goals_blocked", C.c_uint32), ("max_cost", C.c_uint32), ("reserved0", C.c_uint32), ("sum_cost", C.c_uint64), ("rounds", C.c_uint64),
                ("tile_visits", C.c_uint64), ("reserved", C.c_uint32 * 2)]


QN_ROUTE_BLOCKED = 0xfffffffe
QN_ROUTE_UNREACHED = 0xffffffff
QN_ROUTE_MAX_POINTS = 1 << 20
QN_ROUTE_ROUNDS_PER_CHECK = 8


class FrontierParams(_Twinned, C.Structure):
    """qn_frontier_params (32 bytes): the classes that are candidates and those that are unknown (bit 1 << class, no class in both), whether the space outside
    the grid is unknown, the smallest component that is a region, and the band of layers.  The defaults are interface choices, not measurements."""
    TWIN = ("mapfrontier", "FrontierParams")
    _fields_ = [("free_mask", C.c_uint32), ("unknown_mask", C.c_uint32), ("edge_unknown", C.c_uint32), ("min_size", C.c_uint32), ("iz_lo", C.c_int32),
                ("iz_hi", C.c_int32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, free_mask=1 << QN_OCC_FREE, unknown_mask=1 << QN_OCC_UNKNOWN, edge_unknown=1, min_size=8, iz_lo=0, iz_hi=0x7fffffff):
        super().__init__(free_mask, unknown_mask, edge_unknown, min_size, iz_lo, iz_hi)


class FrontierStats(_Twinned, C.Structure):
    """qn_frontier_stats (48 bytes): every field but rounds - a diagnostic of the GPU schedule - is an integer the twin shares"""
    TWIN = ("mapfrontier", "FrontierStats")
    _fields_ = [(f, C.c_uint32) for f in ("candidates", "frontier", "components", "regions", "too_small", "region_voxels", "rejected_voxels", "largest",
                                          "unknown_faces", "rounds")] + [("reserved", C.c_uint32 * 2)]


class FrontierInfo(C.Structure):
    """qn_frontier_info (64 bytes), the layout of mapfrontier.INFO_DTYPE: a region's root, size, box of grid indices, unknown faces and index sums"""
    _fields_ = [("root", C.c_uint32), ("size", C.c_uint32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("faces", C.c_uint32), ("reserved", C.c_uint32),
                ("sum", C.c_uint64 * 3)]


QN_FRONTIER_REJECTED = -1
QN_FRONTIER_NONE = -2


class ViewParams(_Twinned, C.Structure):
    """qn_view_params (32 bytes): the classes whose voxels are gain and those that stop a ray (bit 1 << class, no class in both; stop_mask may be 0), the gain
    voxels a ray may pass through (0: no limit), and the band of layers in which a voxel is marked.  The defaults are interface choices, not measurements."""
    TWIN = ("mapview", "ViewParams")
    _fields_ = [("gain_mask", C.c_uint32), ("stop_mask", C.c_uint32), ("max_through", C.c_uint32), ("iz_lo", C.c_int32), ("iz_hi", C.c_int32), ("reserved", C.c_uint32 * 3)]

    def __init__(self, gain_mask=1 << QN_OCC_UNKNOWN, stop_mask=1 << QN_OCC_OCCUPIED, max_through=0, iz_lo=0, iz_hi=0x7fffffff):
        super().__init__(gain_mask, stop_mask, max_through, iz_lo, iz_hi)


class ViewInfo(C.Structure):
    """qn_view_info (48 bytes), the layout of mapview.VIEW_DTYPE: a viewpoint's status, gain, ray ends, grid voxel and steps"""
    _fields_ = [("status", C.c_uint32), ("gain", C.c_uint32), ("blocked", C.c_uint32), ("escaped", C.c_uint32), ("spent", C.c_uint32), ("reached", C.c_uint32),
                ("ijk", C.c_int32 * 3), ("reserved", C.c_uint32), ("steps", C.c_uint64)]

    def twin(self):
        """-> the one-element mapview.VIEW_DTYPE array with these values"""
        from . import mapview
        return np.frombuffer(bytes(self), mapview.VIEW_DTYPE).copy()


class ViewStats(_Twinned, C.Structure):
    """qn_view_stats (48 bytes): every field but passes - a diagnostic of the GPU schedule - is an integer the twin shares"""
    TWIN = ("mapview", "ViewStats")
    _fields_ = [(f, C.c_uint32) for f in ("viewpoints", "outside", "rays", "covered", "max_cover", "passes")] + [("reserved", C.c_uint32 * 2), ("total_gain", C.c_uint64),
                                                                                                               ("steps", C.c_uint64)]


QN_VIEW_OK = 0
QN_VIEW_OUTSIDE = 1
QN_VIEW_MAX_OFFSET = 1 << 25


class ClusterParams(_Twinned, C.Structure):
    """qn_cluster_params (24 bytes): the joining distance, the smallest and the largest component that is a cluster, and the ground classes that take part
    (0: every finite point).  The defaults are interface choices, not measurements."""
    TWIN = ("mapclusters", "ClusterParams")
    _fields_ = [("tolerance", C.c_double), ("min_size", C.c_uint32), ("max_size", C.c_uint32), ("class_mask", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, tolerance=0.5, min_size=10, max_size=0xffffffff, class_mask=0):
        super().__init__(tolerance, min_size, max_size, class_mask, 0)


class ClusterStats(C.Structure):
    """qn_cluster_stats (56 bytes)"""
    _fields_ = ([(f, C.c_uint32) for f in ("n", "n_finite", "members", "components", "clusters", "too_small", "too_large", "clustered_points", "rejected_points",
                                           "largest")] + [("quant_exp", C.c_int32), ("reserved", C.c_uint32), ("edges", C.c_uint64)])


class ClusterInfo(C.Structure):
    """qn_cluster_info (56 bytes): a cluster's root, size, box and quantised coordinate sums"""
    _fields_ = [("root", C.c_uint32), ("size", C.c_uint32), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("sum_q", C.c_int64 * 3)]


QN_CLUSTER_REJECTED, QN_CLUSTER_NONE = -1, -2
assert (C.sizeof(ClusterParams), C.sizeof(ClusterStats), C.sizeof(ClusterInfo)) == (24, 56, 56)             # the records of include/qn_engine.h


class LocalizeParams(_Twinned, C.Structure):
    """qn_localize_params (32 bytes): the crop radius around the guess, the scan's voxel leaf, the score threshold and the crop shape (QN_LOCALIZE_SPHERE /
    QN_LOCALIZE_CYLINDER); the defaults are config.yaml's radius, voxel and score."""
    TWIN = ("maplocalize", "LocalizeParams")
    _fields_ = [("radius", C.c_double), ("leaf", C.c_double), ("score_thr", C.c_double), ("shape", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, radius=35.0, leaf=0.3, score_thr=1.5, shape=0):
        super().__init__(radius, leaf, score_thr, shape, 0)


class LocalizeStats(C.Structure):
    """qn_localize_stats (40 bytes)"""
    _fields_ = ([(f, C.c_uint32) for f in ("n_map", "n_pairs", "n_scans", "n_crops", "passes", "reserved")] + [("crop_points", C.c_uint64), ("generation", C.c_uint64)])


QN_LOCALIZE_SPHERE, QN_LOCALIZE_CYLINDER = 0, 1
assert (C.sizeof(LocalizeParams), C.sizeof(LocalizeStats)) == (32, 40)                                      # the records of include/qn_engine.h


def _verify_out(n):
    """the output arrays of a verification call over n pairs: records, valid, status, T_total, T_quatro (at least one entry each)"""
    m = max(n, 1)
    return (GicpResult * m)(), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 4, 4)), np.zeros((m, 4, 4))


def _yaw_arg(yaw, n, msg):
    """the optional per-pair yaw list as the C argument: None, or n doubles (ValueError(msg % (n, len)) otherwise)"""
    if yaw is None:
        return None
    y = np.ascontiguousarray(np.atleast_1d(yaw), dtype=np.float64)
    if len(y) != n:
        raise ValueError(msg % (n, len(y)))
    return _p(y)


def _gicp_dicts(results, valid, status, n):
    """one dict per pair of a GICP-form verification: T = the f32 record as f64"""
    return [dict(valid=bool(valid[j]), converged=bool(results[j].converged), score=results[j].fitness, iterations=results[j].iterations,
                 T=np.array(results[j].T, dtype=np.float32).reshape(4, 4).astype(np.float64), status=int(status[j]), record=results[j]) for j in range(n)]


def _c2f_dicts(results, Tt, Tq, valid, status, n):
    """one dict per pair of a coarse-to-fine verification: T = T_gicp * T_quatro"""
    return [dict(valid=bool(valid[j]), converged=bool(results[j].converged), score=results[j].fitness, iterations=results[j].iterations, T=Tt[j].copy(),
                 T_quatro=Tq[j].copy(), T_gicp=np.array(results[j].T, dtype=np.float32).reshape(4, 4).astype(np.float64), status=int(status[j]),
                 record=results[j]) for j in range(n)]


class KeyframeStore:
    """Device-resident keyframe clouds + LoopClosure::setSrcAndDstCloud on the GPU (loop_closure.cpp:58-108)."""

    def __init__(self, device=0):
        self._l = lib(); h = C.c_void_p()
        st = self._l.qn_kf_store_create(C.c_int(device), C.byref(h))
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode())
        self.h = h
        self._l.qn_kf_last_error.restype = C.c_char_p; self._l.qn_kf_last_error.argtypes = [C.c_void_p]
        self._l.qn_kf_store_destroy.argtypes = [C.c_void_p]
        self._sizes = {}                                             # keyframe id -> number of points (for keyframe())

    def close(self):
        if getattr(self, "h", None):
            self._l.qn_kf_store_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode() + ": " + self._l.qn_kf_last_error(self.h).decode())

    def _raise(self, st, ctx):
        """_check for a call that took a context as well: the message carries the store's and the context's side"""
        if st != QN_OK:
            raise EngineError(st, self._l.qn_status_str(st).decode() + ": " + self._l.qn_kf_last_error(self.h).decode() + " / " + lib().qn_last_error(ctx.h).decode())

    # ---- what the wrappers below share (everything a helper does not fit stays written out in its wrapper)
    @staticmethod
    def _ids_poses(ids, poses):
        """the list build_map takes: ids (count,) int32 and one 4x4 f64 per id as (count, 16)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        return ids, np.ascontiguousarray(poses, dtype=np.float64).reshape(len(ids), 16)

    def _slot(self, call, *args, kept=None):
        """a call that replaces the map slot and reports it through (ptr, n) outputs -> (device address, count), _map_n following.  kept: the failure statuses
        that leave the slot as it was (None: all of them); any other failure empties it"""
        ptr = C.c_void_p(); n = C.c_uint32()
        st = call(self.h, *args, C.byref(ptr), C.byref(n))
        if st != QN_OK and kept is not None and st not in kept:
            self._map_n = 0
        self._check(st)
        self._map_n = n.value
        return ptr.value, n.value

    def _read_float4(self, ptr, n, who):
        """the n float4 records at the device address ptr -> (n, 4) float32"""
        out = np.zeros((n, 4), np.float32)
        if n and self._l.hipMemcpy(out.ctypes.data, ptr, 16 * n, 2) != 0:
            raise EngineError(QN_ERR_HIP, who + ": read-back failed")
        return out

    def _grid(self, call, n_arrays, params=None):
        """the first half of a *_grid getter: the call without its n_arrays arrays -> (the occupancy grid's record, the call's leading arguments: the grid and,
        where the call has one, the params record it fills)"""
        g = OccupancyGrid()
        head = [C.byref(g)] + ([] if params is None else [C.byref(params)])
        self._check(call(self.h, *head, *[None] * n_arrays))
        return g, head

    def _volume(self, call, dtypes, params=None, planar=False):
        """a *_grid getter: ask for the grid, allocate (at least one element), ask again -> (info, [params dict,] one (D, H, W) array per dtype); planar: the field
        is one layer when the returned params say so"""
        g, head = self._grid(call, len(dtypes), params)
        W, H, D = int(g.width), int(g.height), int(g.depth)
        if planar and params.planar:
            D = 1 if W * H else 0
        n = W * H * D
        out = [np.zeros(max(n, 1), dt) for dt in dtypes]
        self._check(call(self.h, *head, *[_p(a) for a in out]))
        return (_as_dict(g),) + (() if params is None else (_as_dict(params),)) + tuple(a[:n].reshape(D, H, W) for a in out)

    def _slice(self, g, call, iz_lo, iz_hi, dtype):
        """a *_slice getter over the grid g of _grid: one value per column over the layers iz_lo .. iz_hi -> (H, W)"""
        W, H = int(g.width), int(g.height)
        out = np.zeros(max(W * H, 1), dtype)
        self._check(call(self.h, C.c_int32(int(iz_lo)), C.c_int32(int(iz_hi)), _p(out)))
        return out[:W * H].reshape(H, W)

    def _count(self, call, n_arrays):
        """the capacity probe of a list getter: the call with no room for its n_arrays arrays -> the rows it would write (QN_ERR_CAPACITY says that there are some)"""
        cnt = C.c_uint32()
        st = call(self.h, *[None] * n_arrays, C.c_uint32(0), C.byref(cnt))
        if st != QN_ERR_CAPACITY:
            self._check(st)
        return int(cnt.value)

    def _listed(self, call, *columns):
        """a list getter: probe, allocate (at least one row), ask again -> one array per column (the shape of a row, dtype), cut to the rows written"""
        n = self._count(call, len(columns))
        out = [np.zeros((max(n, 1),) + tuple(shape), dt) for shape, dt in columns]
        cnt = C.c_uint32()
        self._check(call(self.h, *[_p(a) for a in out], C.c_uint32(max(n, 1)), C.byref(cnt)))
        return [a[:cnt.value] for a in out]

    def add(self, xyz, intensity=None):
        """intensity (n,) given: qn_kf_add_xyzi, the keyframe carries it into build_map; otherwise qn_kf_add (intensity 0 in the map)."""
        kid = C.c_int32()
        if intensity is None:
            a, n, stride = _cloud_arg(xyz)
            self._check(self._l.qn_kf_add(self.h, _p(a), C.c_uint32(n), C.c_uint32(stride), C.byref(kid)))
            self._sizes[kid.value] = n
            return kid.value
        xyz = np.asarray(xyz, dtype=np.float32); intensity = np.asarray(intensity, dtype=np.float32).reshape(-1)
        if xyz.ndim != 2 or xyz.shape[1] < 3 or len(intensity) != len(xyz):
            raise ValueError("cloud must be (n, >=3) float32 with n intensities")
        a = np.empty((len(xyz), 4), np.float32); a[:, :3] = xyz[:, :3]; a[:, 3] = intensity
        self._check(self._l.qn_kf_add_xyzi(self.h, _p(a), C.c_uint32(len(a)), C.c_uint32(16), C.c_uint32(12), C.byref(kid)))
        self._sizes[kid.value] = len(a)
        return kid.value

    def add_device(self, ptr, n, stride, intensity_offset=None):
        """qn_kf_add_device: a keyframe from n records in device memory at `ptr` (an int address, e.g. tensor.data_ptr(); the producer's
        stream must be synchronised): xyz at byte 0 of each `stride`-byte record, intensity at `intensity_offset` (None: xyz only, as add)."""
        kid = C.c_int32()
        ioff = -1 if intensity_offset is None else int(intensity_offset)
        self._check(self._l.qn_kf_add_device(self.h, C.c_void_p(ptr), C.c_uint32(n), C.c_uint32(stride), C.c_int32(ioff), C.byref(kid)))
        self._sizes[kid.value] = int(n)
        return kid.value

    def add_lidar_scans(self, prims, sensor, poses, seeds):
        """qn_sim_lidar_to_store: ray-cast one spinning-LiDAR scan (synth.SpinningLidar) of the primitives (synth.PRIM_DTYPE) per pose
        (sensor -> world 4x4) and seed, on the GPU, each straight into the store as an intensity keyframe -> ids (consecutive).
        Each keyframe equals synth.lidar_scan(prims, sensor, pose, seed) bit for bit."""
        from . import synth
        prims = np.ascontiguousarray(prims, dtype=synth.PRIM_DTYPE).reshape(-1)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        if len(seeds) != len(poses):
            raise ValueError("add_lidar_scans: %d poses but %d seeds" % (len(poses), len(seeds)))
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in sensor.tables()]
        sen = SimSensor(sensor.n_beams, sensor.n_cols, *[t.ctypes.data for t in tabs], sensor.min_range, sensor.max_range, sensor.sigma)
        S = len(poses)
        ids = np.zeros(max(S, 1), np.int32); n = np.zeros(max(S, 1), np.uint32)
        self._check(self._l.qn_sim_lidar_to_store(self.h, _p(prims) if len(prims) else None, C.c_uint32(len(prims)), C.byref(sen), _p(poses),
                                                  _p(seeds), C.c_uint32(S), _p(ids), _p(n)))
        self._sizes.update(zip(ids[:S].tolist(), n[:S].tolist()))
        return ids[:S].copy()

    def keyframe(self, kid):
        """-> (n, 4) float32: the resident records of keyframe `kid` (x y z, intensity or 1), qn_kf_download_keyframe"""
        n = self._sizes.get(int(kid))
        if n is None:
            raise ValueError("keyframe(%d): no such keyframe in this store" % kid)
        out = np.zeros((n, 4), np.float32)
        self._check(self._l.qn_kf_download_keyframe(self.h, C.c_int32(kid), _p(out)))
        return out

    def assemble(self, ids, poses, leaf, slot):
        """-> (device pointer of float4 points, count)"""
        ids, poses = self._ids_poses(ids, poses)
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_assemble(self.h, _p(ids), _p(poses), C.c_uint32(len(ids)), C.c_double(leaf), C.c_int(slot), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def download(self, slot, n):
        out = np.zeros((n, 3), np.float32)
        self._check(self._l.qn_kf_download(self.h, C.c_int(slot), _p(out)))
        return out

    def build_map(self, ids, poses, leaf):
        """qn_kf_build_map: the corrected global map (transform every listed keyframe, concatenate in `ids` order, voxel grid with
        intensity) into the store's own map slot -> number of map points."""
        ids, poses = self._ids_poses(ids, poses)
        return self._slot(self._l.qn_kf_build_map, _p(ids), _p(poses), C.c_uint32(len(ids)), C.c_double(leaf), kept=())[1]

    def download_map(self, n):
        """-> (n, 4) float32: x y z intensity of the latest build_map"""
        if n != getattr(self, "_map_n", 0):
            raise ValueError("download_map(%d): the map holds %d points" % (n, getattr(self, "_map_n", 0)))
        out = np.zeros((n, 4), np.float32)
        self._check(self._l.qn_kf_download_map(self.h, _p(out), C.c_uint32(16), C.c_uint32(12)))
        return out

    def assemble_batch(self, lists, poses, leaf):
        """qn_kf_assemble_batch: submap s = lists[s] transformed with poses[s] (one 4x4 per entry), concatenated, voxel grid at `leaf`, all
        submaps in one pass into the store's batch slot -> [(device pointer of float4 points, count, status)] per submap.  Each equals
        assemble() of the same list; a submap with no finite point has status QN_ERR_EMPTY_CLOUD.  Valid until the next assemble_batch."""
        lists = [np.asarray(l, dtype=np.int32).reshape(-1) for l in lists]
        if len(poses) != len(lists):
            raise ValueError("assemble_batch: %d lists but %d pose lists" % (len(lists), len(poses)))
        seg = np.zeros(len(lists) + 1, np.uint32); seg[1:] = np.cumsum([len(l) for l in lists])
        ids = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, np.int32), dtype=np.int32)
        T = np.zeros((max(len(ids), 1), 16), np.float64)
        for l, P, a in zip(lists, poses, seg[:-1]):
            T[a:a + len(l)] = np.asarray(P, dtype=np.float64).reshape(len(l), 16)
        S = len(lists)
        ptrs = (C.c_void_p * max(S, 1))(); n = np.zeros(max(S, 1), np.uint32); st = np.zeros(max(S, 1), np.int32)
        self._batch_n = []
        self._check(self._l.qn_kf_assemble_batch(self.h, _p(ids), _p(T), _p(seg), C.c_uint32(S), C.c_double(leaf), ptrs, _p(n), _p(st)))
        self._batch_n = [int(v) for v in n[:S]]
        return [(ptrs[s], int(n[s]), int(st[s])) for s in range(S)]

    def download_batch(self, seg, n):
        """-> (n, 3) float32: submap `seg` of the latest assemble_batch"""
        have = self._batch_n[seg] if seg < len(getattr(self, "_batch_n", [])) else None
        if n != have:
            raise ValueError("download_batch(%d, %d): the submap holds %s points" % (seg, n, have))
        out = np.zeros((n, 3), np.float32)
        self._check(self._l.qn_kf_download_batch(self.h, C.c_uint32(seg), _p(out)))
        return out

    def loop_submap_pairs(self, poses, query, candidates, submap_range, leaf, enable_quatro=True, enable_submap_matching=False):
        """LoopClosure::setSrcAndDstCloud for one query and K candidates in ONE assemble_batch: the query's submap once, one submap per candidate.
        Store ids are keyframe indices; poses[i] = keyframe i's corrected pose, len(poses) keyframes exist.  -> (pairs, status): pairs[k] =
        (src_ptr, ns, dst_ptr, nt, 16, 1) for gicp_align_batch / coarse_to_fine_align_batch, every pair naming the same source buffer (the batch
        prepares it once); status = [query submap's] + [each candidate submap's]."""
        n_kf = len(poses)
        src = loop_submap_ids(query, query, submap_range, enable_quatro, enable_submap_matching, n_kf)[0]
        lists = [src] + [loop_submap_ids(query, c, submap_range, enable_quatro, enable_submap_matching, n_kf)[1] for c in candidates]
        out = self.assemble_batch(lists, [[poses[i] for i in l] for l in lists], leaf)
        (sp, ns, _), rest = out[0], out[1:]
        return [(sp, ns, dp, nt, 16, 1) for dp, nt, _ in rest], [o[2] for o in out]


    def verify_loop_candidates(self, ctx, query, candidates, yaw, poses, submap_range, leaf, score_thr=1.5):
        """qn_kf_verify_loop_candidates: the query scan in its own sensor frame against each candidate's scan-to-submap window in the candidate's sensor
        frame (keyframe i with scancontext.relative_pose(P_c, P_i)), every pair seeded with scancontext.seed_from_yaw(yaw[j]), all K in ONE batched
        registration on ctx (its NanoGICP parameters).  yaw: per candidate, the candidate's heading minus the query's (scancontext.yaw_of_shift of
        sc_query's shift), or None for 0.  poses[i] = keyframe i's corrected pose.  The store's batch slot holds the clouds afterwards (download_batch:
        segment 0 the source, 1 + j candidate j).  -> one dict per candidate: valid, converged, score, T (inv(P_c) P_query estimate, the f32 record
        as f64), status (QN_ERR_EMPTY_CLOUD for an empty candidate submap)."""
        cand = np.ascontiguousarray(np.atleast_1d(candidates), dtype=np.int32)
        K = len(cand)
        y = _yaw_arg(yaw, K, "verify_loop_candidates: %d candidates but %d yaw values")
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
        results, valid, status, _, _ = _verify_out(K)
        st = self._l.qn_kf_verify_loop_candidates(self.h, ctx.h, C.c_int32(query), _p(cand) if K else None, y, C.c_uint32(K),
                                                  _p(P), C.c_uint32(len(P)), C.c_uint32(submap_range), C.c_double(leaf), C.c_double(score_thr),
                                                  results, _p(valid), _p(status))
        self._raise(st, ctx)
        self._batch_n = []
        for seg in range(K + 1):
            n = C.c_uint32()
            self._check(self._l.qn_kf_batch_count(self.h, C.c_uint32(seg), C.byref(n)))
            self._batch_n.append(n.value)
        return _gicp_dicts(results, valid, status, K)

    # ---- resident Quatro descriptors and the drift-free coarse-to-fine check (qn_kf_quatro_*, qn_kf_verify_loop_candidates_c2f)
    def quatro_describe(self, ctx, ids, leaf):
        """qn_kf_quatro_describe: each keyframe alone in its sensor frame, voxel grid at `leaf` (= assemble([id], [eye(4)], leaf)), and its FPFH rows with
        ctx's Quatro radii, kept resident in the store (describing again replaces) -> per id its status (QN_ERR_EMPTY_CLOUD: nothing left after the voxel grid)."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        st = np.zeros(max(len(ids), 1), np.int32)
        self._check(self._l.qn_kf_quatro_describe(self.h, ctx.h, _p(ids) if len(ids) else None, C.c_uint32(len(ids)), C.c_double(leaf), _p(st)))
        return [int(v) for v in st[:len(ids)]]

    def quatro_cloud(self, kid):
        """-> (device pointer of the described float4 cloud (None when empty), count)"""
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_quatro_cloud(self.h, C.c_int32(kid), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def quatro_features(self, kid):
        """-> (n, 33) float32: the described FPFH rows of keyframe `kid` (original point order; NaN rows where PCL has none)"""
        _, n = self.quatro_cloud(kid)
        out = np.zeros((n, 33), np.float32)
        self._check(self._l.qn_kf_quatro_features(self.h, C.c_int32(kid), _p(out) if n else None))
        return out

    def verify_loop_candidates_c2f(self, ctx, query, candidates, score_thr=1.5):
        """qn_kf_verify_loop_candidates_c2f: the query's described cloud against each candidate's, coarse to fine (Quatro -> transformPcd -> Nano-GICP,
        loop_closure.cpp:138-159) on ctx's lanes, the features borrowed from the store.  No pose is involved.  -> one dict per candidate as
        coarse_to_fine_align_batch's: valid, converged, score, iterations, T (T_gicp * T_quatro: estimates inv(P_c) P_query), T_quatro, T_gicp, status."""
        cand = np.ascontiguousarray(np.atleast_1d(candidates), dtype=np.int32)
        K = len(cand)
        results, valid, status, Tt, Tq = _verify_out(K)
        st = self._l.qn_kf_verify_loop_candidates_c2f(self.h, ctx.h, C.c_int32(query), _p(cand) if K else None, C.c_uint32(K), C.c_double(score_thr),
                                                      results, _p(Tt), _p(Tq), _p(valid), _p(status))
        self._raise(st, ctx)
        return _c2f_dicts(results, Tt, Tq, valid, status, K)

    # ---- many queries in one verification (qn_kf_verify_loop_pairs[_c2f]) and the debug clouds of a verified pair (qn_kf_verify_cloud)
    @staticmethod
    def _pairs(query, cand):
        q = np.ascontiguousarray(np.atleast_1d(query), dtype=np.int32); c = np.ascontiguousarray(np.atleast_1d(cand), dtype=np.int32)
        if len(q) != len(c):
            raise ValueError("%d queries but %d candidates" % (len(q), len(c)))
        return q, c, len(q)

    def verify_loop_pairs(self, ctx, query, cand, yaw, poses, submap_range, leaf, score_thr=1.5):
        """qn_kf_verify_loop_pairs: pair j = (query[j], cand[j], yaw[j]) checked as verify_loop_candidates(ctx, query[j], [cand[j]], [yaw[j]], ...) would,
        record for record, but every pair in ONE assembly (each distinct query scan and each distinct candidate window once) and ONE batched registration.
        yaw None: all 0.  The store's batch slot holds the distinct queries (order of first appearance), then the distinct candidates' windows
        (download_batch).  -> one dict per pair, as verify_loop_candidates'."""
        q, c, n = self._pairs(query, cand)
        y = _yaw_arg(yaw, n, "verify_loop_pairs: %d pairs but %d yaw values")
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
        results, valid, status, _, _ = _verify_out(n)
        st = self._l.qn_kf_verify_loop_pairs(self.h, ctx.h, _p(q) if n else None, _p(c) if n else None, y, C.c_uint32(n),
                                             _p(P), C.c_uint32(len(P)), C.c_uint32(submap_range), C.c_double(leaf), C.c_double(score_thr),
                                             results, _p(valid), _p(status))
        self._raise(st, ctx)
        self._batch_n = []
        for seg in range(len(dict.fromkeys(q.tolist())) + len(dict.fromkeys(c.tolist()))):
            m = C.c_uint32()
            self._check(self._l.qn_kf_batch_count(self.h, C.c_uint32(seg), C.byref(m)))
            self._batch_n.append(m.value)
        return _gicp_dicts(results, valid, status, n)

    def verify_loop_pairs_c2f(self, ctx, query, cand, score_thr=1.5):
        """qn_kf_verify_loop_pairs_c2f: pair j checked as verify_loop_candidates_c2f(ctx, query[j], [cand[j]]) would, record for record, all pairs in one run
        of the batched coarse-to-fine lanes on ctx (both sides borrowed from the described keyframes).  -> one dict per pair, as verify_loop_candidates_c2f's."""
        q, c, n = self._pairs(query, cand)
        results, valid, status, Tt, Tq = _verify_out(n)
        st = self._l.qn_kf_verify_loop_pairs_c2f(self.h, ctx.h, _p(q) if n else None, _p(c) if n else None, C.c_uint32(n), C.c_double(score_thr),
                                                 results, _p(Tt), _p(Tq), _p(valid), _p(status))
        self._raise(st, ctx)
        return _c2f_dicts(results, Tt, Tq, valid, status, n)

    # ---- resident local submaps and the submap-to-submap check (qn_kf_submap_*, qn_kf_verify_loop_pairs_submap[_c2f])
    def submap_describe(self, ctx, ids, poses, submap_range, leaf, with_features=True):
        """qn_kf_submap_describe: for each listed keyframe c its local submap in c's own sensor frame - the keyframes local_submap_ids(c, submap_range,
        len(poses)), keyframe i with scancontext.relative_pose(poses[c], poses[i]), voxel grid at `leaf` (= assemble_batch of that list) - and, with_features,
        its FPFH rows with ctx's Quatro radii; both stay resident in the store (describing again replaces).  -> per id its status (QN_ERR_EMPTY_CLOUD: nothing
        left after the voxel grid; QN_ERR_CAPACITY: more points than ctx takes, no entry)."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
        st = np.zeros(max(len(ids), 1), np.int32)
        rc = self._l.qn_kf_submap_describe(self.h, ctx.h, _p(ids) if len(ids) else None, C.c_uint32(len(ids)), _p(P) if len(P) else None, C.c_uint32(len(P)),
                                           C.c_uint32(submap_range), C.c_double(leaf), C.c_int(1 if with_features else 0), _p(st))
        self._raise(rc, ctx)
        return [int(v) for v in st[:len(ids)]]

    def submap_cloud(self, kid):
        """-> (device pointer of keyframe `kid`'s resident local submap, float4 records (None when empty), count)"""
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_submap_cloud(self.h, C.c_int32(kid), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def submap_features(self, kid):
        """-> (n, 33) float32: the FPFH rows of keyframe `kid`'s local submap (original point order; NaN rows where PCL has none)"""
        _, n = self.submap_cloud(kid)
        out = np.zeros((n, 33), np.float32)
        self._check(self._l.qn_kf_submap_features(self.h, C.c_int32(kid), _p(out) if n else None))
        return out

    def submap_release(self, ids=None):
        """qn_kf_submap_release: free the local submaps of these keyframes (None: of all)"""
        if ids is None:
            self._check(self._l.qn_kf_submap_release(self.h, None, C.c_uint32(0)))
            return
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        self._check(self._l.qn_kf_submap_release(self.h, _p(ids) if len(ids) else None, C.c_uint32(len(ids))))

    def verify_loop_pairs_submap(self, ctx, query, cand, yaw=None, score_thr=1.5):
        """qn_kf_verify_loop_pairs_submap: pair j = query[j]'s resident local submap (source) against cand[j]'s (target), seeded with
        scancontext.seed_from_yaw(yaw[j]) (None: 0), every pair in ONE batched registration on ctx = gicp_align_batch(..., guesses=) on the entry clouds,
        record for record.  -> one dict per pair, as verify_loop_pairs'."""
        q, c, n = self._pairs(query, cand)
        y = _yaw_arg(yaw, n, "verify_loop_pairs_submap: %d pairs but %d yaw values")
        results, valid, status, _, _ = _verify_out(n)
        st = self._l.qn_kf_verify_loop_pairs_submap(self.h, ctx.h, _p(q) if n else None, _p(c) if n else None, y, C.c_uint32(n),
                                                    C.c_double(score_thr), results, _p(valid), _p(status))
        self._raise(st, ctx)
        return _gicp_dicts(results, valid, status, n)

    def verify_loop_pairs_submap_c2f(self, ctx, query, cand, score_thr=1.5):
        """qn_kf_verify_loop_pairs_submap_c2f: pair j coarse to fine (Quatro -> transformPcd -> Nano-GICP) between the two resident local submaps, the lanes
        borrowing their points and FPFH rows = coarse_to_fine_align_batch([ctx]) on the entry clouds, record for record.  -> one dict per pair, as
        verify_loop_pairs_c2f's."""
        q, c, n = self._pairs(query, cand)
        results, valid, status, Tt, Tq = _verify_out(n)
        st = self._l.qn_kf_verify_loop_pairs_submap_c2f(self.h, ctx.h, _p(q) if n else None, _p(c) if n else None, C.c_uint32(n), C.c_double(score_thr),
                                                        results, _p(Tt), _p(Tq), _p(valid), _p(status))
        self._raise(st, ctx)
        return _c2f_dicts(results, Tt, Tq, valid, status, n)

    def verify_loop_candidates_submap(self, ctx, query, candidates, yaw=None, score_thr=1.5):
        """one query's candidates, submap against submap: verify_loop_pairs_submap with the query repeated"""
        cand = np.atleast_1d(candidates)
        return self.verify_loop_pairs_submap(ctx, [query] * len(cand), cand, yaw, score_thr)

    def verify_loop_candidates_submap_c2f(self, ctx, query, candidates, score_thr=1.5):
        """one query's candidates, submap against submap, coarse to fine: verify_loop_pairs_submap_c2f with the query repeated"""
        cand = np.atleast_1d(candidates)
        return self.verify_loop_pairs_submap_c2f(ctx, [query] * len(cand), cand, score_thr)

    def verify_cloud(self, pair, which):
        """qn_kf_verify_cloud: cloud `which` (QN_VERIFY_SRC / _DST / _COARSE / _FINAL) of pair `pair` of the latest verify_loop_pairs[_c2f] -> (n, 3) float32"""
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_verify_cloud(self.h, C.c_uint32(pair), C.c_int(which), C.byref(ptr), C.byref(n)))
        return np.ascontiguousarray(self._read_float4(ptr, n.value, "verify_cloud")[:, :3])

    # ---- the two-way overlap of cloud pairs (qn_kf_overlap_batch / qn_kf_verify_overlap / qn_kf_overlap_points; numpy twin: qn_amd/overlap.py)
    @staticmethod
    def _overlap_records(out, status, n):
        return [dict(_as_dict(out[j]), status=int(status[j])) for j in range(n)]

    def overlap_batch(self, pairs, radius):
        """qn_kf_overlap_batch: pairs = [(ptr_a, n_a, ptr_b, n_b), ...], device pointers (int addresses) of float4 records in one frame -> one dict per pair:
        a_to_b / b_to_a (each n, n_finite, inliers, sum_d2, as overlap.direction's) and status (QN_ERR_EMPTY_CLOUD for a pair with an empty side: a zero
        record).  overlap.overlap_fraction / overlap.inlier_rmse take a direction dict."""
        pairs = list(pairs); n = len(pairs)
        if any(len(p) != 4 for p in pairs):
            raise ValueError("overlap_batch: a pair is (ptr_a, n_a, ptr_b, n_b)")
        pa = (C.c_void_p * max(n, 1))(*[p[0] for p in pairs]); pb = (C.c_void_p * max(n, 1))(*[p[2] for p in pairs])
        na = np.array([p[1] for p in pairs] or [0], np.uint32); nb = np.array([p[3] for p in pairs] or [0], np.uint32)
        out = (Overlap * max(n, 1))(); status = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_overlap_batch(self.h, pa, _p(na), pb, _p(nb), C.c_uint32(n), C.c_double(radius), out, _p(status)))
        self._overlap_n = [(int(p[1]), int(p[3])) if status[j] == QN_OK else (0, 0) for j, p in enumerate(pairs)]
        return self._overlap_records(out, status, n)

    def verify_overlap(self, radius, pairs=None, n_pairs=None):
        """qn_kf_verify_overlap: pair j of the latest verify_loop_pairs[_c2f] / _submap[_c2f] call, A = its QN_VERIFY_FINAL cloud against B = its QN_VERIFY_DST
        cloud.  pairs None: all n_pairs pairs of that call (n_pairs = how many it had).  -> one dict per listed pair, as overlap_batch's (status QN_ERR_NOT_READY
        for a pair whose registration did not run)."""
        if pairs is None:
            if n_pairs is None:
                raise ValueError("verify_overlap: give the pair indices, or n_pairs of the verify call for all of them")
            idx = None; n = int(n_pairs)
        else:
            idx = np.ascontiguousarray(np.atleast_1d(pairs), dtype=np.uint32); n = len(idx)
        out = (Overlap * max(n, 1))(); status = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_verify_overlap(self.h, _p(idx) if idx is not None and n else None, C.c_uint32(n), C.c_double(radius), out, _p(status)))
        self._overlap_n = [(int(out[j].a_to_b.n), int(out[j].b_to_a.n)) for j in range(n)]
        return self._overlap_records(out, status, n)

    def overlap_points(self, pair_slot, direction):
        """qn_kf_overlap_points: the per-point results of the latest overlap_batch / verify_overlap for its pair `pair_slot`, direction 0 (A against B) or
        1 (B against A) -> nn_d2 (n,) float32 (+inf: no partner within the radius), nn_idx (n,) int32 (-1)"""
        sizes = getattr(self, "_overlap_n", None)
        if sizes is None or not 0 <= int(pair_slot) < len(sizes) or direction not in (0, 1):
            raise ValueError("overlap_points: no such pair or direction in the latest overlap call")
        n = sizes[int(pair_slot)][direction]
        d2 = np.zeros(max(n, 1), np.float32); idx = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_overlap_points(self.h, C.c_uint32(pair_slot), C.c_int(direction), _p(d2), _p(idx)))
        return d2[:n].copy(), idx[:n].copy()

    # ---- range images and the free-space check of loop pairs (qn_kf_range_* / qn_kf_freespace_*; numpy twin: qn_amd/freespace.py)
    def range_set_params(self, params=None, **kw):
        """qn_kf_range_set_params: a RangeParams (or a freespace.Params), or its fields as keywords (the rest default).  A change of the shape, the angles or
        min_range discards every image."""
        p = RangeParams(**kw) if params is None else _record(RangeParams, params)
        self._check(self._l.qn_kf_range_set_params(self.h, C.byref(p)))

    def range_params(self):
        p = RangeParams()
        self._check(self._l.qn_kf_range_get_params(self.h, C.byref(p)))
        return p

    def range_describe(self, ids):
        """qn_kf_range_describe: the near / far range images of these keyframes, on the GPU from their resident records (describing again replaces)
        -> per id its status (QN_ERR_EMPTY_CLOUD: no kept point, an all-empty image)"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        status = np.zeros(max(len(ids), 1), np.int32)
        self._check(self._l.qn_kf_range_describe(self.h, _p(ids) if len(ids) else None, C.c_uint32(len(ids)), _p(status)))
        return [int(v) for v in status[:len(ids)]]

    def range_images(self, kid):
        """-> (near, far), each (n_rows, n_cols) float32, of a described keyframe (qn_kf_range_get)"""
        p = self.range_params()
        near = np.zeros((p.n_rows, p.n_cols), np.float32); far = np.zeros((p.n_rows, p.n_cols), np.float32)
        self._check(self._l.qn_kf_range_get(self.h, C.c_int32(kid), _p(near), _p(far)))
        return near, far

    def freespace_batch(self, query, cand, T):
        """qn_kf_freespace_batch: pair j = (query[j], cand[j], T[j]), T[j] the 4x4 f64 that maps the query's sensor frame into the candidate's (what the
        verify calls estimate) -> one dict per pair: q_in_c / c_in_q (each n, n_finite, in_fov, observed, seen_through, occluded, agree, as
        freespace.direction's) and status.  freespace.see_through_fraction takes a direction dict."""
        q, c, n = self._pairs(query, cand)
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(-1, 16))
        if len(T) != n:
            raise ValueError("freespace_batch: %d pairs but %d transforms" % (n, len(T)))
        out = (Freespace * max(n, 1))(); status = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_freespace_batch(self.h, _p(q) if n else None, _p(c) if n else None, _p(T) if n else None, C.c_uint32(n), out, _p(status)))
        self._freespace_n = [(int(out[j].q_in_c.n), int(out[j].c_in_q.n)) for j in range(n)]
        return [dict(_as_dict(out[j]), status=int(status[j])) for j in range(n)]

    def freespace_points(self, pair_slot, direction):
        """qn_kf_freespace_points: the class byte of every record (freespace.DROPPED .. AGREE) of the latest freespace_batch for its pair `pair_slot`,
        direction 0 (the query's records in the candidate's images) or 1 -> (n,) uint8"""
        sizes = getattr(self, "_freespace_n", None)
        if sizes is None or not (0 <= pair_slot < len(sizes)) or direction not in (0, 1):
            raise ValueError("freespace_points: no such pair or direction in the latest freespace call")
        out = np.zeros(max(sizes[pair_slot][direction], 1), np.uint8)
        self._check(self._l.qn_kf_freespace_points(self.h, C.c_uint32(pair_slot), C.c_int(direction), _p(out)))
        return out[:sizes[pair_slot][direction]]

    # ---- the static map: the corrected map without the records other keyframes saw through (qn_kf_static_* / qn_kf_build_map_static; twin: qn_amd/staticmap.py)
    def static_classify(self, ids, poses, witnesses=None, radius=15.0, max_k=8, params=None):
        """qn_kf_static_classify: every record of every listed keyframe (the list and the corrected poses build_map takes) against the range images of its
        entry's witnesses, in one pass.  witnesses = (wit_off, wit), entry positions in CSR form; None: staticmap.witnesses(ids, poses, radius, max_k), the
        up to max_k nearest entries of another keyframe within radius.  The witnesses' keyframes must have range images (range_describe).  params: a
        StaticParams (or a staticmap.StaticParams); None: the defaults (2, 1).  -> dict(removed (count,) uint32, status (count,) list, wit_off, wit).
        The votes stay resident for static_points / build_map_static until the next successful call."""
        from . import staticmap
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n = len(ids)
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
        if len(poses) != n:
            raise ValueError("static_classify: %d entries but %d poses" % (n, len(poses)))
        if witnesses is None:
            witnesses = staticmap.witnesses(ids, poses, radius, max_k)
        off = np.ascontiguousarray(witnesses[0], dtype=np.uint32).reshape(-1); wit = np.ascontiguousarray(witnesses[1], dtype=np.uint32).reshape(-1)
        if len(off) != n + 1 or (n and int(off[-1]) > len(wit)):
            raise ValueError("static_classify: wit_off must be count + 1 offsets into wit")
        p = _record(StaticParams, params)
        removed = np.zeros(max(n, 1), np.uint32); status = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_static_classify(self.h, _p(ids) if n else None, _p(poses) if n else None, C.c_uint32(n), _p(off), _p(wit) if len(wit) else None,
                                                  C.byref(p), _p(removed), _p(status)))
        self._static_n = [self._sizes.get(int(i)) for i in ids]
        return dict(removed=removed[:n].copy(), status=[int(v) for v in status[:n]], wit_off=off, wit=wit)

    def static_points(self, entry):
        """qn_kf_static_points: the votes of every record of entry `entry` of the latest static_classify -> (seen_through, agree, removed), each (n,) uint8"""
        sizes = getattr(self, "_static_n", None)
        if sizes is None or not (0 <= entry < len(sizes)) or sizes[entry] is None:
            raise ValueError("static_points: no such entry in the latest static_classify")
        n = sizes[entry]
        out = [np.zeros(max(n, 1), np.uint8) for _ in range(3)]
        self._check(self._l.qn_kf_static_points(self.h, C.c_uint32(entry), _p(out[0]), _p(out[1]), _p(out[2])))
        return tuple(o[:n] for o in out)

    def build_map_static(self, leaf):
        """qn_kf_build_map_static: the static map of the latest static_classify - build_map of its list and poses without the removed records - into the
        store's map slot -> number of map points (download_map serves it).  May be called again with another leaf."""
        refused = (QN_ERR_NOT_READY, QN_ERR_INVALID_ARG)             # a refused call leaves the map slot as it was
        return self._slot(self._l.qn_kf_build_map_static, C.c_double(leaf), kept=refused)[1]

    # ---- normals and curvature of the map slot (qn_kf_map_normals / qn_kf_download_map_normals / qn_kf_map_moments; numpy twin: qn_amd/mapnormals.py)
    def map_normals(self, params=None, viewpoints=None):
        """qn_kf_map_normals on the map of the latest build_map / build_map_static, then its download.  params: a NormalParams (or a mapnormals.NormalParams);
        None: the defaults (0.6, 5).  viewpoints: (V, 3) f64 the normals are turned towards (the nearest one of each point; the corrected keyframe positions as
        a rule), None or empty: the largest component of each normal is made positive.  -> dict(normals (n, 3) f32, curvature (n,) f32, count (n,) uint32,
        view_idx (n,) int32, ptr (the device address of the n float4 records nx ny nz curvature)), equal to mapnormals.normals of the downloaded map."""
        p = _record(NormalParams, params)
        v = np.zeros((0, 3)) if viewpoints is None else np.ascontiguousarray(np.asarray(viewpoints, dtype=np.float64).reshape(-1, 3))
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_map_normals(self.h, C.byref(p), _p(v) if len(v) else None, C.c_uint32(len(v)), C.byref(ptr), C.byref(n)))
        self._normals_n = n.value
        out = np.zeros((max(n.value, 1), 4), np.float32); cnt = np.zeros(max(n.value, 1), np.uint32); view = np.zeros(max(n.value, 1), np.int32)
        self._check(self._l.qn_kf_download_map_normals(self.h, _p(out), _p(cnt), _p(view)))
        out = out[:n.value]
        return dict(normals=out[:, :3].copy(), curvature=out[:, 3].copy(), count=cnt[:n.value], view_idx=view[:n.value], ptr=ptr.value)

    def map_moments(self):
        """qn_kf_map_moments: the integer moments behind the latest map_normals -> (s1 (n, 3) int64, s2 (n, 6) int64)"""
        n = getattr(self, "_normals_n", None)
        if n is None:
            raise ValueError("map_moments: no map_normals call yet")
        s1 = np.zeros((max(n, 1), 3), np.int64); s2 = np.zeros((max(n, 1), 6), np.int64)
        self._check(self._l.qn_kf_map_moments(self.h, _p(s1), _p(s2)))
        return s1[:n], s2[:n]

    # ---- isolated noise points of the map slot (qn_kf_map_outliers / qn_kf_map_outlier_points / qn_kf_map_remove_outliers; numpy twin: qn_amd/mapoutliers.py)
    def map_outliers(self, params=None):
        """qn_kf_map_outliers on the map of the latest build_map / build_map_static, then its per-point download.  params: an OutlierParams (or a
        mapoutliers.OutlierParams); None: the defaults (1.0, 2.0, 8).  -> (stats, count (n,) uint32, mean_q (n,) uint32, removed (n,) uint8), equal to
        mapoutliers.classify of the downloaded map.  stats: a dict of the fields of qn_outlier_stats plus, in metres, mean, std and threshold (each the _q
        value times 2^-quant_exp).  The map slot is not touched; map_remove_outliers applies the result."""
        p = _record(OutlierParams, params)
        st = OutlierStats()
        self._check(self._l.qn_kf_map_outliers(self.h, C.byref(p), C.byref(st)))
        n = int(st.n)
        cnt = np.zeros(max(n, 1), np.uint32); mq = np.zeros(max(n, 1), np.uint32); rm = np.zeros(max(n, 1), np.uint8)
        self._check(self._l.qn_kf_map_outlier_points(self.h, _p(cnt), _p(mq), _p(rm)))
        stats = _as_dict(st)
        unit = math.ldexp(1.0, -int(st.quant_exp))
        stats.update(mean=st.mean_q * unit, std=st.std_q * unit, threshold=st.thr_q * unit)
        return stats, cnt[:n], mq[:n], rm[:n]

    def map_remove_outliers(self):
        """qn_kf_map_remove_outliers: the records the latest map_outliers kept become the map slot, in order -> (ptr, n): the device address of the n float4
        records x y z intensity.  download_map and map_normals serve the filtered map; the classification and any map normals are stale afterwards."""
        return self._slot(self._l.qn_kf_map_remove_outliers)

    # ---- the ground of the map slot and its occupancy grid (qn_kf_map_ground / _points / _grid / qn_kf_map_keep_classes; numpy twin: qn_amd/mapground.py)
    def map_ground(self, params=None):
        """qn_kf_map_ground on the map of the latest build or filter, then its per-point download.  params: a GroundParams (or a mapground.GroundParams); None:
        the defaults.  -> (stats, classes (n,) uint8, height_q (n,) int32), equal to mapground.classify of the downloaded map; stats: a dict of the fields of
        qn_ground_stats (rounds is the GPU's own).  The map slot is not touched; map_ground_grid serves the grid, map_keep_classes applies the classes."""
        p = _record(GroundParams, params)
        st = GroundStats()
        self._check(self._l.qn_kf_map_ground(self.h, C.byref(p), C.byref(st)))
        n = int(st.n)
        cls = np.zeros(max(n, 1), np.uint8); hq = np.zeros(max(n, 1), np.int32)
        self._check(self._l.qn_kf_map_ground_points(self.h, _p(cls), _p(hq)))
        return _as_dict(st), cls[:n], hq[:n]

    def map_ground_grid(self):
        """qn_kf_map_ground_grid -> (info, ground_q (H, W) int32, occupancy (H, W) uint8) of the latest map_ground: info a dict of origin_x, origin_y, cell, width,
        height, quant_exp; the arrays row-major with y the slow axis; ground_q in units of 2^-quant_exp m; occupancy 0 unknown, 1 free, 2 occupied."""
        g = GroundGrid()
        self._check(self._l.qn_kf_map_ground_grid(self.h, C.byref(g), None, None))
        W, H = int(g.width), int(g.height)
        gq = np.zeros(max(W * H, 1), np.int32); occ = np.zeros(max(W * H, 1), np.uint8)
        self._check(self._l.qn_kf_map_ground_grid(self.h, C.byref(g), _p(gq), _p(occ)))
        return _as_dict(g), gq[:W * H].reshape(H, W), occ[:W * H].reshape(H, W)

    def map_keep_classes(self, mask):
        """qn_kf_map_keep_classes: the records of the latest map_ground whose class bit (1 << class) is set in mask become the map slot, in order -> (ptr, n):
        the device address of the n float4 records x y z intensity.  download_map, map_normals and map_outliers serve the kept map; the ground results, any
        outlier classification and any map normals are stale afterwards."""
        return self._slot(self._l.qn_kf_map_keep_classes, C.c_uint32(int(mask) & 0xffffffff))

    # ---- a 3-D occupancy map by ray carving (qn_kf_map_occupancy / _grid / _list / _slice; numpy twin: qn_amd/mapoccupancy.py)
    def map_occupancy(self, ids, poses, params=None):
        """qn_kf_map_occupancy over the list build_map takes: every record of every listed keyframe is a ray from the entry's sensor position to the world point.
        params: an OccupancyParams (or a mapoccupancy.OccupancyParams); None: the defaults.  -> stats, a dict of the fields of qn_occupancy_stats, equal to
        those of mapoccupancy.classify of the same keyframes.  The map slot is neither read nor touched; map_occupancy_grid / _list / _slice serve the volume."""
        ids, poses = self._ids_poses(ids, poses)
        p = _record(OccupancyParams, params)
        st = OccupancyStats()
        self._check(self._l.qn_kf_map_occupancy(self.h, _p(ids), _p(poses), C.c_uint32(len(ids)), C.byref(p), C.byref(st)))
        return _as_dict(st)

    def map_occupancy_update(self, ids, poses, params=None):
        """qn_kf_map_occupancy_update: the resident volume brought to this list in place - the entries whose id and pose bytes the volume already holds are
        kept, the others are walked in, and what the list no longer names is walked out again.  The arguments are map_occupancy's.  -> (stats, update): stats
        the dict map_occupancy returns for the same list, update a dict of the fields of qn_occupancy_update (dirty_lo, dirty_hi as tuples), equal to
        mapoccupancy.update's.  Afterwards every getter returns the bytes it returns after map_occupancy of the same list."""
        ids, poses = self._ids_poses(ids, poses)
        p = _record(OccupancyParams, params)
        st = OccupancyStats(); up = OccupancyUpdate()
        self._check(self._l.qn_kf_map_occupancy_update(self.h, _p(ids), _p(poses), C.c_uint32(len(ids)), C.byref(p), C.byref(st), C.byref(up)))
        return _as_dict(st), _as_dict(up)

    def map_occupancy_grid(self):
        """qn_kf_map_occupancy_grid -> (info, hits (D, H, W) uint32, misses (D, H, W) uint32, classes (D, H, W) uint8) of the latest map_occupancy: info a dict of
        origin, voxel, width, height, depth, minc; x the fastest axis, z the slowest; classes 0 unknown, 1 free, 2 occupied."""
        return self._volume(self._l.qn_kf_map_occupancy_grid, (np.uint32, np.uint32, np.uint8))

    def map_occupancy_list(self, mask=1 << QN_OCC_OCCUPIED):
        """qn_kf_map_occupancy_list -> (ijk (m, 3) int32 grid indices, hits (m,) uint32, misses (m,) uint32) of the voxels whose class bit (1 << class) is set in
        mask, in ascending linear index"""
        m = C.c_uint32(int(mask) & 0xffffffff); n = C.c_uint32()
        self._check(self._l.qn_kf_map_occupancy_list(self.h, m, C.byref(n), None, None, None))
        k = int(n.value)
        ijk = np.zeros((max(k, 1), 3), np.int32); hits = np.zeros(max(k, 1), np.uint32); misses = np.zeros(max(k, 1), np.uint32)
        if k:
            self._check(self._l.qn_kf_map_occupancy_list(self.h, m, C.byref(n), _p(ijk), _p(hits), _p(misses)))
        return ijk[:k], hits[:k], misses[:k]

    def map_occupancy_slice(self, iz_lo, iz_hi):
        """qn_kf_map_occupancy_slice -> (H, W) uint8: per column over the layers iz_lo .. iz_hi (inclusive, clipped to the grid) 2 if any voxel is occupied, else 1
        if any is free, else 0 - the values of map_ground_grid's occupancy, so mapground.to_pgm / map_yaml serve it"""
        g, _ = self._grid(self._l.qn_kf_map_occupancy_grid, 3)
        return self._slice(g, self._l.qn_kf_map_occupancy_slice, iz_lo, iz_hi, np.uint8)

    # ---- the occupancy map's Euclidean distance field (qn_kf_map_distance / _grid / _slice / _query; numpy twin: qn_amd/mapdistance.py)
    def map_distance(self, params=None):
        """qn_kf_map_distance over the class bytes of the latest map_occupancy: per voxel the squared distance, in voxels, to the nearest voxel whose class bit
        is in site_mask, QN_DIST_FAR beyond max_dist.  params: a DistanceParams (or a mapdistance.DistanceParams); None: the defaults.  -> stats, a dict of the
        fields of qn_distance_stats, equal to those of mapdistance.transform of the downloaded classes.  map_distance_grid / _slice / _query serve the field."""
        p = _record(DistanceParams, params)
        st = DistanceStats()
        self._check(self._l.qn_kf_map_distance(self.h, C.byref(p), C.byref(st)))
        return _as_dict(st)

    def map_distance_grid(self):
        """qn_kf_map_distance_grid -> (info, params, d2 (D, H, W) uint16) of the latest map_distance: info the occupancy grid's dict (map_occupancy_grid),
        params a dict of site_mask and max_dist"""
        return self._volume(self._l.qn_kf_map_distance_grid, (np.uint16,), DistanceParams())

    def map_distance_slice(self, iz_lo, iz_hi):
        """qn_kf_map_distance_slice -> (H, W) uint16: per column the smallest d2 over the layers iz_lo .. iz_hi (inclusive, clipped to the grid), QN_DIST_FAR
        when the band misses the grid: the clearance of an upright body spanning those layers"""
        g, _ = self._grid(self._l.qn_kf_map_distance_grid, 1, DistanceParams())
        return self._slice(g, self._l.qn_kf_map_distance_slice, iz_lo, iz_hi, np.uint16)

    def map_distance_query(self, xyz):
        """qn_kf_map_distance_query: world points (n, 3) f64 -> (d2 (n,) uint16, class (n,) uint8) of the voxel each falls in; QN_DIST_FAR and QN_DIST_OUTSIDE
        for a point that is not finite or outside the grid"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        n = len(xyz)
        d2 = np.zeros(max(n, 1), np.uint16); cls = np.zeros(max(n, 1), np.uint8)
        self._check(self._l.qn_kf_map_distance_query(self.h, _p(xyz), C.c_uint32(n), _p(d2), _p(cls)))
        return d2[:n], cls[:n]

    # ---- planning over the occupancy map: the cost-to-go field and paths (qn_kf_map_route / _grid / _query / _path; numpy twin: qn_amd/maproute.py)
    def map_route(self, goals, params=None):
        """qn_kf_map_route over the latest map_occupancy and map_distance: per voxel (per column in planar mode) the smallest 3-4-5 chamfer path cost to the
        nearest of the world points `goals` (n, 3) f64 through passable voxels, QN_ROUTE_BLOCKED where not passable, QN_ROUTE_UNREACHED where cut off.  params:
        a RouteParams (or a maproute.RouteParams); None: the defaults.  -> stats, a dict of the fields of qn_route_stats; all but rounds and tile_visits equal
        those of maproute.field of the downloaded classes and d2.  map_route_grid / _query / _paths serve the field."""
        p = _record(RouteParams, params)
        xyz = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        st = RouteStats()
        self._check(self._l.qn_kf_map_route(self.h, _p(xyz), C.c_uint32(len(xyz)), C.byref(p), C.byref(st)))
        return _as_dict(st)

    def map_route_grid(self):
        """qn_kf_map_route_grid -> (info, params, cost (D, H, W) uint32, or (1, H, W) in planar mode) of the latest map_route: info the occupancy grid's dict,
        params a dict of the fields of qn_route_params"""
        return self._volume(self._l.qn_kf_map_route_grid, (np.uint32,), RouteParams(), planar=True)

    def map_route_query(self, xyz):
        """qn_kf_map_route_query: world points (n, 3) f64 -> the field's value (n,) uint32 at each; QN_ROUTE_BLOCKED for a point that is not finite or outside"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        n = len(xyz)
        cost = np.zeros(max(n, 1), np.uint32)
        self._check(self._l.qn_kf_map_route_query(self.h, _p(xyz), C.c_uint32(n), _p(cost)))
        return cost[:n]

    def map_route_paths(self, starts, max_len):
        """qn_kf_map_route_path: world points (S, 3) f64 -> (len (S,) uint32: the voxels of each start's path down the field, start and goal included, 0 for a
        start that is outside, blocked or unreached; ijk (S, max_len, 3) int32: the first min(len, max_len) of them, the rest 0).  cost // 3 + 1 bounds len."""
        xyz = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        n, m = len(xyz), int(max_len)
        lens = np.zeros(max(n, 1), np.uint32); ijk = np.zeros((max(n, 1), max(m, 1), 3), np.int32)
        self._check(self._l.qn_kf_map_route_path(self.h, _p(xyz), C.c_uint32(n), C.c_uint32(m), _p(lens), _p(ijk)))
        return lens[:n], ijk[:n]

    # ---- exploration frontiers of the occupancy map (qn_kf_map_frontiers / _frontier_grid / _frontier_regions / _frontier_list / _frontier_costs; numpy twin:
    # qn_amd/mapfrontier.py)
    def map_frontiers(self, params=None):
        """qn_kf_map_frontiers over the class bytes of the latest map_occupancy: the free voxels that border unknown space, grouped into 26-connected regions of
        at least min_size voxels, numbered in ascending root.  params: a FrontierParams (or a mapfrontier.FrontierParams); None: the defaults.  -> stats, a dict
        of the fields of qn_frontier_stats; all but rounds equal those of mapfrontier.frontier of the downloaded classes.  map_frontier_grid / _regions /
        _list / _costs serve the result; neither map_distance nor map_route is needed, only map_frontier_costs reads the route field."""
        p = _record(FrontierParams, params)
        st = FrontierStats()
        self._check(self._l.qn_kf_map_frontiers(self.h, C.byref(p), C.byref(st)))
        return _as_dict(st)

    def map_frontier_grid(self):
        """qn_kf_map_frontier_grid -> (info, params, labels (D, H, W) int32) of the latest map_frontiers: info the occupancy grid's dict, params a dict of the
        fields of qn_frontier_params; a label is the region number, QN_FRONTIER_REJECTED or QN_FRONTIER_NONE"""
        return self._volume(self._l.qn_kf_map_frontier_grid, (np.int32,), FrontierParams())

    def map_frontier_regions(self):
        """qn_kf_map_frontier_regions -> the regions of the latest map_frontiers, a structured array of mapfrontier.INFO_DTYPE in region order"""
        from . import mapfrontier
        return self._listed(self._l.qn_kf_map_frontier_regions, ((), mapfrontier.INFO_DTYPE))[0]

    def map_frontier_list(self):
        """qn_kf_map_frontier_list -> (ijk (m, 3) int32 grid indices, label (m,) int32) of every frontier voxel of the latest map_frontiers, kept or rejected,
        in ascending linear index"""
        return tuple(self._listed(self._l.qn_kf_map_frontier_list, ((3,), np.int32), ((), np.int32)))

    def map_frontier_costs(self):
        """qn_kf_map_frontier_costs with the field of the latest map_route -> (cost (R,) uint32, ijk (R, 3) int32): per region the smallest cost below
        QN_ROUTE_BLOCKED over its voxels and the voxel attaining it (the smallest linear index on a tie); QN_ROUTE_UNREACHED and (0, 0, 0) without one"""
        R = self._count(self._l.qn_kf_map_frontier_regions, 1)
        cost = np.zeros(max(R, 1), np.uint32); ijk = np.zeros((max(R, 1), 3), np.int32)
        self._check(self._l.qn_kf_map_frontier_costs(self.h, _p(cost), _p(ijk)))
        return cost[:R], ijk[:R]

    # ---- view gain over the occupancy map (qn_kf_map_view_gain / _view_grid; numpy twin: qn_amd/mapview.py)
    def map_view_gain(self, viewpoints, offsets, params=None):
        """qn_kf_map_view_gain over the class bytes of the latest map_occupancy: from each of the (Q, 3) f64 world viewpoints the rays of the (R, 3) int32 table
        `offsets` (1024ths of a voxel: mapview.sensor_offsets makes one) are cast until a voxel of stop_mask, the grid's face, max_through gain voxels or their
        end, and the distinct gain voxels they pass through are counted.  params: a ViewParams (or a mapview.ViewParams); None: the defaults.
        -> (info, a structured array of mapview.VIEW_DTYPE, one row per viewpoint; stats, a dict of the fields of qn_view_stats): all but passes equal those of
        mapview.gain of the downloaded classes.  map_view_grid serves the cover volume."""
        from . import mapview
        p = _record(ViewParams, params)
        xyz = np.ascontiguousarray(viewpoints, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        info = np.zeros(max(len(xyz), 1), mapview.VIEW_DTYPE)
        st = ViewStats()
        self._check(self._l.qn_kf_map_view_gain(self.h, _p(xyz), C.c_uint32(len(xyz)), _p(off), C.c_uint32(len(off)), C.byref(p), _p(info), C.byref(st)))
        return info[:len(xyz)], _as_dict(st)

    def map_view_grid(self):
        """qn_kf_map_view_grid -> (info, params, cover (D, H, W) uint32) of the latest map_view_gain: info the occupancy grid's dict, params a dict of the fields
        of qn_view_params; cover[v] is the number of viewpoints that marked voxel v"""
        return self._volume(self._l.qn_kf_map_view_grid, (np.uint32,), ViewParams())

    # ---- the map slot's points clustered into objects (qn_kf_map_clusters / _cluster_points / _cluster_list / qn_kf_map_drop_rejected_clusters; numpy twin:
    # qn_amd/mapclusters.py)
    def map_clusters(self, params=None):
        """qn_kf_map_clusters on the map of the latest build or filter, then its downloads.  params: a ClusterParams (or a mapclusters.ClusterParams); None:
        the defaults.  A class_mask != 0 needs the map_ground of the same map.  -> (stats, label (n,) int32, root (n,) uint32, size (n,) uint32, clusters),
        equal to mapclusters.classify of the downloaded map; stats: a dict of the fields of qn_cluster_stats; clusters: a dict of root (C,) uint32, size (C,)
        uint32, lo and hi (C, 3) float32, sum_q (C, 3) int64 and centroid (C, 3) float64 = sum_q / size * 2^-quant_exp.  The map slot is not touched;
        map_drop_rejected_clusters applies the result."""
        from . import mapclusters
        p = _record(ClusterParams, params)
        st = ClusterStats()
        self._check(self._l.qn_kf_map_clusters(self.h, C.byref(p), C.byref(st)))
        n = int(st.n)
        label = np.zeros(max(n, 1), np.int32); root = np.zeros(max(n, 1), np.uint32); size = np.zeros(max(n, 1), np.uint32)
        self._check(self._l.qn_kf_map_cluster_points(self.h, _p(label), _p(root), _p(size)))
        cnt = C.c_uint32()
        info = np.zeros(max(int(st.clusters), 1), mapclusters.INFO_DTYPE)
        self._check(self._l.qn_kf_map_cluster_list(self.h, _p(info), C.c_uint32(len(info)), C.byref(cnt)))
        info = info[:cnt.value]
        stats = _as_dict(st)
        clusters = {f: info[f].copy() for f in ("root", "size", "lo", "hi", "sum_q")}
        clusters["centroid"] = info["sum_q"].astype(np.float64) / info["size"].astype(np.float64)[:, None] * math.ldexp(1.0, -int(st.quant_exp))
        return stats, label[:n], root[:n], size[:n], clusters

    def map_drop_rejected_clusters(self):
        """qn_kf_map_drop_rejected_clusters: the map slot without the members of the components the latest map_clusters rejected, in order -> (ptr, n): the
        device address of the n float4 records x y z intensity.  Records that were not members stay.  Every result computed from the old slot is stale
        afterwards."""
        return self._slot(self._l.qn_kf_map_drop_rejected_clusters)

    # ---- scans localised in the map slot (qn_kf_map_crop / _crop_get / qn_kf_map_localize[_c2f]; numpy twin of the crop: qn_amd/maplocalize.py)
    def map_crop(self, centres, radius, shape=0):
        """qn_kf_map_crop: the neighbourhoods of `centres` ((Q, 3), rounded to f32) cut out of the map slot, then their downloads -> one dict per centre:
        n, ptr (device address of the n float4 records x y z intensity, None when empty; valid until the next map_crop / map_localize), xyzi (n, 4) float32 and
        idx (n,) uint32 (ascending map indices), equal to maplocalize.crop of the downloaded map."""
        c = np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(-1, 3))
        counts = np.zeros(max(len(c), 1), np.uint32)
        self._check(self._l.qn_kf_map_crop(self.h, _p(c) if len(c) else None, C.c_uint32(len(c)), C.c_double(radius), C.c_uint32(shape), _p(counts)))
        return [self.map_crop_get(k) for k in range(len(c))]

    def map_crop_get(self, crop):
        """qn_kf_map_crop_get and the download of crop `crop` of the latest map_crop / map_localize -> dict(n, ptr, xyzi, idx)"""
        ptr = C.c_void_p(); n = C.c_uint32()
        self._check(self._l.qn_kf_map_crop_get(self.h, C.c_uint32(crop), C.byref(ptr), C.byref(n), None))
        idx = np.zeros(max(n.value, 1), np.uint32)
        if n.value:
            self._check(self._l.qn_kf_map_crop_get(self.h, C.c_uint32(crop), C.byref(ptr), C.byref(n), _p(idx)))
        return dict(n=int(n.value), ptr=ptr.value, xyzi=self._read_float4(ptr, n.value, "map_crop_get"), idx=idx[:n.value].copy())

    def _localize_args(self, query, guesses, params):
        q = np.ascontiguousarray(np.atleast_1d(query), dtype=np.int32)
        g = np.ascontiguousarray(np.asarray(guesses, dtype=np.float64).reshape(-1, 16))
        if len(q) != len(g):
            raise ValueError("map_localize: %d queries but %d guesses" % (len(q), len(g)))
        return q, g, _record(LocalizeParams, params), len(q)

    def map_localize(self, ctx, query, guesses, params=None):
        """qn_kf_map_localize: pair j = keyframe query[j] (alone in its sensor frame, voxel grid at params.leaf) registered against the crop of the map slot
        around the translation of guesses[j] (4x4, map <- sensor, rounded to f32), seeded with that guess = gicp_align_batch(ctx, [(scan cloud, crop)],
        guesses=[g]) record for record.  -> (one dict per pair as verify_loop_pairs', T = the pose in the map; stats: a dict of the fields of qn_localize_stats).
        verify_cloud / verify_overlap serve the pairs afterwards; map_crop_get(k) the k-th distinct crop."""
        q, g, p, n = self._localize_args(query, guesses, params)
        results, valid, status, _, _ = _verify_out(n); st = LocalizeStats()
        rc = self._l.qn_kf_map_localize(self.h, ctx.h, C.byref(p), _p(q) if n else None, _p(g) if n else None, C.c_uint32(n), results, _p(valid), _p(status), C.byref(st))
        self._raise(rc, ctx)
        return _gicp_dicts(results, valid, status, n), _as_dict(st)

    def map_localize_c2f(self, ctx, query, guesses, params=None):
        """qn_kf_map_localize_c2f: the same clouds coarse to fine (Quatro -> transformPcd -> Nano-GICP); only the guess's translation is used, as the crop
        centre = coarse_to_fine_align_batch([ctx], [(scan cloud, crop)]) record for record.  -> (one dict per pair as verify_loop_pairs_c2f's, T = the pose in
        the map; stats)."""
        q, g, p, n = self._localize_args(query, guesses, params)
        results, valid, status, Tt, Tq = _verify_out(n); st = LocalizeStats()
        rc = self._l.qn_kf_map_localize_c2f(self.h, ctx.h, C.byref(p), _p(q) if n else None, _p(g) if n else None, C.c_uint32(n), results, _p(Tt), _p(Tq),
                                            _p(valid), _p(status), C.byref(st))
        self._raise(rc, ctx)
        return _c2f_dicts(results, Tt, Tq, valid, status, n), _as_dict(st)

    # ---- Scan Context loop candidates (qn_kf_sc_*; numpy twin: qn_amd/scancontext.py)
    def sc_set_params(self, params=None, **kw):
        """qn_kf_sc_set_params: a ScParams, or its fields as keywords (the rest default).  A shape change discards every descriptor."""
        p = params if params is not None else ScParams(**kw)
        self._check(self._l.qn_kf_sc_set_params(self.h, C.byref(p)))

    def sc_params(self):
        p = ScParams()
        self._check(self._l.qn_kf_sc_get_params(self.h, C.byref(p)))
        return p

    def sc_describe(self, ids):
        """qn_kf_sc_describe: the descriptors of these keyframes, on the GPU from their resident records (already described ones are kept)"""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        self._check(self._l.qn_kf_sc_describe(self.h, _p(ids) if len(ids) else None, C.c_uint32(len(ids))))

    def sc_descriptor(self, kid):
        """-> (desc (n_rings, n_sectors) f32, ring key (n_rings,) f64, column norms (n_sectors,) f64) of a described keyframe"""
        p = self.sc_params()
        d = np.zeros((p.n_rings, p.n_sectors), np.float32); rk = np.zeros(p.n_rings); cn = np.zeros(p.n_sectors)
        self._check(self._l.qn_kf_sc_get(self.h, C.c_int32(kid), _p(d), _p(rk), _p(cn)))
        return d, rk, cn

    def sc_query(self, query_ids, stamps, tdiff, top_k=10):
        """qn_kf_sc_query: for each query id, the top_k described keyframes older than it by more than tdiff (stamps[q] - stamps[c] > tdiff)
        nearest by Scan Context distance -> list (one per query) of (ids int32, D f64, shift int32) arrays, ascending D, ties to the lower id.
        scancontext.yaw_of_shift(shift, n_sectors) is the candidate's heading minus the query's."""
        q = np.ascontiguousarray(np.atleast_1d(query_ids), dtype=np.int32)
        st = np.ascontiguousarray(stamps, dtype=np.float64)
        nq, k = len(q), int(top_k)
        ids = np.zeros(max(nq * k, 1), np.int32); D = np.zeros(max(nq * k, 1)); sh = np.zeros(max(nq * k, 1), np.int32); n = np.zeros(max(nq, 1), np.uint32)
        self._check(self._l.qn_kf_sc_query(self.h, _p(q) if nq else None, C.c_uint32(nq), _p(st), C.c_uint32(len(st)), C.c_double(tdiff), C.c_uint32(k),
                                           _p(ids), _p(D), _p(sh), _p(n)))
        return [(ids[r * k:r * k + n[r]].copy(), D[r * k:r * k + n[r]].copy(), sh[r * k:r * k + n[r]].copy()) for r in range(nq)]

    # ---- developer / tests: the map units' shared device primitives on caller-supplied inputs (qn_kf_debug_map_prims; the records of include/qn_engine.h)
    MAP_PRIMS_LANE = np.dtype([("i", "<i4"), ("u", "<u4"), ("f", "<f4"), ("zero", "<u4"), ("q", "<u8"), ("s", "<i8")])
    MAP_PRIMS_WAVE = np.dtype([("imin", "<i4"), ("imax", "<i4"), ("usum", "<u4"), ("umin", "<u4"), ("umax", "<u4"), ("fmin", "<f4"), ("fmax", "<f4"), ("zero", "<u4"),
                               ("qsum", "<u8"), ("qmin", "<u8"), ("ssum", "<i8"), ("zero2", "<u8")])
    MAP_PRIMS_KEY_IN = np.dtype([("has", "<u4"), ("key", "<u4")])
    MAP_PRIMS_KEY = np.dtype([("trip", "<u4"), ("lead", "<u4"), ("key", "<u4"), ("served", "<u4"), ("same", "<u8")])
    MAP_PRIMS_BLOCK_IN = np.dtype([("pred", "<u4"), ("a", "<u4", (3,)), ("b", "<u8", (3,))])
    MAP_PRIMS_BLOCK = np.dtype([("count", "<u4", (15,)), ("sum32", "<u4", (6,)), ("max32", "<u4", (6,)), ("again32", "<u4"), ("sum64", "<u8", (6,)),
                                ("max64", "<u8", (6,)), ("again64", "<u8"), ("wide", "<u8", (2,))])
    MAP_PRIMS_U64, MAP_PRIMS_MAX, MAP_PRIMS_IN_PLACE = 0x100, 0x200, 0x80000000
    MAP_PRIMS_WAVES, MAP_PRIMS_KEYS, MAP_PRIMS_BLOCKS, MAP_PRIMS_SLOTS, MAP_PRIMS_SCAN, MAP_PRIMS_RANK, MAP_PRIMS_UNITE, MAP_PRIMS_UNITE_MIN, MAP_PRIMS_GRID = range(9)
    MAP_PRIMS_VOXEL = np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("index", "<u4"), ("tile", "<u4"), ("place", "<u4"), ("pos", "<u4"), ("zero", "<u4")])

    def debug_map_prims(self, which, data, arg=0):
        """qn_kf_debug_map_prims: routine `which` (the MAP_PRIMS_* numbers above) of the map units' shared device primitives on the caller's input.  data -> result:
          WAVES      (256 B,) MAP_PRIMS_LANE                        -> (4 B,) MAP_PRIMS_WAVE
          KEYS       (256 B,) MAP_PRIMS_KEY_IN; arg 1: int32 keys   -> ((256 B,) MAP_PRIMS_KEY, (4 B,) u32 trips)
          BLOCKS     (256 B,) MAP_PRIMS_BLOCK_IN                    -> (B,) MAP_PRIMS_BLOCK
          SLOTS      (nb, K) u32, or u64 with arg = MAP_PRIMS_U64 | K, or (nb,) u32 with arg = MAP_PRIMS_MAX; else arg = K      -> (K,) sums / (1,) the maximum
          SCAN       (rows, nb) u32, arg = rows, | MAP_PRIMS_IN_PLACE     -> ((rows, nb) u32 offsets, (rows,) u32 totals)
          RANK       ((256 B,) u8 keep, (B,) u32 bases)             -> (256 B,) u32
          UNITE(_MIN) (n, (m, 2) u32 edges, None or the (n,) u32 starting forest), arg = edges a lane      -> ((n,) u32 raw parents, (n,) u32 roots)
          GRID       (W, H, D), the sides of a dense grid               -> ((W H D,) MAP_PRIMS_VOXEL, (tiles, 4) i32 tile origins, (26, 3) i32 walk offsets)
        A size that does not fit the routine's records is a ValueError here; everything else is the library's to refuse."""
        u4, u8 = np.dtype("<u4"), np.dtype("<u8")

        def need(a, dt, ok):
            a = np.ascontiguousarray(a)
            if a.dtype != dt or not ok(a):
                raise ValueError("debug_map_prims(%d): %s %s does not fit the routine's records" % (which, a.dtype, a.shape))
            return a

        per_block = lambda a: a.ndim == 1 and len(a) % 256 == 0
        arg = int(arg)
        if which in (self.MAP_PRIMS_WAVES, self.MAP_PRIMS_KEYS, self.MAP_PRIMS_BLOCKS):
            a = need(data, (self.MAP_PRIMS_LANE, self.MAP_PRIMS_KEY_IN, self.MAP_PRIMS_BLOCK_IN)[which], per_block)
            n = len(a) // 256
            parts = [a]
            outs = [((4 * n,), self.MAP_PRIMS_WAVE)] if which == 0 else [((256 * n,), self.MAP_PRIMS_KEY), ((4 * n,), u4)] if which == 1 else [((n,), self.MAP_PRIMS_BLOCK)]
        elif which == self.MAP_PRIMS_SLOTS:
            wide, k = bool(arg & self.MAP_PRIMS_U64), 1 if arg == self.MAP_PRIMS_MAX else arg & 0xff
            a = need(data, u8 if wide else u4, lambda a: a.size % max(k, 1) == 0)
            n, parts, outs = a.size // max(k, 1), [a], [((k,), a.dtype)]
        elif which == self.MAP_PRIMS_SCAN:
            a = need(data, u4, lambda a: a.ndim == 2 and a.shape[0] == (arg & 0x7fffffff))
            n, parts, outs = a.shape[1], [a], [(a.shape, u4), ((a.shape[0],), u4)]
        elif which == self.MAP_PRIMS_RANK:
            keep = need(data[0], np.dtype("u1"), per_block)
            n = len(keep) // 256
            parts, outs = [keep, need(data[1], u4, lambda b: b.shape == (n,))], [((256 * n,), u4)]
        elif which == self.MAP_PRIMS_GRID:
            sides = need(np.asarray(data, u4), u4, lambda a: a.shape == (3,))
            n, parts = int(np.prod(sides.astype(np.uint64))), [sides]
            t = np.uint64(8)                                         # DG_T of csrc/qn_dense_grid.cuh, the tile's side: the routine writes one origin a tile
            tiles = int(np.prod((sides.astype(np.uint64) + t - np.uint64(1)) // t))
            outs = [((n,), self.MAP_PRIMS_VOXEL), ((tiles, 4), np.dtype("<i4")), ((26, 3), np.dtype("<i4"))]
        else:
            n, edges, forest = data
            edges = need(edges, u4, lambda e: e.ndim == 2 and e.shape[1] == 2)
            parts = [np.array([len(edges), 0 if forest is None else 1], u4)] + ([] if forest is None else [need(forest, u4, lambda f: f.shape == (n,))]) + [edges]
            outs = [((n,), u4), ((n,), u4)]
        buf = np.frombuffer(b"".join(p.tobytes() for p in parts) + bytes(16), np.uint8).copy()
        out = np.zeros(sum(int(np.prod(s)) * dt.itemsize for s, dt in outs) + 16, np.uint8)
        self._l.qn_kf_debug_map_prims.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        self._check(self._l.qn_kf_debug_map_prims(self.h, C.c_int(which), _p(buf), C.c_uint32(n), C.c_uint32(arg), _p(out)))
        res, at = [], 0
        for s, dt in outs:
            nbytes = int(np.prod(s)) * dt.itemsize
            res.append(out[at:at + nbytes].view(dt).reshape(s).copy()); at += nbytes
        return res[0] if len(res) == 1 else tuple(res)


def loop_candidates(pos, stamps, query, radius, tdiff, max_k=64):
    pos = np.ascontiguousarray(pos, dtype=np.float64); stamps = np.ascontiguousarray(stamps, dtype=np.float64)
    out = np.zeros(max_k, np.int32); n = C.c_uint32()
    st = lib().qn_loop_candidates(_p(pos), _p(stamps), C.c_uint32(len(pos)), C.c_uint32(query), C.c_double(radius), C.c_double(tdiff), C.c_uint32(max_k), _p(out), C.byref(n))
    if st != QN_OK:
        raise EngineError(st, lib().qn_status_str(st).decode())
    return out[:n.value].copy()


def local_submap_ids(c, submap_range, n_keyframes):
    """the window of keyframe c's resident local submap (KeyframeStore.submap_describe): the keyframes within submap_range of c that exist.  Unlike
    loop_submap_ids it keeps the newest keyframe: the reference drops it because its only query is the newest keyframe itself."""
    return [i for i in range(c - submap_range, c + submap_range + 1) if 0 <= i < n_keyframes]


def loop_submap_ids(src_idx, dst_idx, submap_range, enable_quatro, enable_submap_matching, n_keyframes):
    """LoopClosure::setSrcAndDstCloud's keyframe lists (loop_closure.cpp:58-108) -> (src_ids, dst_ids).  A submap takes the keyframes within
    submap_range of its centre except the newest one (`i < keyframes.size() - 1`); without submap matching the source is src_idx alone, and
    with Quatro so is the destination (dst_idx)."""
    def around(c):
        return [i for i in range(c - submap_range, c + submap_range + 1) if 0 <= i < n_keyframes - 1]
    if enable_submap_matching:
        return around(src_idx), around(dst_idx)
    return [src_idx], ([dst_idx] if enable_quatro else around(dst_idx))
