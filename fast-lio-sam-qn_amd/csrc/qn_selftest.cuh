// qn_selftest.cuh - device self-test of the wave-level primitives the search loops stand on (qn_device.cuh: DPP prefix sums and running maxima, DPP reductions with v_readlane,
// the slot -> segment map of a candidate chunk, the f64 wave sum).  Each is compared, lane by lane, with a plain restatement - serial loops over an LDS copy, the shuffle tree
// the f64 sum replaced - on seeded random data; qn_debug_selftest returns the number of mismatches (tests/test_gpu_selftest.py expects 0).  Test infrastructure: nothing on
// the registration path calls it.
#pragma once
#include "qn_device.cuh"
#include "qn_gicp_kernels.cuh"

namespace qn {

// one wave per block; block b works on in[64 b .. 64 b + 63] (and in2[] for the low words of the 64-bit keys)
static __global__ void __launch_bounds__(64) k_selftest_wave(const uint32_t* __restrict__ in, const uint32_t* __restrict__ in2, uint32_t* __restrict__ bad) {
  __shared__ uint32_t sh[64], sh2[64], marks[64], excl[65];
  const int lane = threadIdx.x & 63;
  const uint32_t v = in[blockIdx.x * 64 + lane], w = in2[blockIdx.x * 64 + lane];
  sh[lane] = v; sh2[lane] = w;
  __syncthreads();
  uint32_t nbad = 0;
  // ---- prefix sum / running maximum
  { uint32_t rs = 0, rm = 0;
    for (int i = 0; i <= lane; i++) { rs += sh[i] & 0xffffu; rm = max(rm, sh[i]); }
    if (wave_incl_scan_u32(v & 0xffffu, lane) != rs) nbad++;
    if (wave_incl_max_u32(v) != rm) nbad++; }
  // ---- reductions (every lane must hold the wave's result)
  { int mn = 0x7fffffff, mx = (int)0x80000000; uint32_t mnu = 0xffffffffu; float fmn = __int_as_float(0x7f800000), fmx = -__int_as_float(0x7f800000); unsigned long long k = QN_INF_KEY;
    for (int i = 0; i < 64; i++) {
      const int s = (int)sh[i]; mn = min(mn, s); mx = max(mx, s); mnu = min(mnu, sh[i]);
      const float f = (float)(sh[i] & 0xfffffu) * 0.37f - 150000.f; fmn = fminf(fmn, f); fmx = fmaxf(fmx, f);
      const unsigned long long ki = ((unsigned long long)(sh[i] & 7u) << 32) | sh2[i];      // (three-bit high words: many ties - the low words decide)
      k = ki < k ? ki : k;
    }
    const float fv = (float)(v & 0xfffffu) * 0.37f - 150000.f;
    if (wave_min_i((int)v) != mn) nbad++;
    if (wave_max_i((int)v) != mx) nbad++;
    if (wave_min_u32(v) != mnu) nbad++;
    if (__float_as_uint(wave_min_f(fv)) != __float_as_uint(fmn)) nbad++;
    if (__float_as_uint(wave_max_f(fv)) != __float_as_uint(fmx)) nbad++;
    if (wave_min_u64(((unsigned long long)(v & 7u) << 32) | w) != k) nbad++; }
  // ---- f64 wave sum: the bits of the tree ((row sums by quad / row mirrors), then (R0 + R1) + (R2 + R3)) the shuffle form left in every lane
  { const double d = (double)(int)(v >> 7) * 1.0000001e-3 + (double)w * 3.3e-11;
    double t = dpp_add_f64(d, 0); t = dpp_add_f64(t, 1); t = dpp_add_f64(t, 2); t = dpp_add_f64(t, 3);
    t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
    if (__double_as_longlong(wave_sum_f64_dpp(d)) != __double_as_longlong(t)) nbad++; }
  // ---- slot -> segment of every chunk of a random segment table (lengths 0..15, a third of them empty)
  { const uint32_t len = (v % 3u == 0u) ? 0u : ((v >> 8) & 15u);
    uint32_t ex = 0; for (int i = 0; i < lane; i++) { const uint32_t li = (sh[i] % 3u == 0u) ? 0u : ((sh[i] >> 8) & 15u); ex += li; }
    excl[lane] = ex; if (lane == 63) excl[64] = ex + len;
    __syncthreads();
    const uint32_t total = excl[64];
    for (uint32_t cb = 0; cb < total; cb += 64) {
      const int j = chunk_segment(marks, cb, ex, ex + len);
      const uint32_t slot = cb + (uint32_t)lane;
      if (slot < total) { int r = 0; for (int i = 0; i < 64; i++) if (excl[i] <= slot && excl[i + 1] > slot) r = i; if (j != r) nbad++; }
    } }
  if (nbad) atomicAdd(bad, nbad);
}

// qn_debug_eig3: the device builds of the two 3 x 3 eigen solvers (qn_eig3.cuh) on caller-supplied matrices, one matrix per lane; which = 0 qn_eig3_jacobi,
// 1 sym_eig3.  a6[6 i ..] = (xx, xy, xz, yy, yz, zz) -> w[3 i ..], V[9 i ..] row major, the eigenvector of w[k] in column k.  tests/test_gpu_eig3.py holds the
// results to a 50-digit reference and to the host build of the same text.
#define QN_EIG3_DEBUG_BLOCK 256
static __global__ void __launch_bounds__(QN_EIG3_DEBUG_BLOCK) k_debug_eig3(int which, const double* __restrict__ a6, uint32_t n, double* __restrict__ w_out, double* __restrict__ v_out) {
  const uint32_t i = blockIdx.x * QN_EIG3_DEBUG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double* a = a6 + 6 * (size_t)i;
  double w[3], V[3][3];
  if (which == 0) {
    qn_eig3_jacobi(a[0], a[1], a[2], a[3], a[4], a[5], w, V);
  } else {
    const double A[6] = {a[0], a[1], a[2], a[3], a[4], a[5]};
    sym_eig3(A, w, V);
  }
  double* wo = w_out + 3 * (size_t)i; double* vo = v_out + 9 * (size_t)i;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    wo[r] = w[r];
#pragma unroll
    for (int k = 0; k < 3; k++) vo[3 * r + k] = V[r][k];
  }
}

// qn_debug_step_math: the device builds of the Gauss-Newton step's small dense f64 routines (qn_step_math.cuh, and d_propose of qn_gicp_kernels.cuh as it is) on
// caller-supplied problems, one problem per lane in blocks of 64 lanes; the pivoted solve's SolveWork sits per lane in LDS (512 B x 64 = 32 KiB a block), as it sits
// in LDS in the controller kernels.  WHICH and the record layouts: include/qn_engine.h at the declaration; WHICH = 1, the pivoted solve called directly, has its
// kernel in qn_step_debug.hip, and that file says why it cannot stand here.  d_propose runs on the lane's own GicpState in global
// memory (states, zeroed by the caller); it does not say which solve it took, so the unpivoted one is called once more on the same input for the path word.
// tests/test_gpu_step_math.py holds the results to a 50-digit reference and to the host build of the same text.
#define QN_STEP_DEBUG_BLOCK 64
template <int WHICH>
static __global__ void __launch_bounds__(QN_STEP_DEBUG_BLOCK) k_debug_step_math(const double* __restrict__ in, uint32_t n, double* __restrict__ out, GicpState* __restrict__ states) {
  __shared__ SolveWork work[QN_STEP_DEBUG_BLOCK];
  const uint32_t i = blockIdx.x * QN_STEP_DEBUG_BLOCK + threadIdx.x;
  if (i >= n) return;
  SolveWork* w = &work[threadIdx.x];                                   // (d_propose's; dropped where WHICH does not use it)
  static_assert(WHICH != 1, "the pivoted solve's own kernel: qn_step_debug.hip");
  if (WHICH == 0) {                                                    // A (36), lambda, b (6) -> x (6), ok
    const double* r = in + 43 * (size_t)i; double* o = out + 7 * (size_t)i;
    double rhs[6], x[6];
    const bool ok = d_ldlt_solve6_fast(r, r[36], rhs, x, r + 37);
#pragma unroll
    for (int k = 0; k < 6; k++) o[k] = x[k];
    o[6] = ok ? 1.0 : 0.0;
  } else if (WHICH == 2) {                                             // H (36), b (6), lambda, x0 (16) -> d (6), delta (16), xi (16), path
    const double* r = in + 59 * (size_t)i; double* o = out + 39 * (size_t)i;
    GicpState* st = states + i;
    for (int k = 0; k < 36; k++) st->H[k] = r[k];
    for (int k = 0; k < 6; k++) st->b[k] = r[36 + k];
    for (int k = 0; k < 16; k++) st->x0[k] = r[43 + k];
    const double lambda = r[42];
    d_propose(st, lambda, w);
    for (int k = 0; k < 6; k++) o[k] = st->d[k];
    for (int k = 0; k < 16; k++) { o[6 + k] = st->delta[k]; o[22 + k] = st->xi[k]; }
    double Hl[36], rhs[6], dl[6];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++) Hl[6 * a + b] = b <= a ? st->H[6 * a + b] : 0.0;
    o[38] = d_ldlt_solve6_fast(Hl, lambda, rhs, dl, st->b) ? 0.0 : 1.0;
  } else if (WHICH == 3) {                                             // om (3) -> R (9) row major
    const double* r = in + 3 * (size_t)i; double* o = out + 9 * (size_t)i;
    const double om[3] = {r[0], r[1], r[2]};
    double R[3][3];
    d_so3_exp(om, R);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) o[3 * a + b] = R[a][b];
  } else if (WHICH == 4) {                                             // M (9) row major -> its inverse (9)
    const double* r = in + 9 * (size_t)i; double* o = out + 9 * (size_t)i;
    M3 m;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) m.m[a][b] = r[3 * a + b];
    const M3 v = m3_inverse(m);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) o[3 * a + b] = v.m[a][b];
  } else {                                                             // delta (16), rotation_epsilon, transformation_epsilon -> converged, mr, mt
    const double* r = in + 18 * (size_t)i; double* o = out + 3 * (size_t)i;
    double delta[16];
#pragma unroll
    for (int k = 0; k < 16; k++) delta[k] = r[k];
    GicpConfig cfg = {};
    cfg.rotation_epsilon = r[16]; cfg.transformation_epsilon = r[17];
    double mr, mt;
    o[0] = d_is_converged(delta, cfg, &mr, &mt) ? 1.0 : 0.0;
    o[1] = mr; o[2] = mt;
  }
}

}  // namespace qn
