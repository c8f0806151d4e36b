// qn_step_math.cuh - the small dense f64 arithmetic of a registration tick, each routine for one thread: the adjugate inverse of the 3 x 3 matrix C_B + R C_A R'
// formed once per correspondence (m3_inverse; qn_tick.cuh, qn_linearize.cuh), and what the controller does with the reduced 6 x 6 system - the two LDL'
// solves of (H + lambda I) d = -b (d_ldlt_solve6_fast, unpivoted and unrolled, and d_ldlt_solve6, diagonally pivoted, which d_propose in qn_gicp_kernels.cuh
// takes when the first meets a pivot that is not positive), the rotation update exp(d[0:3]) (d_so3_exp), the product of two isometries (d_iso_mul) and the
// convergence test on the step (d_is_converged, with the GicpConfig it reads).  Plain C++ as well, so that a host build can check them against a high-precision
// reference (tests/step_math_host.cpp, tests/test_step_math_cpu.py; the device builds: qn_debug_step_math, tests/test_gpu_step_math.py).  The function bodies are
// the ones the kernels have always compiled, and the registration results are pinned to them bit for bit: under hipcc every routine is __device__ with the
// inlining qualifier it had.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define QN_STEP_FN __device__ __forceinline__
#define QN_STEP_INL __device__ inline
#else
#define QN_STEP_FN inline
#define QN_STEP_INL inline
#endif

namespace qn {

struct GicpConfig {                                 // by-value kernel argument
  int k, max_iterations, optimizer, lm_max_iterations, force_iterations;
  double max_corr_dist_sq, transformation_epsilon, rotation_epsilon, lm_init_lambda_factor;
};

// ------------------------------------------------------------------ small dense f64 math
struct M3 { double m[3][3]; };

QN_STEP_FN M3 m3_inverse(const M3& a) {
  const double (*m)[3] = a.m;
  double c00 = m[1][1]*m[2][2] - m[1][2]*m[2][1];
  double c01 = m[1][2]*m[2][0] - m[1][0]*m[2][2];
  double c02 = m[1][0]*m[2][1] - m[1][1]*m[2][0];
  double det = m[0][0]*c00 + m[0][1]*c01 + m[0][2]*c02;
  double id = 1.0 / det;
  M3 r;
  r.m[0][0] = c00*id; r.m[1][0] = c01*id; r.m[2][0] = c02*id;
  r.m[0][1] = (m[0][2]*m[2][1] - m[0][1]*m[2][2])*id;
  r.m[1][1] = (m[0][0]*m[2][2] - m[0][2]*m[2][0])*id;
  r.m[2][1] = (m[0][1]*m[2][0] - m[0][0]*m[2][1])*id;
  r.m[0][2] = (m[0][1]*m[1][2] - m[0][2]*m[1][1])*id;
  r.m[1][2] = (m[0][2]*m[1][0] - m[0][0]*m[1][2])*id;
  r.m[2][2] = (m[0][0]*m[1][1] - m[0][1]*m[1][0])*id;
  return r;
}

// ------------------------------------------------------------------ K6 solver / LM-GN controller
QN_STEP_INL void d_so3_exp(const double om[3], double R[3][3]) {
  double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
  double imag, real;
  if (theta_sq < 1e-10) {
    double theta_quad = theta_sq * theta_sq;
    imag = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * theta_quad;
    real = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * theta_quad;
  } else {
    double theta = sqrt(theta_sq), half = 0.5 * theta;
    imag = sin(half) / theta; real = cos(half);
  }
  double w = real, x = imag * om[0], y = imag * om[1], z = imag * om[2];
  double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz;       R[0][2] = txz + twy;
  R[1][0] = txy + twz;       R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy;       R[2][1] = tyz + twx;       R[2][2] = 1 - (txx + tyy);
}

// Unpivoted LDL^T, fully unrolled (static register indexing).  H + lambda I is SPD in every healthy
// registration; returns false when a pivot is not strictly positive so the caller can take the
// pivoted path (semi-definite systems: too few correspondences).  Same solution as the pivoted
// factorisation up to rounding.
QN_STEP_FN bool d_ldlt_solve6_fast(const double Ain[36], double diag_add, double rhs[6], double x[6], const double* b) {      // rhs = -b, fetched AFTER the factorisation (it is not needed before: six f64 less across it)
  double A[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) A[i][j] = Ain[6 * i + j] + (i == j ? diag_add : 0.0);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double d = A[k][k];
    ok = ok && (d > 0.0) && (d < 1.7976931348623157e308);
    const double inv = 1.0 / d;
    double l[6];
#pragma unroll
    for (int i = k + 1; i < 6; i++) l[i] = A[i][k] * inv;
#pragma unroll
    for (int i = k + 1; i < 6; i++)
#pragma unroll
      for (int j = k + 1; j <= i; j++) A[i][j] -= l[i] * d * l[j];
#pragma unroll
    for (int i = k + 1; i < 6; i++) A[i][k] = l[i];
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) rhs[i] = -b[i];
#pragma unroll
  for (int i = 0; i < 6; i++) { double s = rhs[i];
#pragma unroll
    for (int j = 0; j < i; j++) s -= A[i][j] * y[j]; y[i] = s; }
#pragma unroll
  for (int i = 0; i < 6; i++) y[i] = y[i] / A[i][i];
#pragma unroll
  for (int i = 5; i >= 0; i--) { double s = y[i];
#pragma unroll
    for (int j = i + 1; j < 6; j++) s -= A[j][i] * x[j]; x[i] = s; }
  return ok;
}

// LDL^T with diagonal pivoting (what Eigen::LDLT does), 6x6, f64.  The rarely taken general path: all its dynamically indexed work
// arrays live in LDS (SolveWork) - a kernel whose private arrays go to scratch pays ~5 us more per dispatch on gfx950.
struct SolveWork { double A[6][6]; double l[6], y[6], z[6], rhs[6]; int perm[6]; int pad[2]; };
QN_STEP_INL void d_ldlt_solve6(const double Ain[36], double diag_add, double x[6] /* LDS */, SolveWork* w /* LDS; w->rhs set by the caller */) {
  double (*A)[6] = w->A; int* perm = w->perm; double* l = w->l; double* y = w->y; double* z = w->z;
#pragma unroll 1
  for (int i = 0; i < 6; i++) {                                        // (row by row, not unrolled: unrolled, the 36 entries were all in flight at once - the spill of the kernels that carry this step)
    perm[i] = i;
#pragma unroll
    for (int j = 0; j < 6; j++) A[i][j] = Ain[6 * i + j] + (i == j ? diag_add : 0.0);
  }
  for (int k = 0; k < 6; k++) {
    int piv = k; double best = fabs(A[k][k]);
    for (int i = k + 1; i < 6; i++) if (fabs(A[i][i]) > best) { best = fabs(A[i][i]); piv = i; }
    if (piv != k) {
      for (int j = 0; j < 6; j++) { double t = A[k][j]; A[k][j] = A[piv][j]; A[piv][j] = t; }
      for (int i = 0; i < 6; i++) { double t = A[i][k]; A[i][k] = A[i][piv]; A[i][piv] = t; }
      int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
    }
    double d = A[k][k];
    if (d == 0.0) continue;
    for (int i = k + 1; i < 6; i++) l[i] = A[i][k] / d;
    for (int i = k + 1; i < 6; i++) for (int j = k + 1; j <= i; j++) { A[i][j] -= l[i] * d * l[j]; A[j][i] = A[i][j]; }
    for (int i = k + 1; i < 6; i++) A[i][k] = l[i];
  }
  for (int i = 0; i < 6; i++) { double s = w->rhs[perm[i]]; for (int j = 0; j < i; j++) s -= A[i][j] * y[j]; y[i] = s; }
  for (int i = 0; i < 6; i++) y[i] = (A[i][i] != 0.0) ? y[i] / A[i][i] : 0.0;
  for (int i = 5; i >= 0; i--) { double s = y[i]; for (int j = i + 1; j < 6; j++) s -= A[j][i] * z[j]; z[i] = s; }
  for (int i = 0; i < 6; i++) x[perm[i]] = z[i];
}

QN_STEP_FN void d_iso_mul(const double A[16], const double B[16], double C[16]) {
  double r[16];
#pragma unroll
  for (int i = 0; i < 16; i++) r[i] = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) r[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
    r[4 * i + 3] = A[4 * i] * B[3] + A[4 * i + 1] * B[7] + A[4 * i + 2] * B[11] + A[4 * i + 3];
  }
  r[15] = 1.0;
#pragma unroll
  for (int i = 0; i < 16; i++) C[i] = r[i];
}

QN_STEP_INL bool d_is_converged(const double delta[16], const GicpConfig& cfg, double* mr_out, double* mt_out) {
  double mr = 0, mt = 0;
  for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) mr = fmax(mr, fabs(delta[4 * a + b] - (a == b ? 1.0 : 0.0))); mt = fmax(mt, fabs(delta[4 * a + 3])); }
  if (mr_out) { *mr_out = mr; *mt_out = mt; }
  // std::max(a, b) as the reference writes it, (a < b) ? b : a - NOT fmax: a NaN ratio of the rotation (rotation_epsilon NaN, or 0 with an exact-identity
  // rotation step) must never converge, while fmax would drop it and stop on the translation alone
  const double qr = mr / cfg.rotation_epsilon, qt = mt / cfg.transformation_epsilon;
  return (qr < qt ? qt : qr) < 1.0;
}

}  // namespace qn
