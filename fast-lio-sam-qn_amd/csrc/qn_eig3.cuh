// qn_eig3.cuh - the two eigen decompositions of a symmetric 3 x 3 matrix in f64 by cyclic Jacobi rotations, each for one thread: qn_eig3_jacobi (a fixed sweep
// count; qn_mapnormals.hip) and qn::sym_eig3 (an early exit and a descending sort; the GICP covariance and the Quatro normal kernels), the second at the end of
// the file.  Plain C++ as well, so that a host build can check them against a high-precision reference and LAPACK (tests/eig3_host.cpp, tests/test_eig3_cpu.py;
// the device builds: qn_debug_eig3, tests/test_gpu_eig3.py).
// A = (a00, a01, a02, a11, a12, a22), upper triangle by rows.  QN_EIG3_SWEEPS sweeps over the pairs (0, 1), (0, 2), (1, 2); a rotation whose off-diagonal
// entry is already zero is skipped.  Convergence is quadratic: from any start three sweeps leave the off-diagonal norm below 2^-53 of the matrix norm and the
// fourth squares that again, so six is a fixed count with room, the same in every lane.  The rotation is the textbook one (Rutishauser): t = tan of the angle,
// the smaller root of t^2 + 2 theta t - 1 = 0 with theta = (aqq - app) / (2 apq), |t| <= 1, which keeps the diagonal updates app - t apq / aqq + t apq
// backward stable; theta^2 overflowing to infinity gives t = 0, the right limit.  Scale free: no entry is compared with an absolute number.  That holds for
// matrices down to about 2^-960 in norm: below, theta * theta and t * apq underflow and accuracy is lost (about 1e6 eps at 2^-1040).
// Out: w[3] the diagonal after the sweeps (unsorted), V[3][3] with the eigenvector of w[k] in column k (orthonormal to a few 2^-53).
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define QN_EIG3_HD __host__ __device__
#define QN_EIG3_FN __host__ __device__ __forceinline__
#else
#define QN_EIG3_HD
#define QN_EIG3_FN inline
#endif
#define QN_EIG3_SWEEPS 6

// one rotation in the (p, q) plane; r is the third index: arp / arq its off-diagonal entries, vp / vq the two columns of V
QN_EIG3_FN void qn_eig3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp, double* vq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double h = t * apq;
  app = app - h; aqq = aqq + h; apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq; arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double a = vp[k], b = vq[k];
    vp[k] = c * a - s * b; vq[k] = s * a + c * b;
  }
}

QN_EIG3_FN void qn_eig3_jacobi(double a00, double a01, double a02, double a11, double a12, double a22, double* w, double (*V)[3]) {
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};      // the columns of V
#pragma unroll 1
  for (int sweep = 0; sweep < QN_EIG3_SWEEPS; sweep++) {
    qn_eig3_rotate(a00, a11, a01, a02, a12, v0, v1);
    qn_eig3_rotate(a00, a22, a02, a01, a12, v0, v2);
    qn_eig3_rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  w[0] = a00; w[1] = a11; w[2] = a22;
#pragma unroll
  for (int k = 0; k < 3; k++) { V[k][0] = v0[k]; V[k][1] = v1[k]; V[k][2] = v2[k]; }
}

namespace qn {

// The exit test off <= 1e-17 * diag lies below half an ulp of diag, so it is not met while the off-diagonal is rounding noise: with an exactly repeated eigenvalue
// (a flat, a collinear or an isotropic covariance) a few matrices in a thousand run all 32 sweeps, rotating noise, and stay as accurate as the rest
// (tests/test_eig3_cpu.py).  The registration results are pinned bit for bit to this text: changing the test changes them.
// symmetric 3x3 eigen-decomposition (cyclic Jacobi, f64); eigenvalues descending, V columns.
QN_EIG3_HD inline void sym_eig3(const double A[6] /* xx xy xz yy yz zz */, double w[3], double V[3][3]) {
  double a[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 32; sweep++) {
    double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (off <= 1e-300 || off <= 1e-17 * diag) break;
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      if (a[p][q] == 0.0) continue;
      double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
      double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
      for (int k = 0; k < 3; k++) { double akp = a[k][p], akq = a[k][q]; a[k][p] = c*akp - s*akq; a[k][q] = s*akp + c*akq; }
#pragma unroll
      for (int k = 0; k < 3; k++) { double apk = a[p][k], aqk = a[q][k]; a[p][k] = c*apk - s*aqk; a[q][k] = s*apk + c*aqk; }
#pragma unroll
      for (int k = 0; k < 3; k++) { double vkp = v[k][p], vkq = v[k][q]; v[k][p] = c*vkp - s*vkq; v[k][q] = s*vkp + c*vkq; }
    }
  }
  // sort descending (3-element network), carrying columns
  double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
  int i0 = 0, i1 = 1, i2 = 2;
  if (e0 < e1) { double t = e0; e0 = e1; e1 = t; int ti = i0; i0 = i1; i1 = ti; }
  if (e1 < e2) { double t = e1; e1 = e2; e2 = t; int ti = i1; i1 = i2; i2 = ti; }
  if (e0 < e1) { double t = e0; e0 = e1; e1 = t; int ti = i0; i0 = i1; i1 = ti; }
  w[0] = e0; w[1] = e1; w[2] = e2;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    V[r][0] = i0 == 0 ? v[r][0] : (i0 == 1 ? v[r][1] : v[r][2]);
    V[r][1] = i1 == 0 ? v[r][0] : (i1 == 1 ? v[r][1] : v[r][2]);
    V[r][2] = i2 == 0 ? v[r][0] : (i2 == 1 ? v[r][1] : v[r][2]);
  }
}

}  // namespace qn
