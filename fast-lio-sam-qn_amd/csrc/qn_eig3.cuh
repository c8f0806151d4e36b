// qn_eig3.cuh - the eigen decomposition of a symmetric 3 x 3 matrix in f64 by cyclic Jacobi rotations, for one thread (qn_mapnormals.hip).  Plain C++ as
// well, so that a host build can check it against LAPACK.
// A = (a00, a01, a02, a11, a12, a22), upper triangle by rows.  QN_EIG3_SWEEPS sweeps over the pairs (0, 1), (0, 2), (1, 2); a rotation whose off-diagonal
// entry is already zero is skipped.  Convergence is quadratic: from any start three sweeps leave the off-diagonal norm below 2^-53 of the matrix norm and the
// fourth squares that again, so six is a fixed count with room, the same in every lane.  The rotation is the textbook one (Rutishauser): t = tan of the angle,
// the smaller root of t^2 + 2 theta t - 1 = 0 with theta = (aqq - app) / (2 apq), |t| <= 1, which keeps the diagonal updates app - t apq / aqq + t apq
// backward stable; theta^2 overflowing to infinity gives t = 0, the right limit.  Scale free: no entry is compared with an absolute number.
// Out: w[3] the diagonal after the sweeps (unsorted), V[3][3] with the eigenvector of w[k] in column k (orthonormal to a few 2^-53).
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define QN_EIG3_FN __host__ __device__ __forceinline__
#else
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
