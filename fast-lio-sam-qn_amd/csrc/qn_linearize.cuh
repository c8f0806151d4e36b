// qn_linearize.cuh - one correspondence's contribution to the 28 sums of a GICP linearisation (accumulate_point_n), for one thread.  Plain C++ as well as HIP,
// like qn_step_math.cuh, whose M3 and m3_inverse it uses: a host build can check it against a high-precision reference (tests/linearize_host.cpp,
// tests/test_linearize_cpu.py; the device build: qn_debug_linearize, tests/test_gpu_linearize.py).  The function body is the one the kernels have always
// compiled - under hipcc it is __device__ __forceinline__ with the signature it had.  emit_point (qn_tick.cuh) restates this arithmetic term for term, seven values at a
// time; the tests hold the two to each other bit for bit.
#pragma once
#include "qn_step_math.cuh"

namespace qn {

#define QN_NPART 28            // 21 (upper H) + 6 (b) + 1 (cost)

#if !defined(__HIPCC__)
struct float4 { float x, y, z, w; };      // (the host build: a point as the kernels hand it over)
#endif

// one correspondence's contribution: M = (C_B + R C_A R^T)^-1, e = mu_B - T mu_A, J = [skew(T mu_A) | -I];
// acc[0..20] += upper J^T M J, acc[21..26] += J^T M e (both only when `lin`), acc[27] += e^T M e.
// PLANE-regularised covariances are exactly C = I - 0.999 n n^T, so the kernels carry the normals (3 f64 per point
// instead of 6):  C_B + R C_A R^T = (I - 0.999 n_B n_B^T) + (I - 0.999 m m^T),  m = R n_A.
// Rx: 3x4 pose whose rotation block transforms the source normal (x0); Tx: 3x4 pose the residual is evaluated at (x0 when linearising,
// xi in an LM trial pass).  J = [skew(T mu_A) | -I] is mostly zeros and ones: the products are written out term by term, in the order
// of the dense formula, so the sums are bit-identical to it (adding an exact 0 or multiplying by -1 does not round).
QN_STEP_FN void accumulate_point_n(const double (*Rx)[4], const double (*Tx)[4], const float4 pa, const float4 pb,
                                   const double na[3], const double nb[3], const bool lin, double acc[QN_NPART]) {
  double m[3];
#pragma unroll
  for (int a = 0; a < 3; a++) m[a] = Rx[a][0] * na[0] + Rx[a][1] * na[1] + Rx[a][2] * na[2];
  // R C_A R^T = R R^T - 0.999 m m^T.  R R^T is I to rounding for every pose the optimiser builds from the identity guess of
  // loop_closure.cpp:124, but NOT for a caller's f32 guess with a rotation (pcl::Registration::align(output, guess)): its rows are
  // orthonormal to 6e-8 only, the reference multiplies with the matrix as it is, and the difference is 1e-7 of the cost.
  M3 rcr;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++) {      // the upper triangle, mirrored: the sum of two symmetric matrices, formed once per pair (a, b) - its inverse then has three cofactors less to form
      const double g = Rx[a][0] * Rx[b][0] + Rx[a][1] * Rx[b][1] + Rx[a][2] * Rx[b][2];
      rcr.m[a][b] = ((a == b ? 1.0 : 0.0) - 0.999 * nb[a] * nb[b]) + (g - 0.999 * m[a] * m[b]);
      rcr.m[b][a] = rcr.m[a][b];
    }
  const M3 M = m3_inverse(rcr);
  const double mA[3] = {(double)pa.x, (double)pa.y, (double)pa.z};
  double tA[3], e[3], Me[3];
#pragma unroll
  for (int r = 0; r < 3; r++) tA[r] = Tx[r][0] * mA[0] + Tx[r][1] * mA[1] + Tx[r][2] * mA[2] + Tx[r][3];
  e[0] = (double)pb.x - tA[0]; e[1] = (double)pb.y - tA[1]; e[2] = (double)pb.z - tA[2];
#pragma unroll
  for (int r = 0; r < 3; r++) Me[r] = M.m[r][0] * e[0] + M.m[r][1] * e[1] + M.m[r][2] * e[2];
  acc[27] += e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2];
  if (lin) {
    const double x = tA[0], y = tA[1], z = tA[2];
    // MS = M skew(tA): column 0 = M (0, z, -y), column 1 = M (-z, 0, x), column 2 = M (y, -x, 0);  M J = [MS | -M]
    double MS[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) { MS[r][0] = M.m[r][1] * z + M.m[r][2] * (-y); MS[r][1] = M.m[r][0] * (-z) + M.m[r][2] * x; MS[r][2] = M.m[r][0] * y + M.m[r][1] * (-x); }
    // upper J^T M J, row-major over (r, c >= r):  rows 0..2 = skew(tA)^T [MS | -M], rows 3..5 = M
    // row 0: J[:,0] = (0, z, -y)
    acc[0] += z * MS[1][0] + (-y) * MS[2][0]; acc[1] += z * MS[1][1] + (-y) * MS[2][1]; acc[2] += z * MS[1][2] + (-y) * MS[2][2];
    // (the rotation-translation block -skew(tA)^T M is minus the TRANSPOSE of MS: M is symmetric bit for bit - the inverse of a mirrored matrix - so z (-M10) + (-y)(-M20)
    //  and -(M01 z + M02 (-y)) are the same products and the same rounded sum: nine entries without a multiplication)
    acc[3] += -MS[0][0]; acc[4] += -MS[1][0]; acc[5] += -MS[2][0];
    // row 1: J[:,1] = (-z, 0, x)
    acc[6] += (-z) * MS[0][1] + x * MS[2][1]; acc[7] += (-z) * MS[0][2] + x * MS[2][2];
    acc[8] += -MS[0][1]; acc[9] += -MS[1][1]; acc[10] += -MS[2][1];
    // row 2: J[:,2] = (y, -x, 0)
    acc[11] += y * MS[0][2] + (-x) * MS[1][2];
    acc[12] += -MS[0][2]; acc[13] += -MS[1][2]; acc[14] += -MS[2][2];
    // rows 3..5: (-I)^T (-M) = M
    acc[15] += M.m[0][0]; acc[16] += M.m[0][1]; acc[17] += M.m[0][2]; acc[18] += M.m[1][1]; acc[19] += M.m[1][2]; acc[20] += M.m[2][2];
    // J^T M e
    acc[21] += z * Me[1] + (-y) * Me[2]; acc[22] += (-z) * Me[0] + x * Me[2]; acc[23] += y * Me[0] + (-x) * Me[1];
    acc[24] += -Me[0]; acc[25] += -Me[1]; acc[26] += -Me[2];
  }
}

}  // namespace qn
