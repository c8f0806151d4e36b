// step_math_host.cpp - the host build of the Gauss-Newton step's small dense f64 routines of csrc/qn_step_math.cuh (d_ldlt_solve6_fast, d_ldlt_solve6, d_so3_exp,
// d_iso_mul, d_is_converged, m3_inverse): the same text the device kernels compile, run on the CPU.  tests/test_step_math_cpu.py checks its output against a
// 50-digit reference; tests/test_gpu_step_math.py compares the device (qn_debug_step_math) with it.
//   step_math_host WHICH IN OUT    IN: n records of f64, OUT: n records of f64, with the strides and layouts of qn_debug_step_math (include/qn_engine.h):
//                                  0 fast solve 43 -> 7, 1 pivoted solve 43 -> 6, 2 the proposal 59 -> 39, 3 d_so3_exp 3 -> 9, 4 m3_inverse 9 -> 9,
//                                  5 d_is_converged 18 -> 3.
// WHICH = 2: d_propose itself works on a GicpState and stays in csrc/qn_gicp_kernels.cuh, which is no plain C++.  Its steps are restated here from the header's
// routines in its order - the lower triangle to the fast solve; where that refuses, its right-hand side handed to the pivoted solve of the full matrix;
// d_so3_exp of d[0:3]; delta; xi = delta x0 by d_iso_mul - so that the hand-over and d_iso_mul run in the host and the sanitizer builds too.
// Build: g++ -O2 -std=c++17 -ffp-contract=off (no fused multiply-add, as the library is built); a second time with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "qn_step_math.cuh"

static const int IN_STRIDE[6] = {43, 43, 59, 3, 9, 18}, OUT_STRIDE[6] = {7, 6, 39, 9, 9, 3};

static void run(int which, const double* r, double* o) {
  using namespace qn;
  SolveWork work;
  if (which == 0) {
    double rhs[6], x[6];
    const bool ok = d_ldlt_solve6_fast(r, r[36], rhs, x, r + 37);
    for (int k = 0; k < 6; k++) o[k] = x[k];
    o[6] = ok ? 1.0 : 0.0;
  } else if (which == 1) {
    for (int k = 0; k < 6; k++) work.rhs[k] = -r[37 + k];
    d_ldlt_solve6(r, r[36], o, &work);
  } else if (which == 2) {
    const double* H = r; const double* b = r + 36; const double lambda = r[42]; const double* x0 = r + 43;
    double Hl[36], rhs[6], dl[6];
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) Hl[6 * i + j] = j <= i ? H[6 * i + j] : 0.0;
    double path = 0.0;
    if (!d_ldlt_solve6_fast(Hl, lambda, rhs, dl, b)) {
      for (int i = 0; i < 6; i++) work.rhs[i] = rhs[i];
      double d[6];
      d_ldlt_solve6(H, lambda, d, &work);
      for (int i = 0; i < 6; i++) dl[i] = d[i];
      path = 1.0;
    }
    double R[3][3]; d_so3_exp(dl, R);
    double delta[16], xi[16];
    for (int i = 0; i < 16; i++) delta[i] = 0;
    for (int a = 0; a < 3; a++) { for (int c = 0; c < 3; c++) delta[4 * a + c] = R[a][c]; delta[4 * a + 3] = dl[3 + a]; }
    delta[15] = 1.0;
    d_iso_mul(delta, x0, xi);
    for (int k = 0; k < 6; k++) o[k] = dl[k];
    for (int k = 0; k < 16; k++) { o[6 + k] = delta[k]; o[22 + k] = xi[k]; }
    o[38] = path;
  } else if (which == 3) {
    double R[3][3];
    d_so3_exp(r, R);
    for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) o[3 * a + c] = R[a][c];
  } else if (which == 4) {
    M3 m;
    for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) m.m[a][c] = r[3 * a + c];
    const M3 v = m3_inverse(m);
    for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) o[3 * a + c] = v.m[a][c];
  } else {
    GicpConfig cfg = {};
    cfg.rotation_epsilon = r[16]; cfg.transformation_epsilon = r[17];
    double mr, mt;
    o[0] = d_is_converged(r, cfg, &mr, &mt) ? 1.0 : 0.0;
    o[1] = mr; o[2] = mt;
  }
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: step_math_host WHICH IN OUT\n"); return 2; }
  const int which = std::atoi(argv[1]);
  if (which < 0 || which > 5) { std::fprintf(stderr, "step_math_host: WHICH is 0 .. 5\n"); return 2; }
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::fprintf(stderr, "step_math_host: cannot read %s\n", argv[2]); return 1; }
  const size_t si = IN_STRIDE[which], so = OUT_STRIDE[which];
  std::vector<double> in, rec(si);
  while (std::fread(rec.data(), sizeof(double), si, f) == si) in.insert(in.end(), rec.begin(), rec.end());
  std::fclose(f);
  const size_t n = in.size() / si;
  std::vector<double> out(so * n);
  for (size_t i = 0; i < n; i++) run(which, &in[si * i], &out[so * i]);
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "step_math_host: cannot write %s\n", argv[3]); return 1; }
  std::printf("step_math_host: %zu records of routine %d\n", n, which);
  return 0;
}
