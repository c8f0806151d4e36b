// eig3_host.cpp - the host build of the two 3 x 3 symmetric eigen solvers of csrc/qn_eig3.cuh (qn_eig3_jacobi, qn::sym_eig3): the same text the device
// kernels compile, run on the CPU.  tests/test_eig3_cpu.py checks its output against a 50-digit reference; tests/test_gpu_eig3.py compares the device with it.
//   eig3_host IN OUT    IN: n records of six f64 (xx, xy, xz, yy, yz, zz).  OUT, all f64: w of qn_eig3_jacobi [3 n], its V [9 n] (row major, the eigenvector
//                       of w[k] in column k), then w and V of sym_eig3 in the same layout.
// Build: g++ -O2 -std=c++17 -ffp-contract=off (no fused multiply-add, as the library is built).
#include <cstdio>
#include <vector>
#include "qn_eig3.cuh"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: eig3_host IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "eig3_host: cannot read %s\n", argv[1]); return 1; }
  std::vector<double> a;
  double rec[6];
  while (std::fread(rec, sizeof(double), 6, f) == 6) a.insert(a.end(), rec, rec + 6);
  std::fclose(f);
  const size_t n = a.size() / 6;
  std::vector<double> out(24 * n);
  double* wj = out.data(); double* vj = wj + 3 * n; double* ws = vj + 9 * n; double* vs = ws + 3 * n;
  for (size_t i = 0; i < n; i++) {
    const double* m = &a[6 * i];
    double w[3], V[3][3];
    qn_eig3_jacobi(m[0], m[1], m[2], m[3], m[4], m[5], w, V);
    for (int r = 0; r < 3; r++) { wj[3 * i + r] = w[r]; for (int k = 0; k < 3; k++) vj[9 * i + 3 * r + k] = V[r][k]; }
    qn::sym_eig3(m, w, V);
    for (int r = 0; r < 3; r++) { ws[3 * i + r] = w[r]; for (int k = 0; k < 3; k++) vs[9 * i + 3 * r + k] = V[r][k]; }
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "eig3_host: cannot write %s\n", argv[2]); return 1; }
  std::printf("eig3_host: %zu matrices\n", n);
  return 0;
}
