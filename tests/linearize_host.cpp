// linearize_host.cpp - the host build of accumulate_point_n (csrc/qn_linearize.cuh): the same text the device kernels compile, run on the CPU, one correspondence
// per record with the accumulators starting at zero.  tests/test_linearize_cpu.py checks its output against a 50-digit reference; tests/test_gpu_linearize.py
// compares the device (qn_debug_linearize, which 0) with it bit for bit.
//   linearize_host IN OUT    IN: n records of 37 f64 - Rx (12), Tx (12), pa (3), pb (3), na (3), nb (3), lin -, OUT: n records of 28 f64, the layouts of
//                            qn_debug_linearize's which 0 (include/qn_engine.h).
// Build: g++ -O2 -std=c++17 -ffp-contract=off (no fused multiply-add, as the library is built); a second time with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "qn_linearize.cuh"

static void run(const double* r, double* o) {
  using namespace qn;
  double Rx[3][4], Tx[3][4];
  for (int a = 0; a < 3; a++) for (int b = 0; b < 4; b++) { Rx[a][b] = r[4 * a + b]; Tx[a][b] = r[12 + 4 * a + b]; }
  float4 pa, pb;
  pa.x = (float)r[24]; pa.y = (float)r[25]; pa.z = (float)r[26]; pa.w = 1.f;
  pb.x = (float)r[27]; pb.y = (float)r[28]; pb.z = (float)r[29]; pb.w = 0.f;
  const double na[3] = {r[30], r[31], r[32]}, nb[3] = {r[33], r[34], r[35]};
  double acc[QN_NPART];
  for (int u = 0; u < QN_NPART; u++) acc[u] = 0;
  accumulate_point_n(Rx, Tx, pa, pb, na, nb, r[36] != 0.0, acc);
  for (int u = 0; u < QN_NPART; u++) o[u] = acc[u];
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: linearize_host IN OUT\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "linearize_host: cannot read %s\n", argv[1]); return 1; }
  const size_t si = 37, so = QN_NPART;
  std::vector<double> in, rec(si);
  while (std::fread(rec.data(), sizeof(double), si, f) == si) in.insert(in.end(), rec.begin(), rec.end());
  std::fclose(f);
  const size_t n = in.size() / si;
  std::vector<double> out(so * n);
  for (size_t i = 0; i < n; i++) run(&in[si * i], &out[so * i]);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "linearize_host: cannot write %s\n", argv[2]); return 1; }
  std::printf("linearize_host: %zu records\n", n);
  return 0;
}
