#include <chrono>
// qn_quatro_host.inc - host side of the Quatro coarse stage (included at the end of qn_engine.hip).
// quatro<PointType>::align (call site fast_lio_sam_qn/src/loop_closure.cpp:144, ctor :18-27):
//   FPFH of both clouds and the 33-D feature matching run on the GPU (qn_quatro_kernels.cuh); the
//   small-N tail - distance gate, seeded tuple test, TEASER++ solve with Quatro's yaw-only GNC-TLS
//   rotation (<= ~200 correspondences, SURVEY.md 7.1 step 9 "small-N solve (host first)") - is host C++.
#include "qn_quatro_kernels.cuh"
#include <algorithm>
#include <array>
#include <memory>
#include <numeric>
#include <utility>

// ------------------------------------------------------------------ host solver (f64)
namespace qnq {

typedef std::pair<int, int> Pair;

// Fixed-width bit sets on the stack (W 64-bit words): the branch and bound below copies one per tree node, and heap-backed sets made the
// clique search the largest host cost of a 100k-point Quatro align (3.6 ms of 9).
template <int W>
struct BitSet {
  uint64_t w[W];
  BitSet() { for (int k = 0; k < W; k++) w[k] = 0; }
  void set(int i) { w[i >> 6] |= 1ull << (i & 63); }
  void clr(int i) { w[i >> 6] &= ~(1ull << (i & 63)); }
  bool test(int i) const { return (w[i >> 6] >> (i & 63)) & 1ull; }
  bool empty() const { uint64_t x = 0; for (int k = 0; k < W; k++) x |= w[k]; return x == 0; }
  int count() const { int c = 0; for (int k = 0; k < W; k++) c += __builtin_popcountll(w[k]); return c; }
  int first() const { for (int k = 0; k < W; k++) if (w[k]) return k * 64 + __builtin_ctzll(w[k]); return -1; }
  BitSet operator&(const BitSet& o) const { BitSet r; for (int k = 0; k < W; k++) r.w[k] = w[k] & o.w[k]; return r; }
};

// Maximum clique by branch and bound with a greedy-colouring bound (Tomita & Seki style), then the
// lexicographically smallest maximum clique is built vertex by vertex (PMC's own tie-break is arbitrary).
template <int W>
struct CliqueSolver {
  int n; std::vector<BitSet<W>> adj; int best; int target;
  std::unique_ptr<int[]> order_buf, colour_buf;    // one slab for the whole recursion: depth d uses [d * n, (d + 1) * n) - NOT zero-filled (2 x 53 KB at n = 115 were a fifth of the solve)
  std::vector<int> path, witness;                  // the current branch; the clique that set `best` (empty if `known` was never beaten)
  explicit CliqueSolver(int n_) : n(n_), adj(n_), best(0), target(1 << 30), order_buf(new int[(size_t)(n_ + 1) * n_]), colour_buf(new int[(size_t)(n_ + 1) * n_]), path(n_ + 1) {}
  void expand(BitSet<W> P, int size, int depth) {
    if (best >= target) return;
    if (P.empty()) { if (size > best) { best = size; witness.assign(path.begin(), path.begin() + size); } return; }
    // greedy colouring of P: vertices in colour-class order, bound = colour index
    int* order = order_buf.get() + (size_t)depth * n; int* colour = colour_buf.get() + (size_t)depth * n; int cnt = 0;
    BitSet<W> U = P; int c = 0;
    while (!U.empty()) {
      c++; BitSet<W> Q = U;
      while (!Q.empty()) { const int v = Q.first(); Q.clr(v); U.clr(v); for (int k = 0; k < W; k++) Q.w[k] &= ~adj[v].w[k]; order[cnt] = v; colour[cnt] = c; cnt++; }
    }
    for (int t = cnt - 1; t >= 0; t--) {
      if (size + colour[t] <= best) return;
      const int v = order[t];
      path[size] = v;
      expand(P & adj[v], size + 1, depth + 1);
      if (best >= target) return;
      P.clr(v);
    }
  }
  // the size of a maximum clique of P if it exceeds `known` (else `known`); stops as soon as stop_at is reached.  A caller that only asks
  // "is there a clique of size >= k" passes known = k - 1: every branch that cannot reach k is cut by the colouring bound.
  int max_size(const BitSet<W>& P, int stop_at, int known = 0) { best = known; target = stop_at; witness.clear(); expand(P, 0, 0); return best; }
};

template <int W>
static std::vector<int> max_clique_lex_w(const std::vector<uint8_t>& a, int n) {
  // The search runs on RELABELLED vertices (non-increasing degree: the greedy colouring then starts its classes with the high-degree
  // vertices, the classic MCQ initial order - the colour bound gets tighter and the proof of optimality shorter); sizes do not depend on
  // labels, and the lexicographic construction below works in the original labels, translating each candidate set.
  std::vector<int> deg(n, 0), perm(n), inv(n);
  std::vector<BitSet<W>> adj0(n);                                        // original labels: the byte rows packed 64 at a time, degrees by popcount
  for (int i = 0; i < n; i++) {
    const uint8_t* row = a.data() + (size_t)i * n;
    for (int j0 = 0; j0 < n; j0 += 64) { uint64_t w = 0; const int je = std::min(n, j0 + 64); for (int j = j0; j < je; j++) w |= (uint64_t)(row[j] != 0) << (j - j0); adj0[i].w[j0 >> 6] = w; }
    adj0[i].clr(i);
    deg[i] = adj0[i].count();
  }
  for (int i = 0; i < n; i++) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return deg[x] > deg[y]; });
  for (int k = 0; k < n; k++) inv[perm[k]] = k;
  CliqueSolver<W> cs(n);
  for (int i = 0; i < n; i++) { BitSet<W>& r = cs.adj[inv[i]]; for (int k = 0; k < W; k++) { uint64_t w = adj0[i].w[k]; while (w) { const int j = k * 64 + __builtin_ctzll(w); w &= w - 1; r.set(inv[j]); } } }
  auto relabel = [&](const BitSet<W>& P) { BitSet<W> R; for (int v = 0; v < n; v++) if (P.test(v)) R.set(inv[v]); return R; };
  BitSet<W> all; for (int i = 0; i < n; i++) all.set(i);
  const auto tq0 = std::chrono::steady_clock::now();
  int greedy = 0; BitSet<W> wit;                                         // a greedy clique (highest degree first): the initial lower bound, and the first
  { BitSet<W> P = all; while (!P.empty()) { const int v = P.first(); wit.set(perm[v]); P = P & cs.adj[v]; greedy++; } }      // WITNESS (a maximum clique in original labels)
  const int omega = cs.max_size(all, 1 << 30, greedy);
  if (!cs.witness.empty()) { wit = BitSet<W>(); for (int v : cs.witness) wit.set(perm[v]); }
  const auto tq1 = std::chrono::steady_clock::now();
  // members of a clique of size k inside P have at least k - 1 neighbours inside P: peel everything else off (repeatedly) before searching
  auto peel = [&](BitSet<W> P, int k) {
    for (bool changed = true; changed;) {
      changed = false;
      for (int v = 0; v < n; v++) if (P.test(v) && (P & adj0[v]).count() < k - 1) { P.clr(v); changed = true; }
    }
    return P;
  };
  // Lexicographically smallest maximum clique, vertex by vertex: v joins if some maximum clique contains the chosen ones and v.  A known maximum
  // clique that contains them (the witness) answers that for its own members without a search; only vertices outside it need one, and a
  // successful search replaces the witness.
  std::vector<int> chosen; BitSet<W> cand = all;
  for (int v = 0; v < n && (int)chosen.size() < omega; v++) {
    if (!cand.test(v)) continue;
    BitSet<W> rest = cand & adj0[v];
    for (int u = 0; u <= v; u++) if (u < n) rest.clr(u);                 // later members are larger than v
    const int need = omega - (int)chosen.size() - 1;
    bool ok = wit.test(v) || need == 0;
    if (!ok) {
      rest = peel(rest, need);
      if (rest.count() >= need && cs.max_size(relabel(rest), need, need - 1) >= need) {
        ok = true; wit = BitSet<W>(); for (int c : chosen) wit.set(c); wit.set(v); for (int u : cs.witness) wit.set(perm[u]);
      }
    }
    if (ok) { chosen.push_back(v); cand = rest; }
  }
  if (getenv("QN_SOLVE_TIMING")) fprintf(stderr, "clique: n %d greedy %d omega %d  search %.3f ms  lexicographic %.3f ms\n", n, greedy, omega, std::chrono::duration<double, std::milli>(tq1 - tq0).count(),
                                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq1).count());
  return chosen;
}
static std::vector<int> max_clique_lex(const std::vector<uint8_t>& a, int n) {       // the cap keeps n <= ~203 in practice; advancedMatching has none
  if (n <= 256) return max_clique_lex_w<4>(a, n);
  if (n <= 1024) return max_clique_lex_w<16>(a, n);
  if (n <= 4096) return max_clique_lex_w<64>(a, n);
  if (n <= 16384) return max_clique_lex_w<256>(a, n);
  return max_clique_lex_w<2048>(a, n);
}

static double tls_estimate(std::vector<double> X, double alpha) {      // TEASER++ TLSEstimator, one axis
  if (!(alpha > 0)) {
    // noise_bound = 0: the sweep below would weigh by 1 / 0 and every estimate would be NaN (the translation came out 0 whatever the data).  Defined as the
    // estimate's limit for a bound going to 0: the value the most measurements share exactly, the smallest one on a tie (the first the sweep meets)
    X.erase(std::remove_if(X.begin(), X.end(), [](double v) { return v != v; }), X.end());
    std::sort(X.begin(), X.end());
    double best = 0; int run = 0, best_run = 0;
    for (size_t i = 0; i < X.size(); i++) { run = (i > 0 && X[i] == X[i - 1]) ? run + 1 : 1; if (run > best_run) { best_run = run; best = X[i]; } }
    return best;
  }
  const int N = (int)X.size();
  std::vector<std::pair<double, int>> h; h.reserve(2 * N);
  for (int i = 0; i < N; i++) { h.emplace_back(X[i] - alpha, i + 1); h.emplace_back(X[i] + alpha, -i - 1); }
  std::sort(h.begin(), h.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first || (a.first == b.first && a.second > b.second); });
  const double wgt = 1.0 / (alpha * alpha);
  double out_pen = alpha * N, sxw = 0, sw = 0, sx = 0, sxx = 0, best_cost = 0, best_x = 0; int card = 0; bool have = false;
  for (const auto& e : h) {
    const int idx = std::abs(e.second) - 1, sgn = e.second > 0 ? 1 : -1;
    card += sgn; sw += sgn * wgt; sxw += sgn * wgt * X[idx]; out_pen -= sgn * alpha; sx += sgn * X[idx]; sxx += sgn * X[idx] * X[idx];
    const double xh = sxw / sw;
    const double cost = (card * xh * xh + sxx - 2 * sx * xh) + out_pen;
    if (cost == cost && (!have || cost < best_cost)) { best_cost = cost; best_x = xh; have = true; }
  }
  return best_x;
}


// TEASER++ ScalarTLSEstimator::estimate with one range per measurement (the scale stage: the bound on a TIM's norm ratio is beta / |a_ij|): the same sweep over the sorted interval
// ends, weights 1 / range^2 for the estimate, the UNWEIGHTED squared residuals of the consensus set + the ranges of everything outside it as the cost (upstream registration.cc,
// as recalled - un-vendored, parity unpinned).  inl[k] = |X[k] - estimate| <= R[k].
static double tls_estimate_ranges(const std::vector<double>& X, const std::vector<double>& R, std::vector<uint8_t>* inl) {
  const int N = (int)X.size();
  std::vector<std::pair<double, int>> h; h.reserve(2 * (size_t)N);
  double out_pen = 0;
  for (int i = 0; i < N; i++) { h.emplace_back(X[i] - R[i], i + 1); h.emplace_back(X[i] + R[i], -i - 1); out_pen += R[i]; }
  std::sort(h.begin(), h.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first || (a.first == b.first && a.second > b.second); });
  double sxw = 0, sw = 0, sx = 0, sxx = 0, best_cost = 0, best_x = 1.0; int card = 0; bool have = false;
  for (const auto& e : h) {
    const int idx = std::abs(e.second) - 1, sgn = e.second > 0 ? 1 : -1;
    const double wgt = 1.0 / (R[idx] * R[idx]);
    card += sgn; sw += sgn * wgt; sxw += sgn * wgt * X[idx]; out_pen -= sgn * R[idx]; sx += sgn * X[idx]; sxx += sgn * X[idx] * X[idx];
    const double xh = sxw / sw;
    const double cost = (card * xh * xh + sxx - 2 * sx * xh) + out_pen;
    if (cost == cost && (!have || cost < best_cost)) { best_cost = cost; best_x = xh; have = true; }
  }
  if (inl) { inl->assign(N, 0); for (int i = 0; i < N; i++) (*inl)[i] = (uint8_t)(std::fabs(X[i] - best_x) <= R[i]); }
  return best_x;
}

struct SolveOut { double T[16]; int valid; std::vector<int> clique; int rot_iterations; double scale; };
typedef std::array<double, 3> P3;

// TEASER++ RobustRegistrationSolver::solve with Quatro's rotation on M matched point pairs (S[k] <-> D[k])
static void solve(const std::vector<P3>& S, const std::vector<P3>& D, const qn_quatro_params& p, SolveOut* out) {
  for (int i = 0; i < 16; i++) out->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  out->valid = 0; out->clique.clear(); out->rot_iterations = 0; out->scale = 1.0;
  const int M = (int)S.size();
  if (M == 0) return;
  // translation-invariant measurements + scale-consistency graph (scale fixed to 1 unless estimate_scale - estimat_scale_, loop_closure.h:44 / loop_closure.cpp:24 - is set)
  const auto ts0 = std::chrono::steady_clock::now();
  const double beta = 2.0 * p.noise_bound;
  std::vector<uint8_t> adj((size_t)M * M, 0);
  double scale = 1.0;
  if (p.estimate_scale) {
    // TEASER++ TLSScaleSolver::solveForScale over ALL M (M - 1) / 2 TIMs: s_ij = |b_ij| / |a_ij| with bound beta / |a_ij|, truncated least squares by adaptive voting;
    // the TIMs inside their bound of the estimate are the edges of the consistency graph.  A TIM between two coincident source points carries no scale (|a| = 0): no edge.
    std::vector<double> X, Rg; std::vector<std::pair<int, int>> ij;
    X.reserve((size_t)M * (M - 1) / 2); Rg.reserve(X.capacity()); ij.reserve(X.capacity());
    for (int i = 0; i < M; i++) for (int j = i + 1; j < M; j++) {
      const double a0 = S[j][0] - S[i][0], a1 = S[j][1] - S[i][1], a2 = S[j][2] - S[i][2], b0 = D[j][0] - D[i][0], b1 = D[j][1] - D[i][1], b2 = D[j][2] - D[i][2];
      const double na = std::sqrt((a0 * a0 + a1 * a1) + a2 * a2), nb = std::sqrt((b0 * b0 + b1 * b1) + b2 * b2);
      if (!(na > 0.0) || !(nb == nb)) continue;
      X.push_back(nb / na); Rg.push_back(beta / na); ij.emplace_back(i, j);
    }
    if (X.empty()) return;
    std::vector<uint8_t> inl;
    scale = tls_estimate_ranges(X, Rg, &inl);
    if (!(scale > 0.0) || !(scale == scale)) return;                     // (no consensus on a positive scale: not a registration)
    for (size_t k = 0; k < ij.size(); k++) if (inl[k]) { adj[(size_t)ij[k].first * M + ij[k].second] = 1; adj[(size_t)ij[k].second * M + ij[k].first] = 1; }
    out->scale = scale;
  } else
  {   // same arithmetic, term for term ((0 + a0^2) + a1^2) + a2^2, two correctly rounded square roots), in structure-of-arrays form with a branch-free inner loop: vectorises
      // (13 k square roots at M = 115 were half of the solve); the upper triangle is mirrored afterwards
    std::vector<double> soa((size_t)6 * M);
    double* sx = soa.data(); double* sy = sx + M; double* sz = sy + M; double* dx = sz + M; double* dy = dx + M; double* dz = dy + M;
    for (int i = 0; i < M; i++) { sx[i] = S[i][0]; sy[i] = S[i][1]; sz[i] = S[i][2]; dx[i] = D[i][0]; dy[i] = D[i][1]; dz[i] = D[i][2]; }
    for (int i = 0; i < M; i++) {
      uint8_t* row = adj.data() + (size_t)i * M;
      const double six = sx[i], siy = sy[i], siz = sz[i], dix = dx[i], diy = dy[i], diz = dz[i];
      for (int j = i + 1; j < M; j++) {
        const double a0 = sx[j] - six, a1 = sy[j] - siy, a2 = sz[j] - siz, b0 = dx[j] - dix, b1 = dy[j] - diy, b2 = dz[j] - diz;
        const double na = (a0 * a0 + a1 * a1) + a2 * a2, nb = (b0 * b0 + b1 * b1) + b2 * b2;
        row[j] = (uint8_t)(std::fabs(std::sqrt(nb) - std::sqrt(na)) <= beta);
      }
    }
    for (int i = 0; i < M; i++) for (int j = i + 1; j < M; j++) adj[(size_t)j * M + i] = adj[(size_t)i * M + j];
  }
  const auto ts1 = std::chrono::steady_clock::now();
  const std::vector<int> C = max_clique_lex(adj, M);
  const auto ts2 = std::chrono::steady_clock::now();
  out->clique = C;
  const int m = (int)C.size();
  if (m <= 1) return;
  std::vector<P3> A(m), B(m);                                            // chain TIMs over the clique
  for (int i = 0; i < m; i++) { const int root = C[i], leaf = C[(i + 1) % m]; for (int d = 0; d < 3; d++) { A[i][d] = S[leaf][d] - S[root][d]; B[i][d] = D[leaf][d] - D[root][d]; } }
  if (p.estimate_scale) for (int i = 0; i < m; i++) for (int d = 0; d < 3; d++) B[i][d] *= 1.0 / scale;      // "remove scaling for rotation estimation": pruned_dst_tims_ *= (1 / solution_.scale)
  // Quatro rotation: graduated non-convexity, truncated least squares, yaw only.
  // Noise bound of the rotation stage: RobustRegistrationSolver::solve() rescales the GNC solver's bound before calling it -
  // `params.noise_bound *= (2 / solution_.scale)` (a TIM is the difference of two measurements, each within noise_bound) - and
  // solveForRotation squares THAT: (2 noise_bound)^2 with scale = 1.  (ADVICE r1 asked; upstream TEASER++ registration.cc, not in
  // /root/reference - un-vendored, parity unpinned.)
  const double nbr = p.estimate_scale ? p.noise_bound * (2.0 / scale) : 2.0 * p.noise_bound;      // params.noise_bound *= (2 / solution_.scale)
  double nb2 = p.estimate_scale ? nbr * nbr : 4.0 * p.noise_bound * p.noise_bound; if (nb2 < 1e-16) nb2 = 1e-2;
  std::vector<double> w(m, 1.0), r2(m);
  double mu = 1.0, prev = std::numeric_limits<double>::infinity(), cs = 1.0, sn = 0.0;
  for (int it = 0; it < p.rot_max_iter; it++) {
    out->rot_iterations = it + 1;
    double num = 0, den = 0;
    for (int i = 0; i < m; i++) { num += w[i] * (A[i][0] * B[i][1] - A[i][1] * B[i][0]); den += w[i] * (A[i][0] * B[i][0] + A[i][1] * B[i][1]); }
    const double yaw = std::atan2(num, den); cs = std::cos(yaw); sn = std::sin(yaw);
    double worst = 0;
    for (int i = 0; i < m; i++) {
      const double ex = B[i][0] - (cs * A[i][0] - sn * A[i][1]), ey = B[i][1] - (sn * A[i][0] + cs * A[i][1]), ez = B[i][2] - A[i][2];
      r2[i] = ex * ex + ey * ey + ez * ez; worst = std::max(worst, r2[i]);
    }
    if (it == 0) { mu = 1.0 / (2.0 * worst / nb2 - 1.0); if (mu <= 0) break; }
    const double hi = (mu + 1) / mu * nb2, lo = mu / (mu + 1) * nb2;
    double cost = 0;
    for (int i = 0; i < m; i++) {
      cost += w[i] * r2[i];
      w[i] = r2[i] >= hi ? 0.0 : (r2[i] <= lo ? 1.0 : std::sqrt(nb2 * mu * (mu + 1) / r2[i]) - mu);
    }
    const double change = std::fabs(cost - prev);
    mu *= p.rot_gnc_factor; prev = cost;
    if (change < p.rot_cost_diff_thr) break;
  }
  double t[3];
  for (int d = 0; d < 3; d++) {
    std::vector<double> X(m);
    for (int i = 0; i < m; i++) {
      const P3& s = S[C[i]];
      const double rs[3] = {cs * s[0] - sn * s[1], sn * s[0] + cs * s[1], s[2]};
      X[i] = D[C[i]][d] - (p.estimate_scale ? scale * rs[d] : rs[d]);      // solveForTranslation(scale * R * src, dst)
    }
    t[d] = tls_estimate(X, p.noise_bound);
  }
  const double R[9] = {cs, -sn, 0, sn, cs, 0, 0, 0, 1};
  for (int a = 0; a < 3; a++) { for (int b = 0; b < 3; b++) out->T[4 * a + b] = R[3 * a + b]; out->T[4 * a + 3] = t[a]; }
  out->valid = 1;
  if (getenv("QN_SOLVE_TIMING")) fprintf(stderr, "solve: M %d  graph %.3f ms  clique %.3f ms  gnc + tls %.3f ms\n", M, std::chrono::duration<double, std::milli>(ts1 - ts0).count(),
                                        std::chrono::duration<double, std::milli>(ts2 - ts1).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts2).count());
}

// what the device-side Matcher tail hands over (k_collect_corres): the selected correspondences and their points
struct TailResult {
  std::vector<Pair> mutual;            // cross-checked (+ gated) matches before the tuple test, sorted (debug read-back only)
  std::vector<Pair> corres;            // after the tuple test, sorted unique (src idx, dst idx)
  std::vector<P3> S, D;                // matched points, row k = corres[k]
};

}  // namespace qnq

// ------------------------------------------------------------------ C-ABI
extern "C" void qn_quatro_default_params(qn_quatro_params* p) {            // reference's effective values (SURVEY Appendix C)
  if (!p) return;
  p->fpfh_normal_radius = 0.9; p->fpfh_radius = 1.5; p->noise_bound = 0.3; p->rot_gnc_factor = 1.4; p->rot_cost_diff_thr = 1e-4;
  p->rot_max_iter = 50; p->estimate_scale = 0; p->use_optimized_matching = 1; p->distance_threshold = 35.0; p->max_num_corres = 200;
  p->rng_seed = 1; p->tuple_scale = 0.95;
}
extern "C" int qn_quatro_set_params(qn_ctx* c, const qn_quatro_params* p) {
  if (!c || !p) return QN_ERR_INVALID_ARG;
  // estimate_scale (estimat_scale_, loop_closure.h:44; the shipped config passes false, config.yaml:37): TEASER++'s TLS scale solver on the host (qnq::solve).
  // use_optimized_matching = 0 selects Matcher::advancedMatching (no distance gate, no correspondence cap).
  if (!(p->fpfh_normal_radius > 0) || !(p->fpfh_radius > 0) || !(p->noise_bound >= 0) || p->rot_max_iter < 1 || p->max_num_corres < 3 ||
      !(p->tuple_scale > 0)) return QN_ERR_INVALID_ARG;
  c->qparams = *p; c->qparams_set = true;
  return QN_OK;
}

static int quatro_alloc(qn_ctx* c) {
  if (c->q_ready) return QN_OK;
  const size_t n = c->max_points;
  for (int w = 0; w < 2; w++) {
    HIPCHK(c, hipMalloc(&c->q_normals[w], sizeof(float4) * n));
    HIPCHK(c, hipMalloc(&c->q_spfh[w], sizeof(float) * QN_FROW * n));
    HIPCHK(c, hipMalloc(&c->q_fpfh_s[w], sizeof(float) * QN_FROW * n));
    HIPCHK(c, hipMalloc(&c->q_fpfh[w], sizeof(float) * QN_FROW * n));
    HIPCHK(c, hipMalloc(&c->q_key[w], sizeof(unsigned long long) * n));
    HIPCHK(c, hipMalloc(&c->q_pair[w], sizeof(float) * 68 * (n / 2 + 1)));
    HIPCHK(c, hipMalloc(&c->q_pair_hash[w], sizeof(uint32_t) * (n + 2)));
  }
  HIPCHK(c, hipMalloc(&c->q_hit, sizeof(uint32_t) * (n + 1)));
  HIPCHK(c, hipMalloc(&c->q_list, sizeof(uint32_t) * (n + 1)));
  HIPCHK(c, hipMalloc(&c->q_sel, sizeof(uint32_t) * (n + 1)));
  HIPCHK(c, hipMalloc(&c->q_pairs, sizeof(uint2) * n));
  HIPCHK(c, hipMalloc(&c->q_counts, sizeof(uint32_t) * 8));                  // [0] hit counter, [1..2] query de-duplication, [4..5] tickets of k_means2
  HIPCHK(c, hipMalloc(&c->q_T, sizeof(double) * 16));
  HIPCHK(c, hipMalloc(&c->q_mean, sizeof(float) * 8));
  HIPCHK(c, hipMalloc(&c->q_mean_psum, sizeof(double) * QN_MEAN_BLOCKS * 3 * 2));
  HIPCHK(c, hipHostMalloc(&c->q_host, sizeof(QuatroTailOut) + sizeof(QuatroCorr) * n, hipHostMallocDefault));
  {                                                                          // matrix-core feature matching (qn_feat_mm.cuh)
    const size_t tiles = (n + 31) / 32 + 1;
    HIPCHK(c, hipMalloc(&c->q_mm_c, tiles * QN_MM_KS * 64 * 16));
    HIPCHK(c, hipMalloc(&c->q_mm_q, tiles * QN_MM_KS * 64 * 16));
    HIPCHK(c, hipMalloc(&c->q_mm_qn, sizeof(float) * tiles * 32));
    HIPCHK(c, hipMalloc(&c->q_mm_L, sizeof(uint32_t) * tiles * 32));
    uint32_t m = 1024; while (m < 2 * n) m <<= 1;
    c->q_mm_mask = m - 1;
    HIPCHK(c, hipMalloc(&c->q_mm_table, sizeof(unsigned long long) * m));
    HIPCHK(c, hipMalloc(&c->q_mm_table_q, sizeof(unsigned long long) * m));      // the same table for the QUERY rows (query-side de-duplication of the forward search)
    c->q_mm_cap = (uint32_t)std::min<size_t>(48 * n, 1u << 27);                  // survivor pairs: two thirds in per-block regions, one third shared spill
    HIPCHK(c, hipMalloc(&c->q_mm_pairs, sizeof(uint2) * c->q_mm_cap));
    c->q_mm_ncnt = (uint32_t)(4 + 4608 + 64 * (tiles / (QN_MM_WAVES * QN_MM_QT) + 1) + 16);           // counts[0] total, [1] lost, [3] spill, [4 + block]: blocks <= 2048 + bx
    HIPCHK(c, hipMalloc(&c->q_mm_cnt, sizeof(uint32_t) * c->q_mm_ncnt));
  }
  c->q_ready = true;
  return QN_OK;
}

static int quatro_fpfh(qn_ctx* c, int w) {                                  // K9-K11 on cloud slot w (grid already built)
  CloudBuf& b = c->cloud[w];
  hipStream_t s = c->stream;
  const uint32_t nb = (b.n + QN_BLOCK - 1) / QN_BLOCK;
  const float rn = (float)c->qparams.fpfh_normal_radius, rf = (float)c->qparams.fpfh_radius;
  const float rn2 = (float)(c->qparams.fpfh_normal_radius * c->qparams.fpfh_normal_radius), rf2 = (float)(c->qparams.fpfh_radius * c->qparams.fpfh_radius);
  // lanes per query: a cloud is a small grid for this chip - the fewer its points, the more lanes share a query's neighbourhood walk (knobs normals_fg / fpfh_fg; 0 = by cloud size)
  // measured (tools/gpu_quatro_ab.py, profiles/r5_*_quatro_ab.txt): normals 1 -> 8 lanes: 0.103 -> 0.066 ms at 30k (both clouds), 0.200 -> 0.125 at 100k, 16 lanes slower again;
  // SPFH / FPFH 8 -> 16 lanes: slower at both sizes (the 33 group sums double)
  const int nfg = c->quatro_normals_width();
  const int ffg = c->quatro_fpfh_width();
  { ProfScope ps(c, QN_K_FPFH_NORMALS);
    if (nfg >= 16) hipLaunchKernelGGL((k_normals_group<16>), dim3(nb * 16), dim3(QN_BLOCK), 0, s, b.grid, rn, rn2, c->q_normals[w]);
    else if (nfg >= 8) hipLaunchKernelGGL((k_normals_group<8>), dim3(nb * 8), dim3(QN_BLOCK), 0, s, b.grid, rn, rn2, c->q_normals[w]);
    else hipLaunchKernelGGL(k_normals, dim3(nb), dim3(QN_BLOCK), 0, s, b.grid, rn, rn2, c->q_normals[w]); }
  { ProfScope ps(c, QN_K_FPFH_SPFH);
    if (ffg >= 16) hipLaunchKernelGGL((k_spfh<16>), dim3(nb * 16), dim3(QN_BLOCK), 0, s, b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w]);
    else hipLaunchKernelGGL((k_spfh<8>), dim3(nb * 8), dim3(QN_BLOCK), 0, s, b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w]); }
  { ProfScope ps(c, QN_K_FPFH_FPFH);
    if (ffg >= 16) hipLaunchKernelGGL((k_fpfh<16>), dim3(nb * 16), dim3(QN_BLOCK), 0, s, b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w], c->q_fpfh_s[w]);
    else hipLaunchKernelGGL((k_fpfh<8>), dim3(nb * 8), dim3(QN_BLOCK), 0, s, b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w], c->q_fpfh_s[w]);
    hipLaunchKernelGGL(k_rows_to_original, dim3(nb), dim3(QN_BLOCK), 0, s, b.sorted, b.n, c->q_fpfh_s[w], c->q_fpfh[w], QN_FROW, QN_FROW); }
  HIPCHK(c, hipGetLastError());
  return QN_OK;
}

static void launch_feat_nn(qn_ctx* c, const float* Q, uint32_t nq_max, const uint32_t* qlist, const uint32_t* qlist_n, int cand_slot, uint32_t nc, unsigned long long* keys) {
  const uint32_t bx = (nq_max + QN_BLOCK * QN_FM_QPL - 1) / (QN_BLOCK * QN_FM_QPL);
  uint32_t ny = std::max<uint32_t>(1, std::min<uint32_t>((4096 + bx - 1) / bx, (nc + QN_FM_TILE - 1) / QN_FM_TILE));
  uint32_t chunk = (nc + ny - 1) / ny; chunk = (chunk + QN_FM_TILE - 1) / QN_FM_TILE * QN_FM_TILE; ny = (nc + chunk - 1) / chunk;
  ProfScope ps(c, QN_K_FEAT_MATCH);
  hipLaunchKernelGGL(k_feat_nn, dim3(bx, ny), dim3(QN_BLOCK), 0, c->stream, Q, nq_max, qlist, qlist_n, (const qn_v2f*)c->q_pair[cand_slot], c->q_pair_hash[cand_slot], nc, chunk, keys);
}

// The same search on the matrix cores (qn_feat_mm.cuh): candidate de-duplication, f16 operand images, two screening passes, exact
// re-evaluation of the survivors.  mm_overflow (pinned) is set when the survivor list did not fit: the caller repeats with k_feat_nn.
static void launch_feat_nn_mm(qn_ctx* c, const float* Q, uint32_t nq_max, const uint32_t* qlist, const uint32_t* qlist_n, int cand_slot, uint32_t nc, unsigned long long* keys,
                              uint32_t* mm_overflow, bool reset_done = false) {
  hipStream_t s = c->stream;
  ProfScope ps(c, QN_K_FEAT_MATCH);
  const float* C = c->q_fpfh[cand_slot];
  const uint32_t nc_tiles = (nc + 31) / 32, nq_tiles = (nq_max + 31) / 32;
  if (!reset_done) {                                                         // (quatro_match_enqueue resets the table, the bounds and the counters inside its fused bookkeeping launches)
    (void)hipMemsetAsync(c->q_mm_table, 0xFF, sizeof(unsigned long long) * ((size_t)c->q_mm_mask + 1), s);
    (void)hipMemsetAsync(c->q_mm_L, 0, sizeof(uint32_t) * nq_tiles * 32, s);
    (void)hipMemsetAsync(c->q_mm_cnt, 0, sizeof(uint32_t) * c->q_mm_ncnt, s);
  }
  hipLaunchKernelGGL(k_feat_dedupe, dim3((nc + 255) / 256), dim3(256), 0, s, C, nc, c->q_mm_table, c->q_mm_mask, c->q_mm_cnt + 2);
  hipLaunchKernelGGL(k_feat_prep, dim3((nc_tiles * 32 + 127) / 128), dim3(128), 0, s, C, nc, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0,
                     (const unsigned long long*)c->q_mm_table, c->q_mm_mask, (const uint32_t*)(c->q_mm_cnt + 2), (_Float16*)c->q_mm_c, (float*)nullptr, nc_tiles * 32);
  hipLaunchKernelGGL(k_feat_prep, dim3((nq_tiles * 32 + 127) / 128), dim3(128), 0, s, Q, nq_max, qlist, qlist_n, 1,
                     (const unsigned long long*)nullptr, 0u, (const uint32_t*)nullptr, (_Float16*)c->q_mm_q, c->q_mm_qn, nq_tiles * 32);
  const uint32_t bx = (nq_tiles + QN_MM_WAVES * QN_MM_QT - 1) / (QN_MM_WAVES * QN_MM_QT);
  auto split = [&](uint32_t tiles, uint32_t min_blocks, uint32_t& per, uint32_t& ny) {               // candidate segments along grid.y: ~2048+ blocks, in whole rounds of the
    uint32_t best = 1; double best_eff = 0;                                     // 512 blocks the chip holds (2 per CU): a 4.2-round grid runs as long as a 5-round one
    for (uint32_t cand = 1; cand <= std::min<uint32_t>(tiles, 64); cand++) {
      const uint32_t p = (tiles + cand - 1) / cand, y = (tiles + p - 1) / p; const double blocks = (double)bx * y;
      if (blocks < min_blocks && cand < std::min<uint32_t>(tiles, 64)) continue;
      const double eff = blocks / (512.0 * std::ceil(blocks / 512.0)) - 1e-4 * y;
      if (eff > best_eff) { best_eff = eff; best = cand; }
      if (blocks > 4096) break;
    }
    per = (tiles + best - 1) / best; ny = (tiles + per - 1) / per;
  };
  const uint32_t step = (uint32_t)std::max(1, std::min<int>(c->feat.sample, (int)nc_tiles));
  uint32_t per1, ny1, per2, ny2;
  constexpr uint32_t FULL_MIN_BLOCKS = 1536;      // smallest grid of the full pass: three rounds of the 512 blocks the chip holds
  split((nc_tiles + step - 1) / step, 512, per1, ny1); split(nc_tiles, FULL_MIN_BLOCKS, per2, ny2);      // (the sampled pass is short: fewer, longer blocks - each loads its query fragments once)
  const uint32_t cap_spill = c->q_mm_cap / 3, cap_block = (c->q_mm_cap - cap_spill) / (bx * ny2);      // bx * ny2 <= 2048 + bx regions
  uint2* spill = c->q_mm_pairs + (size_t)cap_block * bx * ny2;
  hipLaunchKernelGGL((k_feat_mm<1>), dim3(bx, ny1), dim3(64 * QN_MM_WAVES), 0, s, (const qn_u4*)c->q_mm_q, nq_max, qlist ? qlist_n : (const uint32_t*)nullptr,
                     (const qn_u4*)c->q_mm_c, nc_tiles, per1, step, c->q_mm_L, (const float*)c->q_mm_qn, c->q_mm_pairs, c->q_mm_cnt, cap_block, spill, cap_spill);
  hipLaunchKernelGGL((k_feat_mm<2>), dim3(bx, ny2), dim3(64 * QN_MM_WAVES), 0, s, (const qn_u4*)c->q_mm_q, nq_max, qlist ? qlist_n : (const uint32_t*)nullptr,
                     (const qn_u4*)c->q_mm_c, nc_tiles, per2, 1u, c->q_mm_L, (const float*)c->q_mm_qn, c->q_mm_pairs, c->q_mm_cnt, cap_block, spill, cap_spill);
  hipLaunchKernelGGL(k_feat_exact, dim3(bx * ny2 + 256), dim3(256), 0, s, (const uint2*)c->q_mm_pairs, (const uint32_t*)c->q_mm_cnt, cap_block, bx * ny2, (const uint2*)spill, cap_spill,
                     Q, qlist, C, nc, keys, mm_overflow);
  if (c->knob.feat_verify) {                                                      // developer check: the VALU search of the same queries, compared key by key
    if (!c->q_mm_vkeys) { (void)hipMalloc(&c->q_mm_vkeys, sizeof(unsigned long long) * c->max_points); (void)hipMalloc(&c->q_mm_vcnt, 16); (void)hipMemsetAsync(c->q_mm_vcnt, 0, 16, s); }
    hipLaunchKernelGGL(k_fill_u64, dim3((c->max_points + 255) / 256), dim3(256), 0, s, c->q_mm_vkeys, (uint32_t)c->max_points, QN_INF_KEY);
    hipLaunchKernelGGL(k_pair_rows, dim3((((nc + 1) / 2) * 34 + 255) / 256), dim3(256), 0, s, C, nc, (qn_v2f*)c->q_pair[cand_slot], c->q_pair_hash[cand_slot]);
    launch_feat_nn(c, Q, nq_max, qlist, qlist_n, cand_slot, nc, c->q_mm_vkeys);
    hipLaunchKernelGGL(k_feat_compare, dim3((nq_max + 255) / 256), dim3(256), 0, s, (const unsigned long long*)keys, (const unsigned long long*)c->q_mm_vkeys, nq_max, qlist, qlist_n, c->q_mm_vcnt);
  }
}

// Matcher::calculateCorrespondences on the descriptor sets in c->q_fpfh[0] (ns rows) / c->q_fpfh[1] (nt rows) and the clouds in
// c->cloud[0/1].raw, all on the device: feature NN j -> i for every j of the smaller cloud, lazy reverse search for the hit i,
// cross-check, distance gate (optimizedMatching), seeded tuple test + cap; ONE small download at the end (SURVEY A.2.3).
// (two halves: quatro_match_enqueue puts every launch of the stage on the context's stream and returns; quatro_match_collect - after the caller has synchronised
//  that stream - reads the pinned hand-over block.  quatro_match_tail = enqueue + synchronise + collect, the one-pair path; the batched coarse-to-fine path enqueues
//  the stage of B pairs back to back before its ONE synchronisation, qn_coarse_to_fine_align_batch.)
static int quatro_match_tail(qn_ctx* c, uint32_t ns, uint32_t nt, const qn_quatro_params& p, bool want_mutual, qnq::TailResult& out);
static int quatro_match_enqueue(qn_ctx* c, uint32_t ns, uint32_t nt, const qn_quatro_params& p) {
  const bool swapped = nt > ns;
  const int I = swapped ? 1 : 0, J = swapped ? 0 : 1;                        // I = larger cloud, J = smaller (SURVEY A.2.3)
  const uint32_t ni = swapped ? nt : ns, nj = swapped ? ns : nt;
  hipStream_t s = c->stream;
  const float4* Pi = c->cloud[I].raw; const float4* Pj = c->cloud[J].raw;
  float* mean_i = c->q_mean + 4 * I; float* mean_j = c->q_mean + 4 * J;
  QuatroTailOut* head = (QuatroTailOut*)c->q_host; QuatroCorr* recs = (QuatroCorr*)(head + 1);
  head->n_cand = 0; head->n_sel = 0; head->overflow = 0; head->pad = 0;
  if (join_target(c) != QN_OK) return QN_ERR_HIP;                            // the target's descriptors were made on the second stream
  const bool mm = c->feat.mfma && !c->feat_mm_retry;
  const bool fused = mm && !(c->feat.query_dedupe && !c->knob.feat_verify);      // the fused bookkeeping launches (round 5); without the matrix-core search, or with the query de-duplication: the one-launch-per-step sequence
  const uint32_t mm_table_n = c->q_mm_mask + 1u;
  if (fused) {      // ONE launch: counters, hit flags, both key arrays, both row-hash passes, and the matrix-core search's table / bounds / counters for the forward search
    ProfScope ps(c, QN_K_FEAT_MATCH);
    MatchInitArgs ia{c->q_counts, 8u, c->q_hit, ni, c->q_key[J], nj, c->q_key[I], c->q_fpfh[0], ns, c->q_fpfh[1], nt,
                     c->q_mm_table, mm_table_n, c->q_mm_L, ((nj + 31) / 32) * 32, c->q_mm_cnt, c->q_mm_ncnt};
    hipLaunchKernelGGL(k_match_init, dim3(std::min<uint32_t>(1024u, (std::max(std::max(ni, nj), mm_table_n) + 255) / 256)), dim3(256), 0, s, ia);
  } else {
  HIPCHK(c, hipMemsetAsync(c->q_counts, 0, sizeof(uint32_t) * 8, s));
  HIPCHK(c, hipMemsetAsync(c->q_hit, 0, sizeof(uint32_t) * ni, s));
  hipLaunchKernelGGL(k_fill_u64, dim3((nj + 255) / 256), dim3(256), 0, s, c->q_key[J], nj, QN_INF_KEY);
  hipLaunchKernelGGL(k_fill_u64, dim3((ni + 255) / 256), dim3(256), 0, s, c->q_key[I], ni, QN_INF_KEY);
  { ProfScope ps(c, QN_K_FEAT_MATCH);
    for (int w = 0; w < 2; w++) {                                                                        // row hashes + the pair-interleaved candidate layout of both sets
      const uint32_t nw = w == 0 ? ns : nt;
      hipLaunchKernelGGL(k_row_hash, dim3((nw + 255) / 256), dim3(256), 0, s, c->q_fpfh[w], nw);
      if (!mm) hipLaunchKernelGGL(k_pair_rows, dim3((((nw + 1) / 2) * 34 + 255) / 256), dim3(256), 0, s, c->q_fpfh[w], nw, (qn_v2f*)c->q_pair[w], c->q_pair_hash[w]);
    } }
  }
  if (mm && c->feat.query_dedupe && !c->knob.feat_verify) {                       // every DISTINCT row of j -> nearest i, the other rows copy their representative's key (the developer check verifies every query: all of them are searched then)
    { ProfScope ps(c, QN_K_FEAT_MATCH);
      (void)hipMemsetAsync(c->q_mm_table_q, 0xFF, sizeof(unsigned long long) * ((size_t)c->q_mm_mask + 1), s);
      hipLaunchKernelGGL(k_feat_dedupe, dim3((nj + 255) / 256), dim3(256), 0, s, (const float*)c->q_fpfh[J], nj, c->q_mm_table_q, c->q_mm_mask, &c->q_counts[2]);
      hipLaunchKernelGGL(k_query_reps, dim3((nj + 255) / 256), dim3(256), 0, s, (const float*)c->q_fpfh[J], nj, (const unsigned long long*)c->q_mm_table_q, c->q_mm_mask, (const uint32_t*)&c->q_counts[2], c->q_list, &c->q_counts[1]); }
    launch_feat_nn_mm(c, c->q_fpfh[J], nj, c->q_list, &c->q_counts[1], I, ni, c->q_key[J], &head->pad);
    { ProfScope ps(c, QN_K_FEAT_MATCH);
      hipLaunchKernelGGL(k_query_propagate, dim3((nj + 255) / 256), dim3(256), 0, s, (const float*)c->q_fpfh[J], nj, (const unsigned long long*)c->q_mm_table_q, c->q_mm_mask, (const uint32_t*)&c->q_counts[2], c->q_key[J]); }
  }
  else if (mm) launch_feat_nn_mm(c, c->q_fpfh[J], nj, nullptr, nullptr, I, ni, c->q_key[J], &head->pad, fused);
  else launch_feat_nn(c, c->q_fpfh[J], nj, nullptr, nullptr, I, ni, c->q_key[J]);                        // every j -> nearest i
  if (fused) {      // two launches between the searches: mark + survivor count + table / bounds reset, then compact + counter reset
    { ProfScope ps(c, QN_K_FEAT_MATCH);      // (its own scope, closed before launch_feat_nn_mm opens one: profiling spans do not nest - an outer span whose end event is never recorded poisons hipGetLastError)
      const uint32_t gb = std::min<uint32_t>(1024u, (std::max(std::max(ni, nj), mm_table_n) + 255) / 256);
      hipLaunchKernelGGL(k_mark_hits_reset, dim3(gb), dim3(256), 0, s, c->q_key[J], nj, c->q_hit, (const uint32_t*)c->q_mm_cnt, &head->survivors, c->q_mm_table, mm_table_n, c->q_mm_L, ((ni + 31) / 32) * 32);
      hipLaunchKernelGGL(k_compact_hits_reset, dim3(gb), dim3(256), 0, s, c->q_hit, ni, c->q_list, &c->q_counts[0], c->q_mm_cnt, c->q_mm_ncnt); }
    launch_feat_nn_mm(c, c->q_fpfh[I], ni, c->q_list, &c->q_counts[0], J, nj, c->q_key[I], &head->pad, true);
  } else {
  hipLaunchKernelGGL(k_mark_hits, dim3((nj + 255) / 256), dim3(256), 0, s, c->q_key[J], nj, c->q_hit);
  hipLaunchKernelGGL(k_compact_hits, dim3((ni + 255) / 256), dim3(256), 0, s, c->q_hit, ni, c->q_list, &c->q_counts[0]);
  if (mm) { hipLaunchKernelGGL(k_feat_survivors, dim3(1), dim3(1), 0, s, (const uint32_t*)c->q_mm_cnt, &head->survivors);
            launch_feat_nn_mm(c, c->q_fpfh[I], ni, c->q_list, &c->q_counts[0], J, nj, c->q_key[I], &head->pad); }
  else launch_feat_nn(c, c->q_fpfh[I], ni, c->q_list, &c->q_counts[0], J, nj, c->q_key[I]);              // the hit i's -> nearest j (lazy reverse search)
  }
  { ProfScope ps(c, QN_K_MATCH_TAIL);
    if (fused) hipLaunchKernelGGL(k_means2, dim3(2 * QN_MEAN_BLOCKS), dim3(QN_BLOCK), 0, s, (const float4*)c->cloud[0].raw, c->cloud[0].n, (const float4*)c->cloud[1].raw, c->cloud[1].n, c->q_mean_psum, c->q_counts + 4, c->q_mean);
    else for (int w = 0; w < 2; w++) {                                                                   // normalizePoints: each cloud's own mean
      hipLaunchKernelGGL(k_mean_partial, dim3(QN_MEAN_BLOCKS), dim3(QN_BLOCK), 0, s, c->cloud[w].raw, c->cloud[w].n, c->q_mean_psum + w * QN_MEAN_BLOCKS * 3);
      hipLaunchKernelGGL(k_mean_final, dim3(1), dim3(64), 0, s, c->q_mean_psum + w * QN_MEAN_BLOCKS * 3, c->cloud[w].n, c->q_mean + 4 * w);
    }
    uint32_t* flag = c->q_hit; uint32_t* pos = c->q_list; uint2* cand = c->fb_list;                     // q_hit / q_list are free again; fb_list is GICP scratch
    hipLaunchKernelGGL(k_mutual_gate, dim3((nj + 255) / 256), dim3(256), 0, s, c->q_key[J], nj, c->q_key[I], Pi, Pj, mean_i, mean_j,
                       (float)p.distance_threshold, p.use_optimized_matching ? 1 : 0, flag, c->q_pairs);
    const uint32_t sb = (nj + QN_BLOCK * QN_SCAN_ITEMS - 1) / (QN_BLOCK * QN_SCAN_ITEMS);
    hipLaunchKernelGGL(k_scan_block, dim3(sb), dim3(QN_BLOCK), 0, s, flag, nj, pos, c->scan_sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(QN_BLOCK), 0, s, c->scan_sums, sb);
    hipLaunchKernelGGL(k_scan_add_total, dim3(sb), dim3(QN_BLOCK), 0, s, pos, nj, c->scan_sums, flag);   // pos[nj] = number of candidates
    hipLaunchKernelGGL(k_compact_cand, dim3((nj + 255) / 256), dim3(256), 0, s, flag, pos, c->q_pairs, nj, cand);
    HIPCHK(c, hipMemsetAsync(c->q_sel, 0, sizeof(uint32_t) * nj, s));                                    // one flag per candidate
    hipLaunchKernelGGL(k_tuple_test, dim3(1), dim3(QN_TUPLE_THREADS), 0, s, cand, pos + nj, Pi, Pj, mean_i, mean_j, (float)p.tuple_scale, p.rng_seed,
                       p.use_optimized_matching ? 1 : 0, p.max_num_corres, c->q_sel);
    hipLaunchKernelGGL(k_collect_corres, dim3(1), dim3(QN_TUPLE_THREADS), 0, s, cand, pos + nj, c->q_sel, Pi, Pj, c->max_points, head, recs); }
  HIPCHK(c, hipGetLastError());
  return QN_OK;
}
static int quatro_match_collect(qn_ctx* c, uint32_t ns, uint32_t nt, const qn_quatro_params& p, bool want_mutual, qnq::TailResult& out) {
  const bool swapped = nt > ns;
  QuatroTailOut* head = (QuatroTailOut*)c->q_host; QuatroCorr* recs = (QuatroCorr*)(head + 1);
  const bool mm = c->feat.mfma && !c->feat_mm_retry;
  c->prof_collect();
  { const int vrc = clouds_valid(c); if (vrc != QN_OK) return vrc; }
  if (mm && head->pad) {                                                     // survivor list overflow (pathological descriptor sets): the VALU search, same answer
    c->feat_fallbacks++; c->feat_mm_retry = true;
    const int rc2 = quatro_match_tail(c, ns, nt, p, want_mutual, out);
    c->feat_mm_retry = false;
    return rc2;
  }
  if (mm) c->feat_survivors = head->survivors;
  out.mutual.clear(); out.corres.clear(); out.S.clear(); out.D.clear();
  const uint32_t m = head->n_sel;
  std::vector<uint32_t> order(m);
  std::iota(order.begin(), order.end(), 0u);
  auto key = [&](uint32_t e) { return swapped ? qnq::Pair((int)recs[e].j, (int)recs[e].i) : qnq::Pair((int)recs[e].i, (int)recs[e].j); };
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });      // corres_: sorted (src, dst); the candidates are unique already
  for (uint32_t e : order) {
    out.corres.push_back(key(e));
    const float* a = swapped ? recs[e].pj : recs[e].pi; const float* b = swapped ? recs[e].pi : recs[e].pj;
    out.S.push_back({(double)a[0], (double)a[1], (double)a[2]}); out.D.push_back({(double)b[0], (double)b[1], (double)b[2]});
  }
  if (want_mutual && head->n_cand) {
    std::vector<uint2> cd(head->n_cand);
    HIPCHK(c, hipMemcpy(cd.data(), c->fb_list, sizeof(uint2) * head->n_cand, hipMemcpyDeviceToHost));
    for (const uint2& q : cd) out.mutual.emplace_back(swapped ? (int)q.y : (int)q.x, swapped ? (int)q.x : (int)q.y);
    std::sort(out.mutual.begin(), out.mutual.end());
  }
  return QN_OK;
}
static int quatro_match_tail(qn_ctx* c, uint32_t ns, uint32_t nt, const qn_quatro_params& p, bool want_mutual, qnq::TailResult& out) {
  int rc = quatro_match_enqueue(c, ns, nt, p);
  if (rc != QN_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return quatro_match_collect(c, ns, nt, p, want_mutual, out);
}

// FPFH of both clouds (grid cell = r_f / 2: 5x5x5-cell stencils); descriptors stay on the device
static int quatro_features(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, bool on_device) {
  int rc;
  if (!c->qparams_set) qn_quatro_default_params(&c->qparams), c->qparams_set = true;
  if ((rc = quatro_alloc(c)) != QN_OK) return rc;
  const double save = c->lane.cell_override;
  c->lane.cell_override = c->qparams.fpfh_radius * 0.5;
  rc = set_cloud(c, QN_SOURCE, src, ns, stride, on_device);
  if (rc == QN_OK) rc = set_cloud(c, QN_TARGET, dst, nt, stride, on_device);     // on the second stream when the context has one (TargetScope, qn_engine.hip)
  c->lane.cell_override = save;
  if (rc != QN_OK) return rc;
  if ((rc = quatro_fpfh(c, 0)) != QN_OK) return rc;
  // the target's descriptors follow its grid build on the second stream, concurrently with the source's on the first (the clouds are
  // small grids for this chip); quatro_match_tail joins before it reads them
  TargetScope scope(c, c->tgt_on_stream2 && !c->prof_on && c->stream2 != nullptr);
  return quatro_fpfh(c, 1);
}

// the TARGET half of quatro_features alone: the lane borrows the source cloud and its descriptors from another lane of the run (qn_coarse_to_fine_align_batch: the candidates of ONE
// loop-closure query share their source cloud - its grid, normals, SPFH and FPFH are made once per run, not once per candidate)
static int quatro_features_target_only(qn_ctx* c, const float* dst, uint32_t nt, uint32_t stride, bool on_device) {
  int rc;
  if (!c->qparams_set) qn_quatro_default_params(&c->qparams), c->qparams_set = true;
  if ((rc = quatro_alloc(c)) != QN_OK) return rc;
  const double save = c->lane.cell_override;
  c->lane.cell_override = c->qparams.fpfh_radius * 0.5;
  rc = set_cloud(c, QN_TARGET, dst, nt, stride, on_device);
  c->lane.cell_override = save;
  if (rc != QN_OK) return rc;
  return quatro_fpfh(c, 1);
}

// qn_fpfh: pcl::FPFHEstimationOMP on one cloud with the radii of the context's Quatro parameters (upstream Quatro
// fpfh.cc -> `computeFPFHFeatures`, SURVEY A.2.2); out = n x 33 f32 in the caller's point order, NaN rows where PCL has none.
extern "C" int qn_fpfh(qn_ctx* c, const float* xyz, uint32_t n, uint32_t stride, float* fpfh33) {
  if (!c || !xyz || !fpfh33) return QN_ERR_INVALID_ARG;
  if (n == 0) return QN_ERR_EMPTY_CLOUD;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (!c->qparams_set) qn_quatro_default_params(&c->qparams), c->qparams_set = true;
  if ((rc = quatro_alloc(c)) != QN_OK) return rc;
  const double save = c->lane.cell_override;
  c->lane.cell_override = c->qparams.fpfh_radius * 0.5;
  rc = set_cloud(c, QN_SOURCE, xyz, n, stride, false);
  c->lane.cell_override = save;
  if (rc != QN_OK) return rc;
  if ((rc = quatro_fpfh(c, 0)) != QN_OK) return rc;
  std::vector<float> rows((size_t)n * QN_FROW);
  HIPCHK(c, hipMemcpyAsync(rows.data(), c->q_fpfh[0], sizeof(float) * QN_FROW * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->prof_collect();
  { const int vrc = clouds_valid(c); if (vrc != QN_OK) return vrc; }
  for (uint32_t i = 0; i < n; i++) memcpy(fpfh33 + (size_t)i * 33, rows.data() + (size_t)i * QN_FROW, sizeof(float) * 33);
  return QN_OK;
}

// caller-order cloud into slot `which` WITHOUT a search grid (the matcher only needs the points)
static int upload_raw(qn_ctx* c, int which, const float* xyz, uint32_t n, uint32_t stride) {
  CloudBuf& b = c->cloud[which];
  b.n = 0; b.has_grid = b.has_cov = false;
  if (!xyz || stride < 12 || (stride & 3)) return QN_ERR_INVALID_ARG;
  if (n > c->max_points) return QN_ERR_CAPACITY;
  const char* dsrc = nullptr;
  { const int rc = upload_host_cloud(c, xyz, n, stride, c->stream, &dsrc); if (rc != QN_OK) return rc; }
  b.n = n;
  hipLaunchKernelGGL(k_pack_points, dim3((n + QN_BLOCK - 1) / QN_BLOCK), dim3(QN_BLOCK), 0, c->stream, dsrc, stride, n, b.raw);
  return QN_OK;
}

// qn_match_optimized: teaser::Matcher::optimizedMatching(thr_dist, num_max_corres, tuple_scale) (upstream Quatro matcher.cc,
// reached from quatro<>::align when use_optimized_matching_, loop_closure.cpp:25) on two clouds and THEIR 33-D descriptors as
// the caller holds them: mutual feature NN, distance gate, seeded tuple test and the cap, all on the GPU.
// pairs_out = (src index, dst index) x *n_out, at most `cap` pairs are written.
extern "C" int qn_match_optimized(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride,
                                  const float* src_fpfh33, const float* dst_fpfh33, float thr_dist, int num_max_corres, float tuple_scale,
                                  int32_t* pairs_out, uint32_t cap, uint32_t* n_out) {
  if (!c || !src || !dst || !src_fpfh33 || !dst_fpfh33 || !pairs_out || !n_out || num_max_corres < 1) return QN_ERR_INVALID_ARG;
  *n_out = 0;
  if (ns == 0 || nt == 0) return QN_ERR_EMPTY_CLOUD;
  if (ns > c->max_points || nt > c->max_points) return QN_ERR_CAPACITY;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (!c->qparams_set) qn_quatro_default_params(&c->qparams), c->qparams_set = true;
  if ((rc = quatro_alloc(c)) != QN_OK) return rc;
  if ((rc = upload_raw(c, 0, src, ns, stride)) != QN_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));                                // the staging buffer is reused for the second cloud
  if ((rc = upload_raw(c, 1, dst, nt, stride)) != QN_OK) return rc;
  const float* F[2] = {src_fpfh33, dst_fpfh33}; const uint32_t N[2] = {ns, nt};
  std::vector<float> rows;
  for (int w = 0; w < 2; w++) {                                             // 33 -> 36-float rows (9 x float4)
    rows.assign((size_t)N[w] * QN_FROW, 0.f);
    for (uint32_t i = 0; i < N[w]; i++) memcpy(rows.data() + (size_t)i * QN_FROW, F[w] + (size_t)i * 33, sizeof(float) * 33);
    HIPCHK(c, hipMemcpy(c->q_fpfh[w], rows.data(), sizeof(float) * QN_FROW * N[w], hipMemcpyHostToDevice));
  }
  qn_quatro_params p = c->qparams;
  p.distance_threshold = thr_dist; p.max_num_corres = num_max_corres; p.tuple_scale = tuple_scale; p.use_optimized_matching = 1;
  qnq::TailResult tr;
  if ((rc = quatro_match_tail(c, ns, nt, p, false, tr)) != QN_OK) return rc;
  const uint32_t m = std::min<uint32_t>((uint32_t)tr.corres.size(), cap);
  for (uint32_t e = 0; e < m; e++) { pairs_out[2 * e] = tr.corres[e].first; pairs_out[2 * e + 1] = tr.corres[e].second; }
  *n_out = (uint32_t)tr.corres.size();
  return QN_OK;
}

static int quatro_align_impl(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, bool on_device, double T[16], int* valid,
                             qnq::TailResult* tr_out, qnq::SolveOut* so_out) {
  if (!c || !T || !valid) return QN_ERR_INVALID_ARG;
  for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  *valid = 0;
  if (ns == 0 || nt == 0) return QN_ERR_EMPTY_CLOUD;
  HIPCHK(c, hipSetDevice(c->device));
  const auto w0 = std::chrono::steady_clock::now();
  int rc = quatro_features(c, src, ns, dst, nt, stride, on_device);
  if (rc != QN_OK) return rc;
  const auto w1 = std::chrono::steady_clock::now();
  qnq::TailResult tr;
  if ((rc = quatro_match_tail(c, ns, nt, c->qparams, tr_out != nullptr, tr)) != QN_OK) return rc;
  const auto w2 = std::chrono::steady_clock::now();
  qnq::SolveOut so;
  qnq::solve(tr.S, tr.D, c->qparams, &so);               // empty correspondences -> valid = 0 (README.md:110 "fixed for empty matches")
  memcpy(T, so.T, sizeof(so.T)); *valid = so.valid; c->q_last_scale = so.scale;
  const auto w3 = std::chrono::steady_clock::now();
  c->q_wall_ms[0] = std::chrono::duration<double, std::milli>(w1 - w0).count();       // uploads + grids, FPFH enqueued (includes the two bbox syncs)
  c->q_wall_ms[1] = std::chrono::duration<double, std::milli>(w2 - w1).count();       // waiting for FPFH + matching + the Matcher tail
  c->q_wall_ms[2] = std::chrono::duration<double, std::milli>(w3 - w2).count();       // host solver: max clique + GNC-TLS
  if (tr_out) *tr_out = tr;
  if (so_out) *so_out = so;
  return QN_OK;
}

extern "C" int qn_quatro_align(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, double T[16], int* valid) {
  return quatro_align_impl(c, src, ns, dst, nt, stride, false, T, valid, nullptr, nullptr);
}
extern "C" int qn_quatro_align_device(qn_ctx* c, const float* d_src, uint32_t ns, const float* d_dst, uint32_t nt, uint32_t stride, double T[16], int* valid) {
  return quatro_align_impl(c, d_src, ns, d_dst, nt, stride, true, T, valid, nullptr, nullptr);
}

// test read-backs: last Quatro run's descriptors (original point order) and matches
extern "C" int qn_quatro_get_features(qn_ctx* c, int which, float* normals3, float* spfh33, float* fpfh33) {
  if (!c || (which != 0 && which != 1) || !c->q_ready) return QN_ERR_NOT_READY;
  CloudBuf& b = c->cloud[which];
  if (!b.n) return QN_ERR_EMPTY_CLOUD;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t n = b.n;
  std::vector<float4> srt(n), nrm(n); std::vector<float> sp((size_t)n * QN_FROW), fp((size_t)n * QN_FROW);
  HIPCHK(c, hipMemcpy(srt.data(), b.sorted, sizeof(float4) * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(nrm.data(), c->q_normals[which], sizeof(float4) * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(sp.data(), c->q_spfh[which], sizeof(float) * QN_FROW * n, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(fp.data(), c->q_fpfh[which], sizeof(float) * QN_FROW * n, hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < n; t++) {
    uint32_t i; memcpy(&i, &srt[t].w, 4);
    if (normals3) { normals3[3 * (size_t)i] = nrm[t].x; normals3[3 * (size_t)i + 1] = nrm[t].y; normals3[3 * (size_t)i + 2] = nrm[t].z; }
    if (spfh33) for (int b2 = 0; b2 < 33; b2++) spfh33[(size_t)33 * i + b2] = sp[(size_t)QN_FROW * t + b2];
  }
  if (fpfh33) for (uint32_t i = 0; i < n; i++) for (int b2 = 0; b2 < 33; b2++) fpfh33[(size_t)33 * i + b2] = fp[(size_t)QN_FROW * i + b2];
  return QN_OK;
}

extern "C" int qn_quatro_align_debug(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, double T[16], int* valid,
                                     int32_t* mutual_pairs, uint32_t* n_mutual, int32_t* corres_pairs, uint32_t* n_corres, uint32_t cap,
                                     int32_t* clique, uint32_t* n_clique, int32_t* rot_iterations) {
  qnq::TailResult tr; qnq::SolveOut so;
  int rc = quatro_align_impl(c, src, ns, dst, nt, stride, false, T, valid, &tr, &so);
  if (rc != QN_OK) return rc;
  if (n_mutual) { *n_mutual = (uint32_t)tr.mutual.size(); for (size_t i = 0; i < tr.mutual.size() && i < cap; i++) { mutual_pairs[2 * i] = tr.mutual[i].first; mutual_pairs[2 * i + 1] = tr.mutual[i].second; } }
  if (n_corres) { *n_corres = (uint32_t)tr.corres.size(); for (size_t i = 0; i < tr.corres.size() && i < cap; i++) { corres_pairs[2 * i] = tr.corres[i].first; corres_pairs[2 * i + 1] = tr.corres[i].second; } }
  if (n_clique) { *n_clique = (uint32_t)so.clique.size(); for (size_t i = 0; i < so.clique.size() && i < cap; i++) clique[i] = so.clique[i]; }
  if (rot_iterations) *rot_iterations = so.rot_iterations;
  return QN_OK;
}

// host solver on given correspondences (for solver-only parity tests; needs no GPU work)
extern "C" int qn_quatro_solve(const float* src, const float* dst, uint32_t stride, const int32_t* corres_pairs, uint32_t n_corres, const qn_quatro_params* p,
                               double T[16], int* valid, int32_t* clique, uint32_t* n_clique) {
  if (!src || !dst || !p || !T || !valid || (n_corres && !corres_pairs)) return QN_ERR_INVALID_ARG;
  auto at = [](const float* base, uint32_t st, int i) { return (const float*)((const char*)base + (size_t)i * st); };
  std::vector<qnq::P3> S(n_corres), D(n_corres);
  for (uint32_t k = 0; k < n_corres; k++) for (int d = 0; d < 3; d++) { S[k][d] = at(src, stride, corres_pairs[2 * k])[d]; D[k][d] = at(dst, stride, corres_pairs[2 * k + 1])[d]; }
  qnq::SolveOut so; qnq::solve(S, D, *p, &so);
  memcpy(T, so.T, sizeof(so.T)); *valid = so.valid;
  if (n_clique) { *n_clique = (uint32_t)so.clique.size(); if (clique) for (size_t i = 0; i < so.clique.size(); i++) clique[i] = so.clique[i]; }
  return QN_OK;
}

extern "C" int qn_quatro_solve_scaled(const float* src, const float* dst, uint32_t stride, const int32_t* corres_pairs, uint32_t n_corres, const qn_quatro_params* p,
                                      double T[16], int* valid, int32_t* clique, uint32_t* n_clique, double* scale) {
  int32_t it;
  return qn_quatro_solve_iter(src, dst, stride, corres_pairs, n_corres, p, T, valid, clique, n_clique, scale, &it);
}
extern "C" int qn_quatro_solve_iter(const float* src, const float* dst, uint32_t stride, const int32_t* corres_pairs, uint32_t n_corres, const qn_quatro_params* p,
                                    double T[16], int* valid, int32_t* clique, uint32_t* n_clique, double* scale, int32_t* rot_iterations) {
  if (!src || !dst || !p || !T || !valid || !scale || !rot_iterations || (n_corres && !corres_pairs)) return QN_ERR_INVALID_ARG;
  auto at = [](const float* base, uint32_t st, int i) { return (const float*)((const char*)base + (size_t)i * st); };
  std::vector<qnq::P3> S(n_corres), D(n_corres);
  for (uint32_t k = 0; k < n_corres; k++) for (int d = 0; d < 3; d++) { S[k][d] = at(src, stride, corres_pairs[2 * k])[d]; D[k][d] = at(dst, stride, corres_pairs[2 * k + 1])[d]; }
  qnq::SolveOut so; qnq::solve(S, D, *p, &so);
  memcpy(T, so.T, sizeof(so.T)); *valid = so.valid; *scale = so.scale; *rot_iterations = so.rot_iterations;
  if (n_clique) { *n_clique = (uint32_t)so.clique.size(); if (clique) for (size_t i = 0; i < so.clique.size(); i++) clique[i] = so.clique[i]; }
  return QN_OK;
}
extern "C" int qn_quatro_get_scale(qn_ctx* c, double* scale) { if (!c || !scale) return QN_ERR_INVALID_ARG; *scale = c->q_last_scale; return QN_OK; }

// LoopClosure::coarseToFineAlignment (loop_closure.cpp:138-159): Quatro -> transformPcd(src, T_q) -> icpAlignment -> T_gicp * T_q.
// on_device: both clouds are HIP device pointers (e.g. the voxelised submaps qn_kf_assemble left on the GPU, loop_closure.cpp:177-192):
// nothing but the <= ~6 KB of selected correspondences and the result record crosses PCIe.
static int coarse_to_fine(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, bool on_device, double score_thr,
                          qn_gicp_result* out, double T_total[16], double T_quatro[16], int* valid, int* stage = nullptr) {
  if (!c || !out || !T_total || !valid) return QN_ERR_INVALID_ARG;
  *valid = 0;
  if (stage) *stage = 0;                                                          // (stage: 1 = Quatro solved, 2 = the fine stage ran too)
  memset(out, 0, sizeof(*out)); out->fitness = DBL_MAX;
  for (int i = 0; i < 4; i++) { out->T[5 * i] = 1.f; out->T64[5 * i] = 1.0; }      // (a pair Quatro cannot register reports the identity, like the batched entry point - ADVICE r5: the two paths' records are the same bytes)
  for (int i = 0; i < 16; i++) T_total[i] = (i % 5 == 0) ? 1.0 : 0.0;
  double Tq[16]; int qvalid = 0;
  int rc = quatro_align_impl(c, src, ns, dst, nt, stride, on_device, Tq, &qvalid, nullptr, nullptr);   // :144
  if (T_quatro) memcpy(T_quatro, Tq, sizeof(Tq));
  if (rc != QN_OK) return rc;
  if (stage) *stage = 1;
  if (!qvalid) return QN_OK;                                                      // :145-148
  // :152 coarse_aligned_ = transformPcd(src, T_q) - done on the device from the source cloud already resident (slot 0, caller order)
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->q_T, Tq, sizeof(Tq), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_transform_cloud_f64, dim3((ns + 255) / 256), dim3(256), 0, s, c->cloud[0].raw, ns, c->q_T, c->aligned);
  int gvalid = 0;
  rc = icp_alignment(c, (const float*)c->aligned, ns, dst, nt, stride, score_thr, out, &gvalid, on_device ? 3 : 2);   // :153 (the coarse-aligned source stays on the device)
  if (rc != QN_OK) return rc;
  if (stage) *stage = 2;
  *valid = gvalid;
  for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) {                        // :156 pose_between = T_gicp * T_quatro (the f32 GICP result cast to double, :133)
    double v = 0; for (int k = 0; k < 4; k++) v += (double)out->T[4 * a + k] * Tq[4 * k + b];
    T_total[4 * a + b] = v;
  }
  return QN_OK;
}
extern "C" int qn_coarse_to_fine_alignment(qn_ctx* c, const float* src, uint32_t ns, const float* dst, uint32_t nt, uint32_t stride, double score_thr,
                                           qn_gicp_result* out, double T_total[16], double T_quatro[16], int* valid) {
  return coarse_to_fine(c, src, ns, dst, nt, stride, false, score_thr, out, T_total, T_quatro, valid);
}
extern "C" int qn_coarse_to_fine_alignment_device(qn_ctx* c, const float* d_src, uint32_t ns, const float* d_dst, uint32_t nt, uint32_t stride, double score_thr,
                                                  qn_gicp_result* out, double T_total[16], double T_quatro[16], int* valid) {
  return coarse_to_fine(c, d_src, ns, d_dst, nt, stride, true, score_thr, out, T_total, T_quatro, valid);
}


// ------------------------------------------------------------------ batched coarse-to-fine (the reference's DEFAULT per-candidate path, many candidates at once)
// LoopClosure::performLoopClosure dispatches to coarseToFineAlignment whenever enable_quatro_ is set (include/loop_closure.h:54 `true`, config.yaml:31;
// dispatch src/loop_closure.cpp:188-192, body :138-159): Quatro -> transformPcd -> Nano-GICP -> T_gicp * T_quatro.  qn_gicp_align_batch / qn_multi_align_best
// registered GICP-only lanes; this is the same fan-out for the default path.  Per context (= one stream, one host worker from the pool), in runs of B = batch_lanes pairs:
//   1. the Quatro device stages (grids, K9-K11 FPFH of both clouds, K12 matching on the matrix cores, K13 Matcher tail) of all B pairs are ENQUEUED back to back, each
//      pair on the buffers of its own lane (sub-context), all on the context's stream: no host round trip between pairs, the stream never drains inside a run;
//   2. ONE synchronisation; per pair the <= ~6 KB hand-over block is read and the host solver runs (max clique, GNC-TLS yaw, TLS translation: 0.07 ms at 30k) -
//      while this worker solves, the other contexts' streams keep the GPU busy;
//   3. transformPcd of every accepted pair on the device (k_transform_cloud_f64, f64 matrix on f32 points, utilities.hpp:164-175) into the lane's c2f_src, the target's
//      float4 image (caller order) into c2f_dst; then the B coarse-aligned pairs go through batch_register - the GICP lanes, the pair as a grid dimension;
//   4. pose_between = T_gicp * T_quatro (loop_closure.cpp:156), valid = Quatro converged && GICP converged && score < thr (:145-148, :129).
// Every stage is the one-pair path's code on the same arguments (quatro_features / quatro_match_enqueue / quatro_match_collect / qnq::solve / batch_register), so a
// record equals qn_coarse_to_fine_alignment[_device] of that pair bit for bit (tests/test_gpu_c2f_batch.py).
namespace {
struct C2fSlot { uint32_t pair = 0; qn_ctx* c = nullptr; int rc = QN_OK; bool enq = false; int qvalid = 0; double Tq[16]; int alias = -1; };
// what a lane borrows from the lane that prepared the shared source: the cloud (grid, raw points, pinned grid numbers) and the four per-point arrays of the FPFH stage
struct C2fBorrow {
  qn_ctx* c = nullptr; CloudBuf cloud; float4* nrm; float* spfh; float* fpfh_s; float* fpfh;
  void take(qn_ctx* lane, qn_ctx* from) {
    c = lane; cloud = lane->cloud[0]; nrm = lane->q_normals[0]; spfh = lane->q_spfh[0]; fpfh_s = lane->q_fpfh_s[0]; fpfh = lane->q_fpfh[0];
    lane->cloud[0] = from->cloud[0]; lane->q_normals[0] = from->q_normals[0]; lane->q_spfh[0] = from->q_spfh[0]; lane->q_fpfh_s[0] = from->q_fpfh_s[0]; lane->q_fpfh[0] = from->q_fpfh[0];
  }
  void give_back() {
    if (!c) return;
    c->cloud[0] = cloud; c->q_normals[0] = nrm; c->q_spfh[0] = spfh; c->q_fpfh_s[0] = fpfh_s; c->q_fpfh[0] = fpfh;
    c->cloud[0].has_grid = c->cloud[0].has_cov = false; c->cloud[0].n = 0;
    c = nullptr;
  }
};

// a pair whose clouds and FPFH rows are resident already (qn_kf_verify_loop_candidates_c2f: the store's described keyframes): the lane borrows both sides - points and
// descriptor rows, which is all the matching reads - and builds no grid and no feature (the rows are the ones quatro_fpfh makes of the same cloud: qn_kf_quatro_describe).
// C2fCached itself: qn_kf_internal.h
struct C2fCacheBorrow {
  qn_ctx* c = nullptr; CloudBuf cloud[2]; float* fpfh[2];
  void take(qn_ctx* lane, const C2fCached& k, uint32_t ns, uint32_t nt) {
    c = lane;
    for (int w = 0; w < 2; w++) { cloud[w] = lane->cloud[w]; fpfh[w] = lane->q_fpfh[w]; }
    CloudBuf& s = lane->cloud[0]; CloudBuf& d = lane->cloud[1];
    s.raw = k.src_pts; s.n = ns; d.raw = k.dst_pts; d.n = nt;
    for (int w = 0; w < 2; w++) { lane->cloud[w].has_grid = lane->cloud[w].has_cov = false; lane->cloud[w].knn_tab = nullptr; }
    lane->q_fpfh[0] = k.src_rows; lane->q_fpfh[1] = k.dst_rows;
  }
  void give_back() {
    if (!c) return;
    for (int w = 0; w < 2; w++) { c->cloud[w] = cloud[w]; c->q_fpfh[w] = fpfh[w]; c->cloud[w].has_grid = c->cloud[w].has_cov = false; c->cloud[w].n = 0; c->cloud[w].knn_tab = nullptr; }
    c = nullptr;
  }
};

int c2f_alloc(qn_ctx* owner, qn_ctx* l) {
  if (l->c2f_src) return QN_OK;
  HIPCHK(owner, hipMalloc(&l->c2f_src, sizeof(float4) * l->max_points));
  HIPCHK(owner, hipMalloc(&l->c2f_dst, sizeof(float4) * l->max_points));
  return QN_OK;
}

// one run of m <= B pairs on `owner`'s lanes.  idx[l] = the pair lane l carries.  cached (or null) = per pair, its resident points and rows (C2fCached)
int c2f_run(qn_ctx* owner, const qn_pair_desc* pairs, const uint32_t* idx, uint32_t m, double thr, qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status,
            const C2fCached* cached, int* stage) {
  hipStream_t s = owner->stream;
  std::vector<C2fSlot> S(m);
  std::vector<C2fBorrow> borrowed(m);
  std::vector<C2fCacheBorrow> borrowed_cache(m);
  struct GiveBack { std::vector<C2fBorrow>& b; std::vector<C2fCacheBorrow>& k; ~GiveBack() { for (auto& x : b) x.give_back(); for (auto& x : k) x.give_back(); } } give_back{borrowed, borrowed_cache};      // (every exit path: the lanes get their own buffers back)
  // ---- 1. enqueue the Quatro device stages of every pair (loop_closure.cpp:144 up to the hand-over).  Grid builds and K9-K11 of ALL lanes' clouds ride in NINE launches
  // (k_lanes<F>: blockIdx.y = one cloud of one pair, the machinery of qn_batch.inc) - per-lane launches were 18 per pair, most of them ~5 us of work, 140 per run of eight
  // pairs on a stream that serialises them; the matching stage (K12 / K13) follows per lane.  MEASURED NEUTRAL TO SLIGHTLY SLOWER (qn_context.h, EXPERIMENTS.md round 5): with 3-8 contexts in
  // flight the small launches of one stream hide behind the other streams' kernels and the FPFH kernels themselves are issue-bound - so the default (knob c2f_lanes_fpfh = 0) is
  // that every lane launches its own, the one-pair path's calls; the lanes form stays as a tested variant (tests/test_gpu_c2f_batch.py).
  const bool lanes_fpfh = owner->knob.c2f_lanes_fpfh && owner->feat.normals_fg <= 0 && owner->feat.fpfh_fg <= 0;
  LanePlan plan(owner);
  std::vector<LaneEntry<PackBBoxK::Args>> v_pack; std::vector<LaneEntry<CellCountK::Args>> v_count; std::vector<LaneEntry<ScanLookbackK::Args>> v_scan;
  std::vector<LaneEntry<ScatterK::Args>> v_scat; std::vector<LaneEntry<StableCellsK::Args>> v_stab;
  std::vector<LaneEntry<NormalsK<8>::Args>> v_nrm; std::vector<LaneEntry<SpfhK<8>::Args>> v_spfh; std::vector<LaneEntry<FpfhK<8>::Args>> v_fpfh; std::vector<LaneEntry<RowsToOriginalK::Args>> v_rows;
  auto push_grid = [&](const GridLaunch& G) {
    lane_push(v_pack, G.pack, G.pack_nb); lane_push(v_count, G.count, G.nb); lane_push(v_scan, G.scan, G.scan_nb); lane_push(v_scat, G.scat, G.nb);
    lane_push(v_stab, G.stab, G.nb);
  };
  auto push_fpfh = [&](qn_ctx* c, int w) {      // quatro_fpfh(c, w) as table entries
    CloudBuf& b = c->cloud[w];
    const uint32_t nb = (b.n + QN_BLOCK - 1) / QN_BLOCK;
    const float rn = (float)c->qparams.fpfh_normal_radius, rf = (float)c->qparams.fpfh_radius;
    const float rn2 = (float)(c->qparams.fpfh_normal_radius * c->qparams.fpfh_normal_radius), rf2 = (float)(c->qparams.fpfh_radius * c->qparams.fpfh_radius);
    lane_push(v_nrm, NormalsK<8>::Args{b.grid, rn, rn2, c->q_normals[w]}, nb * 8u);
    lane_push(v_spfh, SpfhK<8>::Args{b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w]}, nb * 8u);
    lane_push(v_fpfh, FpfhK<8>::Args{b.grid, rf, rf2, c->q_normals[w], c->q_spfh[w], c->q_fpfh_s[w]}, nb * 8u);
    lane_push(v_rows, RowsToOriginalK::Args{b.sorted, b.n, c->q_fpfh_s[w], c->q_fpfh[w], QN_FROW, QN_FROW}, nb);
  };
  std::vector<char> pending(m, 0);
  for (uint32_t l = 0; l < m; l++) {
    C2fSlot& q = S[l]; q.pair = idx[l]; q.c = owner->lanes[l];
    qn_ctx* c = q.c; const qn_pair_desc& pd = pairs[q.pair];
    qn_gicp_result* out = &results[q.pair];
    valid[q.pair] = 0; memset(out, 0, sizeof(*out)); out->fitness = DBL_MAX;
    for (int i = 0; i < 4; i++) { out->T[5 * i] = 1.f; out->T64[5 * i] = 1.0; }
    for (int i = 0; i < 16; i++) { q.Tq[i] = (i % 5 == 0) ? 1.0 : 0.0; T_total[16 * (size_t)q.pair + i] = q.Tq[i]; if (T_quatro) T_quatro[16 * (size_t)q.pair + i] = q.Tq[i]; }
    if (c != owner) { c->qparams = owner->qparams; c->qparams_set = owner->qparams_set; c->feat = owner->feat; }
    c->knob.pair_pipeline = false; c->tgt_pending = false; c->tgt_on_stream2 = false;
    if (pd.ns == 0 || pd.nt == 0) { q.rc = QN_ERR_EMPTY_CLOUD; continue; }
    if ((q.rc = c2f_alloc(owner, c)) != QN_OK) return q.rc;
    if ((q.rc = quatro_alloc(c)) != QN_OK) { owner->last_error = c->last_error; return q.rc; }      // (the lane's own buffers exist before any of them is swapped out)
    if (cached) {                                                                 // resident features: the matching stage straight away, on borrowed points and rows
      if (pd.ns > c->max_points || pd.nt > c->max_points) { q.rc = QN_ERR_CAPACITY; continue; }      // (what set_cloud says of such a cloud)
      borrowed_cache[l].take(c, cached[q.pair], pd.ns, pd.nt);
      q.rc = quatro_match_enqueue(c, pd.ns, pd.nt, c->qparams);
      if (q.rc == QN_ERR_HIP) { owner->last_error = c->last_error; return q.rc; }
      q.enq = q.rc == QN_OK;
      continue;
    }
    // the candidates of ONE query name the same source buffer: the first lane of the run that carries it prepares it (grid, normals, SPFH, FPFH), the others borrow
    // the result (read-only from here on: the matching reads raw points and descriptor rows, the row hashes written into the rows are the same for every borrower)
    if (owner->knob.batch_share_source && pd.src != nullptr) {
      for (uint32_t j = 0; j < l; j++) {
        const qn_pair_desc& pj = pairs[S[j].pair];
        if ((S[j].enq || pending[j]) && S[j].alias < 0 && pj.src == pd.src && pj.ns == pd.ns && pj.stride_bytes == pd.stride_bytes && pj.on_device == pd.on_device) { q.alias = (int)j; break; }
      }
    }
    if (!lanes_fpfh) {
      if (q.alias >= 0) { borrowed[l].take(c, S[q.alias].c); q.rc = quatro_features_target_only(c, pd.dst, pd.nt, pd.stride_bytes, pd.on_device != 0); }
      else q.rc = quatro_features(c, pd.src, pd.ns, pd.dst, pd.nt, pd.stride_bytes, pd.on_device != 0);
      if (q.rc == QN_ERR_HIP) { owner->last_error = c->last_error; return q.rc; }
      if (q.rc != QN_OK) continue;
      q.rc = quatro_match_enqueue(c, pd.ns, pd.nt, c->qparams);
      if (q.rc == QN_ERR_HIP) { owner->last_error = c->last_error; return q.rc; }
      q.enq = q.rc == QN_OK;
      continue;
    }
    // setInputCloud of both clouds as table entries (validation and upload as set_cloud; FPFH grid: cell = r_f / 2), the target with the second scratch set
    const double save = c->lane.cell_override;
    c->lane.cell_override = c->qparams.fpfh_radius * 0.5;
    GridLaunch gs, gt; int rc = QN_OK;
    if (q.alias < 0) rc = lane_set_cloud(c, QN_SOURCE, pd.src, pd.ns, pd.stride_bytes, pd.on_device != 0, s, &gs);
    if (rc == QN_OK) { ScratchSwap sw(c); rc = lane_set_cloud(c, QN_TARGET, pd.dst, pd.nt, pd.stride_bytes, pd.on_device != 0, s, &gt); }
    c->lane.cell_override = save;
    if (rc == QN_ERR_HIP) { owner->last_error = c->last_error; return rc; }
    q.rc = rc;
    if (rc != QN_OK) { if (q.alias < 0) { c->cloud[0].has_grid = false; c->cloud[0].n = 0; } c->cloud[1].has_grid = false; c->cloud[1].n = 0; q.alias = -1; continue; }
    if (q.alias < 0) { push_grid(gs); push_fpfh(c, 0); }
    else borrowed[l].take(c, S[q.alias].c);
    push_grid(gt); push_fpfh(c, 1);
    pending[l] = 1;
  }
  if (lanes_fpfh) {
    plan.add<PackBBoxK>(v_pack, QN_K_GRID_BUILD); plan.add<CellCountK>(v_count, QN_K_GRID_BUILD); plan.add<ScanLookbackK>(v_scan, QN_K_GRID_BUILD); plan.add<ScatterK>(v_scat, QN_K_GRID_BUILD); plan.add<StableCellsK>(v_stab, QN_K_GRID_BUILD);
    plan.add<NormalsK<8>>(v_nrm, QN_K_FPFH_NORMALS); plan.add<SpfhK<8>>(v_spfh, QN_K_FPFH_SPFH); plan.add<FpfhK<8>>(v_fpfh, QN_K_FPFH_FPFH); plan.add<RowsToOriginalK>(v_rows, QN_K_FPFH_FPFH);
    const int prc = plan.run();
    if (prc != QN_OK) return prc;
    for (uint32_t l = 0; l < m; l++) {      // K12 / K13 of every pair, lane by lane, behind the shared launches
      if (!pending[l]) continue;
      C2fSlot& q = S[l]; const qn_pair_desc& pd = pairs[q.pair];
      q.rc = quatro_match_enqueue(q.c, pd.ns, pd.nt, q.c->qparams);
      if (q.rc == QN_ERR_HIP) { owner->last_error = q.c->last_error; return q.rc; }
      q.enq = q.rc == QN_OK;
    }
  }
  // ---- 2. one synchronisation, then the hand-over blocks and the host solver, pair by pair
  HIPCHK(owner, hipStreamSynchronize(s));
  std::vector<qn_pair_desc> gp(m); std::vector<uint32_t> gidx; gidx.reserve(m);
  for (uint32_t l = 0; l < m; l++) {
    C2fSlot& q = S[l]; qn_ctx* c = q.c; const qn_pair_desc& pd = pairs[q.pair];
    if (q.enq) {
      qnq::TailResult tr;
      q.rc = quatro_match_collect(c, pd.ns, pd.nt, c->qparams, false, tr);      // (a survivor-list overflow repeats the matching with the VALU search, synchronously: same answer)
      if (q.rc == QN_ERR_HIP) { owner->last_error = c->last_error; return q.rc; }
      if (q.rc == QN_OK) {
        qnq::SolveOut so;
        qnq::solve(tr.S, tr.D, c->qparams, &so);
        memcpy(q.Tq, so.T, sizeof(so.T)); q.qvalid = so.valid;
        if (T_quatro) memcpy(T_quatro + 16 * (size_t)q.pair, q.Tq, sizeof(q.Tq));
        if (stage) stage[q.pair] = 1;
      }
    }
    status[q.pair] = q.rc;
    if (q.rc != QN_OK || !q.qvalid) continue;                                     // :145-148: Quatro did not converge -> the pair is invalid, no fine stage
    // ---- 3. transformPcd on the device (:152); both clouds of the fine stage as float4 in caller order
    HIPCHK(owner, hipMemcpyAsync(c->q_T, q.Tq, sizeof(q.Tq), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_transform_cloud_f64, dim3((pd.ns + 255) / 256), dim3(256), 0, s, c->cloud[0].raw, pd.ns, c->q_T, c->c2f_src);
    HIPCHK(owner, hipMemcpyAsync(c->c2f_dst, c->cloud[1].raw, sizeof(float4) * pd.nt, hipMemcpyDeviceToDevice, s));
    gp[l] = qn_pair_desc{(const float*)c->c2f_src, pd.ns, (const float*)c->c2f_dst, pd.nt, 16u, 1};
    gidx.push_back(l);
  }
  HIPCHK(owner, hipGetLastError());
  for (auto& x : borrowed_cache) x.give_back();
  for (auto& x : borrowed) x.give_back();      // the transforms above are enqueued: from here on every lane works on its own source buffers again (the GICP lanes pack into them)
  if (gidx.empty()) return QN_OK;
  // ---- the fine stage (:153): the accepted pairs through the GICP lanes (lane j of the GICP run = the j-th accepted pair; its clouds live in the Quatro lane's c2f buffers)
  std::vector<qn_gicp_result> gres(m); std::vector<int> gval(m, 0), gst(m, QN_ERR_HIP);
  std::vector<const float*> last_src(owner->lanes.size(), nullptr); std::vector<uint64_t> last_key(owner->lanes.size(), 0);
  const int rc = batch_register(owner, gp.data(), gidx.data(), (uint32_t)gidx.size(), thr, gres.data(), gval.data(), gst.data(), last_src, last_key, nullptr);
  if (rc != QN_OK) return rc;
  // ---- 4. compose (:156) and accept (:129)
  for (uint32_t l : gidx) {
    const C2fSlot& q = S[l];
    status[q.pair] = gst[l];
    if (gst[l] != QN_OK) continue;
    if (stage) stage[q.pair] = 2;
    results[q.pair] = gres[l]; valid[q.pair] = gval[l];
    double* Tt = T_total + 16 * (size_t)q.pair;
    for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) { double v = 0; for (int k = 0; k < 4; k++) v += (double)gres[l].T[4 * a + k] * q.Tq[4 * k + b]; Tt[4 * a + b] = v; }
  }
  return QN_OK;
}
}  // namespace

// the driver of qn_coarse_to_fine_align_batch; cached (or null): per pair, resident points and FPFH rows the lanes borrow (qn_kf_verify_loop_candidates_c2f);
// stage (or null): per pair 0, 1 when T_quatro was solved, 2 when the fine stage ran as well (qn_kf_verify_cloud)
static int c2f_batch(qn_ctx* const* ctxs, uint32_t n_ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr,
                     qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status, const C2fCached* cached, int* stage = nullptr) {
  if (!ctxs || n_ctx == 0 || (n_pairs && (!pairs || !results || !T_total || !valid || !status))) return QN_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n_ctx; i++) if (!ctxs[i]) return QN_ERR_INVALID_ARG;
  if (n_pairs == 0) return QN_OK;
  if (stage) for (uint32_t i = 0; i < n_pairs; i++) stage[i] = 0;
  std::atomic<uint32_t> next{0}, final_share{0};
  std::vector<int> wrc(n_ctx, QN_OK);
  auto worker = [&](uint32_t w) {
    qn_ctx* c = ctxs[w];
    if (hipSetDevice(c->device) != hipSuccess) { wrc[w] = QN_ERR_HIP; return; }
    if (join_target(c) != QN_OK) { wrc[w] = QN_ERR_HIP; return; }
    if (!c->qparams_set) { qn_quatro_default_params(&c->qparams); c->qparams_set = true; }
    const bool lanes_ok = batch_supported(c) && batch_ensure_lanes(c) == QN_OK;
    const bool sp = c->knob.pair_pipeline, sb = c->knob.persist_batch_off;
    if (!lanes_ok) {                                                              // (knobs that rule the lanes out: the one-pair path, pair by pair - same records)
      for (;;) {
        const uint32_t i = next.fetch_add(1);
        if (i >= n_pairs) break;
        const qn_pair_desc& p = pairs[i];
        status[i] = coarse_to_fine(c, p.src, p.ns, p.dst, p.nt, p.stride_bytes, p.on_device != 0, score_thr, &results[i], T_total + 16 * (size_t)i, T_quatro ? T_quatro + 16 * (size_t)i : nullptr, &valid[i],
                                   stage ? &stage[i] : nullptr);
      }
      return;
    }
    const uint32_t B = (uint32_t)c->lanes.size();
    std::vector<uint32_t> idx(B);
    for (;;) {
      uint32_t base = next.load(), m = 0;
      for (;;) {                                                                  // runs of B; the last round in n_ctx equal shares so that the contexts finish together (as qn_icp_alignment_batch)
        if (base >= n_pairs) break;
        const uint32_t rem = n_pairs - base;
        if (rem > n_ctx * B) m = B;
        else {
          uint32_t q = final_share.load();
          if (q == 0) { uint32_t want = std::min<uint32_t>(B, std::max<uint32_t>((uint32_t)std::max(1, ctxs[0]->knob.batch_min_share), (rem + n_ctx - 1) / n_ctx)); if (final_share.compare_exchange_strong(q, want)) q = want; }
          m = std::min(q, rem);
        }
        m = std::min(m, B);                                             // (never more pairs than THIS context has lanes: the share was fixed with the first context's lane count - ADVICE r5)
        if (next.compare_exchange_weak(base, base + m)) break;
      }
      if (base >= n_pairs) break;
      for (uint32_t l = 0; l < m; l++) idx[l] = base + l;
      const int rc = c2f_run(c, pairs, idx.data(), m, score_thr, results, T_total, T_quatro, valid, status, cached, stage);
      if (rc != QN_OK) { (void)hipStreamSynchronize(c->stream); for (uint32_t l = 0; l < m; l++) { status[base + l] = rc; valid[base + l] = 0; } wrc[w] = rc; }
    }
    c->knob.pair_pipeline = sp; c->knob.persist_batch_off = sb;
  };
  qn::WorkerPool::instance().run(n_ctx, worker);
  return QN_OK;
}
extern "C" int qn_coarse_to_fine_align_batch(qn_ctx* const* ctxs, uint32_t n_ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr,
                                             qn_gicp_result* results, double* T_total, double* T_quatro, int* valid, int* status) {
  return c2f_batch(ctxs, n_ctx, pairs, n_pairs, score_thr, results, T_total, T_quatro, valid, status, nullptr);
}
// the same on one context, with each pair's stage and, when the clouds are resident, their rows (for another translation unit: the pair driver of qn_verify.hip)
int qn_ctx_int_c2f_batch_stage(qn_ctx* ctx, const qn_pair_desc* pairs, uint32_t n_pairs, double score_thr, qn_gicp_result* results, double* T_total, double* T_quatro,
                               int* valid, int* status, const C2fCached* cached, int* stage) {
  qn_ctx* const one[1] = {ctx};
  return c2f_batch(one, 1, pairs, n_pairs, score_thr, results, T_total, T_quatro, valid, status, cached, stage);
}
