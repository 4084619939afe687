// tps_amd/csrc/limiter.hpp on the host, alone, under the sanitizers (tests/test_limiter_host.py): the per-element row step
// and pressure step for N = 4, 9, 27, 64, 216 nodes against closed forms -- an untouched, a limited, a clamped and a NaN
// element, and the three outcomes of the pressure step.  Prints LIMITER CLEAN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../tps_amd/csrc/limiter.hpp"

using namespace tpsrhs;

namespace {
int failures = 0;
#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      failures++;                                  \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                    \
      std::printf("\n");                           \
    }                                              \
  } while (0)

const double EPS = std::numeric_limits<double>::epsilon();

bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}
long double wsum(const std::vector<double> &W, int ws, const std::vector<double> &v, int vs, int N, bool absolute = false) {
  long double s = 0.0L;
  for (int n = 0; n < N; n++) s += static_cast<long double>(W[n * ws]) * (absolute ? std::fabs(v[n * vs]) : v[n * vs]);
  return s;
}

// ws, vs: the strides the arrays are laid out with (1, 1 as on the device; others to cross the index arithmetic)
void row_cases(int N, int ws, int vs, double f) {
  std::vector<double> W(static_cast<size_t>(N) * ws, -7.0), v(static_cast<size_t>(N) * vs, -9.0e9), before;
  long double SW = 0.0L;
  for (int n = 0; n < N; n++) {
    W[n * ws] = 1.0 + 0.01 * n;
    SW += W[n * ws];
  }
  // untouched: everything above the floor; the minimum ON the floor counts as untouched too
  for (int n = 0; n < N; n++) v[n * vs] = f + 1.0 + 0.01 * n;
  before = v;
  EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_UNTOUCHED, "N=%d untouched: outcome", N);
  EXPECT(same_bits(v, before), "N=%d untouched: bits changed", N);
  v[(N - 1) * vs] = f;
  before = v;
  EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_UNTOUCHED, "N=%d minimum on the floor: outcome", N);
  EXPECT(same_bits(v, before), "N=%d minimum on the floor: bits changed", N);
  // limited: node 0 at f - 1, the others at f + 2: mean = f + 2 - 3 W_0 / SW, theta = (mean - f) / (mean - f + 1),
  // node 0 lands on the floor and the others on mean + theta (f + 2 - mean)
  for (int n = 0; n < N; n++) v[n * vs] = f + 2.0;
  v[0] = f - 1.0;
  before = v;
  EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_SCALED, "N=%d limited: outcome", N);
  {
    const long double mean = f + 2.0L - 3.0L * W[0] / SW, theta = (mean - f) / (mean - f + 1.0L);
    const long double other = mean + theta * (f + 2.0L - mean);
    const double tol = 8.0 * N * EPS * (std::fabs(f) + 2.0);
    EXPECT(v[0] >= f && v[0] - f <= tol, "N=%d limited: node 0 = %.17g, floor %.17g", N, v[0], f);
    for (int n = 1; n < N; n++) {
      EXPECT(v[n * vs] >= f, "N=%d limited: node %d below the floor", N, n);
      EXPECT(std::fabs(v[n * vs] - static_cast<double>(other)) <= tol, "N=%d limited: node %d = %.17g, closed form %.17g", N, n,
             v[n * vs], static_cast<double>(other));
    }
    const long double drift = wsum(W, ws, v, vs, N) - wsum(W, ws, before, vs, N);
    EXPECT(std::fabs(static_cast<double>(drift)) <= (N + 4) * EPS * static_cast<double>(wsum(W, ws, before, vs, N, true)),
           "N=%d limited: the element integral moved by %.3e", N, static_cast<double>(drift));
    std::vector<double> once = v;  // idempotent: the second application finds m >= f
    EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_UNTOUCHED, "N=%d limited twice: outcome", N);
    EXPECT(same_bits(v, once), "N=%d limited twice: bits changed", N);
  }
  // clamped: the mean is below the floor: the reference's clamp, node 0 (above the floor) keeps its bits
  for (int n = 0; n < N; n++) v[n * vs] = f - 1.0;
  v[0] = f + 0.1;
  before = v;
  EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_CLAMPED, "N=%d clamped: outcome", N);
  EXPECT(v[0] == before[0], "N=%d clamped: node 0 changed", N);
  for (int n = 1; n < N; n++) EXPECT(v[n * vs] == f, "N=%d clamped: node %d = %.17g", N, n, v[n * vs]);
  // NaN: one NaN node makes the mean NaN: the element is left as it is, although another node is below the floor
  for (int n = 0; n < N; n++) v[n * vs] = f + 1.0;
  v[0] = f - 1.0;
  v[(N / 2) * vs] = std::numeric_limits<double>::quiet_NaN();
  before = v;
  EXPECT(limit_row(N, W.data(), ws, v.data(), vs, f) == LIMITER_NAN, "N=%d NaN: outcome", N);
  EXPECT(same_bits(v, before), "N=%d NaN: bits changed", N);
  // the padding between strided entries is never written
  for (int n = 0; n < N; n++)
    for (int k = 1; k < vs; k++) EXPECT(v[n * vs + k] == -9.0e9, "N=%d: padding written", N);
}

void pressure_cases(int N, int nvel) {
  const int neq = nvel + 2;
  const double gm1 = 0.4, fp = 0.5;
  std::vector<double> W(N), U(static_cast<size_t>(neq) * N), before;  // the device layout: U[row][node]
  for (int n = 0; n < N; n++) W[n] = 1.0 + 0.01 * n;
  auto fill = [&](double E) {
    for (int n = 0; n < N; n++) {
      U[n] = 1.0 + 0.001 * n;
      for (int d = 1; d <= nvel; d++) U[d * N + n] = 0.1 * d;
      U[(nvel + 1) * N + n] = E;
    }
  };
  auto p_at = [&](const std::vector<double> &A, int n) { return limiter_pressure(A.data() + n, N, nvel, gm1); };
  // p = 0.4 (2.5 - small) ~ 1 everywhere: nothing happens
  fill(2.5);
  before = U;
  EXPECT(limit_pressure(N, W.data(), 1, U.data(), 1, N, neq, nvel, gm1, fp) == LIMITER_P_UNTOUCHED, "N=%d pressure untouched", N);
  EXPECT(same_bits(U, before), "N=%d pressure untouched: bits changed", N);
  // a dip at node 0 (less energy, more momentum): p_0 < f_p < pbar: scaled, every row mean kept, p >= f_p everywhere
  U[(nvel + 1) * N] = 0.6;
  U[N] = 0.5;
  before = U;
  EXPECT(p_at(U, 0) < fp, "N=%d pressure dip: p_0 = %g", N, p_at(U, 0));
  EXPECT(limit_pressure(N, W.data(), 1, U.data(), 1, N, neq, nvel, gm1, fp) == LIMITER_P_SCALED, "N=%d pressure scaled", N);
  for (int n = 0; n < N; n++) EXPECT(p_at(U, n) >= fp * (1.0 - 1e-12), "N=%d pressure scaled: p_%d = %.17g", N, n, p_at(U, n));
  EXPECT(p_at(U, 0) <= fp * 1.2, "N=%d pressure scaled: node 0 moved further than the concavity bound explains", N);
  for (int r = 0; r < neq; r++) {
    std::vector<double> a(U.begin() + r * N, U.begin() + (r + 1) * N), b(before.begin() + r * N, before.begin() + (r + 1) * N);
    const long double drift = wsum(W, 1, a, 1, N) - wsum(W, 1, b, 1, N);
    EXPECT(std::fabs(static_cast<double>(drift)) <= (N + 4) * EPS * static_cast<double>(wsum(W, 1, b, 1, N, true)),
           "N=%d pressure scaled: row %d integral moved by %.3e", N, r, static_cast<double>(drift));
  }
  // the mean pressure itself below the floor: untouched
  fill(0.6);
  before = U;
  EXPECT(limit_pressure(N, W.data(), 1, U.data(), 1, N, neq, nvel, gm1, fp) == LIMITER_P_UNFIXABLE, "N=%d pressure unfixable", N);
  EXPECT(same_bits(U, before), "N=%d pressure unfixable: bits changed", N);
}
}  // namespace

int main() {
  const int sizes[5] = {4, 9, 27, 64, 216};
  for (int N : sizes) {
    row_cases(N, 1, 1, 0.0);
    row_cases(N, 1, 1, 0.25);
    row_cases(N, 3, 2, -1.5);
    pressure_cases(N, 2);
    pressure_cases(N, 3);
  }
  // the decisions on their own, at the edges
  EXPECT(limiter_row_outcome(std::nan(""), -1.0, 0.0) == LIMITER_NAN, "NaN mean");
  EXPECT(limiter_row_outcome(0.0, -1.0, 0.0) == LIMITER_CLAMPED, "mean on the floor is inadmissible");
  EXPECT(limiter_row_outcome(1.0, INFINITY, 0.0) == LIMITER_UNTOUCHED, "no finite minimum");
  EXPECT(limiter_pressure_outcome(1.0, 0.5, 0.5) == LIMITER_P_UNTOUCHED, "p_min on the floor");
  EXPECT(limiter_pressure_outcome(std::nan(""), 0.1, 0.5) == LIMITER_P_UNFIXABLE, "NaN mean pressure");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("LIMITER CLEAN\n");
  return 0;
}
