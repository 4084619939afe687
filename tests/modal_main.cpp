// tps_amd/csrc/modal.hpp on the host, alone, under the sanitizers (tests/test_modal_host.py): V V^-1 = I for every order and
// both node sets, the closed values of sigma, the scalar restatement of the three operations on the elements of the fixture
// file (argv[1], written by tests/modal_util.py in long double: one 2-D and one 3-D element), and every refusal of the plan.
// Prints MODAL CLEAN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "../tps_amd/csrc/basis.hpp"
#include "../tps_amd/csrc/modal.hpp"

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

void matrices() {
  for (int lobatto = 0; lobatto <= 1; lobatto++)
    for (int p = 1; p <= TPSRHS_MAXORDER; p++) {
      const int n1 = p + 1;
      double nodes[MODAL_MAXN1], wts[MODAL_MAXN1];
      segment_rule01(lobatto, n1, nodes, wts);
      const ModalBasis b = modal_basis(lobatto, n1, nodes);
      EXPECT(b.n1 == n1, "n1");
      for (int i = 0; i < n1; i++)
        for (int j = 0; j < n1; j++) {
          long double s = 0.0L, sa = 0.0L;
          for (int k = 0; k < n1; k++) {
            s += static_cast<long double>(b.V.m[i * n1 + k]) * b.Vinv.m[k * n1 + j];
            sa += std::fabs(static_cast<long double>(b.V.m[i * n1 + k]) * b.Vinv.m[k * n1 + j]);
          }
          // every entry of the two factors is within half an ulp of the exact one
          EXPECT(std::fabs(static_cast<double>(s - (i == j ? 1.0L : 0.0L))) <= 2.0 * EPS * static_cast<double>(sa) + 1e-300,
                 "basis %d p=%d: (V Vinv)[%d][%d] = %.17Lg", lobatto, p, i, j, s);
        }
      for (int a = 0; a < n1; a++) {
        EXPECT(b.V.m[a * n1] == 1.0, "P_0 = 1");
        EXPECT(std::fabs(b.V.m[a * n1 + 1] - (2.0 * nodes[a] - 1.0)) <= 2.0 * EPS, "P_1 = z");
      }
      for (int k = 0; k < n1; k++) EXPECT(b.gamma[k] == 1.0 / (2.0 * k + 1.0), "gamma_%d", k);
      // F keeps constants (sigma_0 = 1) and, with every sigma_k = 1 up to k_c = p - 1 and alpha tiny, is nearly the identity
      for (int kc = 0; kc < p; kc++) {
        const ModalMatrix F = modal_filter_matrix(lobatto, n1, nodes, kc, 36.0, 4);
        for (int a = 0; a < n1; a++) {
          long double s = 0.0L, sa = 0.0L;
          for (int i = 0; i < n1; i++) {
            s += F.m[a * n1 + i];
            sa += std::fabs(F.m[a * n1 + i]);
          }
          EXPECT(std::fabs(static_cast<double>(s - 1.0L)) <= 2.0 * EPS * static_cast<double>(sa), "basis %d p=%d k_c=%d: row %d of F sums to %.17Lg",
                 lobatto, p, kc, a, s);
        }
      }
    }
}

void sigmas() {
  long double s[MODAL_MAXN1];
  modal_sigma(4, 1, 2.5, 1, s);  // eta = 0, 0, 1/3, 2/3, 1
  EXPECT(s[0] == 1.0L && s[1] == 1.0L, "sigma below the cutoff");
  for (int k = 2; k <= 4; k++)
    EXPECT(std::fabs(static_cast<double>(s[k] - std::exp(-2.5L * (k - 1) / 3.0L))) <= 4 * EPS, "sigma_%d, s = 1", k);
  modal_sigma(5, 0, 36.0, 16, s);
  EXPECT(s[0] == 1.0L, "sigma_0");
  EXPECT(std::fabs(static_cast<double>(s[5] / std::exp(-36.0L) - 1.0L)) <= 4 * EPS, "sigma_p = exp(-alpha)");
  EXPECT(std::fabs(static_cast<double>(s[1] - std::exp(-36.0L * std::pow(0.2L, 16)))) <= 4 * EPS, "sigma_1, s = 16");
  for (int k = 1; k <= 5; k++) EXPECT(s[k] < s[k - 1] || s[k - 1] == 1.0L, "sigma decreases");
  modal_sigma(1, 0, 0.5, 3, s);  // p = 1: the only filtered mode has eta = 1
  EXPECT(std::fabs(static_cast<double>(s[1] - std::exp(-0.5L))) <= 4 * EPS, "sigma_1 at p = 1");
}

// the fixture: see tests/test_modal_host.py::_fixture for the order of the numbers
void fixture(const char *path) {
  std::ifstream in(path);
  EXPECT(in.good(), "cannot read %s", path);
  int ncases = 0;
  in >> ncases;
  EXPECT(ncases >= 2, "the fixture holds %d cases", ncases);
  for (int c = 0; c < ncases; c++) {
    int dim, p, lobatto, neq, expect_filtered;
    tpsrhs_modal_filter f = {};
    in >> dim >> p >> lobatto >> neq >> f.cutoff >> f.alpha >> f.exponent >> f.conservative >> f.sensor_row >> f.sensor_threshold >>
        expect_filtered;
    f.num_rows = -1;
    const int n1 = p + 1, npe = dim == 3 ? n1 * n1 * n1 : n1 * n1;
    std::vector<double> W(npe), x(static_cast<size_t>(neq) * npe), uh(npe), duh(npe), E(n1), dE(n1), xf(x.size()), dxf(x.size());
    double S, dS;
    auto read = [&](std::vector<double> &v) {
      for (double &a : v) in >> a;
    };
    read(W), read(x), read(uh), read(duh), read(E), read(dE);
    in >> S >> dS;
    read(xf), read(dxf);
    EXPECT(!in.fail(), "case %d: the fixture ends early", c);
    double nodes[MODAL_MAXN1], wts[MODAL_MAXN1];
    segment_rule01(lobatto, n1, nodes, wts);
    const ModalBasis b = modal_basis(lobatto, n1, nodes);
    // 1. the forward transform of row 0, then back: in place
    std::vector<double> t(npe);
    modal_apply_element(dim, n1, b.Vinv.m, x.data(), 1, t.data(), 1);
    for (int n = 0; n < npe; n++)
      EXPECT(std::fabs(t[n] - uh[n]) <= duh[n] + EPS * std::fabs(uh[n]), "case %d: u^[%d] = %.17g, expected %.17g +- %.3g", c, n, t[n],
             uh[n], duh[n]);
    modal_apply_element(dim, n1, b.V.m, t.data(), 1, t.data(), 1);
    for (int n = 0; n < npe; n++) {
      double scale = 0.0;
      for (int m = 0; m < npe; m++) scale = std::fmax(scale, std::fabs(x[m]));
      EXPECT(std::fabs(t[n] - x[n]) <= 64.0 * dim * n1 * n1 * EPS * scale, "case %d: inverse(forward) at node %d: %.17g against %.17g", c, n,
             t[n], x[n]);
    }
    // 2. shell energies and sensor of row 0
    std::vector<double> Eg(n1);
    const double Sg = modal_energy_element(dim, b, x.data(), 1, Eg.data());
    for (int m = 0; m < n1; m++)
      EXPECT(std::fabs(Eg[m] - E[m]) <= dE[m] + EPS * E[m], "case %d: E_%d = %.17g, expected %.17g +- %.3g", c, m, Eg[m], E[m], dE[m]);
    EXPECT(std::fabs(Sg - S) <= dS + EPS * S, "case %d: S = %.17g, expected %.17g +- %.3g", c, Sg, S, dS);
    // 3. the filter with decision and correction
    const ModalPlan pl = plan_modal_filter(f, neq, p, "fixture");
    EXPECT(pl.num_rows == neq, "num_rows = -1 lists every row");
    const ModalMatrix F = modal_filter_matrix(lobatto, n1, nodes, pl.cutoff, pl.alpha, pl.exponent);
    std::vector<double> y = x;
    double Sf = -1.0;
    const bool filtered = modal_filter_element(dim, b, F, pl, W.data(), 1, y.data(), 1, npe, &Sf);
    EXPECT(filtered == (expect_filtered != 0), "case %d: filtered = %d", c, filtered ? 1 : 0);
    if (!filtered) EXPECT(std::memcmp(y.data(), x.data(), sizeof(double) * x.size()) == 0, "case %d: an unfiltered element was written", c);
    for (size_t n = 0; n < y.size(); n++)
      EXPECT(std::fabs(y[n] - xf[n]) <= dxf[n] + EPS * std::fabs(xf[n]), "case %d: filtered[%zu] = %.17g, expected %.17g +- %.3g", c, n, y[n],
             xf[n], dxf[n]);
    if (filtered && pl.conservative) {
      for (int r = 0; r < neq; r++) {
        long double a = 0.0L, bsum = 0.0L, s1 = 0.0L;
        for (int n = 0; n < npe; n++) {
          a += static_cast<long double>(W[n]) * y[r * npe + n];
          bsum += static_cast<long double>(W[n]) * x[r * npe + n];
          s1 += std::fabs(static_cast<long double>(W[n])) * (std::fabs(x[r * npe + n]) + std::fabs(y[r * npe + n]));
        }
        EXPECT(std::fabs(static_cast<double>(a - bsum)) <= (npe + 4) * EPS * static_cast<double>(s1), "case %d row %d: the integral moved by %.3Lg",
               c, r, a - bsum);
      }
    }
    // strided layouts cross the index arithmetic: nodes 2 apart, rows 3 npe apart, weights 3 apart
    std::vector<double> ys(static_cast<size_t>(neq) * 3 * npe, -9.0e9), Ws(3 * npe, -7.0);
    for (int r = 0; r < neq; r++)
      for (int n = 0; n < npe; n++) ys[r * 3 * npe + 2 * n] = x[r * npe + n];
    for (int n = 0; n < npe; n++) Ws[3 * n] = W[n];
    modal_filter_element(dim, b, F, pl, Ws.data(), 3, ys.data(), 2, 3 * npe);
    for (int r = 0; r < neq; r++)
      for (int n = 0; n < npe; n++) {
        EXPECT(ys[r * 3 * npe + 2 * n] == y[r * npe + n], "case %d: strided result differs at row %d node %d", c, r, n);
        EXPECT(ys[r * 3 * npe + 2 * n + 1] == -9.0e9, "case %d: padding written", c);
      }
  }
}

template <class F>
void refused(const char *name, const char *fragment, F &&call) {
  try {
    call();
    EXPECT(false, "%s: not refused", name);
  } catch (const std::invalid_argument &e) {
    EXPECT(std::strstr(e.what(), fragment) != nullptr && std::strstr(e.what(), "who") != nullptr, "%s: message '%s'", name, e.what());
  }
}

void refusals() {
  const int neq = 5, p = 3;
  tpsrhs_modal_filter ok = {};
  ok.num_rows = 2;
  ok.rows[0] = 0;
  ok.rows[1] = 4;
  ok.cutoff = 2;
  ok.alpha = 36.0;
  ok.exponent = 16;
  ok.conservative = 7;
  ok.sensor_row = -1;
  ok.sensor_threshold = std::numeric_limits<double>::infinity();  // valid: never
  const ModalPlan pl = plan_modal_filter(ok, neq, p, "who");
  EXPECT(pl.num_rows == 2 && pl.rows[0] == 0 && pl.rows[1] == 4 && pl.conservative == 1 && pl.cutoff == 2 && pl.sensor_row == -1, "valid plan");
  auto with = [&](auto change) {
    tpsrhs_modal_filter f = ok;
    change(f);
    return f;
  };
  const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
  refused("row_negative", "outside", [&] { plan_modal_filter(with([](auto &f) { f.rows[1] = -1; }), neq, p, "who"); });
  refused("row_too_large", "outside", [&] { plan_modal_filter(with([&](auto &f) { f.rows[1] = neq; }), neq, p, "who"); });
  refused("row_twice", "twice", [&] { plan_modal_filter(with([](auto &f) { f.rows[1] = 0; }), neq, p, "who"); });
  refused("num_rows_low", "num_rows", [&] { plan_modal_filter(with([](auto &f) { f.num_rows = -2; }), neq, p, "who"); });
  refused("num_rows_high", "num_rows", [&] { plan_modal_filter(with([&](auto &f) { f.num_rows = neq + 1; }), neq, p, "who"); });
  refused("cutoff_negative", "cutoff", [&] { plan_modal_filter(with([](auto &f) { f.cutoff = -1; }), neq, p, "who"); });
  refused("cutoff_p", "cutoff", [&] { plan_modal_filter(with([&](auto &f) { f.cutoff = p; }), neq, p, "who"); });
  refused("alpha_zero", "alpha", [&] { plan_modal_filter(with([](auto &f) { f.alpha = 0.0; }), neq, p, "who"); });
  refused("alpha_negative", "alpha", [&] { plan_modal_filter(with([](auto &f) { f.alpha = -1.0; }), neq, p, "who"); });
  refused("alpha_nan", "alpha", [&] { plan_modal_filter(with([&](auto &f) { f.alpha = nan; }), neq, p, "who"); });
  refused("alpha_inf", "alpha", [&] { plan_modal_filter(with([&](auto &f) { f.alpha = inf; }), neq, p, "who"); });
  refused("exponent_zero", "exponent", [&] { plan_modal_filter(with([](auto &f) { f.exponent = 0; }), neq, p, "who"); });
  refused("sensor_row_low", "sensor_row", [&] { plan_modal_filter(with([](auto &f) { f.sensor_row = -2; }), neq, p, "who"); });
  refused("sensor_row_high", "sensor_row", [&] { plan_modal_filter(with([&](auto &f) { f.sensor_row = neq; }), neq, p, "who"); });
  refused("threshold_nan", "sensor_threshold", [&] { plan_modal_filter(with([&](auto &f) { f.sensor_threshold = nan; }), neq, p, "who"); });
  // the decisions at the edges
  EXPECT(modal_sensor(0.0, 0.0) == 0.0, "a zero element has S = 0");
  EXPECT(modal_sensor(nan, nan) != modal_sensor(nan, nan), "a NaN element has a NaN sensor");
  EXPECT(!modal_filtered(nan, 0.0), "a NaN sensor does not filter");
  EXPECT(!modal_filtered(1.0, inf), "threshold +inf filters nothing");
  EXPECT(!modal_filtered(0.5, 0.5) && modal_filtered(0.5, 0.25), "S > threshold, strictly");
}
}  // namespace

int main(int argc, char **argv) {
  matrices();
  sigmas();
  refusals();
  if (argc > 1) fixture(argv[1]);
  EXPECT(argc > 1, "no fixture file given");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("MODAL CLEAN\n");
  return 0;
}
