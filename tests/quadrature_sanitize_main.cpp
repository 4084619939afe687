// Stand-alone driver of tps_amd/csrc/quadrature_points.hpp for the host sanitizers (tests/test_quadrature_sanitize.py builds
// it with -fsanitize=address,undefined and runs it as a child process): a warped box of hexahedra and a ring of
// quadrilaterals at every order, output arrays of exactly the needed size (a write behind them is an overflow), either
// output NULL, the sum of the weights against the known volume, the refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tps_amd/csrc/quadrature_points.hpp"

namespace {
int g_failures = 0;
void check(bool ok, const char *what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    g_failures++;
  }
}

// MFEM corner order
const int kQuad[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
const int kHex[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};

struct Mesh {
  std::vector<double> ex;
  tpsrhs_mesh m = {};
  void finish(int dim) {
    m.dim = dim;
    m.num_elements = static_cast<int>(ex.size() / static_cast<size_t>((1 << dim) * dim));
    m.elem_coords = ex.data();
  }
};

void run(const tpsrhs_mesh &m, double volume) {
  for (int order = 1; order <= TPSRHS_MAXORDER; order++) {
    const int nq = order + 2;
    const int64_t expect = static_cast<int64_t>(m.num_elements) * (m.dim == 3 ? nq * nq * nq : nq * nq);
    int64_t n = -1;
    check(tpsrhs::quadrature_points(&m, order, nullptr, nullptr, &n) == TPSRHS_OK && n == expect, "count without outputs");
    std::vector<double> xyz(static_cast<size_t>(expect) * m.dim), w(static_cast<size_t>(expect));
    n = -1;
    check(tpsrhs::quadrature_points(&m, order, xyz.data(), w.data(), &n) == TPSRHS_OK && n == expect, "both outputs");
    std::vector<double> xyz2(xyz.size()), w2(w.size());
    check(tpsrhs::quadrature_points(&m, order, xyz2.data(), nullptr, &n) == TPSRHS_OK, "points only");
    check(tpsrhs::quadrature_points(&m, order, nullptr, w2.data(), &n) == TPSRHS_OK, "weights only");
    double sum = 0.0;
    for (size_t i = 0; i < w.size(); i++) {
      check(w[i] > 0.0 && w[i] == w2[i], "a positive weight, the same with and without the points");
      sum += w[i];
    }
    for (size_t i = 0; i < xyz.size(); i++) check(std::isfinite(xyz[i]) && xyz[i] == xyz2[i], "a finite point, the same both ways");
    check(std::fabs(sum - volume) <= 1e-12 * volume, "the weights add up to the volume");
  }
}
}  // namespace

int main() {
  {  // 3 x 2 x 2 hexahedra on the unit cube, the interior vertices moved: trilinear elements, volume 1
    const int n[3] = {3, 2, 2};
    auto coord = [&](int I, int J, int K, int d) {
      const int idx[3] = {I, J, K};
      double x = static_cast<double>(idx[d]) / n[d];
      const bool interior = I > 0 && I < n[0] && J > 0 && J < n[1] && K > 0 && K < n[2];
      if (interior) x += 0.15 / n[d] * std::sin(1.0 + I + 2.0 * J + 3.0 * K + d);
      return x;
    };
    Mesh M;
    for (int k = 0; k < n[2]; k++)
      for (int j = 0; j < n[1]; j++)
        for (int i = 0; i < n[0]; i++)
          for (int v = 0; v < 8; v++)
            for (int d = 0; d < 3; d++) M.ex.push_back(coord(i + kHex[v][0], j + kHex[v][1], k + kHex[v][2], d));
    M.finish(3);
    run(M.m, 1.0);
  }
  {  // a ring of 2 x 8 quadrilaterals between the radii 0.5 and 2: the area of the two octagons' difference
    const int nr = 2, nt = 8;
    const double pi = std::acos(-1.0), r[3] = {0.5, 1.1, 2.0};
    Mesh M;
    for (int j = 0; j < nt; j++)
      for (int i = 0; i < nr; i++)
        for (int v = 0; v < 4; v++) {
          const double th = 2.0 * pi * (j + kQuad[v][1]) / nt, rad = r[i + kQuad[v][0]];
          M.ex.push_back(rad * std::cos(th));
          M.ex.push_back(rad * std::sin(th));
        }
    M.finish(2);
    run(M.m, 0.5 * nt * std::sin(2.0 * pi / nt) * (r[2] * r[2] - r[0] * r[0]));
    // an empty mesh: zero points, nothing read or written
    tpsrhs_mesh empty = {};
    empty.dim = 2;
    int64_t n = -1;
    double dummy = 0.0;
    check(tpsrhs::quadrature_points(&empty, 3, &dummy, &dummy, &n) == TPSRHS_OK && n == 0 && dummy == 0.0, "an empty mesh");
    // the refusals
    const int bad = TPSRHS_ERR_INVALID_ARGUMENT;
    check(tpsrhs::quadrature_points(nullptr, 2, nullptr, nullptr, &n) == bad, "NULL mesh");
    check(tpsrhs::quadrature_points(&M.m, 2, nullptr, nullptr, nullptr) == bad, "NULL count");
    check(tpsrhs::quadrature_points(&M.m, 0, nullptr, nullptr, &n) == bad, "order 0");
    check(tpsrhs::quadrature_points(&M.m, TPSRHS_MAXORDER + 1, nullptr, nullptr, &n) == bad, "order 6");
    tpsrhs_mesh wrong = M.m;
    wrong.dim = 1;
    check(tpsrhs::quadrature_points(&wrong, 2, nullptr, nullptr, &n) == bad, "dim 1");
    wrong.dim = 4;
    check(tpsrhs::quadrature_points(&wrong, 2, nullptr, nullptr, &n) == bad, "dim 4");
    wrong = M.m;
    wrong.elem_coords = nullptr;
    check(tpsrhs::quadrature_points(&wrong, 2, nullptr, nullptr, &n) == bad, "elements without coordinates");
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("QUADRATURE POINTS CLEAN\n");
  return 0;
}
