// Stand-alone driver of tps_amd/csrc/point_locate.hpp for the host sanitizers (tests/test_locate_sanitize.py builds it with
// -fsanitize=address,undefined and runs it as a child process): the round trip map(elem, xi) -> locate -> (elem, xi) on a
// warped hexahedral box and on a quadrilateral ring with a hole, points outside both, and the plane lattice.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tps_amd/csrc/point_locate.hpp"

namespace {
unsigned long long g_state = 88172645463325252ULL;
double uniform() {  // xorshift64: a number in (0, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (static_cast<double>(g_state >> 11) + 0.5) / 9007199254740992.0;
}

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

template <int DIM>
void mfem_map(const double *ex, const double *xi, double *x) {
  for (int a = 0; a < DIM; a++) x[a] = 0.0;
  for (int v = 0; v < (1 << DIM); v++) {
    double w = 1.0;
    for (int d = 0; d < DIM; d++) {
      const int c = DIM == 2 ? kQuad[v][d] : kHex[v][d];
      w *= c ? xi[d] : 1.0 - xi[d];
    }
    for (int a = 0; a < DIM; a++) x[a] += ex[v * DIM + a] * w;
  }
}

template <int DIM>
void round_trip(const std::vector<double> &coords, int ne, int npts, const std::vector<double> &outside) {
  tpsrhs_mesh mesh = {};
  mesh.dim = DIM;
  mesh.num_elements = ne;
  mesh.elem_coords = coords.data();
  const int nout = static_cast<int>(outside.size()) / DIM, total = npts + nout;
  std::vector<double> xyz(static_cast<size_t>(total) * DIM), xi(static_cast<size_t>(npts) * DIM);
  std::vector<int> elem(npts);
  for (int i = 0; i < npts; i++) {
    elem[i] = static_cast<int>(uniform() * ne) % ne;
    double x[DIM], r[DIM];
    for (int d = 0; d < DIM; d++) r[d] = xi[i * DIM + d] = 0.02 + 0.96 * uniform();
    mfem_map<DIM>(&coords[static_cast<size_t>(elem[i]) * (1 << DIM) * DIM], r, x);
    for (int d = 0; d < DIM; d++) xyz[i + static_cast<size_t>(d) * total] = x[d];
  }
  for (int i = 0; i < nout; i++)
    for (int d = 0; d < DIM; d++) xyz[npts + i + static_cast<size_t>(d) * total] = outside[i * DIM + d];
  std::vector<int32_t> got(total);
  std::vector<double> ref(static_cast<size_t>(total) * DIM);
  check(tpsrhs::locate_points(&mesh, total, xyz.data(), 0.0, got.data(), ref.data()) == TPSRHS_OK, "status");
  for (int i = 0; i < npts; i++) {
    check(got[i] == elem[i], "element of a point made inside it");
    for (int d = 0; d < DIM; d++) check(std::fabs(ref[i + static_cast<size_t>(d) * total] - xi[i * DIM + d]) <= 1e-12, "reference coordinate");
  }
  for (int i = npts; i < total; i++) {
    check(got[i] == -1, "a point outside the mesh is not found");
    for (int d = 0; d < DIM; d++) check(ref[i + static_cast<size_t>(d) * total] == 0.0, "reference coordinates of a point that was not found");
  }
}
}  // namespace

int main() {
  {  // 3 x 2 x 2 hexahedra on [0,1.5] x [0,1] x [0,0.7], interior vertices displaced
    const int n[3] = {3, 2, 2};
    const double L[3] = {1.5, 1.0, 0.7};
    auto vertex = [&](int i, int j, int k, double *x) {
      const int ijk[3] = {i, j, k};
      for (int d = 0; d < 3; d++) x[d] = L[d] * ijk[d] / n[d];
      const bool inner = i > 0 && i < n[0] && j > 0 && j < n[1] && k > 0 && k < n[2];
      if (inner) {
        x[0] += 0.05 * ((i + 2 * j + k) % 3 - 1);
        x[1] += 0.04 * ((2 * i + j + k) % 3 - 1);
        x[2] -= 0.03 * ((i + j + 2 * k) % 3 - 1);
      }
    };
    std::vector<double> coords;
    for (int k = 0; k < n[2]; k++)
      for (int j = 0; j < n[1]; j++)
        for (int i = 0; i < n[0]; i++)
          for (int v = 0; v < 8; v++) {
            double x[3];
            vertex(i + kHex[v][0], j + kHex[v][1], k + kHex[v][2], x);
            coords.insert(coords.end(), x, x + 3);
          }
    round_trip<3>(coords, 12, 400, {-0.1, 0.5, 0.3, 0.7, 1.2, 0.3, 0.7, 0.5, 0.71, 5.0, 5.0, 5.0});
  }
  {  // a ring of 4 x 12 quadrilaterals, radii 0.5 .. 2: the disc inside is a hole
    const int nr = 4, nt = 12;
    std::vector<double> coords;
    for (int t = 0; t < nt; t++)
      for (int r = 0; r < nr; r++)
        for (int v = 0; v < 4; v++) {
          const double rad = 0.5 + 1.5 * (r + kQuad[v][0]) / nr, th = 2.0 * M_PI * (t + kQuad[v][1]) / nt;
          coords.push_back(rad * std::cos(th));
          coords.push_back(rad * std::sin(th));
        }
    round_trip<2>(coords, nr * nt, 400, {0.0, 0.0, 0.1, -0.2, 3.0, 0.0, 1.9, 1.9, -2.5, -2.5});
  }
  {  // the plane lattice, one normal per major direction, and the refused arguments
    const double p[3] = {0.1, 0.2, 0.3}, b0[3] = {0, 0, 0}, b1[3] = {1, 2, 3};
    const double normals[3][3] = {{1.0, 0.2, 0.1}, {0.1, -1.0, 0.3}, {0.0, 0.0, 2.0}};
    for (const auto &nrm : normals) {
      std::vector<double> out(3 * 25);
      check(tpsrhs::plane_points(p, nrm, b0, b1, 5, out.data()) == TPSRHS_OK, "plane status");
      for (int i = 0; i < 25; i++) {
        double r = 0.0;
        for (int d = 0; d < 3; d++) r += nrm[d] * (out[i + d * 25] - p[d]);
        check(std::fabs(r) <= 1e-13, "a lattice point lies on the plane");
      }
    }
    double one[3];
    check(tpsrhs::plane_points(p, normals[0], b0, b1, 1, one) == TPSRHS_ERR_INVALID_ARGUMENT, "n < 2 is refused");
    check(tpsrhs::locate_points(nullptr, 1, one, 0.0, nullptr, nullptr) == TPSRHS_ERR_INVALID_ARGUMENT, "NULL mesh is refused");
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("LOCATE CLEAN\n");
  return 0;
}
