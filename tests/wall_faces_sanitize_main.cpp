// Stand-alone driver of tps_amd/csrc/wall_faces.hpp for the host sanitizers (tests/test_wall_faces_sanitize.py builds it
// with -fsanitize=address,undefined and runs it as a child process): a box of hexahedra with walls all round and a ring of
// quadrilaterals that is periodic in the angle, both selection rules, every capacity from 0 to beyond the count, the refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tps_amd/csrc/wall_faces.hpp"

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
  std::vector<int> ev, bv, ba;
  std::vector<double> ex;
  tpsrhs_mesh m = {};
  void finish(int dim, int nverts) {
    m.dim = dim;
    m.num_vertices = nverts;
    m.num_elements = static_cast<int>(ev.size()) >> dim;
    m.elem_vertices = ev.data();
    m.elem_coords = ex.data();
    m.num_bdr_faces = static_cast<int>(ba.size());
    m.bdr_vertices = bv.data();
    m.bdr_attributes = ba.data();
  }
};

// every capacity from 0 to count + 2 writes min(count, capacity) faces and nothing behind them
void sweep_capacity(const tpsrhs_mesh &m, int nbc, const tpsrhs_bc *bcs, int natt, const int *att, int64_t expect) {
  const int per = (1 << (m.dim - 1)) * m.dim;
  int64_t n = -1;
  check(tpsrhs::wall_faces(&m, nbc, bcs, natt, att, 0, nullptr, &n) == TPSRHS_OK && n == expect, "count with capacity 0");
  std::vector<double> full(static_cast<size_t>(expect) * per + 1, 0.0);
  check(tpsrhs::wall_faces(&m, nbc, bcs, natt, att, expect, full.data(), &n) == TPSRHS_OK && n == expect, "full list");
  for (int64_t cap = 0; cap <= expect + 2; cap++) {
    std::vector<double> out(static_cast<size_t>(cap) * per);  // exactly the capacity: a write behind it is an overflow
    n = -1;
    check(tpsrhs::wall_faces(&m, nbc, bcs, natt, att, cap, cap ? out.data() : nullptr, &n) == TPSRHS_OK && n == expect, "capacity sweep");
    const int64_t w = cap < expect ? cap : expect;
    for (int64_t i = 0; i < w * per; i++) check(out[static_cast<size_t>(i)] == full[static_cast<size_t>(i)], "a prefix of the full list");
  }
}
}  // namespace

int main() {
  {  // 3 x 2 x 2 hexahedra on the unit cube, attribute 1 + 2 d + s on the side x_d = s
    const int n[3] = {3, 2, 2};
    auto vid = [&](int i, int j, int k) { return i + (n[0] + 1) * (j + (n[1] + 1) * k); };
    Mesh M;
    for (int k = 0; k < n[2]; k++)
      for (int j = 0; j < n[1]; j++)
        for (int i = 0; i < n[0]; i++)
          for (int v = 0; v < 8; v++) {
            const int I = i + kHex[v][0], J = j + kHex[v][1], K = k + kHex[v][2];
            M.ev.push_back(vid(I, J, K));
            M.ex.push_back(static_cast<double>(I) / n[0]);
            M.ex.push_back(static_cast<double>(J) / n[1]);
            M.ex.push_back(static_cast<double>(K) / n[2]);
          }
    for (int d = 0; d < 3; d++)
      for (int s = 0; s < 2; s++) {
        const int a = (d == 0) ? 1 : 0, b = (d == 2) ? 1 : 2;
        for (int q = 0; q < n[b]; q++)
          for (int p = 0; p < n[a]; p++) {
            // NOT a cyclic order: (0,0) (1,0) (0,1) (1,1), as tpsrhs_mesh allows
            for (int c = 0; c < 4; c++) {
              int ijk[3];
              ijk[d] = s * n[d];
              ijk[a] = p + (c & 1);
              ijk[b] = q + (c >> 1);
              M.bv.push_back(vid(ijk[0], ijk[1], ijk[2]));
            }
            M.ba.push_back(1 + 2 * d + s);
          }
      }
    M.finish(3, (n[0] + 1) * (n[1] + 1) * (n[2] + 1));
    const int bottom[1] = {5}, two[2] = {1, 6};
    sweep_capacity(M.m, 0, nullptr, 1, bottom, 6);
    sweep_capacity(M.m, 0, nullptr, 2, two, 4 + 6);
    sweep_capacity(M.m, 0, nullptr, 0, nullptr, 0);
    int64_t cnt = 0;
    std::vector<double> out(6 * 12);
    check(tpsrhs::wall_faces(&M.m, 0, nullptr, 1, bottom, 6, out.data(), &cnt) == TPSRHS_OK, "bottom");
    for (int f = 0; f < 6; f++)
      for (int c = 0; c < 4; c++) {
        check(out[(f * 4 + c) * 3 + 2] == 0.0, "a bottom face lies in z = 0");
        // ascending elements (i fastest), corner = ta + 2 tb with ta along x and tb along y
        check(out[(f * 4 + c) * 3 + 0] == static_cast<double>(f % 3 + (c & 1)) / 3, "x of a bottom corner");
        check(out[(f * 4 + c) * 3 + 1] == static_cast<double>(f / 3 + (c >> 1)) / 2, "y of a bottom corner");
      }
    tpsrhs_bc bcs[6] = {};
    for (int k = 0; k < 6; k++) {
      bcs[k].attribute = k + 1;
      bcs[k].category = TPSRHS_WALL;
      bcs[k].type = k;  // INV SLIP VISC_ADIAB VISC_ISOTH VISC_GNRL and one value beyond
    }
    bcs[5].category = TPSRHS_OUTLET;
    sweep_capacity(M.m, 6, bcs, -1, nullptr, 4 + 6 + 6 + 6);  // sides 2, 3, 4, 5: every wall but the inviscid one
    // refusals
    check(tpsrhs::wall_faces(nullptr, 0, nullptr, 1, bottom, 0, nullptr, &cnt) == TPSRHS_ERR_INVALID_ARGUMENT, "NULL mesh");
    check(tpsrhs::wall_faces(&M.m, 0, nullptr, 1, bottom, 0, nullptr, nullptr) == TPSRHS_ERR_INVALID_ARGUMENT, "NULL count");
    check(tpsrhs::wall_faces(&M.m, 0, nullptr, 1, bottom, 3, nullptr, &cnt) == TPSRHS_ERR_INVALID_ARGUMENT, "capacity, no array");
    check(tpsrhs::wall_faces(&M.m, 3, nullptr, -1, nullptr, 0, nullptr, &cnt) == TPSRHS_ERR_INVALID_ARGUMENT, "default rule, no bcs");
    tpsrhs_mesh bad = M.m;
    bad.dim = 4;
    check(tpsrhs::wall_faces(&bad, 0, nullptr, 1, bottom, 0, nullptr, &cnt) == TPSRHS_ERR_INVALID_ARGUMENT, "dim 4");
    std::vector<int> bv = M.bv;
    bv[0] = vid(1, 1, 1);  // an interior vertex: the record is no element's face
    bad = M.m;
    bad.bdr_vertices = bv.data();
    check(tpsrhs::wall_faces(&bad, 0, nullptr, 1, bottom, 0, nullptr, &cnt) == TPSRHS_ERR_INVALID_ARGUMENT, "a record that is no face");
  }
  {  // a ring of 3 x 8 quadrilaterals, radii 0.5 .. 2, periodic in the angle: inner circle 3, outer circle 1
    const int nr = 3, nt = 8;
    Mesh M;
    for (int t = 0; t < nt; t++)
      for (int r = 0; r < nr; r++)
        for (int v = 0; v < 4; v++) {
          const int R = r + kQuad[v][0], T = t + kQuad[v][1];
          M.ev.push_back(R + (nr + 1) * (T % nt));
          const double rad = 0.5 + 1.5 * R / nr, th = 2.0 * M_PI * T / nt;
          M.ex.push_back(rad * std::cos(th));
          M.ex.push_back(rad * std::sin(th));
        }
    for (int t = 0; t < nt; t++) {
      M.bv.push_back(0 + (nr + 1) * ((t + 1) % nt));  // the two vertices in either order
      M.bv.push_back(0 + (nr + 1) * t);
      M.ba.push_back(3);
      M.bv.push_back(nr + (nr + 1) * t);
      M.bv.push_back(nr + (nr + 1) * ((t + 1) % nt));
      M.ba.push_back(1);
    }
    M.finish(2, (nr + 1) * nt);
    const int inner[1] = {3}, both[2] = {3, 1};
    sweep_capacity(M.m, 0, nullptr, 1, inner, nt);
    sweep_capacity(M.m, 0, nullptr, 2, both, 2 * nt);
    int64_t cnt = 0;
    std::vector<double> out(nt * 4);
    check(tpsrhs::wall_faces(&M.m, 0, nullptr, 1, inner, nt, out.data(), &cnt) == TPSRHS_OK && cnt == nt, "inner circle");
    for (int i = 0; i < nt * 2; i++) check(std::fabs(std::hypot(out[2 * i], out[2 * i + 1]) - 0.5) <= 1e-15, "radius of an inner corner");
    // the last cell keeps its own geometry across the periodic seam: its second corner is at angle 2 pi, not 0
    check(std::fabs(out[(nt - 1) * 4 + 2] - 0.5 * std::cos(2.0 * M_PI)) <= 1e-15 && std::fabs(out[(nt - 1) * 4 + 3] - 0.5 * std::sin(2.0 * M_PI)) <= 1e-15,
          "the seam");
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("WALL FACES CLEAN\n");
  return 0;
}
