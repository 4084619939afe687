// Stand-alone driver of tpsrhs::patch_faces (tps_amd/csrc/wall_faces.hpp) for the host sanitizers
// (tests/test_patch_faces.py builds it with -fsanitize=address,undefined and runs it as a child process).  It reads meshes
// from the text file named on the command line -- per mesh: dim, num_vertices, num_elements, num_bdr_faces, num_attributes,
// then the attributes, elem_vertices, elem_coords, bdr_vertices and bdr_attributes -- runs every capacity from 0 to beyond
// the count into arrays of exactly that size, the refusals, and prints the face list of every mesh:
//   mesh <index> <count>
//   <element> <local face> <patch>      (count lines)
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  int dim, nv, ne, nb, natt;
  for (int index = 0; in >> dim >> nv >> ne >> nb >> natt; index++) {
    if (dim != 2 && dim != 3) return 2;
    const int nvpe = 1 << dim, nfv = 1 << (dim - 1);
    std::vector<int> att(static_cast<size_t>(natt)), ev(static_cast<size_t>(ne) * nvpe), bv(static_cast<size_t>(nb) * nfv),
        ba(static_cast<size_t>(nb));
    std::vector<double> ex(static_cast<size_t>(ne) * nvpe * dim);
    for (auto &a : att) in >> a;
    for (auto &v : ev) in >> v;
    for (auto &x : ex) in >> x;
    for (auto &v : bv) in >> v;
    for (auto &a : ba) in >> a;
    if (!in) return 2;
    tpsrhs_mesh m = {};
    m.dim = dim;
    m.num_vertices = nv;
    m.num_elements = ne;
    m.elem_vertices = ev.data();
    m.elem_coords = ex.data();
    m.num_bdr_faces = nb;
    m.bdr_vertices = bv.data();
    m.bdr_attributes = ba.data();

    int64_t count = -1;
    check(tpsrhs::patch_faces(&m, natt, att.data(), 0, nullptr, nullptr, nullptr, &count) == TPSRHS_OK && count >= 0, "count with capacity 0");
    std::vector<int32_t> fe(static_cast<size_t>(count)), ff(fe.size()), fp(fe.size());
    int64_t n = -1;
    check(tpsrhs::patch_faces(&m, natt, att.data(), count, fe.data(), ff.data(), fp.data(), &n) == TPSRHS_OK && n == count, "full list");
    // every capacity from 0 to count + 2 writes min(count, capacity) faces and nothing behind them
    for (int64_t cap = 0; cap <= count + 2; cap++) {
      std::vector<int32_t> e(static_cast<size_t>(cap)), f(e.size()), p(e.size());  // exactly the capacity
      n = -1;
      check(tpsrhs::patch_faces(&m, natt, att.data(), cap, cap ? e.data() : nullptr, cap ? f.data() : nullptr, cap ? p.data() : nullptr, &n) == TPSRHS_OK && n == count,
            "capacity sweep");
      const int64_t w = cap < count ? cap : count;
      for (int64_t i = 0; i < w; i++) {
        const size_t k = static_cast<size_t>(i);
        check(e[k] == fe[k] && f[k] == ff[k] && p[k] == fp[k], "a prefix of the full list");
      }
    }
    for (int64_t i = 1; i < count; i++) {
      const size_t k = static_cast<size_t>(i);
      check(fe[k - 1] < fe[k] || (fe[k - 1] == fe[k] && ff[k - 1] < ff[k]), "ascending (element, local face)");
    }
    // the refusals
    const int I = TPSRHS_ERR_INVALID_ARGUMENT;
    check(tpsrhs::patch_faces(nullptr, natt, att.data(), 0, nullptr, nullptr, nullptr, &n) == I, "NULL mesh");
    check(tpsrhs::patch_faces(&m, natt, att.data(), 0, nullptr, nullptr, nullptr, nullptr) == I, "NULL count");
    check(tpsrhs::patch_faces(&m, 0, att.data(), 0, nullptr, nullptr, nullptr, &n) == I, "no attribute");
    check(tpsrhs::patch_faces(&m, natt, att.data(), -1, nullptr, nullptr, nullptr, &n) == I, "negative capacity");
    check(tpsrhs::patch_faces(&m, natt, att.data(), 1, nullptr, nullptr, nullptr, &n) == I, "capacity, no arrays");
    std::vector<int> twice(att);
    twice.push_back(att[0]);
    check(tpsrhs::patch_faces(&m, natt + 1, twice.data(), 0, nullptr, nullptr, nullptr, &n) == I, "an attribute listed twice");
    tpsrhs_mesh bad = m;
    bad.dim = 4;
    check(tpsrhs::patch_faces(&bad, natt, att.data(), 0, nullptr, nullptr, nullptr, &n) == I, "dim 4");
    if (nb > 0) {
      // a record of one vertex repeated is no element's face
      std::vector<int> bv2(bv);
      for (int i = 1; i < nfv; i++) bv2[static_cast<size_t>(i)] = bv2[0];
      bad = m;
      bad.bdr_vertices = bv2.data();
      check(tpsrhs::patch_faces(&bad, natt, att.data(), 0, nullptr, nullptr, nullptr, &n) == I, "a record that is no face");
    }
    std::printf("mesh %d %lld\n", index, static_cast<long long>(count));
    for (size_t k = 0; k < fe.size(); k++) std::printf("%d %d %d\n", fe[k], ff[k], fp[k]);
  }
  if (g_failures) {
    std::printf("%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("PATCH FACES CLEAN\n");
  return 0;
}
