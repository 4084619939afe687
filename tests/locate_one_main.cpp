// Stand-alone driver of tps_amd/csrc/point_locate.hpp (tests/test_locate_one.py builds it with plain g++, once without and once
// with -fsanitize=address,undefined, and runs it as a child process): the search structure built once (build_locate_grid) and
// the per-point function locate_one, the text the device kernel k_locate runs, point by point against locate_points --
// element and reference coordinates bit-equal.  Input, a file of native-endian binary: int32 dim, ne, npts; double
// elem_coords[ne][2^dim][dim] (MFEM vertex order); double xyz[dim][npts].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tps_amd/csrc/point_locate.hpp"

namespace {
template <int DIM>
int64_t compare(int ne, const std::vector<double> &coords, int64_t npts, const std::vector<double> &xyz, double tol_in) {
  tpsrhs_mesh mesh = {};
  mesh.dim = DIM;
  mesh.num_elements = ne;
  mesh.elem_coords = coords.data();
  std::vector<int32_t> elem(static_cast<size_t>(npts));
  std::vector<double> ref(static_cast<size_t>(npts) * DIM);
  if (tpsrhs::locate_points(&mesh, npts, xyz.data(), tol_in, elem.data(), ref.data()) != TPSRHS_OK) return -1;
  const double tol = tol_in > 0.0 ? tol_in : tpsrhs::LOCATE_DEFAULT_TOL;
  constexpr int NV = 1 << DIM;
  std::vector<double> verts(static_cast<size_t>(ne) * NV * DIM);
  for (int e = 0; e < ne; e++)
    for (int v = 0; v < NV; v++)
      for (int d = 0; d < DIM; d++)
        verts[(static_cast<size_t>(e) * NV + tpsrhs::mfem_to_lex_corner(v)) * DIM + d] = coords[(static_cast<size_t>(e) * NV + v) * DIM + d];
  const tpsrhs::LocateGrid grid = tpsrhs::build_locate_grid<DIM>(ne, verts.data(), tol);
  const tpsrhs::LocateGridView<DIM> view = tpsrhs::locate_grid_view<DIM>(grid);
  int64_t bad = 0, found = 0;
  for (int64_t i = 0; i < npts; i++) {
    double p[DIM], xi[DIM];
    for (int d = 0; d < DIM; d++) p[d] = xyz[static_cast<size_t>(i + d * npts)];
    const int32_t e = tpsrhs::locate_one<DIM>(view, verts.data(), p, tol, xi);
    bool same = e == elem[static_cast<size_t>(i)];
    for (int d = 0; d < DIM; d++) same = same && std::memcmp(&xi[d], &ref[static_cast<size_t>(i + d * npts)], sizeof(double)) == 0;
    if (e < 0)
      for (int d = 0; d < DIM; d++) same = same && xi[d] == 0.0;
    if (!same) {
      if (bad < 10) std::printf("point %lld: locate_one %d, locate_points %d\n", static_cast<long long>(i), e, elem[static_cast<size_t>(i)]);
      bad++;
    }
    found += e >= 0;
  }
  std::printf("points %lld found %lld\n", static_cast<long long>(npts), static_cast<long long>(found));
  return bad;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[3] = {0, 0, 0};
  if (std::fread(head, sizeof(int32_t), 3, f) != 3 || (head[0] != 2 && head[0] != 3) || head[1] < 1 || head[2] < 0) return 2;
  const int dim = head[0], ne = head[1];
  const int64_t npts = head[2];
  std::vector<double> coords(static_cast<size_t>(ne) * (1 << dim) * dim), xyz(static_cast<size_t>(npts) * dim);
  const bool ok = std::fread(coords.data(), sizeof(double), coords.size(), f) == coords.size() &&
                  std::fread(xyz.data(), sizeof(double), xyz.size(), f) == xyz.size();
  std::fclose(f);
  if (!ok) return 2;
  const double tol = argc > 2 ? std::atof(argv[2]) : 0.0;
  const int64_t bad = dim == 2 ? compare<2>(ne, coords, npts, xyz, tol) : compare<3>(ne, coords, npts, xyz, tol);
  if (bad != 0) {
    std::printf("%lld points differ\n", static_cast<long long>(bad));
    return 1;
  }
  std::printf("LOCATE_ONE EQUAL\n");
  return 0;
}
