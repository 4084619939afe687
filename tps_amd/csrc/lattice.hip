// The element lattice of libtpsrhs.so (lattice.hpp): tpsrhs_lattice_size, tpsrhs_lattice_coordinates and
// tpsrhs_lattice_fields -- what a ParaView output step evaluates.  Stateless: everything a call needs (the 1-D matrix B, the
// abscissae) is formed on the host from the operator's order and basis and goes to the kernels by value.
#include "abi_support.hpp"
#include "lattice.hpp"

#include <string>

namespace {

bool levels_ok(int levels) { return levels >= 1 && levels <= TPSRHS_MAXLATTICE; }

std::string levels_message(const char *who, int levels) {
  return std::string(who) + ": levels " + std::to_string(levels) + " is outside 1.." + std::to_string(TPSRHS_MAXLATTICE);
}

int64_t lattice_points_per_element(const tpsrhs_operator *h, int levels) {
  const int64_t n = levels + 1;
  return h->dim == 3 ? n * n * n : n * n;
}

// B[a][i] = l_i(a / L) on the operator's own nodes, the product of quotients of basis.hpp::lagrange
LatticeBasis lattice_basis(const tpsrhs_operator *h, int levels) {
  LatticeBasis lb = {};
  double x[TPSRHS_MAXORDER + 1], wts[TPSRHS_MAXORDER + 1];
  const int n1 = h->order + 1;
  segment_rule01(h->nc, n1, x, wts);  // the nodes of the operator's basis, as sample_field takes them
  lb.n = levels + 1;
  lb.rn = 1.0f / static_cast<float>(lb.n);
  for (int a = 0; a <= levels; a++) {
    const double t = static_cast<double>(a) / static_cast<double>(levels);
    for (int i = 0; i < n1; i++) lb.b[a * n1 + i] = lagrange(x, n1, i, t);
  }
  return lb;
}

template <int DIM, int P>
void launch_lattice(tpsrhs_operator *h, const LatticeBasis &lb, int nrows, const double *field, void *out, bool f32) {
  constexpr int N1 = P + 1;
  constexpr int EPB = lattice_elems_per_block(DIM == 3 ? N1 * N1 * N1 : N1 * N1);
  const int64_t grid = (static_cast<int64_t>(h->ne) + EPB - 1) / EPB;
  if (grid == 0) return;
  const int64_t npts = static_cast<int64_t>(h->ne) * lattice_points_per_element(h, lb.n - 1);
  const size_t lds = sizeof(double) * lattice_lds_doubles(DIM, P, lb.n);
  if (f32)
    hipLaunchKernelGGL((k_lattice<DIM, P, true>), dim3(static_cast<unsigned>(grid)), dim3(LATTICE_BLOCK), lds, h->stream, h->ne,
                       nrows, h->ndofs, npts, lb, field, out);
  else
    hipLaunchKernelGGL((k_lattice<DIM, P, false>), dim3(static_cast<unsigned>(grid)), dim3(LATTICE_BLOCK), lds, h->stream, h->ne,
                       nrows, h->ndofs, npts, lb, field, out);
  HIP_CHECK(hipGetLastError());
}

void lattice_coordinates(tpsrhs_operator *h, int levels, double *xyz_out) {
  LatticeAbscissae ab = {};
  ab.n = levels + 1;
  for (int a = 0; a <= levels; a++) ab.t[a] = static_cast<double>(a) / static_cast<double>(levels);
  constexpr int BLOCK = 256;
  const int64_t npts = static_cast<int64_t>(h->ne) * lattice_points_per_element(h, levels);
  const int64_t grid = (npts + BLOCK - 1) / BLOCK;
  if (grid == 0) return;
  if (grid >= (int64_t(1) << 31)) throw Unsupported("tpsrhs_lattice_coordinates: more than 2^39 lattice points");
  if (h->dim == 2)
    hipLaunchKernelGGL((k_lattice_coordinates<2, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, npts, ab,
                       h->d_verts.get(), xyz_out);
  else if (h->dim == 3)
    hipLaunchKernelGGL((k_lattice_coordinates<3, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), 0, h->stream, npts, ab,
                       h->d_verts.get(), xyz_out);
  else
    throw Unsupported("tpsrhs_lattice_coordinates: dim 2 or 3");
  HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int tpsrhs_lattice_size(tpsrhs_handle h, int levels, int64_t *points_per_element, int64_t *npts) {
  if (!h || !points_per_element || !npts) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_lattice_size: NULL argument");
  if (!levels_ok(levels)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, levels_message("tpsrhs_lattice_size", levels));
  *points_per_element = lattice_points_per_element(h, levels);
  *npts = static_cast<int64_t>(h->ne) * *points_per_element;
  return TPSRHS_OK;
}

int tpsrhs_lattice_coordinates(tpsrhs_handle h, int levels, double *xyz_out) {
  if (!h || !xyz_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_lattice_coordinates: NULL argument");
  if (!levels_ok(levels)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, levels_message("tpsrhs_lattice_coordinates", levels));
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    lattice_coordinates(h, levels, xyz_out);
  });
}

int tpsrhs_lattice_fields(tpsrhs_handle h, int levels, int nrows, const double *field, void *out, int out_float32) {
  if (!h || !field || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_lattice_fields: NULL argument");
  if (!levels_ok(levels)) return fail(TPSRHS_ERR_INVALID_ARGUMENT, levels_message("tpsrhs_lattice_fields", levels));
  if (nrows < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_lattice_fields: nrows " + std::to_string(nrows) + " < 1");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const LatticeBasis lb = lattice_basis(h, levels);
    with_dim_order(h, "tpsrhs_lattice_fields", [&](auto dim, auto p) {
      launch_lattice<decltype(dim)::value, decltype(p)::value>(h, lb, nrows, field, out, out_float32 != 0);
    });
  });
}

}  // extern "C"
