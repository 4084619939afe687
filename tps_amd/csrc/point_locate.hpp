// Point location on the order-1 geometry of a tpsrhs_mesh, and the point set of a sampling plane: the host half of what the
// reference delegates to gslib's FindPointsGSLIB (src/gslib_interpolator.cpp:53-84: Setup on the mesh, FindPoints and Interpolate at xyz)
// and PlaneInterpolator::setInterpolationPoints (:121-190).  Plain C++: no HIP, no device, nothing but tpsrhs.h -- a
// stand-alone program can include this file alone (tests/test_locate_sanitize.py does, under the sanitizers).
//
// Geometry: element e maps the reference cube [0,1]^dim to physical space with the bi-/trilinear vertex map
//   x(xi) = sum_c verts[e][c] prod_d (c_d ? xi_d : 1 - xi_d),    c = c_0 + 2 c_1 + 4 c_2  (lexicographic corners)
// which is how the kernels read Topology::verts; MFEM's vertex order (tpsrhs_mesh::elem_coords) is converted on entry.
//
// Search: a uniform grid of bins over the bounding box of the mesh; every element is listed, in ascending order, in the
// bins its own (inflated) bounding box overlaps.  A point looks at the elements of its one bin, lowest index first, skips
// those whose box does not hold it, inverts the map of the others by Newton from the element centre, and takes the FIRST
// whose reference coordinates all lie in [-tol, 1 + tol]: on a face between two elements, where a DG field has two
// values, the element with the lower index answers.  That choice is part of the contract (include/tpsrhs.h).
//
// Two parts: build_locate_grid makes the search structure (host only), locate_one is the rule for ONE point, and it, with
// what it calls, is marked TPSRHS_HD -- __host__ __device__ when hipcc compiles sampling.hip, nothing for a plain C++ compiler --
// so that the device locator (locate_device.hpp: k_locate) runs this very text.
#ifndef TPSRHS_POINT_LOCATE_HPP_
#define TPSRHS_POINT_LOCATE_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tpsrhs.h"
#include "division_mode.hpp"

// IEEE divisions (TPSRHS_IEEE_DIVISION) in the functions of this header that divide: the plane lattice is the reference's
// bit for bit, and the Newton corrections are what a restatement computes.

// The per-point half (locate_one and what it calls) runs on the host and, in sampling.hip, on the device (locate_device.hpp)
#if defined(__HIPCC__)
#define TPSRHS_HD __host__ __device__
#else
#define TPSRHS_HD
#endif

namespace tpsrhs {

constexpr double LOCATE_DEFAULT_TOL = 1e-10;
constexpr int LOCATE_MAX_NEWTON = 50;

// MFEM corner v of a quadrilateral / hexahedron -> lexicographic corner (bit d = reference coordinate d)
inline int mfem_to_lex_corner(int v) {
  static const int quad[4] = {0, 1, 3, 2};
  return (v & 4) | quad[v & 3];
}

// x(xi) of one element (v: [2^dim][dim], lexicographic corners) and, when J is non-NULL, J[a * dim + d] = dx_a / dxi_d
template <int DIM>
TPSRHS_HD inline void vertex_map(const double *v, const double *xi, double *x, double *J) {
  constexpr int NV = 1 << DIM;
  for (int a = 0; a < DIM; a++) x[a] = 0.0;
  if (J)
    for (int a = 0; a < DIM * DIM; a++) J[a] = 0.0;
  for (int c = 0; c < NV; c++) {
    double f[DIM], w = 1.0;
    for (int d = 0; d < DIM; d++) {
      f[d] = ((c >> d) & 1) ? xi[d] : 1.0 - xi[d];
      w *= f[d];
    }
    for (int a = 0; a < DIM; a++) x[a] += v[c * DIM + a] * w;
    if (!J) continue;
    for (int d = 0; d < DIM; d++) {
      double dw = ((c >> d) & 1) ? 1.0 : -1.0;
      for (int k = 0; k < DIM; k++)
        if (k != d) dw *= f[k];
      for (int a = 0; a < DIM; a++) J[a * DIM + d] += v[c * DIM + a] * dw;
    }
  }
}

// s = J^{-1} r by Cramer's rule; false when J is singular to working precision
template <int DIM>
TPSRHS_HD inline bool solve_small(const double *J, const double *r, double *s) {
  TPSRHS_IEEE_DIVISION
  if (DIM == 2) {
    const double det = J[0] * J[3] - J[1] * J[2];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    s[0] = (r[0] * J[3] - J[1] * r[1]) / det;
    s[1] = (J[0] * r[1] - r[0] * J[2]) / det;
    return true;
  }
  const double c0 = J[4] * J[8] - J[5] * J[7], c1 = J[5] * J[6] - J[3] * J[8], c2 = J[3] * J[7] - J[4] * J[6];
  const double det = J[0] * c0 + J[1] * c1 + J[2] * c2;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  s[0] = (r[0] * c0 + r[1] * (J[2] * J[7] - J[1] * J[8]) + r[2] * (J[1] * J[5] - J[2] * J[4])) / det;
  s[1] = (r[0] * c1 + r[1] * (J[0] * J[8] - J[2] * J[6]) + r[2] * (J[2] * J[3] - J[0] * J[5])) / det;
  s[2] = (r[0] * c2 + r[1] * (J[1] * J[6] - J[0] * J[7]) + r[2] * (J[0] * J[4] - J[1] * J[3])) / det;
  return true;
}

// Newton on x(xi) = p from the element centre.  true: converged (the last correction is below 1e-13, so by quadratic
// convergence the remaining error is rounding); the reference coordinates are NOT clamped.
template <int DIM>
TPSRHS_HD inline bool invert_vertex_map(const double *v, const double *p, double *xi) {
  for (int d = 0; d < DIM; d++) xi[d] = 0.5;
  for (int it = 0; it < LOCATE_MAX_NEWTON; it++) {
    double x[DIM], J[DIM * DIM], r[DIM], s[DIM];
    vertex_map<DIM>(v, xi, x, J);
    for (int d = 0; d < DIM; d++) r[d] = p[d] - x[d];
    if (!solve_small<DIM>(J, r, s)) return false;
    double step = 0.0;
    for (int d = 0; d < DIM; d++) {
      xi[d] += s[d];
      step = std::max(step, std::fabs(s[d]));
    }
    if (!std::isfinite(step) || step > 1e6) return false;  // left the neighbourhood of the element for good
    if (step <= 1e-13) return true;
  }
  return false;
}

// The search structure of one mesh and one tolerance (the element boxes are inflated by it): what FindPointsGSLIB::Setup
// leaves behind.  Built on the host; the device locator (locate_device.hpp) reads an uploaded copy through the same view.
struct LocateGrid {
  int dim = 0, nb = 1;                                            // nb bins in every direction
  double glo[3] = {0.0, 0.0, 0.0}, ghi[3] = {0.0, 0.0, 0.0};      // bounding box of the inflated element boxes
  double inv_h[3] = {0.0, 0.0, 0.0};                              // bins per unit length
  std::vector<double> lo, hi;                                     // [ne][dim] inflated element boxes
  std::vector<int64_t> start;                                     // [nb^dim + 1] CSR offsets into list
  std::vector<int32_t> list;                                      // the elements of every bin, ascending in e
};

// Raw pointers into a LocateGrid, host or device: what locate_one reads.  Passed by value (a kernel argument on the device).
template <int DIM>
struct LocateGridView {
  double glo[DIM], ghi[DIM], inv_h[DIM];
  int nb;
  const double *lo, *hi;
  const int64_t *start;
  const int32_t *list;
};

template <int DIM>
inline LocateGridView<DIM> locate_grid_view(const LocateGrid &g, const double *lo, const double *hi, const int64_t *start,
                                            const int32_t *list) {
  LocateGridView<DIM> v;
  for (int d = 0; d < DIM; d++) {
    v.glo[d] = g.glo[d];
    v.ghi[d] = g.ghi[d];
    v.inv_h[d] = g.inv_h[d];
  }
  v.nb = g.nb;
  v.lo = lo;
  v.hi = hi;
  v.start = start;
  v.list = list;
  return v;
}
template <int DIM>
inline LocateGridView<DIM> locate_grid_view(const LocateGrid &g) {
  return locate_grid_view<DIM>(g, g.lo.data(), g.hi.data(), g.start.data(), g.list.data());
}

// monotone in x: a point inside an element's box falls in a bin the element lists
TPSRHS_HD inline int locate_bin_of(double glo, double inv_h, int nb, double x) {
  const double t = (x - glo) * inv_h;
  if (!(t > 0.0)) return 0;
  return t >= nb ? nb - 1 : static_cast<int>(t);
}

// verts: [ne][2^dim][dim] with lexicographic corners, ne >= 1.
template <int DIM>
inline LocateGrid build_locate_grid(int ne, const double *verts, double tol) {
  constexpr int NV = 1 << DIM;
  LocateGrid g;
  g.dim = DIM;
  // element boxes.  A point with reference coordinates in [-tol, 1 + tol] lies within tol * (sum of the edge extents) of the
  // vertex hull, which is at most DIM * tol * (box size) per direction: the boxes are inflated by that much.
  std::vector<double> &lo = g.lo, &hi = g.hi;
  lo.resize(static_cast<size_t>(ne) * DIM);
  hi.resize(static_cast<size_t>(ne) * DIM);
  double *glo = g.glo, *ghi = g.ghi;
  for (int e = 0; e < ne; e++) {
    const double *v = verts + static_cast<size_t>(e) * NV * DIM;
    for (int d = 0; d < DIM; d++) {
      double a = v[d], b = v[d];
      for (int c = 1; c < NV; c++) {
        a = std::min(a, v[c * DIM + d]);
        b = std::max(b, v[c * DIM + d]);
      }
      const double pad = DIM * tol * (b - a);
      lo[static_cast<size_t>(e) * DIM + d] = a - pad;
      hi[static_cast<size_t>(e) * DIM + d] = b + pad;
      if (e == 0 || a - pad < glo[d]) glo[d] = a - pad;
      if (e == 0 || b + pad > ghi[d]) ghi[d] = b + pad;
    }
  }
  // bins: about one element per bin, the same count in every direction
  int nb = static_cast<int>(std::floor(std::pow(static_cast<double>(ne), 1.0 / DIM) + 0.5));
  nb = std::max(1, std::min(nb, DIM == 2 ? 2048 : 160));
  g.nb = nb;
  double *inv_h = g.inv_h;
  for (int d = 0; d < DIM; d++) inv_h[d] = ghi[d] > glo[d] ? nb / (ghi[d] - glo[d]) : 0.0;
  auto for_bins = [&](int e, auto &&f) {
    int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
    for (int d = 0; d < DIM; d++) {
      b0[d] = locate_bin_of(glo[d], inv_h[d], nb, lo[static_cast<size_t>(e) * DIM + d]);
      b1[d] = locate_bin_of(glo[d], inv_h[d], nb, hi[static_cast<size_t>(e) * DIM + d]);
    }
    for (int k = b0[2]; k <= b1[2]; k++)
      for (int j = b0[1]; j <= b1[1]; j++)
        for (int i = b0[0]; i <= b1[0]; i++) f((static_cast<size_t>(k) * nb + j) * nb + i);
  };
  size_t nbins = 1;
  for (int d = 0; d < DIM; d++) nbins *= nb;
  std::vector<int64_t> &start = g.start;
  start.assign(nbins + 1, 0);
  for (int e = 0; e < ne; e++) for_bins(e, [&](size_t b) { start[b + 1]++; });
  for (size_t b = 0; b < nbins; b++) start[b + 1] += start[b];
  g.list.resize(static_cast<size_t>(start[nbins]));
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int e = 0; e < ne; e++) for_bins(e, [&](size_t b) { g.list[static_cast<size_t>(fill[b]++)] = e; });  // ascending in e
  }
  return g;
}

// One point p[DIM]: the element that holds it (-1: none; xi_out is then 0) and its reference coordinates.  Host and device
// run this text; the device contracts a * b + c into an FMA, so its reference coordinates differ from the host's in the
// last bits, and the accepted element can differ only for a point whose coordinate lies within rounding of -tol or
// 1 + tol -- 1e-10 outside an element, not on a face.
template <int DIM>
TPSRHS_HD inline int32_t locate_one(const LocateGridView<DIM> &g, const double *verts, const double *p, double tol,
                                    double *xi_out) {
  constexpr int NV = 1 << DIM;
  for (int d = 0; d < DIM; d++) xi_out[d] = 0.0;
  bool inside = true;
  for (int d = 0; d < DIM; d++) inside = inside && p[d] >= g.glo[d] && p[d] <= g.ghi[d];  // false for a NaN
  if (!inside) return -1;
  size_t b = 0;
  for (int d = DIM - 1; d >= 0; d--) b = b * g.nb + locate_bin_of(g.glo[d], g.inv_h[d], g.nb, p[d]);
  for (int64_t q = g.start[b]; q < g.start[b + 1]; q++) {
    const int32_t e = g.list[static_cast<size_t>(q)];
    bool in_box = true;
    for (int d = 0; d < DIM; d++)
      in_box = in_box && p[d] >= g.lo[static_cast<size_t>(e) * DIM + d] && p[d] <= g.hi[static_cast<size_t>(e) * DIM + d];
    if (!in_box) continue;
    double xi[DIM];
    if (!invert_vertex_map<DIM>(verts + static_cast<size_t>(e) * NV * DIM, p, xi)) continue;
    bool accept = true;
    for (int d = 0; d < DIM; d++) accept = accept && xi[d] >= -tol && xi[d] <= 1.0 + tol;
    if (!accept) continue;
    for (int d = 0; d < DIM; d++) xi_out[d] = xi[d];
    return e;
  }
  return -1;
}

// verts: [ne][2^dim][dim] with lexicographic corners.  The layouts of xyz, elem_out, ref_out: tpsrhs_locate_points.
template <int DIM>
inline void locate_points_lex(int ne, const double *verts, int64_t npts, const double *xyz, double tol, int32_t *elem_out,
                              double *ref_out) {
  for (int64_t i = 0; i < npts; i++) {
    elem_out[i] = -1;
    for (int d = 0; d < DIM; d++) ref_out[i + d * npts] = 0.0;
  }
  if (ne <= 0 || npts <= 0) return;
  const LocateGrid grid = build_locate_grid<DIM>(ne, verts, tol);
  const LocateGridView<DIM> g = locate_grid_view<DIM>(grid);
  for (int64_t i = 0; i < npts; i++) {
    double p[DIM], xi[DIM];
    for (int d = 0; d < DIM; d++) p[d] = xyz[i + d * npts];
    elem_out[i] = locate_one<DIM>(g, verts, p, tol, xi);
    for (int d = 0; d < DIM; d++) ref_out[i + d * npts] = xi[d];
  }
}

// tpsrhs_locate_points without the error text: a tpsrhs_status
inline int locate_points(const tpsrhs_mesh *mesh, int64_t npts, const double *xyz, double tol, int32_t *elem_out,
                         double *ref_out) {
  if (!mesh || npts < 0 || (npts > 0 && (!xyz || !elem_out || !ref_out))) return TPSRHS_ERR_INVALID_ARGUMENT;
  if ((mesh->dim != 2 && mesh->dim != 3) || mesh->num_elements < 0 || (mesh->num_elements > 0 && !mesh->elem_coords))
    return TPSRHS_ERR_INVALID_ARGUMENT;
  if (std::isnan(tol)) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (!(tol > 0.0)) tol = LOCATE_DEFAULT_TOL;
  const int dim = mesh->dim, nv = 1 << dim, ne = mesh->num_elements;
  std::vector<double> verts(static_cast<size_t>(ne) * nv * dim);
  for (int e = 0; e < ne; e++)
    for (int v = 0; v < nv; v++)
      for (int d = 0; d < dim; d++)
        verts[(static_cast<size_t>(e) * nv + mfem_to_lex_corner(v)) * dim + d] = mesh->elem_coords[(static_cast<size_t>(e) * nv + v) * dim + d];
  if (dim == 2)
    locate_points_lex<2>(ne, verts.data(), npts, xyz, tol, elem_out, ref_out);
  else
    locate_points_lex<3>(ne, verts.data(), npts, xyz, tol, elem_out, ref_out);
  return TPSRHS_OK;
}

// tpsrhs_plane_points without the error text.  The major direction m is the first of x, y, z whose |normal| component is
// the largest; the n x n lattice spans the bounding box in the other two directions a < b, a running fastest, and the
// coordinate along m follows from normal . (x - point) = 0 in the reference's order of operations.
inline int plane_points(const double point[3], const double normal[3], const double bb0[3], const double bb1[3], int n,
                        double *xyz_out) {
  TPSRHS_IEEE_DIVISION
  if (!point || !normal || !bb0 || !bb1 || !xyz_out || n < 2) return TPSRHS_ERR_INVALID_ARGUMENT;
  double ndotp = 0.0;
  for (int d = 0; d < 3; d++) ndotp += normal[d] * point[d];
  double big = std::max(std::fabs(normal[0]), std::fabs(normal[1]));
  big = std::max(big, std::fabs(normal[2]));
  const int m = big == std::fabs(normal[0]) ? 0 : (big == std::fabs(normal[1]) ? 1 : 2);
  const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
  const double cells = static_cast<double>(n - 1);
  const double da = (bb1[a] - bb0[a]) / cells, db = (bb1[b] - bb0[b]) / cells;
  const int64_t total = static_cast<int64_t>(n) * n;
  int64_t at = 0;
  for (int j = 0; j < n; j++)
    for (int i = 0; i < n; i++, at++) {
      const double pa = da * static_cast<double>(i) + bb0[a];
      const double pb = db * static_cast<double>(j) + bb0[b];
      const double pm = (ndotp - (normal[a] * pa) - (normal[b] * pb)) / normal[m];
      xyz_out[at + a * total] = pa;
      xyz_out[at + b * total] = pb;
      xyz_out[at + m * total] = pm;
    }
  return TPSRHS_OK;
}

}  // namespace tpsrhs
#endif
