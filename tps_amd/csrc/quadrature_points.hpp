// The quadrature rule of the volume integrals (tpsrhs_quadrature_points, tpsrhs_integrate): MFEM's default rule of
// GridFunction::ComputeLpError, which M2ulPhyS::checkSolutionError prints its L2 errors with (src/masa_handler.cpp:139-152)
// [third party: MFEM fem/gridfunc.cpp, Gauss-Legendre of order 2p + 3], on the order-1 geometry of a tpsrhs_mesh.
// Plain C++: no HIP, no device, nothing but tpsrhs.h and basis.hpp -- a stand-alone program can include this file alone
// (tests/test_quadrature_sanitize.py does, under the sanitizers).  quad_geometry is also what the device kernel of
// integrals.hpp calls per point, so that the host's weights and the device's are the same expression.
//
//   rule      tensor Gauss-Legendre, NQ = p + 2 points per direction on [0,1]
//   point     q = e * NQ^dim + (i + j NQ + k NQ^2),  xi_q = (g_i, g_j, g_k)
//   geometry  x(xi) = sum_c verts[e][c] prod_d (c_d ? xi_d : 1 - xi_d),  c = c_0 + 2 c_1 + 4 c_2  (lexicographic corners)
//   weight    W_q = w_i w_j (w_k) |det dx/dxi (xi_q)|
#ifndef TPSRHS_QUADRATURE_POINTS_HPP_
#define TPSRHS_QUADRATURE_POINTS_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/tpsrhs.h"
#include "basis.hpp"

#if defined(__HIPCC__)
#define TPSRHS_HOST_DEVICE __host__ __device__
#else
#define TPSRHS_HOST_DEVICE
#endif

namespace tpsrhs {

constexpr int QUAD_MAXQ = TPSRHS_MAXORDER + 2;  // 7 points per direction at p = 5

inline int quad_points_1d(int order) { return order + 2; }

// for the reduction kernels (integrals.hpp, surface.hpp): b^e, and the power of two >= n, at most 64 -- the lanes of a wave
// that share one element or face
constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }
constexpr int lanes_per_element(int n) { return n >= 64 ? 64 : (n <= 1 ? 1 : 2 * lanes_per_element((n + 1) / 2)); }

// x(xi) and det dx/dxi of one element; v: [2^DIM][DIM], lexicographic corners
template <int DIM>
TPSRHS_HOST_DEVICE inline void quad_geometry(const double *v, const double *xi, double *x, double *det) {
  if constexpr (DIM == 2) {
    const double a0 = 1.0 - xi[0], a1 = xi[0], b0 = 1.0 - xi[1], b1 = xi[1];
    double J[4];
    for (int a = 0; a < 2; a++) {
      const double v00 = v[0 * 2 + a], v10 = v[1 * 2 + a], v01 = v[2 * 2 + a], v11 = v[3 * 2 + a];
      x[a] = (v00 * a0 + v10 * a1) * b0 + (v01 * a0 + v11 * a1) * b1;
      J[a * 2 + 0] = (v10 - v00) * b0 + (v11 - v01) * b1;
      J[a * 2 + 1] = (v01 - v00) * a0 + (v11 - v10) * a1;
    }
    *det = J[0] * J[3] - J[1] * J[2];
  } else {
    const double a0 = 1.0 - xi[0], a1 = xi[0], b0 = 1.0 - xi[1], b1 = xi[1], c0 = 1.0 - xi[2], c1 = xi[2];
    double J[9];
    for (int a = 0; a < 3; a++) {
      const double v000 = v[0 * 3 + a], v100 = v[1 * 3 + a], v010 = v[2 * 3 + a], v110 = v[3 * 3 + a];
      const double v001 = v[4 * 3 + a], v101 = v[5 * 3 + a], v011 = v[6 * 3 + a], v111 = v[7 * 3 + a];
      // the four edges along xi_0, the bottom and top faces along xi_1
      const double e00 = v000 * a0 + v100 * a1, e10 = v010 * a0 + v110 * a1, e01 = v001 * a0 + v101 * a1,
                   e11 = v011 * a0 + v111 * a1;
      const double f0 = e00 * b0 + e10 * b1, f1 = e01 * b0 + e11 * b1;
      x[a] = f0 * c0 + f1 * c1;
      J[a * 3 + 0] = ((v100 - v000) * b0 + (v110 - v010) * b1) * c0 + ((v101 - v001) * b0 + (v111 - v011) * b1) * c1;
      J[a * 3 + 1] = (e10 - e00) * c0 + (e11 - e01) * c1;
      J[a * 3 + 2] = f1 - f0;
    }
    *det = J[0] * (J[4] * J[8] - J[5] * J[7]) + J[1] * (J[5] * J[6] - J[3] * J[8]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
  }
}

// verts: [ne][2^DIM][DIM] with lexicographic corners; g, w: the NQ points and weights of the 1-D rule
template <int DIM>
inline void quadrature_points_lex(int ne, const double *verts, int nq, const double *g, const double *w, double *xyz_out,
                                  double *w_out) {
  constexpr int NV = 1 << DIM;
  const int64_t nqd = DIM == 3 ? static_cast<int64_t>(nq) * nq * nq : static_cast<int64_t>(nq) * nq;
  const int64_t npts = nqd * ne;
  for (int e = 0; e < ne; e++) {
    const double *v = verts + static_cast<size_t>(e) * NV * DIM;
    for (int k = 0; k < (DIM == 3 ? nq : 1); k++)
      for (int j = 0; j < nq; j++)
        for (int i = 0; i < nq; i++) {
          const double xi[3] = {g[i], g[j], g[k]};
          double x[DIM], det;
          quad_geometry<DIM>(v, xi, x, &det);
          const int64_t q = e * nqd + (i + static_cast<int64_t>(nq) * (j + static_cast<int64_t>(nq) * k));
          if (xyz_out)
            for (int d = 0; d < DIM; d++) xyz_out[q + d * npts] = x[d];
          if (w_out) w_out[q] = (DIM == 3 ? w[i] * w[j] * w[k] : w[i] * w[j]) * std::fabs(det);
        }
  }
}

// tpsrhs_quadrature_points without the error text: a tpsrhs_status
inline int quadrature_points(const tpsrhs_mesh *mesh, int order, double *xyz_out, double *w_out, int64_t *npts_out) {
  if (!mesh || !npts_out || (mesh->dim != 2 && mesh->dim != 3) || order < 1 || order > TPSRHS_MAXORDER)
    return TPSRHS_ERR_INVALID_ARGUMENT;
  if (mesh->num_elements < 0 || (mesh->num_elements > 0 && !mesh->elem_coords)) return TPSRHS_ERR_INVALID_ARGUMENT;
  const int dim = mesh->dim, nv = 1 << dim, ne = mesh->num_elements, nq = quad_points_1d(order);
  *npts_out = static_cast<int64_t>(ne) * (dim == 3 ? nq * nq * nq : nq * nq);
  if (!xyz_out && !w_out) return TPSRHS_OK;
  static const int lex_of_mfem_corner[8] = {0, 1, 3, 2, 4, 5, 7, 6};
  double g[QUAD_MAXQ], w[QUAD_MAXQ];
  gauss_legendre01(nq, g, w);
  // one element at a time through a small buffer: no allocation of the size of the mesh
  double v[8 * 3];
  const int64_t nqd = dim == 3 ? nq * nq * nq : nq * nq, npts = *npts_out;
  double xyz_e[3 * QUAD_MAXQ * QUAD_MAXQ * QUAD_MAXQ], w_e[QUAD_MAXQ * QUAD_MAXQ * QUAD_MAXQ];
  for (int e = 0; e < ne; e++) {
    for (int c = 0; c < nv; c++)
      for (int d = 0; d < dim; d++)
        v[lex_of_mfem_corner[c] * dim + d] = mesh->elem_coords[(static_cast<size_t>(e) * nv + c) * dim + d];
    if (dim == 2)
      quadrature_points_lex<2>(1, v, nq, g, w, xyz_e, w_e);
    else
      quadrature_points_lex<3>(1, v, nq, g, w, xyz_e, w_e);
    for (int64_t q = 0; q < nqd; q++) {
      if (xyz_out)
        for (int d = 0; d < dim; d++) xyz_out[e * nqd + q + d * npts] = xyz_e[q + d * nqd];
      if (w_out) w_out[e * nqd + q] = w_e[q];
    }
  }
  return TPSRHS_OK;
}

}  // namespace tpsrhs
#endif
