// Host geometry of the elements, from their corners alone: the element sizes the sub-grid scale models filter with and
// the inverse mass matrices of the non-collocated pair.  Plain C++17, no HIP: tpsrhs.hip uploads the results,
// tests/operator_plan_main.cpp checks them on the host.
#ifndef TPSRHS_ELEMENT_GEOMETRY_HPP_
#define TPSRHS_ELEMENT_GEOMETRY_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <thread>
#include <vector>

#include "basis.hpp"

namespace tpsrhs {

// mfem::Mesh::GetElementSize(e, 1): the smallest singular value of the Jacobian at the element centre
// (src/rhs_operator.cpp:154, src/face_integrator.cpp:253).  sqrt of the smallest eigenvalue of J^T J by cyclic
// Jacobi rotations.  verts: [ne][2^dim][dim] lexicographic corners.
inline std::vector<double> element_sizes(const std::vector<double> &verts, int dim, int ne) {
  std::vector<double> h(ne);
  const int nv = 1 << dim;
  for (int e = 0; e < ne; e++) {
    const double *V = &verts[static_cast<size_t>(e) * nv * dim];
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // J[i][a] = d x_i / d xi_a at the centre
    for (int v = 0; v < nv; v++)
      for (int a = 0; a < dim; a++) {
        const double sgn = ((v >> a) & 1) ? 1.0 : -1.0;
        for (int i = 0; i < dim; i++) J[i][a] += sgn * V[v * dim + i] / (nv / 2);
      }
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < dim; a++)
      for (int b = 0; b < dim; b++) {
        double t = 0.0;
        for (int i = 0; i < dim; i++) t += J[i][a] * J[i][b];
        A[a][b] = t;
      }
    for (int sweep = 0; sweep < 30; sweep++) {
      double off = 0.0;
      for (int a = 0; a < dim; a++)
        for (int b = a + 1; b < dim; b++) off += A[a][b] * A[a][b];
      if (off == 0.0) break;
      for (int a = 0; a < dim; a++)
        for (int b = a + 1; b < dim; b++) {
          if (A[a][b] == 0.0) continue;
          const double theta = (A[b][b] - A[a][a]) / (2.0 * A[a][b]);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
          const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
          for (int k = 0; k < dim; k++) {  // A <- A R
            const double aka = A[k][a], akb = A[k][b];
            A[k][a] = c * aka - sn * akb;
            A[k][b] = sn * aka + c * akb;
          }
          for (int k = 0; k < dim; k++) {  // A <- R^T A
            const double aak = A[a][k], abk = A[b][k];
            A[a][k] = c * aak - sn * abk;
            A[b][k] = sn * aak + c * abk;
          }
        }
    }
    double lmin = A[0][0];
    for (int a = 1; a < dim; a++) lmin = std::min(lmin, A[a][a]);
    h[e] = std::sqrt(std::max(lmin, 0.0));
  }
  return h;
}

// Inverse element mass matrices of the non-collocated pair: M_jk = sum_q w_q det J(q) phi_j(q) phi_k(q) with the
// order-2p rule of the same family (MassIntegrator, src/rhs_operator.cpp:179-187), inverted per element
// (Cholesky; the reference calls DenseMatrix::Invert, :205-212) -- the role of Me_inv, built once, on the host,
// on all cores.  verts: [ne][2^dim][dim] lexicographic corners.
inline std::vector<double> inverse_mass_matrices(const std::vector<double> &verts, int dim, int order, int ne) {
  const Tables1D t = make_tables(order, dim, 1, 1);
  const int n1 = order + 1, qv = rule_points(1, 2 * order);
  const int npe = (dim == 3) ? n1 * n1 * n1 : n1 * n1, nq = (dim == 3) ? qv * qv * qv : qv * qv, nv = 1 << dim;
  // Phi[q][j]: tensor basis at the tensor rule
  std::vector<double> Phi(static_cast<size_t>(nq) * npe), wq(nq), xq(static_cast<size_t>(nq) * dim);
  for (int q = 0; q < nq; q++) {
    int qi[3] = {q % qv, (q / qv) % qv, q / (qv * qv)};
    wq[q] = 1.0;
    for (int d = 0; d < dim; d++) {
      wq[q] *= t.wv[qi[d]];
      xq[static_cast<size_t>(q) * dim + d] = t.xv[qi[d]];
    }
    for (int j = 0; j < npe; j++) {
      int ji[3] = {j % n1, (j / n1) % n1, j / (n1 * n1)};
      double v = 1.0;
      for (int d = 0; d < dim; d++) v *= t.Bv[qi[d] * n1 + ji[d]];
      Phi[static_cast<size_t>(q) * npe + j] = v;
    }
  }
  std::vector<double> out(static_cast<size_t>(ne) * npe * npe);
  auto work = [&](int e_begin, int e_end) {
    std::vector<double> M(static_cast<size_t>(npe) * npe), Wp(static_cast<size_t>(nq) * npe), L(static_cast<size_t>(npe) * npe);
    for (int e = e_begin; e < e_end; e++) {
      const double *V = &verts[static_cast<size_t>(e) * nv * dim];
      for (int q = 0; q < nq; q++) {  // det J at the point (multilinear map of the 2^dim corners)
        const double *xi = &xq[static_cast<size_t>(q) * dim];
        double J[9] = {0};
        for (int c = 0; c < nv; c++) {
          for (int m2 = 0; m2 < dim; m2++) {
            double g = 1.0;  // d/dxi_m2 of the corner's shape function
            for (int d = 0; d < dim; d++) {
              const int bit = (c >> d) & 1;
              if (d == m2)
                g *= bit ? 1.0 : -1.0;
              else
                g *= bit ? xi[d] : 1.0 - xi[d];
            }
            for (int i = 0; i < dim; i++) J[i + m2 * dim] += g * V[c * dim + i];
          }
        }
        const double det = (dim == 2) ? J[0] * J[3] - J[2] * J[1]
                                      : J[0] * (J[4] * J[8] - J[7] * J[5]) - J[3] * (J[1] * J[8] - J[7] * J[2]) +
                                            J[6] * (J[1] * J[5] - J[4] * J[2]);
        const double wd = wq[q] * det;
        for (int j = 0; j < npe; j++) Wp[static_cast<size_t>(q) * npe + j] = wd * Phi[static_cast<size_t>(q) * npe + j];
      }
      std::fill(M.begin(), M.end(), 0.0);
      for (int q = 0; q < nq; q++)
        for (int j = 0; j < npe; j++) {
          const double pj = Phi[static_cast<size_t>(q) * npe + j];
          const double *wrow = &Wp[static_cast<size_t>(q) * npe];
          double *mrow = &M[static_cast<size_t>(j) * npe];
          for (int k = 0; k < npe; k++) mrow[k] += pj * wrow[k];
        }
      // Cholesky M = L L^T, then M^-1 = L^-T L^-1
      std::fill(L.begin(), L.end(), 0.0);
      for (int j = 0; j < npe; j++) {
        double d = M[static_cast<size_t>(j) * npe + j];
        for (int k = 0; k < j; k++) d -= L[static_cast<size_t>(j) * npe + k] * L[static_cast<size_t>(j) * npe + k];
        if (!(d > 0.0)) throw std::runtime_error("element mass matrix is not positive definite (inverted element?)");
        const double ljj = std::sqrt(d);
        L[static_cast<size_t>(j) * npe + j] = ljj;
        for (int i = j + 1; i < npe; i++) {
          double v = M[static_cast<size_t>(i) * npe + j];
          for (int k = 0; k < j; k++) v -= L[static_cast<size_t>(i) * npe + k] * L[static_cast<size_t>(j) * npe + k];
          L[static_cast<size_t>(i) * npe + j] = v / ljj;
        }
      }
      // Linv (lower) in M's storage
      std::fill(M.begin(), M.end(), 0.0);
      for (int j = 0; j < npe; j++) {
        M[static_cast<size_t>(j) * npe + j] = 1.0 / L[static_cast<size_t>(j) * npe + j];
        for (int i = j + 1; i < npe; i++) {
          double v = 0.0;
          for (int k = j; k < i; k++) v -= L[static_cast<size_t>(i) * npe + k] * M[static_cast<size_t>(k) * npe + j];
          M[static_cast<size_t>(i) * npe + j] = v / L[static_cast<size_t>(i) * npe + i];
        }
      }
      double *o = &out[static_cast<size_t>(e) * npe * npe];
      for (int i = 0; i < npe; i++)
        for (int j = 0; j <= i; j++) {
          double v = 0.0;
          for (int k = i; k < npe; k++) v += M[static_cast<size_t>(k) * npe + i] * M[static_cast<size_t>(k) * npe + j];
          o[static_cast<size_t>(i) * npe + j] = o[static_cast<size_t>(j) * npe + i] = v;
        }
    }
  };
  const int nthreads = std::max(1, std::min<int>(static_cast<int>(std::thread::hardware_concurrency()), std::min(32, ne / 64 + 1)));
  std::vector<std::thread> pool;
  std::vector<std::exception_ptr> errs(nthreads);
  for (int t2 = 0; t2 < nthreads; t2++) {
    const int b = static_cast<int>(static_cast<int64_t>(ne) * t2 / nthreads), en = static_cast<int>(static_cast<int64_t>(ne) * (t2 + 1) / nthreads);
    pool.emplace_back([&, b, en, t2] {
      try {
        work(b, en);
      } catch (...) {
        errs[t2] = std::current_exception();
      }
    });
  }
  for (auto &th : pool) th.join();
  for (auto &e : errs)
    if (e) std::rethrow_exception(e);
  return out;
}

}  // namespace tpsrhs
#endif
