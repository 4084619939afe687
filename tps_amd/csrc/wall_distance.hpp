// The wall-distance function on the device: distance from every DG node to the nearest wall boundary face, what the
// reference computes at start-up with evaluateDistanceSerial (src/utils.cpp:371-514; called from src/M2ulPhyS.cpp:371-437
// when flow/computeDistance is set) in one serial host loop over nodes x wall faces.  Included by wall_distance.hip only: the
// kernel families do not see it.  The host half -- which faces are walls -- is wall_faces.hpp.
//
// A face is X(s, t) = a + b s + c t + d s t on [0,1]^2 (3-D; a = X00, b = X10 - X00, c = X01 - X00, d = X11 - X10 - X01 + X00
// with corner = ta + 2 tb) or X(s) = a + b s (2-D).  Per (node, face) pair, from xi = centre:
//   dx = xp - X(xi),  res = -J^T dx,  r0 = |res|
//   while (|res| > 1e-16 && |res| / r0 > 1e-10 && iter < 20)  xi += (J^T J)^{-1} J^T dx   (Gauss-Newton: the Hessian of the
//   map is neglected, as in the reference), dx and res again
//   clamp xi to [0,1]^(dim-1);  dist = |xp - X(xi)|;  kept when dist < best (best starts at 1e30; a NaN never wins).
// The reference's non-convergence warning has no counterpart, on purpose (include/tpsrhs.h says why).
#ifndef TPSRHS_WALL_DISTANCE_HPP_
#define TPSRHS_WALL_DISTANCE_HPP_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/tpsrhs.h"

namespace tpsrhs {

constexpr int WD_BLOCK = 256;
constexpr int WD_TILE = 128;  // faces staged through LDS at a time: 16 KB (3-D) / 8 KB (2-D) per block
// doubles per face: the map's coefficients, then the centre X(1/2) and the padded radius of the bounding sphere (the cull)
template <int DIM>
constexpr int wd_ncoef() {
  return DIM == 3 ? 16 : 8;
}
constexpr double WD_CULL_SLACK = 1e-12;  // relative; rounding in a distance is some 1e-15 of the coordinates' size

struct WdNodes {
  double x[TPSRHS_MAXORDER + 1];  // the operator's 1-D nodes on [0,1]
};

// Host: the per-face table [nfaces][wd_ncoef] from the corners face_xyz[nfaces][2^(dim-1)][dim].
// The sphere: centre X(1/2, 1/2), radius the largest distance to a corner (a bilinear patch lies in the convex hull of its
// corners), padded by WD_CULL_SLACK times the size of everything that enters, so that rounding cannot make the cull skip a
// face whose COMPUTED distance would have won.
template <int DIM>
inline void wd_face_table(int64_t nfaces, const double *face_xyz, std::vector<double> &coef) {
  constexpr int NC = wd_ncoef<DIM>(), NFV = 1 << (DIM - 1);
  coef.assign(static_cast<size_t>(nfaces) * NC, 0.0);
  for (int64_t f = 0; f < nfaces; f++) {
    const double *X = face_xyz + static_cast<size_t>(f) * NFV * DIM;
    double *o = coef.data() + static_cast<size_t>(f) * NC;
    double ctr[DIM], size = 0.0;
    for (int k = 0; k < DIM; k++) {
      if (DIM == 3) {
        const double a = X[k], b = X[DIM + k] - X[k], c = X[2 * DIM + k] - X[k];
        const double d = (X[3 * DIM + k] - X[DIM + k]) - (X[2 * DIM + k] - X[k]);
        o[k] = a, o[3 + k] = b, o[6 + k] = c, o[9 + k] = d;
        ctr[k] = a + 0.5 * b + 0.5 * c + 0.25 * d;
      } else {
        const double a = X[k], b = X[DIM + k] - X[k];
        o[k] = a, o[2 + k] = b;
        ctr[k] = a + 0.5 * b;
      }
      size += std::fabs(ctr[k]);
    }
    double r2 = 0.0;
    for (int v = 0; v < NFV; v++) {
      double s = 0.0;
      for (int k = 0; k < DIM; k++) s += (X[v * DIM + k] - ctr[k]) * (X[v * DIM + k] - ctr[k]);
      r2 = std::max(r2, s);
    }
    const double R = std::sqrt(r2);
    double *tail = o + (DIM == 3 ? 12 : 4);
    for (int k = 0; k < DIM; k++) tail[k] = ctr[k];
    tail[DIM] = R + WD_CULL_SLACK * (size + 4.0 * R);
  }
}

// Distance from xp to one face (c: its wd_ncoef doubles, in LDS).  IEEE division, correctly rounded sqrt.
__device__ inline double wd_face_distance3(const double *c, const double xp0, const double xp1, const double xp2) {
#pragma clang fp reciprocal(off)
  const double a0 = c[0], a1 = c[1], a2 = c[2], b0 = c[3], b1 = c[4], b2 = c[5];
  const double c0 = c[6], c1 = c[7], c2 = c[8], d0 = c[9], d1 = c[10], d2 = c[11];
  double s = 0.5, t = 0.5;
  double j0, j1, j2, k0, k1, k2, dx0, dx1, dx2, g1, g2;
  auto eval = [&]() {  // J1 = dX/ds = b + d t (j), J2 = dX/dt = c + d s (k), dx = xp - X, g = J^T dx = -res
    j0 = b0 + d0 * t, j1 = b1 + d1 * t, j2 = b2 + d2 * t;
    k0 = c0 + d0 * s, k1 = c1 + d1 * s, k2 = c2 + d2 * s;
    dx0 = xp0 - (a0 + s * j0 + t * c0), dx1 = xp1 - (a1 + s * j1 + t * c1), dx2 = xp2 - (a2 + s * j2 + t * c2);
    g1 = j0 * dx0 + j1 * dx1 + j2 * dx2;
    g2 = k0 * dx0 + k1 * dx1 + k2 * dx2;
  };
  eval();
  const double r0 = sqrt(g1 * g1 + g2 * g2);
  double rnorm = r0;
  int iter = 0;
  while (rnorm > 1e-16 && rnorm / r0 > 1e-10 && iter < 20) {
    const double A11 = j0 * j0 + j1 * j1 + j2 * j2, A12 = j0 * k0 + j1 * k1 + j2 * k2, A22 = k0 * k0 + k1 * k1 + k2 * k2;
    const double det = A11 * A22 - A12 * A12;
    s += (A22 * g1 - A12 * g2) / det;
    t += (A11 * g2 - A12 * g1) / det;
    eval();
    rnorm = sqrt(g1 * g1 + g2 * g2);
    iter++;
  }
  // outside the reference square: back to the closest point inside (a NaN stays a NaN and never wins the minimum)
  const double sc = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s), tc = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  if (sc != s || tc != t) {
    s = sc, t = tc;
    eval();
  }
  return sqrt(dx0 * dx0 + dx1 * dx1 + dx2 * dx2);
}

__device__ inline double wd_face_distance2(const double *c, const double xp0, const double xp1) {
#pragma clang fp reciprocal(off)
  const double a0 = c[0], a1 = c[1], b0 = c[2], b1 = c[3];
  double s = 0.5;
  double dx0 = xp0 - (a0 + s * b0), dx1 = xp1 - (a1 + s * b1);
  double g = b0 * dx0 + b1 * dx1;
  const double r0 = fabs(g);  // the 2-norm of a vector of one entry
  double rnorm = r0;
  int iter = 0;
  while (rnorm > 1e-16 && rnorm / r0 > 1e-10 && iter < 20) {
    s += g / (b0 * b0 + b1 * b1);
    dx0 = xp0 - (a0 + s * b0), dx1 = xp1 - (a1 + s * b1);
    g = b0 * dx0 + b1 * dx1;
    rnorm = fabs(g);
    iter++;
  }
  const double sc = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  if (sc != s) {
    s = sc;
    dx0 = xp0 - (a0 + s * b0), dx1 = xp1 - (a1 + s * b1);
  }
  return sqrt(dx0 * dx0 + dx1 * dx1);
}

// One lane per node n (element n / NPE); the lane forms its coordinates from the element's vertices (lexicographic
// corners, as every kernel reads Topology::verts) and the 1-D nodes, keeps its minimum in a register and writes it once.
// The faces pass through LDS a tile at a time; every lane of a wave reads the same face, which LDS serves as a broadcast.
// The Newton loop's trip count differs per lane: accepted.  No atomics, no scratch.
// CULL: a face whose padded bounding sphere lies farther away than the best distance so far cannot win and is skipped;
// the result is bit-equal to that of CULL = false.
template <int DIM, bool CULL>
__global__ void __launch_bounds__(WD_BLOCK)
    k_wall_distance(int64_t ndofs, int n1, WdNodes nodes, const double *__restrict__ verts, int64_t nfaces,
                    const double *__restrict__ coef, double *__restrict__ out) {
  constexpr int NC = wd_ncoef<DIM>(), NV = 1 << DIM;
  __shared__ double tile[WD_TILE * NC];
  const int64_t n = blockIdx.x * static_cast<int64_t>(WD_BLOCK) + threadIdx.x;
  const bool live = n < ndofs;
  double xp[DIM], size = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; a++) xp[a] = 0.0;
  if (live) {
    const int npe = DIM == 3 ? n1 * n1 * n1 : n1 * n1;
    const int64_t e = n / npe;
    const int l = static_cast<int>(n - e * npe);
    const int idx[3] = {l % n1, (l / n1) % n1, l / (n1 * n1)};
    double xi[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) {
      double v = nodes.x[0];
#pragma unroll
      for (int a = 1; a <= TPSRHS_MAXORDER; a++) v = idx[d] == a ? nodes.x[a] : v;  // no run-time index into the argument
      xi[d] = v;
    }
    const double *v = verts + e * (NV * DIM);
#pragma unroll
    for (int c = 0; c < NV; c++) {
      double w = 1.0;
#pragma unroll
      for (int d = 0; d < DIM; d++) w *= ((c >> d) & 1) ? xi[d] : 1.0 - xi[d];
#pragma unroll
      for (int a = 0; a < DIM; a++) xp[a] += v[c * DIM + a] * w;
    }
#pragma unroll
    for (int a = 0; a < DIM; a++) size += fabs(xp[a]);
  }
  const double slack = WD_CULL_SLACK * size;
  double best = 1e30;
  for (int64_t f0 = 0; f0 < nfaces; f0 += WD_TILE) {
    const int nt = static_cast<int>(nfaces - f0 < WD_TILE ? nfaces - f0 : WD_TILE);
    __syncthreads();  // the previous tile has been read by every wave
    for (int i = threadIdx.x; i < nt * NC; i += WD_BLOCK) tile[i] = coef[f0 * NC + i];
    __syncthreads();
    if (!live) continue;
    for (int f = 0; f < nt; f++) {
      const double *c = tile + f * NC;
      if constexpr (CULL) {
        const double *q = c + (DIM == 3 ? 12 : 4);  // centre, padded radius
        double dc2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; a++) dc2 += (xp[a] - q[a]) * (xp[a] - q[a]);
        const double reach = best + q[DIM] + slack;
        if (dc2 > reach * reach) continue;
      }
      double dist;
      if constexpr (DIM == 3)
        dist = wd_face_distance3(c, xp[0], xp[1], xp[2]);
      else
        dist = wd_face_distance2(c, xp[0], xp[1]);
      if (dist < best) best = dist;
    }
  }
  if (live) out[n] = best;
}

}  // namespace tpsrhs
#endif
