// Values of a byNODES DG field on the closed uniform lattice of every element: what ParaViewDataCollection::Save evaluates
// with SetLevelsOfDetail (GridFunction::GetValues at the points of a RefinedGeometry; src/M2ulPhyS.cpp:1877-1906).
// Included by lattice.hip only: the kernel families do not see it.  Conventions: include/tpsrhs.h, the lattice section.
//
// For levels = L the lattice has n = L + 1 points t_a = a / L per direction, and with B[a][i] = l_i(t_a)
//   out[e n^dim + a + b n + c n^2] = sum_k B[c][k] sum_j B[b][j] sum_i B[a][i] u[e (p+1)^dim + i + j (p+1) + k (p+1)^2]
// evaluated direction by direction: dim (p + 1) multiply-adds per value, where the arbitrary-point sampler (sampling.hpp)
// forms (p + 1)^dim products and reads a location record per point.
#ifndef TPSRHS_LATTICE_HPP_
#define TPSRHS_LATTICE_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tpsrhs.h"
#include "point_locate.hpp"

namespace tpsrhs {

constexpr int LATTICE_BLOCK = 64;  // one wave: the barriers between the directions cost next to nothing

// What the host forms per call and the kernels take by value.
struct LatticeBasis {
  double b[(TPSRHS_MAXLATTICE + 1) * (TPSRHS_MAXORDER + 1)];  // B[a * (p+1) + i] = l_i(a / L), rows a = 0..L
  float rn;                                                   // 1 / (L + 1) rounded: see lattice_div
  int n;                                                      // L + 1
};
struct LatticeAbscissae {
  double t[TPSRHS_MAXLATTICE + 1];  // a / L, the host's IEEE quotient: t[0] = 0 and t[L] = 1 exactly
  int n;
};

// elements per block: as many as fill one wave with nodes.  2-D: 16, 7, 4, 2, 1 for p = 1..5; 3-D: 8, 2, 1, 1, 1.
constexpr int lattice_elems_per_block(int npe) { return npe >= LATTICE_BLOCK ? 1 : LATTICE_BLOCK / npe; }

// doubles of LDS a block needs: B, the nodal tiles, and the intermediates of the contraction
inline size_t lattice_lds_doubles(int dim, int p, int n) {
  const int n1 = p + 1, npe = dim == 3 ? n1 * n1 * n1 : n1 * n1, epb = lattice_elems_per_block(npe);
  size_t d = static_cast<size_t>(n) * n1 + static_cast<size_t>(epb) * npe;
  d += static_cast<size_t>(epb) * (npe / n1) * n;             // v1[..][a]: the first direction contracted
  if (dim == 3) d += static_cast<size_t>(epb) * n1 * n * n;  // v2[s][k][b][a]: the second
  return d;
}

// x / n for 0 <= x < 2^13 and n = 1 / rn <= 9: (x + 1/2) / n is at least 1 / 18 away from an integer, the float product is
// within 1e-3 of it.  Five conversions and multiplies instead of the ~25 instructions of an integer division by a run-time
// divisor, per value and direction.
__device__ inline int lattice_div(int x, float rn) { return static_cast<int>((static_cast<float>(x) + 0.5f) * rn); }

// One block = EPB consecutive elements (the last block of the grid may hold fewer), LATTICE_BLOCK lanes.  Per row: the nodal
// tiles of the block's elements are one contiguous run of the field and go through registers into LDS (the next row's run
// is fetched while this one is contracted); each direction is one pass in which the lanes stride over the outputs of that
// pass; the last pass writes the block's lattice values, again one contiguous run, to `out`.  The index arithmetic of a
// pass does not depend on the row but is redone per row: holding it would take a run-time number of registers.
// B is selected out of the kernel argument with an unrolled chain (no run-time index into the argument) into LDS once.
// No atomics, no scratch.
template <int DIM, int P, bool F32>
__global__ void __launch_bounds__(LATTICE_BLOCK)
    k_lattice(int ne, int nrows, int64_t ndofs, int64_t npts, LatticeBasis basis, const double *__restrict__ field,
              void *__restrict__ out_) {
  constexpr int N1 = P + 1;
  constexpr int NPE = DIM == 3 ? N1 * N1 * N1 : N1 * N1;
  constexpr int EPB = lattice_elems_per_block(NPE);
  constexpr int NB = (TPSRHS_MAXLATTICE + 1) * N1;
  constexpr int TL = (EPB * NPE + LATTICE_BLOCK - 1) / LATTICE_BLOCK;  // tile values per lane
  static_assert(NB <= LATTICE_BLOCK, "one lane per entry of B");
  extern __shared__ double lds[];
  const int n = basis.n, nn = n * n;
  const float rn = basis.rn;
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * EPB;
  const int nel = min(EPB, ne - e0);  // >= 1 by the size of the grid
  const int ntile = nel * NPE;

  double *sB = lds;               // [n][N1]
  double *su = sB + n * N1;       // [EPB][NPE]
  double *v1 = su + EPB * NPE;    // [EPB * NPE / N1][n]
  double *v2 = v1 + EPB * (NPE / N1) * n;  // 3-D only: [EPB * N1][n][n]
  {
    double v = 0.0;
#pragma unroll
    for (int t = 0; t < NB; t++) v = tid == t ? basis.b[t] : v;
    if (tid < n * N1) sB[tid] = v;
  }

  const double *src = field + static_cast<int64_t>(e0) * NPE;
  const int64_t obase = static_cast<int64_t>(e0) * (DIM == 3 ? nn * n : nn);
  double nxt[TL];
#pragma unroll
  for (int q = 0; q < TL; q++) {
    const int idx = tid + q * LATTICE_BLOCK;
    nxt[q] = idx < ntile ? src[idx] : 0.0;
  }
  for (int r = 0; r < nrows; r++) {
#pragma unroll
    for (int q = 0; q < TL; q++) {
      const int idx = tid + q * LATTICE_BLOCK;
      if (idx < ntile) su[idx] = nxt[q];
    }
    __syncthreads();  // su (and, in the first row, sB) written; the last pass of the row before has read v1 / v2
    if (r + 1 < nrows) {
      src += ndofs;
#pragma unroll
      for (int q = 0; q < TL; q++) {
        const int idx = tid + q * LATTICE_BLOCK;
        if (idx < ntile) nxt[q] = src[idx];
      }
    }
    // direction 0: v1[R][a] = sum_i B[a][i] u[R][i], R = (slot, k, j) -- the rows of N1 values of the tiles
    const int c1 = nel * (NPE / N1) * n;
    for (int idx = tid; idx < c1; idx += LATTICE_BLOCK) {
      const int R = lattice_div(idx, rn), a = idx - R * n;
      const double *u = su + R * N1, *w = sB + a * N1;
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < N1; i++) s += w[i] * u[i];
      v1[idx] = s;
    }
    __syncthreads();
    if constexpr (DIM == 3) {
      // direction 1: v2[S][b][a] = sum_j B[b][j] v1[S][j][a], S = (slot, k)
      const int c2 = nel * N1 * nn;
      for (int idx = tid; idx < c2; idx += LATTICE_BLOCK) {
        const int t = lattice_div(idx, rn), a = idx - t * n;
        const int S = lattice_div(t, rn), b = t - S * n;
        const double *u = v1 + S * N1 * n + a, *w = sB + b * N1;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < N1; j++) s += w[j] * u[j * n];
        v2[idx] = s;
      }
      __syncthreads();
    }
    // the last direction, to the block's run of `out`: [slot][c][b][a] (3-D) or [slot][b][a]
    const int plane = DIM == 3 ? nn : n;  // values below the contracted index
    const int c3 = nel * plane * n;
    const double *vin = DIM == 3 ? v2 : v1;
    const int64_t o = static_cast<int64_t>(r) * npts + obase;
    for (int idx = tid; idx < c3; idx += LATTICE_BLOCK) {
      int t = lattice_div(idx, rn);
      int low = idx - t * n;  // a
      if constexpr (DIM == 3) {
        const int t2 = lattice_div(t, rn);
        low += (t - t2 * n) * n;  // a + b n
        t = t2;
      }
      const int s = lattice_div(t, rn), c = t - s * n;
      const double *u = vin + s * N1 * plane + low, *w = sB + c * N1;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < N1; k++) acc += w[k] * u[k * plane];
      if constexpr (F32)
        static_cast<float *>(out_)[o + idx] = static_cast<float>(acc);  // one conversion, round to nearest
      else
        static_cast<double *>(out_)[o + idx] = acc;
    }
    // no barrier here: the next row writes su, which direction 0 finished reading before the barrier above it
  }
}

// A double-double value hi + lo, |lo| <= ulp(hi) / 2, for the coordinates of the lattice points: sums and products through the
// error-free transformations (Knuth's two-sum, the FMA two-product), nothing contracted or reassociated behind their back.
struct LatticeDD {
  double hi, lo;
};
__device__ inline LatticeDD lattice_two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ inline LatticeDD lattice_dd_add(LatticeDD a, LatticeDD b) {
#pragma clang fp contract(off)
  const LatticeDD s = lattice_two_sum(a.hi, b.hi);
  return lattice_two_sum(s.hi, s.lo + (a.lo + b.lo));
}
__device__ inline LatticeDD lattice_dd_mul(LatticeDD a, LatticeDD b) {
#pragma clang fp contract(off)
  const double p = a.hi * b.hi, e = __builtin_fma(a.hi, b.hi, -p);
  return lattice_two_sum(p, e + (a.hi * b.lo + a.lo * b.hi));
}

// xyz[i + d * npts] of lattice point i = e * n^DIM + (a + b n + c n^2): the order-1 vertex map at (t_a, t_b, t_c).  The
// shape weights are products of t and 1 - t, the sum runs over the corners in lexicographic order (point_locate.hpp:
// vertex_map); at a corner one weight is 1, the others are 0 and the point is the vertex bit for bit.  1 - t, the products
// and the sum are carried in double-double and rounded once at the end, so a coordinate is the correctly rounded image of
// the doubles t: whoever inverts the map at these points (the sampler's Newton iteration) starts from half an ulp, not from
// the 1 - 2 ulp of |x| a plain evaluation leaves, which an element of size h magnifies by 1 / h in the reference
// coordinates.  Once per mesh: the arithmetic does not matter.  The abscissa is picked with an unrolled select, as
// k_node_coordinates does.
template <int DIM, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_lattice_coordinates(int64_t npts, LatticeAbscissae ab, const double *__restrict__ verts, double *__restrict__ xyz) {
  constexpr int NV = 1 << DIM;
  const int64_t i = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
  if (i >= npts) return;
  const int n = ab.n;
  const int nl = DIM == 3 ? n * n * n : n * n;
  const int64_t e = i / nl;
  int l = static_cast<int>(i - e * nl);
  LatticeDD f1[DIM], f0[DIM];  // t and 1 - t per direction
#pragma unroll
  for (int d = 0; d < DIM; d++) {
    const int a = l % n;
    l /= n;
    double t = ab.t[0];
#pragma unroll
    for (int j = 1; j <= TPSRHS_MAXLATTICE; j++) t = j == a ? ab.t[j] : t;
    f1[d] = {t, 0.0};
    f0[d] = lattice_two_sum(1.0, -t);
  }
  const double *v = verts + e * (NV * DIM);
  LatticeDD x[DIM];
#pragma unroll
  for (int d = 0; d < DIM; d++) x[d] = {0.0, 0.0};
#pragma unroll
  for (int c = 0; c < NV; c++) {
    LatticeDD w = ((c & 1) ? f1 : f0)[0];
#pragma unroll
    for (int d = 1; d < DIM; d++) w = lattice_dd_mul(w, ((c >> d) & 1) ? f1[d] : f0[d]);
#pragma unroll
    for (int d = 0; d < DIM; d++) x[d] = lattice_dd_add(x[d], lattice_dd_mul({v[c * DIM + d], 0.0}, w));
  }
#pragma unroll
  for (int d = 0; d < DIM; d++) xyz[i + d * npts] = x[d].hi + x[d].lo;
}

}  // namespace tpsrhs
#endif
