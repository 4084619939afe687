// Reductions over a byNODES DG field on the device: volume integrals and L2 errors (tpsrhs_integrate: what the reference
// prints from M2ulPhyS::checkSolutionError through GridFunction::ComputeLpError, src/masa_handler.cpp:139-152), the range
// of every row and the mean |value| (tpsrhs_nodal_stats: RHSoperator::computeMeanTimeDerivatives, src/rhs_operator.cpp:833-849),
// and the monitor records the device time loop keeps of them.  Included by integrals.hip only: the kernel families do not see
// it.  The rule and its host half are quadrature_points.hpp.
//
// Summation structure (the contract of include/tpsrhs.h): the terms of one element are summed first, the element sums of
// one block are added in ascending element order, and a last single-block kernel adds the per-block partials in a fixed
// order.  No floating-point atomics: two calls on the same input are bit-equal.
//
// Shape of the kernels.  A block is ONE wave, so its barriers cost a wait and no s_barrier, and 32 of them share a CU.  The
// 64 lanes are cut into EB = 64 / LPE segments of LPE lanes (LPE: the power of two >= the points of an element, at most
// 64); a segment owns one element of a batch of EB consecutive elements, and a block walks a fixed run of batches.
//   k_integrate<DIM, P>: per batch the weights W_q go to LDS once; then, for each of up to INTEG_ROWS rows, the batch's
//   nodal values are loaded into LDS (consecutive addresses: the field is read once, coalesced), interpolated to the points
//   direction by direction through LDS with the 1-D matrix B (NQ x N1, in LDS), and every lane forms W g and W g^2 of its
//   points; a butterfly over the segment's lanes gives the element sums, which the segment's first lane adds to its running
//   partial in LDS.  Rows beyond INTEG_ROWS are further launches.  (Interpolating four rows together -- one read of a
//   coefficient of B for four products, a quarter of the barriers -- was measured and was slower: DESIGN.md.)
//   k_nodal_stats: the same segmentation by nodes, one row per blockIdx.y, four batches in flight; min / max with `<` / `>`.
//   k_integrate_final / k_nodal_stats_final: one block of 1024 threads adds the per-block partials of every row.
#ifndef TPSRHS_INTEGRALS_HPP_
#define TPSRHS_INTEGRALS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/tpsrhs.h"
#include "device_buffer.hpp"
#include "quadrature_points.hpp"
#include "record_log.hpp"

// the monitor records (tpsrhs_monitor_configure); cadence.interval 0: off
struct tpsrhs_monitor_log {
  tpsrhs::StepCadence cadence;  // count: steps of tpsrhs_advance / tpsrhs_advance_with since tpsrhs_monitor_configure
  tpsrhs::RecordIndex index;
  DevBuf<double> d_times, d_dts;            // [capacity], copied from d_ctl on the stream
  DevBuf<double> d_totals, d_mins, d_maxs;  // [capacity][neq]
};

// behind tpsrhs_operator::integrals; created by integrals.hip at the first use, owned by the operator
struct tpsrhs_integrals_state {
  int integ_blocks = 0, integ_run = 0, integ_eb = 1;  // grid, elements per block (a multiple of integ_eb), segments
  int stat_blocks = 0, stat_run = 0, stat_lpe = 64;
  DevBuf<double> d_partial;  // [INTEG_ROWS][max(2 * integ_blocks * integ_eb, 3 * stat_blocks * stat_eb)]
  tpsrhs_monitor_log monitor;
};

namespace tpsrhs {

constexpr int INTEG_ROWS = 16;      // rows per launch: their running partials live in LDS
constexpr int INTEG_MAXBLOCKS = 8192;  // 32 one-wave blocks on each of the 256 CUs

struct QuadTab {
  double B[QUAD_MAXQ * (TPSRHS_MAXORDER + 1)];  // B[q * N1 + a] = l_a(g_q)
  double g[QUAD_MAXQ], w[QUAD_MAXQ];
};

template <int DIM, int P>
struct IntegCfg {
  static constexpr int N1 = P + 1, NQ = P + 2;
  static constexpr int NPE = ipow(N1, DIM), NQD = ipow(NQ, DIM);
  static constexpr int LPE = lanes_per_element(NQD), EB = 64 / LPE;
};

// partial: [nrows][2][gridDim.x * EB]; run: elements per block, a multiple of EB
template <int DIM, int P>
__global__ void __launch_bounds__(64)
    k_integrate(int ne, int run, int nrows, int64_t ndofs, int64_t npts, int radial, QuadTab tab,
                const double *__restrict__ verts, const double *__restrict__ field, const double *__restrict__ exact,
                double *__restrict__ partial) {
  typedef IntegCfg<DIM, P> C;
  constexpr int N1 = C::N1, NQ = C::NQ, NPE = C::NPE, NQD = C::NQD, LPE = C::LPE, EB = C::EB;
  constexpr int M1 = NPE / N1;             // lines along direction 0 of one element
  constexpr int S1 = M1 * NQ;              // values of one element after direction 0
  constexpr int S2 = DIM == 3 ? N1 * NQ * NQ : 1;  // ... after direction 1 (3-D)
  __shared__ double sB[NQ * N1], sg[NQ], sw[NQ];
  __shared__ double su[EB * NPE], s1[EB * S1], s2[EB * S2], sW[EB * NQD];
  __shared__ double sacc[INTEG_ROWS * EB * 2];
  const int lane = threadIdx.x, seg = lane / LPE, l = lane % LPE;
  for (int i = lane; i < NQ * N1; i += 64) sB[i] = tab.B[i];
  if (lane < NQ) {
    sg[lane] = tab.g[lane];
    sw[lane] = tab.w[lane];
  }
  if (l == 0)
    for (int r = 0; r < nrows; r++) sacc[(r * EB + seg) * 2] = sacc[(r * EB + seg) * 2 + 1] = 0.0;
  const int e_begin = blockIdx.x * run, e_end = min(ne, e_begin + run);
  for (int e0 = e_begin; e0 < e_end; e0 += EB) {
    const int nb = min(EB, e_end - e0);  // elements of this batch
    __syncthreads();                     // the tables are in place; the last batch's weights have been read
    for (int idx = lane; idx < nb * NQD; idx += 64) {
      const int el = idx / NQD, q = idx % NQD;
      const int qi = q % NQ, qj = (q / NQ) % NQ, qk = q / (NQ * NQ);
      const double xi[3] = {sg[qi], sg[qj], sg[DIM == 3 ? qk : 0]};
      double x[DIM], det;
      quad_geometry<DIM>(verts + static_cast<int64_t>(e0 + el) * (1 << DIM) * DIM, xi, x, &det);
      double W = (DIM == 3 ? sw[qi] * sw[qj] * sw[qk] : sw[qi] * sw[qj]) * fabs(det);
      if (radial) W *= x[0];
      sW[idx] = W;
    }
    for (int r = 0; r < nrows; r++) {
      const double *u = field + r * ndofs + static_cast<int64_t>(e0) * NPE;
      __syncthreads();  // the last row's interpolation has read su, s1, s2 (and sW is written)
      for (int idx = lane; idx < nb * NPE; idx += 64) su[idx] = u[idx];
      __syncthreads();
      for (int idx = lane; idx < nb * S1; idx += 64) {  // direction 0: s1[el][m][q] = sum_a B[q][a] u[el][m][a]
        const int q = idx % NQ, m = idx / NQ;          // m: element and line
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < N1; a++) s += sB[q * N1 + a] * su[m * N1 + a];
        s1[idx] = s;
      }
      __syncthreads();
      if constexpr (DIM == 3) {
        for (int idx = lane; idx < nb * S2; idx += 64) {  // direction 1: s2[el][c][qj][qi] = sum_b B[qj][b] s1[el][c][b][qi]
          const int qi = idx % NQ, qj = (idx / NQ) % NQ, ec = idx / (NQ * NQ);  // ec: element and plane
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < N1; b++) s += sB[qj * N1 + b] * s1[(ec * N1 + b) * NQ + qi];
          s2[idx] = s;
        }
        __syncthreads();
      }
      // the last direction, at the points of this lane's element; lanes without an element carry zeros through the butterfly
      double t1 = 0.0, t2 = 0.0;
      if (seg < nb) {
        const double *ex = exact ? exact + r * npts + static_cast<int64_t>(e0 + seg) * NQD : nullptr;
        for (int q = l; q < NQD; q += LPE) {
          const int qi = q % NQ, qj = (q / NQ) % NQ;
          double v = 0.0;
          if constexpr (DIM == 3) {
            const int qk = q / (NQ * NQ);
#pragma unroll
            for (int c = 0; c < N1; c++) v += sB[qk * N1 + c] * s2[((seg * N1 + c) * NQ + qj) * NQ + qi];
          } else {
#pragma unroll
            for (int b = 0; b < N1; b++) v += sB[qj * N1 + b] * s1[(seg * N1 + b) * NQ + qi];
          }
          const double g = ex ? v - ex[q] : v;
          const double wg = sW[seg * NQD + q] * g;
          t1 += wg;
          t2 += wg * g;
        }
      }
#pragma unroll
      for (int off = LPE / 2; off > 0; off >>= 1) {
        t1 += __shfl_xor(t1, off, 64);
        t2 += __shfl_xor(t2, off, 64);
      }
      if (l == 0) {  // this lane alone touches its entries: no barrier
        sacc[(r * EB + seg) * 2] += t1;
        sacc[(r * EB + seg) * 2 + 1] += t2;
      }
    }
  }
  if (l == 0) {
    const int64_t np = static_cast<int64_t>(gridDim.x) * EB, at = static_cast<int64_t>(blockIdx.x) * EB + seg;
    for (int r = 0; r < nrows; r++) {
      partial[(r * 2) * np + at] = sacc[(r * EB + seg) * 2];
      partial[(r * 2 + 1) * np + at] = sacc[(r * EB + seg) * 2 + 1];
    }
  }
}

// One block: out_k[r] = the sum of partial[r][k][0 .. np), in a fixed order -- thread t adds the entries t, t + BLOCK, ... in
// ascending order, a butterfly adds the 64 lanes of a wave, and one thread adds the waves' sums in ascending order; NULL
// outputs are skipped.  No barrier inside the loop over the sums: their loads follow each other without waiting (a partial
// is read once, and the block is alone on the device: its time is load latency).
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_integrate_final(int nrows, int64_t np, const double *__restrict__ partial, double *__restrict__ sum_out,
                      double *__restrict__ sumsq_out) {
  constexpr int NW = BLOCK / 64;
  __shared__ double red[2 * INTEG_ROWS][NW];
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  for (int pair = 0; pair < 2 * nrows; pair++) {
    if (!((pair & 1) ? sumsq_out : sum_out)) continue;
    const double *p = partial + pair * np;
    double s = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < np; i += BLOCK) s += p[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red[pair][wave] = s;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < 2 * nrows) {
    const int pair = threadIdx.x;
    double *out = (pair & 1) ? sumsq_out : sum_out;
    if (out) {
      double s = 0.0;
      for (int w = 0; w < NW; w++) s += red[pair][w];
      out[pair >> 1] = s;
    }
  }
}

// partial: [gridDim.y][3][gridDim.x * (64 / lpe)] = min, max, sum |f| of each segment's elements; blockIdx.y: the row
__global__ void __launch_bounds__(64)
    k_nodal_stats(int ne, int run, int npe, int lpe, int64_t ndofs, const double *__restrict__ field,
                  double *__restrict__ partial) {
  const int lane = threadIdx.x, seg = lane / lpe, l = lane % lpe, eb = 64 / lpe;
  const double *f = field + blockIdx.y * ndofs;
  const int e_begin = blockIdx.x * run, e_end = min(ne, e_begin + run);
  double mn = INFINITY, mx = -INFINITY, acc = 0.0;
  constexpr int UNR = 4;  // batches in flight: their loads and their butterflies overlap
  for (int e0 = e_begin; e0 < e_end; e0 += UNR * eb) {
    double t[UNR] = {};
#pragma unroll
    for (int k = 0; k < UNR; k++) {
      const int e = e0 + k * eb + seg;
      if (e < e_end) {
        const double *u = f + static_cast<int64_t>(e) * npe;
        for (int n = l; n < npe; n += lpe) {
          const double v = u[n];
          if (v < mn) mn = v;
          if (v > mx) mx = v;
          t[k] += fabs(v);
        }
      }
    }
    for (int off = lpe / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < UNR; k++) t[k] += __shfl_xor(t[k], off, 64);
    }
#pragma unroll
    for (int k = 0; k < UNR; k++) acc += t[k];  // each element's sum first, then onto the elements before it, in order
  }
  for (int off = lpe / 2; off > 0; off >>= 1) {
    const double a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
    if (a < mn) mn = a;
    if (b > mx) mx = b;
  }
  if (l == 0) {
    const int64_t np = static_cast<int64_t>(gridDim.x) * eb, at = static_cast<int64_t>(blockIdx.x) * eb + seg;
    double *p = partial + static_cast<int64_t>(blockIdx.y) * 3 * np;
    p[at] = mn;
    p[np + at] = mx;
    p[2 * np + at] = acc;
  }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_nodal_stats_final(int nrows, int64_t np, int64_t ndofs, const double *__restrict__ partial, double *__restrict__ min_out,
                        double *__restrict__ max_out, double *__restrict__ meanabs_out) {
#pragma clang fp reciprocal(off)  // the mean is an IEEE division, whatever the unit switched on before
  constexpr int NW = BLOCK / 64;  // the structure of k_integrate_final
  __shared__ double rmn[INTEG_ROWS][NW], rmx[INTEG_ROWS][NW], rs[INTEG_ROWS][NW];
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  for (int r = 0; r < nrows; r++) {
    const double *p = partial + static_cast<int64_t>(r) * 3 * np;
    double mn = INFINITY, mx = -INFINITY, s = 0.0;
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < np; i += BLOCK) {
      const double a = p[i], b = p[np + i];
      if (a < mn) mn = a;
      if (b > mx) mx = b;
      s += p[2 * np + i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
      if (a < mn) mn = a;
      if (b > mx) mx = b;
      s += __shfl_xor(s, off, 64);
    }
    if (lane == 0) {
      rmn[r][wave] = mn;
      rmx[r][wave] = mx;
      rs[r][wave] = s;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < nrows) {
    const int r = threadIdx.x;
    double mn = INFINITY, mx = -INFINITY, s = 0.0;
    for (int w = 0; w < NW; w++) {
      if (rmn[r][w] < mn) mn = rmn[r][w];
      if (rmx[r][w] > mx) mx = rmx[r][w];
      s += rs[r][w];
    }
    if (min_out) min_out[r] = mn;
    if (max_out) max_out[r] = mx;
    if (meanabs_out) meanabs_out[r] = s / static_cast<double>(ndofs);
  }
}

}  // namespace tpsrhs
#endif
