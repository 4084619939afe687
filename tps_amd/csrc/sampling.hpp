// Values of a byNODES DG field at arbitrary points, and probe records taken inside the device time loop: what the reference
// does with gslib (FindPointsGSLIB::Interpolate, src/gslib_interpolator.cpp:69-84) for its plane dump
// (the planeDump block of M2ulPhyS::solveStep, src/M2ulPhyS.cpp:2052-2096).  Included by sampling.hip only: the kernel families do not see it.
// The host half -- which element holds a point, and where in it -- is point_locate.hpp.
//
// A field value at a point of element e with reference coordinates xi in [0,1]^dim is
//   u(xi) = sum_{i,j,k} l_i(xi_0) l_j(xi_1) l_k(xi_2) u[e * (p+1)^dim + i + j (p+1) + k (p+1)^2]
// with l_a the Lagrange polynomials on the operator's p + 1 nodes (Gauss-Legendre or Gauss-Lobatto on [0,1]),
//   l_a(t) = prod_{j != a} (t - x_j) / (x_a - x_j)         -- a product of p quotients, as basis.hpp::lagrange forms it.
#ifndef TPSRHS_SAMPLING_HPP_
#define TPSRHS_SAMPLING_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/tpsrhs.h"
#include "device_buffer.hpp"
#include "point_locate.hpp"
#include "record_log.hpp"

struct tpsrhs_operator;

// behind tpsrhs_sampler_handle; owned by its operator (tpsrhs_sampling_state::samplers)
struct tpsrhs_sampler {
  tpsrhs_operator *owner = nullptr;
  int64_t npts = 0, nfound = 0;
  double fill = 0.0;
  std::vector<int32_t> elem;  // [npts], the caller's order; -1: not found
  std::vector<double> ref;    // [dim][npts], the caller's order
  // device, SORTED by element (the points that were not found last): neighbouring lanes read the same element
  DevBuf<int32_t> d_elem;  // [npts]
  DevBuf<double> d_ref;    // [dim][npts]
  DevBuf<int64_t> d_perm;  // [npts] sorted position -> the caller's index
  // tpsrhs_sampler_create_device: located by k_locate (locate_device.hpp), in the caller's order (d_perm is the identity);
  // nfound, elem and ref above are copied from the device the first time they are asked for
  bool on_device = false, host_valid = true;
  DevBuf<unsigned long long> d_nfound;
};

// one uploaded search grid (point_locate.hpp: LocateGrid) of the operator's mesh; the element boxes depend on the tolerance
struct tpsrhs_locate_grid_dev {
  double tol = 0.0;
  tpsrhs::LocateGrid host;  // the scalars; its vectors are emptied after the upload
  DevBuf<double> d_lo, d_hi;
  DevBuf<int64_t> d_start;
  DevBuf<int32_t> d_list;
};

// tpsrhs_transfer: the sampler on this operator (the source) at the nodes of `dst`
struct tpsrhs_transfer_entry {
  tpsrhs_operator *dst = nullptr;
  double tol = 0.0;
  tpsrhs_sampler *sampler = nullptr;
};

// the probe records (tpsrhs_probe_configure); sampler NULL: off
struct tpsrhs_probe_log {
  tpsrhs_sampler *sampler = nullptr;
  tpsrhs::StepCadence cadence;  // count: steps of tpsrhs_advance / tpsrhs_advance_with since tpsrhs_probe_configure
  tpsrhs::RecordIndex index;
  DevBuf<double> d_values;  // [capacity][neq][npts]
  DevBuf<double> d_times;   // [capacity], copied from d_ctl[1] on the stream
};

// behind tpsrhs_operator::sampling; created by sampling.hip, owned by the operator
struct tpsrhs_sampling_state {
  std::vector<std::unique_ptr<tpsrhs_sampler>> samplers;
  tpsrhs_probe_log probe;
  // device location (tpsrhs_sampler_create_device): one grid per tolerance, uploaded at first use
  std::vector<std::unique_ptr<tpsrhs_locate_grid_dev>> grids;
  // tpsrhs_transfer with this operator as the source: one sampler per (dst, tol), and how often it was made / found
  std::vector<tpsrhs_transfer_entry> transfers;
  int64_t num_located = 0, num_cache_hits = 0;
};

namespace tpsrhs {

struct SampleNodes {
  double x[TPSRHS_MAXORDER + 1];  // the operator's 1-D nodes on [0,1]
};

// One lane per point, in the sorted order.  The lane forms its DIM x (P + 1) Lagrange values once, in registers (every loop
// is unrolled: no register array is indexed at run time), and reuses them over the rows; per row it reads the (P + 1)^DIM
// nodal values of its element -- the same addresses as the neighbouring lanes of that element, so one fetch serves them --
// and writes one value at the caller's index.  No LDS, no atomics.  A point that was not found writes `fill` and reads
// nothing.  The DIM (P + 1) P divisions per point are negligible next to the nrows (P + 1)^DIM loads.
template <int DIM, int P, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_sample(int64_t npts, int nrows, int64_t ndofs, SampleNodes nodes, const int32_t *__restrict__ elem,
             const double *__restrict__ ref, const int64_t *__restrict__ perm, double fill, const double *__restrict__ field,
             double *__restrict__ out) {
#pragma clang fp reciprocal(off)  // the quotients of the weights are IEEE divisions, whatever the unit switched on before
  constexpr int N1 = P + 1;
  constexpr int NPE = DIM == 3 ? N1 * N1 * N1 : N1 * N1;
  const int64_t i = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
  if (i >= npts) return;
  const int e = elem[i];
  double *o = out + perm[i];
  if (e < 0) {
    for (int r = 0; r < nrows; r++) o[r * npts] = fill;
    return;
  }
  double w[DIM][N1];
#pragma unroll
  for (int d = 0; d < DIM; d++) {
    const double t = ref[i + d * npts];
#pragma unroll
    for (int a = 0; a < N1; a++) {
      double v = 1.0;
#pragma unroll
      for (int j = 0; j < N1; j++)
        if (j != a) v *= (t - nodes.x[j]) / (nodes.x[a] - nodes.x[j]);
      w[d][a] = v;
    }
  }
  const double *u = field + static_cast<int64_t>(e) * NPE;
  for (int r = 0; r < nrows; r++, u += ndofs) {
    double s = 0.0;
    if constexpr (DIM == 3) {
#pragma unroll
      for (int c = 0; c < N1; c++) {
        double sc = 0.0;
#pragma unroll
        for (int b = 0; b < N1; b++) {
          double sb = 0.0;
#pragma unroll
          for (int a = 0; a < N1; a++) sb += w[0][a] * u[a + N1 * (b + N1 * c)];
          sc += w[1][b] * sb;
        }
        s += w[2][c] * sc;
      }
    } else {
#pragma unroll
      for (int b = 0; b < N1; b++) {
        double sb = 0.0;
#pragma unroll
        for (int a = 0; a < N1; a++) sb += w[0][a] * u[a + N1 * b];
        s += w[1][b] * sb;
      }
    }
    o[r * npts] = s;
  }
}

}  // namespace tpsrhs
#endif
