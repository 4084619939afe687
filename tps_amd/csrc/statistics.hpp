// Running mean of the primitive state and running velocity covariances (the reference's "rms" field): what
// Averaging::addSample computes once per sampled iteration of the time loop (src/M2ulPhyS.cpp:2099;
// src/averaging.cpp:198-234 the sampling condition and the counters, :331-435 the update), stored by the reference as
// /meanSolution and /rmsData.  Included by statistics.hip only: the kernel families do not see it.
//
// State: mean[neq][ndofs] in the layout of x (byNODES); vari[nvar][ndofs], nvar = nvel (nvel + 1) / 2, the diagonal first,
// then the pairs i < j in row-major order -- uu vv ww uv uw vw for three velocity components, uu vv uv for two
// (src/M2ulPhyS.cpp:665-675); the counters ns_mean and ns_vari, kept apart because restartRMS zeroes one and not the other.
//
// One sample of a state x: s = prim(x) with the temperature row replaced by the pressure, then per node
//   mean = (ns_mean * mean + s) / (ns_mean + 1)                          every row
//   vari = (vari * ns_vari + d_i d_j) / (ns_vari + 1),  d_i = s_i - mean_i  with the UPDATED mean, velocity rows only
// and both counters go up by one.  This is the reference's recurrence, not the textbook variance: two samples a, b give
// (b - a)^2 / 8.  The quotients are multiplications by the reciprocal of the divisor (TPSRHS_RECIPROCAL_DIVISION in both
// functions below): what the library has always been compiled to, a rounding away from a restatement that divides
// (DESIGN.md section 9 keeps the IEEE form as an open decision).  A field whose counter is 0 counts as zero whatever it
// holds (addSample zeroes it first: 0 * NaN would be NaN).
//
// Two deliberate differences from the reference:
//  (a) The reference samples the grid function Up, which holds the primitives of the input of the step's LAST Mult
//      (updatePrimitives is called from Mult): a stage state.  Here the primitives of the NEW x are sampled, after the NaN
//      census and the species clamp -- what the statistic is meant to be, whatever the integrator.
//  (b) The reference replaces row 1 + dim by the pressure (src/averaging.cpp:390-398), which in the axisymmetric
//      formulation (dim = 2, three velocity components) is the swirl velocity.  Here it is the temperature row, 1 + nvel, in
//      every formulation.
#ifndef TPSRHS_STATISTICS_HPP_
#define TPSRHS_STATISTICS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buffer.hpp"
#include "division_mode.hpp"
#include "record_log.hpp"

// behind tpsrhs_operator::stats (tpsrhs_stats_configure); created by statistics.hip, owned by the operator
struct tpsrhs_stats_state {
  // interval, start: the reference's sampleFreq and startIter; count: the steps taken by tpsrhs_advance /
  // tpsrhs_advance_with (+ tpsrhs_stats_set_iter)
  tpsrhs::StepCadence cadence;
  int ns_mean = 0, ns_vari = 0;
  int nvar = 0;  // 0: no covariances
  DevBuf<double> d_mean, d_vari;
  DevBuf<double> d_scratch;  // [neq + 1][ndofs]: the primitives and the pressure of the sampled state
};

namespace tpsrhs {

// One node.  prim, mean, vari point at the node's entry of row 0, rows are `n` apart; sp is the node's pressure.
template <int NVEL, bool VARI>
__device__ __forceinline__ void stats_node(int neq, int64_t n, double nm, double nv, bool mean_is_zero, bool vari_is_zero,
                                           const double *__restrict__ prim, double sp, double *__restrict__ mean,
                                           double *__restrict__ vari) {
  TPSRHS_RECIPROCAL_DIVISION
  auto update = [&](int r, double s) {
    const double m = mean_is_zero ? 0.0 : mean[r * n];
    const double mn = (nm * m + s) / (nm + 1.0);
    mean[r * n] = mn;
    return mn;
  };
  update(0, prim[0]);
  double d[NVEL];
#pragma unroll
  for (int i = 0; i < NVEL; i++) {
    const double s = prim[(1 + i) * n];
    d[i] = s - update(1 + i, s);
  }
  update(1 + NVEL, sp);
  for (int r = 2 + NVEL; r < neq; r++) update(r, prim[r * n]);
  if constexpr (VARI) {
    auto cov = [&](int row, double dd) {
      const double v = vari_is_zero ? 0.0 : vari[row * n];
      vari[row * n] = (v * nv + dd) / (nv + 1.0);
    };
    int row = 0;
#pragma unroll
    for (int i = 0; i < NVEL; i++) cov(row++, d[i] * d[i]);
#pragma unroll
    for (int i = 0; i < NVEL - 1; i++)
#pragma unroll
      for (int j = i + 1; j < NVEL; j++) cov(row++, d[i] * d[j]);
  }
}

// A streaming pass over the nodes, written like k_rk_stage (time_integrators.hpp): no LDS, no atomics, the counters by value.
// Reads neq rows of prim (the temperature row is not read: the pressure takes its place) and p, reads and writes mean and
// vari.  VEC: ndofs is even and every array is 16-byte aligned (the host checks), so every row is: a lane moves two nodes
// per access.  An odd ndofs leaves every other row on an odd 8-byte offset: the scalar form.
template <int NVEL, bool VARI, bool VEC, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_stats_sample(int neq, int64_t n, int ns_mean, int ns_vari, const double *__restrict__ prim, const double *__restrict__ p,
                   double *__restrict__ mean, double *__restrict__ vari) {
  TPSRHS_RECIPROCAL_DIVISION
  const double nm = static_cast<double>(ns_mean), nv = static_cast<double>(ns_vari);
  const bool mz = ns_mean == 0, vz = ns_vari == 0;
  const int64_t first = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x, stride = static_cast<int64_t>(gridDim.x) * BLOCK;
  if constexpr (VEC) {
    const int64_t npairs = n >> 1;  // n is even
    auto row2 = [&](const double *a, int r, int64_t j) { return reinterpret_cast<const double2 *>(a + r * n)[j]; };
    auto put2 = [&](double *a, int r, int64_t j, double2 v) { reinterpret_cast<double2 *>(a + r * n)[j] = v; };
    for (int64_t j = first; j < npairs; j += stride) {
      auto update = [&](int r, double2 s) {
        double2 m = make_double2(0.0, 0.0);
        if (!mz) m = row2(mean, r, j);
        m.x = (nm * m.x + s.x) / (nm + 1.0);
        m.y = (nm * m.y + s.y) / (nm + 1.0);
        put2(mean, r, j, m);
        return m;
      };
      update(0, row2(prim, 0, j));
      double2 d[NVEL];
#pragma unroll
      for (int i = 0; i < NVEL; i++) {
        const double2 s = row2(prim, 1 + i, j);
        const double2 m = update(1 + i, s);
        d[i] = make_double2(s.x - m.x, s.y - m.y);
      }
      update(1 + NVEL, reinterpret_cast<const double2 *>(p)[j]);
      for (int r = 2 + NVEL; r < neq; r++) update(r, row2(prim, r, j));
      if constexpr (VARI) {
        auto cov = [&](int row, double2 dd) {
          double2 v = make_double2(0.0, 0.0);
          if (!vz) v = row2(vari, row, j);
          v.x = (v.x * nv + dd.x) / (nv + 1.0);
          v.y = (v.y * nv + dd.y) / (nv + 1.0);
          put2(vari, row, j, v);
        };
        int row = 0;
#pragma unroll
        for (int i = 0; i < NVEL; i++) cov(row++, make_double2(d[i].x * d[i].x, d[i].y * d[i].y));
#pragma unroll
        for (int i = 0; i < NVEL - 1; i++)
#pragma unroll
          for (int k = i + 1; k < NVEL; k++) cov(row++, make_double2(d[i].x * d[k].x, d[i].y * d[k].y));
      }
    }
  } else {
    for (int64_t i = first; i < n; i += stride)
      stats_node<NVEL, VARI>(neq, n, nm, nv, mz, vz, prim + i, p[i], mean + i, VARI ? vari + i : nullptr);
  }
}

}  // namespace tpsrhs
#endif
