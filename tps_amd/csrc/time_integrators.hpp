// The stage combinations of the reference's other explicit integrators (src/M2ulPhyS.cpp:721-739, 2722-2736: MFEM's
// ForwardEulerSolver, RK2Solver(1.0) and RK3SSPSolver [third party: MFEM >= 4.4, linalg/ode.cpp]) around the plain Mult.
// With them the kernels of the loop itself: RK4's stage pass (the form without the fusion into k_flux), the end of a step
// and the reduction of the per-block maximum speeds.  Included by time_loop.hip and, for k_reduce_max, by tpsrhs.hip: the
// kernel families do not see it.
#ifndef TPSRHS_TIME_INTEGRATORS_HPP_
#define TPSRHS_TIME_INTEGRATORS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "division_mode.hpp"

namespace tpsrhs {

// One stage combination = one pass over the state.  In MFEM's order of operations, k = f(.) being the Mult before the pass:
//   forward Euler   k = f(x);  x = x + dt*k                                              RK_EULER
//   RK2(a = 1)      k = f(x);  x1 = x + (dt/2)*k;  y = x + dt*k                          RK2_STAGE1 (x1 takes x's place)
//                   k = f(y);  x = x1 + (dt/2)*k                                         RK2_STAGE2
//   RK3-SSP         k = f(x);  y = x + dt*k                                              RK3_STAGE1
//                   k = f(y);  y = y + dt*k;  y = (3/4)*x + (1/4)*y                      RK3_STAGE2
//                   k = f(y);  y = y + dt*k;  x = (1/3)*x + (2/3)*y                      RK3_STAGE3
// State vectors read + written per step: 3 (Euler), 4 + 3 (RK2), 3 + 4 + 4 (RK3).  Nothing is written that the next stage
// does not read; RK2's x1 is only ever read by the stage that turns it into the new x, so it lives in x.
enum RkOp { RK_EULER = 0, RK2_STAGE1, RK2_STAGE2, RK3_STAGE1, RK3_STAGE2, RK3_STAGE3 };

template <int OP>
struct RkOpTraits {
  static constexpr bool reads_y = (OP == RK3_STAGE2 || OP == RK3_STAGE3);
  static constexpr bool writes_y = (OP == RK2_STAGE1 || OP == RK3_STAGE1 || OP == RK3_STAGE2);
  static constexpr bool writes_x = (OP == RK_EULER || OP == RK2_STAGE1 || OP == RK2_STAGE2 || OP == RK3_STAGE3);
  static constexpr bool last = (OP == RK_EULER || OP == RK2_STAGE2 || OP == RK3_STAGE3);  // the step's final state
};

template <int OP>
__device__ __forceinline__ void rk_combine(double dt, double &x, double k, double &y) {
  TPSRHS_RECIPROCAL_DIVISION
  if constexpr (OP == RK_EULER) {
    x = x + dt * k;
  } else if constexpr (OP == RK2_STAGE1) {
    y = x + dt * k;
    x = x + (dt / 2) * k;
  } else if constexpr (OP == RK2_STAGE2) {
    x = x + (dt / 2) * k;
  } else if constexpr (OP == RK3_STAGE1) {
    y = x + dt * k;
  } else if constexpr (OP == RK3_STAGE2) {
    y = (3.0 / 4.0) * x + (1.0 / 4.0) * (y + dt * k);
  } else {
    x = (1.0 / 3.0) * x + (2.0 / 3.0) * (y + dt * k);
  }
}

// Check_NAN, then Check_Undershoot (src/M2ulPhyS.cpp:2463-2548) on entry i of the step's final state.  The species rows
// [sp_first, sp_last) of the [neq][ndofs] state are the contiguous entries [clamp_lo, clamp_hi): two comparisons, no division.
__device__ __forceinline__ double rk_final_entry(double v, int64_t i, int64_t clamp_lo, int64_t clamp_hi, unsigned long long &bad) {
  if (v != v) bad++;
  if (i >= clamp_lo && i < clamp_hi) v = fmax(v, 0.0);
  return v;
}

// VEC: every vector is 16-byte aligned (the host checks), a lane moves two entries per access and lane 0 of the grid
// takes the last entry of an odd length.  dt by value, or from device memory inside tpsrhs_advance_with (dt_dev).
template <int OP, bool VEC, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_rk_stage(int64_t n, int64_t clamp_lo, int64_t clamp_hi, double dt_host, const double *__restrict__ dt_dev,
               double *__restrict__ x, const double *__restrict__ k, double *__restrict__ y,
               unsigned long long *__restrict__ nan_count) {
  typedef RkOpTraits<OP> T;
  const double dt = dt_dev ? *dt_dev : dt_host;
  unsigned long long bad = 0;
  const int64_t first = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x, stride = static_cast<int64_t>(gridDim.x) * BLOCK;
  auto entry = [&](int64_t i) {
    double xi = x[i], yi = 0.0;
    if constexpr (T::reads_y) yi = y[i];
    rk_combine<OP>(dt, xi, k[i], yi);
    if constexpr (T::last) xi = rk_final_entry(xi, i, clamp_lo, clamp_hi, bad);
    if constexpr (T::writes_y) y[i] = yi;
    if constexpr (T::writes_x) x[i] = xi;
  };
  if constexpr (VEC) {
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    double2 *__restrict__ y2 = reinterpret_cast<double2 *>(y);
    const double2 *__restrict__ k2 = reinterpret_cast<const double2 *>(k);
    const int64_t npairs = n >> 1;
    for (int64_t j = first; j < npairs; j += stride) {
      double2 xv = x2[j], yv = make_double2(0.0, 0.0);
      const double2 kv = k2[j];
      if constexpr (T::reads_y) yv = y2[j];
      rk_combine<OP>(dt, xv.x, kv.x, yv.x);
      rk_combine<OP>(dt, xv.y, kv.y, yv.y);
      if constexpr (T::last) {
        xv.x = rk_final_entry(xv.x, 2 * j, clamp_lo, clamp_hi, bad);
        xv.y = rk_final_entry(xv.y, 2 * j + 1, clamp_lo, clamp_hi, bad);
      }
      if constexpr (T::writes_y) y2[j] = yv;
      if constexpr (T::writes_x) x2[j] = xv;
    }
    if ((n & 1) && first == 0) entry(n - 1);
  } else {
    for (int64_t i = first; i < n; i += stride) entry(i);
  }
  if constexpr (T::last) {
    if (bad) atomicAdd(nan_count, bad);
  }
}

// One block reduces the 50 176 per-block maxima of cfg2: a lane's loads must not wait for each other (round 2: one
// dependent load per iteration, 196 iterations of a full memory latency = 75 us per call of the time loop's k_step_end)
template <int BLOCK>
__device__ inline double strided_max(int n, const double *__restrict__ v) {
  constexpr int UN = 8;
  double m[UN];
#pragma unroll
  for (int u = 0; u < UN; u++) m[u] = 0.0;
  int i = threadIdx.x;
  for (; i + (UN - 1) * BLOCK < n; i += UN * BLOCK) {
    double t[UN];
#pragma unroll
    for (int u = 0; u < UN; u++) t[u] = v[i + u * BLOCK];  // UN independent loads in flight
#pragma unroll
    for (int u = 0; u < UN; u++) m[u] = fmax(m[u], t[u]);
  }
  for (; i < n; i += BLOCK) m[0] = fmax(m[0], v[i]);
#pragma unroll
  for (int u = 1; u < UN; u++) m[0] = fmax(m[0], m[u]);
  return m[0];
}

// max over the per-block maxima written by k_flux (one block)
template <int BLOCK>
__global__ void k_reduce_max(int n, const double *__restrict__ v, double *__restrict__ out) {
  __shared__ double s[BLOCK];
  const double m = strided_max<BLOCK>(n, v);
  s[threadIdx.x] = m;
  __syncthreads();
  for (int off = BLOCK / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s[0];
}

// =============================================================================================
// RK4 stage combinations (MFEM RK4Solver::Step) as one streaming pass per stage:
//   stage 1: y = x + dt/2 k, z = x + dt/6 k     stage 2: y = x + dt/2 k, z += dt/3 k
//   stage 3: y = x + dt k,   z += dt/3 k        stage 4: x = z + dt/6 k (+ NaN census, species clamp)
// =============================================================================================
template <int BLOCK>
__global__ void k_rk4_stage(int stage, int64_t n, int64_t ndofs, int sp_first, int sp_last, double dt_host,
                            const double *__restrict__ dt_dev, double *__restrict__ x, const double *__restrict__ k,
                            double *__restrict__ y, double *__restrict__ z, unsigned long long *__restrict__ nan_count) {
  TPSRHS_IEEE_DIVISION
  const double dt = dt_dev ? *dt_dev : dt_host;  // tpsrhs_advance keeps dt in device memory
  unsigned long long bad = 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * BLOCK) {
    const double ki = k[i];
    if (stage == 1) {
      const double xi = x[i];
      y[i] = xi + (dt / 2) * ki;
      z[i] = xi + (dt / 6) * ki;
    } else if (stage == 2) {
      y[i] = x[i] + (dt / 2) * ki;
      z[i] += (dt / 3) * ki;
    } else if (stage == 3) {
      y[i] = x[i] + dt * ki;
      z[i] += (dt / 3) * ki;
    } else {
      double v = z[i] + (dt / 6) * ki;
      if (v != v) bad++;
      const int64_t eq = i / ndofs;
      if (eq >= sp_first && eq < sp_last) v = fmax(v, 0.0);  // Check_Undershoot
      x[i] = v;
    }
  }
  if (stage == 4 && bad) atomicAdd(nan_count, bad);
}

// End of a step of tpsrhs_advance (src/M2ulPhyS.cpp:2004-2016): time += dt; with a variable time step
// dt = CFL hmin / max_char_speed / dim from the per-block maxima the last k_flux left.  ctl = {dt, time, speed}.
template <int BLOCK>
__global__ void k_step_end(int n, const double *__restrict__ block_speed, double *__restrict__ ctl, int constant_dt,
                           double cfl_hmin_over_dim) {
  TPSRHS_IEEE_DIVISION
  __shared__ double s[BLOCK];
  const double m = strided_max<BLOCK>(n, block_speed);
  s[threadIdx.x] = m;
  __syncthreads();
  for (int off = BLOCK / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl[1] += ctl[0];
    ctl[2] = s[0];
    if (!constant_dt) ctl[0] = cfl_hmin_over_dim / s[0];
  }
}

}  // namespace tpsrhs
#endif
