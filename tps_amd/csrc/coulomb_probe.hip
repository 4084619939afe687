// The probe of the Coulomb table's LDS window (tpsrhs_coulomb_eval, route 3; include/tpsrhs.h): part of the core library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "physics_plasma.hpp"

using namespace tpsrhs;

namespace {
// COULOMB_PROBE_BLOCKS one-wave blocks stride over the chunks of 64 arguments -- chunk c goes to block c % COULOMB_PROBE_BLOCKS --
// so that a wave evaluates several chunks in sequence and carries its window from one to the next.  1 / Tp^2 = 1.
constexpr int COULOMB_PROBE_BLOCKS = 4;
__global__ __launch_bounds__(64) void k_coulomb_eval_window(const double *tab, int64_t n, const double *__restrict__ x,
                                                            double *__restrict__ out) {
  typedef coll::Window<TPSRHS_COULOMB_WINDOW_W> Win;
  __shared__ __attribute__((aligned(16))) double mem[Win::DOUBLES];
  Win win;
  win.create(mem, true);
  for (int64_t c0 = static_cast<int64_t>(blockIdx.x) * 64; c0 < n; c0 += static_cast<int64_t>(gridDim.x) * 64) {
    const int64_t i = c0 + threadIdx.x;
    if (i < n) {
      coll::Arg a;
      a.ln = x[i];
      a.inv2 = 1.0;
      double g[8];
      coll::cfit_tab<8>(tab, a, g, win);
#pragma unroll
      for (int f = 0; f < 8; f++) out[f * n + i] = g[f];
    }
  }
}
}  // namespace

// n > 0; tab, x, out: device pointers; the caller checks hipGetLastError and synchronises
void coulomb_probe_window(const double *tab, int64_t n, const double *x, double *out) {
  hipLaunchKernelGGL(k_coulomb_eval_window, dim3(static_cast<unsigned>(std::min<int64_t>((n + 63) / 64, COULOMB_PROBE_BLOCKS))),
                     dim3(64), 0, nullptr, tab, n, x, out);
}
