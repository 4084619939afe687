// The arithmetic probes of libtpsrhs.so (include/tpsrhs.h): tpsrhs_math_eval (fastmath.hpp), tpsrhs_coulomb_eval (the
// routes of the Coulomb fits, coulomb_table.hpp) and tpsrhs_table_eval (LinearTable on the device).  They take no operator
// and run on the NULL stream of the current device.
#include "abi_support.hpp"
#include "operator_plan.hpp"  // check_table2d
#include "physics_plasma.hpp"
#include "table2d.hpp"

#include <algorithm>

namespace {
extern "C" {  // the three older probes keep the plain names profilers and the device-code comparison know them by
__global__ void k_table_eval(TableDev t, int64_t n, const double *__restrict__ x, double *__restrict__ f) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) f[i] = table_eval(t, x[i]);
}

__global__ void k_math_eval(int fn, int64_t n, const double *__restrict__ x, double *__restrict__ y) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  switch (fn) {
    case 0: r = fexp(v); break;
    case 1: r = fexp<false>(v); break;
    case 2: r = flog(v); break;
    case 3: r = flog_pos(v); break;
    case 4: r = fast_rcp(v); break;
    case 5: r = fast_sqrt(v); break;
    default: r = fast_rsqrt(v); break;
  }
  y[i] = r;
}

// route 0: cfit_n; 1: the table with two wave-uniform rounds, then lane by lane; 2: lane by lane only.  1 / Tp^2 = 1.
__global__ void k_coulomb_eval(int route, const double *tab, int64_t n, const double *__restrict__ x, double *__restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  coll::Arg a;
  a.ln = x[i];
  a.inv2 = 1.0;
  double g[8];
  if (route == 0 || !coulomb::in_range(a.ln)) {
    coll::cfit_tab<8>(nullptr, a, g);
  } else if (route == 1) {
    coll::ctab_eval<8, 2>(tab, a.ln, true, g);
  } else {
    coll::ctab_eval<8, 0>(tab, a.ln, true, g);
  }
#pragma unroll
  for (int f = 0; f < 8; f++) out[f * n + i] = g[f];
}
}  // extern "C"

// Route 3, the LDS window of a wave.  COULOMB_PROBE_BLOCKS one-wave blocks stride over the chunks of 64 arguments -- chunk c
// goes to block c % COULOMB_PROBE_BLOCKS -- so that a wave evaluates several chunks in sequence and carries its window from
// one to the next.  1 / Tp^2 = 1.
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

extern "C" {

int tpsrhs_math_eval(int function, int64_t n, const double *x, double *y) {
  if (function < 0 || function > 6 || n < 0 || !x || !y) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "math_eval");
  return guarded([&] {
    require_device();
    if (n > 0) {
      hipLaunchKernelGGL(k_math_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, function, n, x, y);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int tpsrhs_coulomb_eval(int route, int64_t n, const double *x, double *out) {
  if (route < 0 || route > 3 || n < 0 || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "coulomb_eval");
  return guarded([&] {
    require_device();
    DevBuf<double> tab(coulomb_table_host());  // its own table, from the same fill as an operator's
    if (n > 0 && route == 3) {
      const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((n + 63) / 64, COULOMB_PROBE_BLOCKS));
      hipLaunchKernelGGL(k_coulomb_eval_window, dim3(blocks), dim3(64), 0, nullptr, tab.get(), n, x, out);
      HIP_CHECK(hipGetLastError());
    } else if (n > 0) {
      hipLaunchKernelGGL(k_coulomb_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, route, tab.get(), n, x, out);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int tpsrhs_table_eval(const tpsrhs_table *table, int64_t n, const double *x, double *f) {
  if (!table || n < 0 || !x || !f) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "table_eval");
  return guarded([&] {
    require_device();
    std::vector<DevBuf<void>> owner;  // the device copy of the table, for the duration of the call
    const TableDev td = upload_table(owner, *table);
    if (n > 0) {
      hipLaunchKernelGGL(k_table_eval, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, td, n, x, f);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipDeviceSynchronize());
  });
}

// GslTableInterpolator2D::eval / eval_x / eval_y with the bilinear interpolant (src/table.cpp:262-300), on the host: the text
// of table2d.hpp the kernels of the two-dimensional table gas run
int tpsrhs_table2d_eval(const tpsrhs_table2d *table, int what, int64_t n, const double *x, const double *y, double *out) {
  if (!table || n < 0 || !x || !y || !out || what < 0 || what > 2) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "table2d_eval");
  return guarded([&] {
    check_table2d(*table, "tpsrhs_table2d_eval");
    const Grid2Dev g = make_grid2d(*table, [](const void *src, size_t) { return src; });  // (the caller's axes, in place)
    const std::vector<BilinearCell> cells = make_cells(*table);
    for (int64_t i = 0; i < n; i++) out[i] = table2d_at(g, cells.data(), x[i], y[i], what);
  });
}

}  // extern "C"
