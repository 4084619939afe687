// Restart of a species plasma from an LTE solution on the device (include/tpsrhs.h: tpsrhs_lte_composition,
// tpsrhs_species_from_lte; lte_restart.hpp is the text of both routines).  One lane per node, one kernel for every mixture:
// the species count is a run-time number.  The report is reduced without floating-point atomics, in the manner of
// integrals.hip: per-block partials in a fixed order, then one block over the partials.
#include "abi_support.hpp"
#include "lte_restart.hpp"
#include "time_integrators.hpp"

namespace {

constexpr int LTE_BLOCK = 256, LTE_MAXBLOCKS = 1024, LTE_REPORT = 5;

// the rows of one node in a byNODES vector [neq][ndofs]: consecutive lanes read consecutive entries of a row
struct NodeRows {
  double *p;
  int64_t stride;
  __device__ double &operator[](int k) const { return p[k * stride]; }
};
// up_out = NULL: the primitives go nowhere
struct NoRows {
  struct Sink {
    __device__ void operator=(double) const {}
  };
  __device__ Sink operator[](int) const { return Sink(); }
};

__global__ void __launch_bounds__(LTE_BLOCK)
    k_lte_composition(LteRestartParams P, int64_t n, const double *__restrict__ T, const double *__restrict__ p,
                      double *__restrict__ n_sp_out) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(LTE_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * LTE_BLOCK) {
    double n_sp[LTE_MAXSP] = {};
    lte_composition(P, T[i], p[i], n_sp);
#pragma unroll
    for (int sp = 0; sp < LTE_MAXSP; sp++)
      if (sp < P.num_species) n_sp_out[sp * n + i] = n_sp[sp];
  }
}

// partial: [LTE_REPORT][gridDim.x] = nodes not converged, nodes invalid, max density change, min T, max T of each block
template <bool WRITE_UP>
__global__ void __launch_bounds__(LTE_BLOCK)
    k_species_from_lte(LteRestartParams P, LteRestartTables LT, int64_t ndofs, int sp_first, int sp_last, double *__restrict__ x,
                       double *__restrict__ up, double *__restrict__ partial) {
  double nnc = 0.0, ninv = 0.0, chg = 0.0, tmin = INFINITY, tmax = -INFINITY;
  const int64_t clamp_lo = sp_first * ndofs, clamp_hi = sp_last * ndofs;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(LTE_BLOCK) + threadIdx.x; i < ndofs; i += static_cast<int64_t>(gridDim.x) * LTE_BLOCK) {
    NodeRows U = {x + i, ndofs};
    LteNode nd;
    if constexpr (WRITE_UP)
      nd = species_from_lte(P, LT, U, NodeRows{up + i, ndofs});
    else
      nd = species_from_lte(P, LT, U, NoRows());
    // Check_Undershoot (src/M2ulPhyS.cpp:2526-2548) on the species rows of the new state: the time loop's function
    unsigned long long bad = 0;
    for (int eq = sp_first; eq < sp_last; eq++) {
      const int64_t at = eq * ndofs + i;
      x[at] = rk_final_entry(x[at], at, clamp_lo, clamp_hi, bad);
    }
    if (nd.flags & LTE_NOT_CONVERGED) nnc += 1.0;
    if (nd.flags & LTE_INVALID) ninv += 1.0;
    if (nd.density_change > chg) chg = nd.density_change;
    if (nd.T < tmin) tmin = nd.T;
    if (nd.T > tmax) tmax = nd.T;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nnc += __shfl_xor(nnc, off, 64);
    ninv += __shfl_xor(ninv, off, 64);
    const double a = __shfl_xor(chg, off, 64), b = __shfl_xor(tmin, off, 64), c = __shfl_xor(tmax, off, 64);
    if (a > chg) chg = a;
    if (b < tmin) tmin = b;
    if (c > tmax) tmax = c;
  }
  constexpr int NW = LTE_BLOCK / 64;
  __shared__ double red[LTE_REPORT][NW];
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  if (lane == 0) {
    red[0][wave] = nnc;
    red[1][wave] = ninv;
    red[2][wave] = chg;
    red[3][wave] = tmin;
    red[4][wave] = tmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) {
      nnc += red[0][w];
      ninv += red[1][w];
      if (red[2][w] > chg) chg = red[2][w];
      if (red[3][w] < tmin) tmin = red[3][w];
      if (red[4][w] > tmax) tmax = red[4][w];
    }
    const int64_t nb = gridDim.x;
    partial[blockIdx.x] = nnc;
    partial[nb + blockIdx.x] = ninv;
    partial[2 * nb + blockIdx.x] = chg;
    partial[3 * nb + blockIdx.x] = tmin;
    partial[4 * nb + blockIdx.x] = tmax;
  }
}

// one wave over the partials of at most LTE_MAXBLOCKS blocks: out[LTE_REPORT]
__global__ void __launch_bounds__(64) k_lte_report(int nb, const double *__restrict__ partial, double *__restrict__ out) {
  double nnc = 0.0, ninv = 0.0, chg = 0.0, tmin = INFINITY, tmax = -INFINITY;
  for (int b = threadIdx.x; b < nb; b += 64) {
    nnc += partial[b];
    ninv += partial[nb + b];
    if (partial[2 * nb + b] > chg) chg = partial[2 * nb + b];
    if (partial[3 * nb + b] < tmin) tmin = partial[3 * nb + b];
    if (partial[4 * nb + b] > tmax) tmax = partial[4 * nb + b];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nnc += __shfl_xor(nnc, off, 64);
    ninv += __shfl_xor(ninv, off, 64);
    const double a = __shfl_xor(chg, off, 64), b = __shfl_xor(tmin, off, 64), c = __shfl_xor(tmax, off, 64);
    if (a > chg) chg = a;
    if (b < tmin) tmin = b;
    if (c > tmax) tmax = c;
  }
  if (threadIdx.x == 0) {
    out[0] = nnc;
    out[1] = ninv;
    out[2] = chg;
    out[3] = tmin;
    out[4] = tmax;
  }
}

unsigned grid_for(int64_t n) { return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + LTE_BLOCK - 1) / LTE_BLOCK, LTE_MAXBLOCKS))); }

}  // namespace

extern "C" {

int tpsrhs_lte_composition(tpsrhs_handle h, int64_t n, const double *T, const double *p, double *n_sp_out) {
  if (!h || n < 0 || !T || !p || !n_sp_out)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_lte_composition: needs a handle, n >= 0 and the device arrays T, p, n_sp_out");
  return guarded([&] {
    check_lte_restart_mixture(h->phys, "tpsrhs_lte_composition");
    const LteRestartParams P = lte_restart_params(h->phys.mixture, h->nvel);
    HIP_CHECK(hipSetDevice(h->device));
    if (n > 0) {
      hipLaunchKernelGGL(k_lte_composition, dim3(grid_for(n)), dim3(LTE_BLOCK), 0, h->stream, P, n, T, p, n_sp_out);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

int tpsrhs_species_from_lte(tpsrhs_handle h, const tpsrhs_lte_restart *tables, double *x, double *up_out,
                            tpsrhs_lte_restart_report *report) {
  if (!h || !tables || !x)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_species_from_lte: needs a handle, the tables and the device state x");
  return guarded([&] {
    check_lte_restart_mixture(h->phys, "tpsrhs_species_from_lte");
    check_lte_restart_tables(*tables);
    const LteRestartParams P = lte_restart_params(h->phys.mixture, h->nvel);
    HIP_CHECK(hipSetDevice(h->device));
    std::vector<DevBuf<void>> owner;  // the device copies of the tables, for the duration of the call
    const LteRestartTables LT = make_lte_restart_tables(*tables, [&owner](const void *src, size_t bytes) {
      const unsigned char *b = static_cast<const unsigned char *>(src);
      owner.emplace_back(DevBuf<unsigned char>(std::vector<unsigned char>(b, b + bytes)));
      return static_cast<const void *>(owner.back().get());
    });
    const unsigned nb = grid_for(h->ndofs);
    DevBuf<double> partial(static_cast<size_t>(LTE_REPORT) * nb + LTE_REPORT);
    double *d_out = partial.get() + static_cast<size_t>(LTE_REPORT) * nb;
    double out[LTE_REPORT] = {0.0, 0.0, 0.0, INFINITY, -INFINITY};  // of no nodes
    if (h->ndofs > 0) {
      if (up_out)
        hipLaunchKernelGGL(k_species_from_lte<true>, dim3(nb), dim3(LTE_BLOCK), 0, h->stream, P, LT, h->ndofs, h->loop.sp_first,
                           h->loop.sp_last, x, up_out, partial.get());
      else
        hipLaunchKernelGGL(k_species_from_lte<false>, dim3(nb), dim3(LTE_BLOCK), 0, h->stream, P, LT, h->ndofs, h->loop.sp_first,
                           h->loop.sp_last, x, static_cast<double *>(nullptr), partial.get());
      HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(k_lte_report, dim3(1), dim3(64), 0, h->stream, static_cast<int>(nb), partial.get(), d_out);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));  // before the tables and the partials go
    if (report) {
      report->num_not_converged = static_cast<int64_t>(out[0]);
      report->num_invalid = static_cast<int64_t>(out[1]);
      report->max_density_change = out[2];
      report->t_min = out[3];
      report->t_max = out[4];
    }
  });
}

}  // extern "C"
