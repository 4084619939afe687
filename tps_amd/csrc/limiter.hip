// The conservative positivity limiter of libtpsrhs.so (limiter.hpp holds the operation and the plan): tpsrhs_limiter_weights,
// tpsrhs_limit, tpsrhs_limiter_configure, tpsrhs_limiter_read, and the two functions the device time loop calls after the
// stages of a step (abi_support.hpp: limiter_replaces_clamp, limiter_apply).
//
// Shape of the kernels.
//   k_limiter_weights<DIM, P>: once per operator.  One wave per element (grid-stride): the NQ^dim weights W_q of the rule go
//   to LDS, then the transpose of k_integrate's interpolation, one direction after the other: W_n = sum_q W_q l_n(xi_q).
//   k_limit<LPE, VPL>: a group of LPE lanes (4, 8, 16, 32 or 64: the power of two >= the N nodes of an element) owns one
//   element, a lane VPL of its nodes (one below 65 nodes; up to four at p = 5 in 3-D, 216 nodes).  A wave walks 64 / LPE
//   elements at a time, the grid is capped and strides over the groups.  sum W v, sum W and the minimum are butterflies
//   over the group's lanes (no LDS); every lane of a group ends with the same numbers and takes the same decision, so
//   nothing is broadcast.  The weights and the row are read once, coalesced; an untouched element writes nothing.  The
//   pressure step reads the rows again after the row steps have written them (every lane reads what it wrote itself).
//   Counters: 64-bit integers, summed per block in LDS (integer atomics of the groups' first lanes: a firing is rare), then
//   one integer atomic per block and non-zero counter.  Integer sums do not depend on the order of arrival; there is no
//   floating-point atomic.
#include "abi_support.hpp"
#include "quadrature_points.hpp"  // before limiter.hpp: TPSRHS_HOST_DEVICE is defined there
#include "limiter.hpp"

struct tpsrhs_limiter_state {
  DevBuf<double> d_w;                     // [NDofs], the weights W_n
  DevBuf<unsigned long long> d_counters;  // [LIMITER_NCOUNTERS]
  bool active = false;                    // tpsrhs_limiter_configure: the time loop applies `plan` after every step
  LimiterPlan plan;
};

namespace {

constexpr int LIMIT_BLOCK = 256;
constexpr int LIMIT_MAXBLOCKS = 4096;  // 16 blocks of four waves on each of the 256 CUs

struct WeightTab {
  double B[QUAD_MAXQ * (TPSRHS_MAXORDER + 1)];  // B[q * N1 + a] = l_a(g_q)
  double g[QUAD_MAXQ], w[QUAD_MAXQ];
};

template <int DIM, int P>
__global__ void __launch_bounds__(64)
    k_limiter_weights(int ne, int radial, WeightTab tab, const double *__restrict__ verts, double *__restrict__ w_out) {
  constexpr int N1 = P + 1, NQ = P + 2, NPE = ipow(N1, DIM), NQD = ipow(NQ, DIM);
  constexpr int S1 = (NQD / NQ) * N1;                  // after direction 0: [qk][qj][a]
  constexpr int S2 = DIM == 3 ? NQ * N1 * N1 : 1;      // after direction 1 (3-D): [qk][b][a]
  __shared__ double sB[NQ * N1], sg[NQ], sw[NQ];
  __shared__ double sW[NQD], s1[S1], s2[S2];
  const int lane = threadIdx.x;
  for (int i = lane; i < NQ * N1; i += 64) sB[i] = tab.B[i];
  if (lane < NQ) {
    sg[lane] = tab.g[lane];
    sw[lane] = tab.w[lane];
  }
  for (int e = blockIdx.x; e < ne; e += gridDim.x) {
    __syncthreads();  // the tables are in place; the last element's s1 / s2 have been read
    for (int q = lane; q < NQD; q += 64) {
      const int qi = q % NQ, qj = (q / NQ) % NQ, qk = q / (NQ * NQ);
      const double xi[3] = {sg[qi], sg[qj], sg[DIM == 3 ? qk : 0]};
      double x[DIM], det;
      quad_geometry<DIM>(verts + static_cast<int64_t>(e) * (1 << DIM) * DIM, xi, x, &det);
      double W = (DIM == 3 ? sw[qi] * sw[qj] * sw[qk] : sw[qi] * sw[qj]) * fabs(det);
      if (radial) W *= x[0];
      sW[q] = W;
    }
    __syncthreads();
    for (int idx = lane; idx < S1; idx += 64) {  // direction 0: s1[m][a] = sum_qi B[qi][a] W[m][qi], m = (qk, qj)
      const int a = idx % N1, m = idx / N1;
      double s = 0.0;
#pragma unroll
      for (int qi = 0; qi < NQ; qi++) s += sB[qi * N1 + a] * sW[m * NQ + qi];
      s1[idx] = s;
    }
    __syncthreads();
    double *out = w_out + static_cast<int64_t>(e) * NPE;
    if constexpr (DIM == 3) {
      for (int idx = lane; idx < S2; idx += 64) {  // direction 1: s2[qk][b][a] = sum_qj B[qj][b] s1[qk][qj][a]
        const int a = idx % N1, b = (idx / N1) % N1, qk = idx / (N1 * N1);
        double s = 0.0;
#pragma unroll
        for (int qj = 0; qj < NQ; qj++) s += sB[qj * N1 + b] * s1[(qk * NQ + qj) * N1 + a];
        s2[idx] = s;
      }
      __syncthreads();
      for (int n = lane; n < NPE; n += 64) {  // direction 2: W[c][b][a] = sum_qk B[qk][c] s2[qk][b][a]
        const int ab = n % (N1 * N1), c = n / (N1 * N1);
        double s = 0.0;
#pragma unroll
        for (int qk = 0; qk < NQ; qk++) s += sB[qk * N1 + c] * s2[qk * N1 * N1 + ab];
        out[n] = s;
      }
    } else {
      for (int n = lane; n < NPE; n += 64) {  // direction 1: W[b][a] = sum_qj B[qj][b] s1[qj][a]
        const int a = n % N1, b = n / N1;
        double s = 0.0;
#pragma unroll
        for (int qj = 0; qj < NQ; qj++) s += sB[qj * N1 + b] * s1[qj * N1 + a];
        out[n] = s;
      }
    }
  }
}

// the sum / the minimum (kept with `<`) over the LPE lanes of a group: every lane gets the result
template <int LPE>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = LPE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int LPE>
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
  for (int off = LPE / 2; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    if (o < v) v = o;
  }
  return v;
}

// x: [neq][ndofs], an element's npe nodes contiguous per row; w: [ndofs]
template <int LPE, int VPL>
__global__ void __launch_bounds__(LIMIT_BLOCK)
    k_limit(int ne, int npe, int64_t ndofs, LimiterPlan pl, const double *__restrict__ w, double *__restrict__ x,
            unsigned long long *__restrict__ counters) {
  constexpr int EPW = 64 / LPE;                   // elements a wave holds at a time
  constexpr int EPB = EPW * (LIMIT_BLOCK / 64);   // ... and a block
  __shared__ unsigned long long s_cnt[LIMITER_NCOUNTERS];
  for (int i = threadIdx.x; i < LIMITER_NCOUNTERS; i += LIMIT_BLOCK) s_cnt[i] = 0;
  __syncthreads();
  const int slot = threadIdx.x / LPE, l = threadIdx.x % LPE;
  const int64_t ngroups = (static_cast<int64_t>(ne) + EPB - 1) / EPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t e = g * EPB + slot;
    const bool have = e < ne;  // the same for every lane of a group: the shuffles below stay inside a group
    const int64_t base = e * npe;
    double W[VPL];
    bool mine[VPL];
#pragma unroll
    for (int k = 0; k < VPL; k++) {
      mine[k] = have && l + k * LPE < npe;
      W[k] = mine[k] ? w[base + l + k * LPE] : 0.0;
    }
    double sw = 0.0;
#pragma unroll
    for (int k = 0; k < VPL; k++) sw += W[k];
    sw = group_sum<LPE>(sw);
    for (int i = 0; i < pl.num_rows; i++) {
      const int row = pl.rows[i];
      const double f = pl.floors[i];
      double *v = x + row * ndofs + base;
      double val[VPL], swv = 0.0, m = INFINITY;
#pragma unroll
      for (int k = 0; k < VPL; k++) {
        val[k] = mine[k] ? v[l + k * LPE] : 0.0;
        swv += W[k] * val[k];
        if (mine[k] && val[k] < m) m = val[k];
      }
      swv = group_sum<LPE>(swv);
      m = group_min<LPE>(m);
      if (!have) continue;
      const double mean = limiter_mean(swv, sw);
      const int outcome = limiter_row_outcome(mean, m, f);
      if (outcome == LIMITER_SCALED || outcome == LIMITER_CLAMPED) {
        const double theta = outcome == LIMITER_SCALED ? limiter_theta(mean, m, f) : 0.0;
#pragma unroll
        for (int k = 0; k < VPL; k++)
          if (mine[k]) v[l + k * LPE] = limiter_row_value(outcome, val[k], mean, theta, f);
        if (l == 0) atomicAdd(&s_cnt[(outcome == LIMITER_SCALED ? LIMITER_LIMITED : LIMITER_CLAMPED_AT) + row], 1ull);
      }
    }
    if (pl.pressure_floor > 0.0) {  // dry air: neq = nvel + 2 <= 5 rows
      constexpr int MAXROWS = 5;
      const int nrows = pl.nvel + 2;
      double U[MAXROWS][VPL], ubar[MAXROWS];
#pragma unroll
      for (int r = 0; r < MAXROWS; r++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < VPL; k++) {
          U[r][k] = (r < nrows && mine[k]) ? x[r * ndofs + base + l + k * LPE] : 0.0;
          s += W[k] * U[r][k];
        }
        ubar[r] = limiter_mean(group_sum<LPE>(s), sw);
      }
      // rows in registers: rho, nvel momenta, the energy at row nvel + 1
      const bool v3 = pl.nvel == 3;
      auto pressure = [&](double u0, double u1, double u2, double u3, double u4) {
        return limiter_pressure_of(u0, u1, u2, v3 ? u3 : 0.0, v3 ? u4 : u3, pl.gm1);
      };
      double pmin = INFINITY;
#pragma unroll
      for (int k = 0; k < VPL; k++) {
        const double p = pressure(U[0][k], U[1][k], U[2][k], U[3][k], U[4][k]);
        if (mine[k] && p < pmin) pmin = p;
      }
      pmin = group_min<LPE>(pmin);
      if (have) {
        const double pbar = pressure(ubar[0], ubar[1], ubar[2], ubar[3], ubar[4]);
        const int outcome = limiter_pressure_outcome(pbar, pmin, pl.pressure_floor);
        if (outcome == LIMITER_P_SCALED) {
          const double theta = limiter_theta(pbar, pmin, pl.pressure_floor);
#pragma unroll
          for (int r = 0; r < MAXROWS; r++)
#pragma unroll
            for (int k = 0; k < VPL; k++)
              if (r < nrows && mine[k]) x[r * ndofs + base + l + k * LPE] = limiter_scale(U[r][k], ubar[r], theta);
        }
        if (l == 0 && outcome != LIMITER_P_UNTOUCHED)
          atomicAdd(&s_cnt[outcome == LIMITER_P_SCALED ? LIMITER_P_LIMITED : LIMITER_P_UNFIXABLE_AT], 1ull);
      }
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) s_cnt[LIMITER_CALLS] = 1;  // (after the barrier: this thread's own entry)
  for (int i = threadIdx.x; i < LIMITER_NCOUNTERS; i += LIMIT_BLOCK)
    if (s_cnt[i]) atomicAdd(&counters[i], s_cnt[i]);
}

LimiterFacts facts_of(const tpsrhs_operator *h) {
  LimiterFacts f;
  f.neq = h->neq;
  f.nvel = h->nvel;
  f.sp_first = h->loop.sp_first;
  f.sp_last = h->loop.sp_last;
  f.dry_air = h->phys.working_fluid == TPSRHS_DRY_AIR;
  f.gamma = h->phys.dry_air.specific_heat_ratio;
  return f;
}

template <int DIM, int P>
void launch_weights(tpsrhs_operator *h, const WeightTab &tab, double *w_out) {
  const int radial = (h->dim == 2 && h->nvel == 3) ? 1 : 0;  // the operator's axisymmetric flag, as the monitor's totals
  hipLaunchKernelGGL((k_limiter_weights<DIM, P>), dim3(std::min(h->ne, 8192)), dim3(64), 0, h->stream, h->ne, radial, tab,
                     h->d_verts.get(), w_out);
  HIP_CHECK(hipGetLastError());
}

// the state with the weights and the zeroed counters, at the first use; everything on the operator's stream
tpsrhs_limiter_state *limiter_of(tpsrhs_operator *h) {
  if (h->limiter) return h->limiter.get();
  std::unique_ptr<tpsrhs_limiter_state> ls(new tpsrhs_limiter_state());
  ls->d_w = DevBuf<double>(h->ndofs);
  ls->d_counters = DevBuf<unsigned long long>(LIMITER_NCOUNTERS);
  HIP_CHECK(hipMemsetAsync(ls->d_counters.get(), 0, sizeof(unsigned long long) * LIMITER_NCOUNTERS, h->stream));
  if (h->ne > 0) {
    WeightTab tab = {};
    const int n1 = h->order + 1, nq = quad_points_1d(h->order);
    double nodes[TPSRHS_MAXORDER + 1], wts[TPSRHS_MAXORDER + 1];
    segment_rule01(h->nc, n1, nodes, wts);  // the nodes of the operator's basis, as tpsrhs_integrate places them
    gauss_legendre01(nq, tab.g, tab.w);
    for (int q = 0; q < nq; q++)
      for (int a = 0; a < n1; a++) tab.B[q * n1 + a] = lagrange(nodes, n1, a, tab.g[q]);
    with_dim_order(h, "tpsrhs_limiter_weights", [&](auto dim, auto p) {
      launch_weights<decltype(dim)::value, decltype(p)::value>(h, tab, ls->d_w.get());
    });
  }
  h->limiter = owned_state(std::move(ls));
  return h->limiter.get();
}

template <int LPE, int VPL>
void launch_limit(tpsrhs_operator *h, const tpsrhs_limiter_state *ls, const LimiterPlan &pl, int npe, double *x) {
  constexpr int EPB = (64 / LPE) * (LIMIT_BLOCK / 64);
  const int64_t ngroups = (static_cast<int64_t>(h->ne) + EPB - 1) / EPB;
  const int grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ngroups, LIMIT_MAXBLOCKS)));
  hipLaunchKernelGGL((k_limit<LPE, VPL>), dim3(grid), dim3(LIMIT_BLOCK), 0, h->stream, h->ne, npe, h->ndofs, pl, ls->d_w.get(), x,
                     ls->d_counters.get());
  HIP_CHECK(hipGetLastError());
}

// one application on the operator's stream (an empty plan still counts as a call)
void apply(tpsrhs_operator *h, const tpsrhs_limiter_state *ls, const LimiterPlan &pl, double *x) {
  const int npe = static_cast<int>(h->ndofs / std::max(h->ne, 1));
  switch (npe > 128 ? 256 : (npe > 64 ? 128 : lanes_per_element(npe))) {
    case 256: launch_limit<64, 4>(h, ls, pl, npe, x); break;
    case 128: launch_limit<64, 2>(h, ls, pl, npe, x); break;
    case 64: launch_limit<64, 1>(h, ls, pl, npe, x); break;
    case 32: launch_limit<32, 1>(h, ls, pl, npe, x); break;
    case 16: launch_limit<16, 1>(h, ls, pl, npe, x); break;
    case 8: launch_limit<8, 1>(h, ls, pl, npe, x); break;
    default: launch_limit<4, 1>(h, ls, pl, npe, x); break;
  }
}

}  // namespace

bool limiter_active(const tpsrhs_operator *h) { return h->limiter && h->limiter->active; }
bool limiter_replaces_clamp(const tpsrhs_operator *h) { return limiter_active(h) && h->limiter->plan.covers_species; }
void limiter_apply(tpsrhs_operator *h, double *x) { apply(h, h->limiter.get(), h->limiter->plan, x); }
const double *limiter_weights_device(tpsrhs_operator *h) { return limiter_of(h)->d_w.get(); }

extern "C" {

int tpsrhs_limiter_weights(tpsrhs_handle h, double *w_out) {
  if (!h || !w_out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_limiter_weights: needs a handle and the device array w_out");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const tpsrhs_limiter_state *ls = limiter_of(h);
    if (h->ndofs)
      HIP_CHECK(hipMemcpyAsync(w_out, ls->d_w.get(), sizeof(double) * h->ndofs, hipMemcpyDeviceToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

int tpsrhs_limit(tpsrhs_handle h, const tpsrhs_limiter *lim, double *x) {
  if (!h || !lim || !x) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_limit: needs a handle, a limiter and the device state x");
  return guarded([&] {
    const LimiterPlan pl = plan_limiter(*lim, facts_of(h), false, "tpsrhs_limit");
    HIP_CHECK(hipSetDevice(h->device));
    apply(h, limiter_of(h), pl, x);
  });
}

int tpsrhs_limiter_configure(tpsrhs_handle h, const tpsrhs_limiter *lim) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_limiter_configure: NULL handle");
  return guarded([&] {
    if (!lim) {
      if (limiter_active(h)) {
        h->limiter->active = false;
        h->loop.config_epoch++;
      }
      return;
    }
    const LimiterPlan pl = plan_limiter(*lim, facts_of(h), true, "tpsrhs_limiter_configure");
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_limiter_state *ls = limiter_of(h);  // with the weights: a step allocates nothing
    ls->plan = pl;
    ls->active = true;
    h->loop.config_epoch++;  // a step graph captured before this call is not replayed (trace_chain.hpp)
  });
}

int tpsrhs_limiter_read(tpsrhs_handle h, tpsrhs_limiter_report *out, int reset) {
  if (!h || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_limiter_read: needs a handle and the report");
  return guarded([&] {
    unsigned long long c[LIMITER_NCOUNTERS] = {};
    HIP_CHECK(hipSetDevice(h->device));
    if (h->limiter) {
      unsigned long long *d = h->limiter->d_counters.get();
      HIP_CHECK(hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, h->stream));
      if (reset) HIP_CHECK(hipMemsetAsync(d, 0, sizeof(c), h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    *out = tpsrhs_limiter_report();
    out->calls = static_cast<int64_t>(c[LIMITER_CALLS]);
    for (int r = 0; r < TPSRHS_MAXEQUATIONS; r++) {
      out->limited[r] = static_cast<int64_t>(c[LIMITER_LIMITED + r]);
      out->clamped[r] = static_cast<int64_t>(c[LIMITER_CLAMPED_AT + r]);
    }
    out->pressure_limited = static_cast<int64_t>(c[LIMITER_P_LIMITED]);
    out->pressure_unfixable = static_cast<int64_t>(c[LIMITER_P_UNFIXABLE_AT]);
  });
}

}  // extern "C"
