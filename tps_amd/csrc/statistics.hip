// Running mean and velocity covariances (statistics.hpp): tpsrhs_stats_*.  An observer of the device time loop
// (abi_support.hpp: stats_cadence, stats_sample).
#include "abi_support.hpp"
#include "statistics.hpp"

namespace {
template <int NVEL, bool VARI>
void launch_stats_sample(tpsrhs_operator *h) {
  tpsrhs_stats_state *st = h->stats.get();
  const int64_t n = h->ndofs;
  const double *prim = st->d_scratch.get(), *p = prim + h->neq * n;
  double *mean = st->d_mean.get(), *vari = st->d_vari.get();
  const uintptr_t bits = reinterpret_cast<uintptr_t>(prim) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(vari);
  const bool vec = (n & 1) == 0 && (bits & 15) == 0;  // then every row of every array is 16-byte aligned, p included
  const int64_t items = vec ? n / 2 : n;
  const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 8192));  // the grid cap of k_rk_stage
  if (grid == 0) return;
  if (vec)
    hipLaunchKernelGGL((k_stats_sample<NVEL, VARI, true, 256>), dim3(grid), dim3(256), 0, h->stream, h->neq, n, st->ns_mean,
                       st->ns_vari, prim, p, mean, vari);
  else
    hipLaunchKernelGGL((k_stats_sample<NVEL, VARI, false, 256>), dim3(grid), dim3(256), 0, h->stream, h->neq, n, st->ns_mean,
                       st->ns_vari, prim, p, mean, vari);
  HIP_CHECK(hipGetLastError());
}

// the statistics of h, or NULL with the error text set
tpsrhs_stats_state *stats_of(tpsrhs_handle h, const char *who) {
  if (!h) {
    fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL handle");
    return nullptr;
  }
  if (!h->stats) fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": statistics are not configured (tpsrhs_stats_configure)");
  return h->stats.get();
}
}  // namespace

StepCadence *stats_cadence(tpsrhs_operator *h) { return h->stats ? &h->stats->cadence : nullptr; }

// One sample of the device vector x, stream-ordered: the primitives and the pressure from the gas model's own point-wise
// kernel (tpsrhs_eval_pointwise quantities 0 and 1: no physics here), then the update.  The counters are host integers.
void stats_sample(tpsrhs_operator *h, const double *x) {
  tpsrhs_stats_state *st = h->stats.get();
  const int64_t n = h->ndofs;
  h->point_eval(h, 0, n, x, st->d_scratch.get());
  h->point_eval(h, 1, n, x, st->d_scratch.get() + h->neq * n);
  const bool vari = st->nvar > 0;
  if (h->nvel == 3)
    vari ? launch_stats_sample<3, true>(h) : launch_stats_sample<3, false>(h);
  else
    vari ? launch_stats_sample<2, true>(h) : launch_stats_sample<2, false>(h);
  st->ns_mean++;
  st->ns_vari++;
}

extern "C" {

int tpsrhs_stats_configure(tpsrhs_handle h, int64_t sample_interval, int64_t start_iter, int compute_variances) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_configure: NULL handle");
  if (sample_interval < 0 || start_iter < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_configure: needs sample_interval >= 0 (0: off) and start_iter >= 0");
  if (sample_interval > 0 && h->nvel != 2 && h->nvel != 3)
    return fail(TPSRHS_ERR_UNSUPPORTED, "tpsrhs_stats_configure: two or three velocity components");
  return guarded([&] {
    if (h->stats) {
      (void)hipSetDevice(h->device);
      (void)hipStreamSynchronize(h->stream);  // a sample may still be running
      h->stats.reset();
    }
    if (sample_interval == 0) return;
    HIP_CHECK(hipSetDevice(h->device));
    std::unique_ptr<tpsrhs_stats_state> st(new tpsrhs_stats_state());
    st->cadence.interval = sample_interval;
    st->cadence.start = start_iter;
    st->nvar = compute_variances ? h->nvel * (h->nvel + 1) / 2 : 0;
    const int64_t n = h->ndofs;
    st->d_mean = DevBuf<double>(h->neq * n);
    if (st->nvar) st->d_vari = DevBuf<double>(st->nvar * n);
    st->d_scratch = DevBuf<double>((h->neq + 1) * n);
    HIP_CHECK(hipMemsetAsync(st->d_mean.get(), 0, sizeof(double) * h->neq * n, h->stream));
    if (st->nvar) HIP_CHECK(hipMemsetAsync(st->d_vari.get(), 0, sizeof(double) * st->nvar * n, h->stream));
    h->stats = owned_state(std::move(st));  // complete: a call that throws above leaves the statistics off
  });
}

int tpsrhs_stats_set_iter(tpsrhs_handle h, int64_t iter) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_set_iter");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (iter < 0) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set_iter: needs iter >= 0");
  st->cadence.count = iter;
  return TPSRHS_OK;
}

int tpsrhs_stats_add_sample(tpsrhs_handle h, const double *x) {
  if (!stats_of(h, "tpsrhs_stats_add_sample")) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (!x) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_add_sample: NULL argument");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    stats_sample(h, x);
  });
}

int tpsrhs_stats_get(tpsrhs_handle h, double *mean_out, double *vari_out, int *ns_mean, int *ns_vari, int64_t *iter) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_get");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (vari_out && !st->nvar)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_get: the covariances are not computed (compute_variances = 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int64_t n = h->ndofs;
    if (mean_out) HIP_CHECK(hipMemcpyAsync(mean_out, st->d_mean.get(), sizeof(double) * h->neq * n, hipMemcpyDeviceToDevice, h->stream));
    if (vari_out) HIP_CHECK(hipMemcpyAsync(vari_out, st->d_vari.get(), sizeof(double) * st->nvar * n, hipMemcpyDeviceToDevice, h->stream));
    if (ns_mean) *ns_mean = st->ns_mean;
    if (ns_vari) *ns_vari = st->ns_vari;
    if (iter) *iter = st->cadence.count;
  });
}

int tpsrhs_stats_set(tpsrhs_handle h, const double *mean, const double *vari, int ns_mean, int ns_vari) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_set");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (ns_mean < 0 || ns_vari < 0 || (ns_mean > 0 && !mean))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set: needs counters >= 0 and the mean field of ns_mean > 0 samples");
  if (vari && ns_vari > 0 && !st->nvar)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_set: the covariances are not computed (compute_variances = 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const int64_t n = h->ndofs;
    const bool keep_vari = vari && ns_vari > 0;  // else restartRMS: the covariances start again
    if (ns_mean > 0)
      HIP_CHECK(hipMemcpyAsync(st->d_mean.get(), mean, sizeof(double) * h->neq * n, hipMemcpyDeviceToDevice, h->stream));
    else
      HIP_CHECK(hipMemsetAsync(st->d_mean.get(), 0, sizeof(double) * h->neq * n, h->stream));
    if (st->nvar) {
      if (keep_vari)
        HIP_CHECK(hipMemcpyAsync(st->d_vari.get(), vari, sizeof(double) * st->nvar * n, hipMemcpyDeviceToDevice, h->stream));
      else
        HIP_CHECK(hipMemsetAsync(st->d_vari.get(), 0, sizeof(double) * st->nvar * n, h->stream));
    }
    st->ns_mean = ns_mean;
    st->ns_vari = keep_vari ? ns_vari : 0;
  });
}

int tpsrhs_stats_num_variances(tpsrhs_handle h, int *num_variances) {
  tpsrhs_stats_state *st = stats_of(h, "tpsrhs_stats_num_variances");
  if (!st) return TPSRHS_ERR_INVALID_ARGUMENT;
  if (!num_variances) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_stats_num_variances: NULL argument");
  *num_variances = st->nvar;
  return TPSRHS_OK;
}

}  // extern "C"
