// What the units of the C ABI share besides the operator (operator.hpp) and the statuses (status.hpp: fail, guarded, the
// last error): the dispatch over (dim, order), the read-back of a record log, and the few functions that cross from one
// unit to another -- plain C++ functions inside the library, as pick_dryair_axisym is.  No kernel in here.
#ifndef TPSRHS_ABI_SUPPORT_HPP_
#define TPSRHS_ABI_SUPPORT_HPP_

#include <type_traits>

#include "operator.hpp"
#include "record_log.hpp"

namespace tpsrhs {
struct TableDev;  // physics_plasma.hpp
}

// ---- tpsrhs.hip
// LinearTable::LinearTable (src/table.cpp:39-50): interval coefficients (plasma_params_host.hpp), uploaded with the
// abscissae into a buffer that `owner` keeps
tpsrhs::TableDev upload_table(std::vector<DevBuf<void>> &owner, const tpsrhs_table &t);
// the polynomial table of the Coulomb fits (coulomb_table.hpp), filled once per process from the literals of the closure
const std::vector<double> &coulomb_table_host();
// the per-node passes of a plasma operator's family (plasma_vis_family.hpp: tpsrhs_visualization_fields, and
// external_rates.hip), loaded on demand; `who` starts the message of a refusal
void load_plasma_vis_family(tpsrhs_operator *h, const char *who);

// ---- flux_fields.hip
// the pass of tpsrhs_get_flux on the operator's stream, after tpsrhs_update_gradients' work unless the caller holds Up / gradUp
// of x (tpsrhs_surface_loads composes it with the FLUX reduction)
void get_flux(tpsrhs_operator *h, const double *x, int part, int gradients_current, double *out);

// ---- the observers of the device time loop (time_loop.hip: after_step / work_due_after_next).  The loop knows each by its
// StepCadence (record_log.hpp; NULL: not configured, interval 0: off) and by the function that does its work on the
// operator's stream once the cadence says so.
tpsrhs::StepCadence *stats_cadence(tpsrhs_operator *h);    // statistics.hip
void stats_sample(tpsrhs_operator *h, const double *x);
tpsrhs::StepCadence *probe_cadence(tpsrhs_operator *h);    // sampling.hip
void probe_record(tpsrhs_operator *h, const double *x);
tpsrhs::StepCadence *monitor_cadence(tpsrhs_operator *h);  // integrals.hip
void monitor_record(tpsrhs_operator *h, const double *x);
tpsrhs::StepCadence *surface_cadence(tpsrhs_operator *h);  // surface.hip
void surface_record(tpsrhs_operator *h, const double *x);

// ---- limiter.hip: the conservative limiter the time loop applies after the stages of every step (limiter.hpp)
bool limiter_active(const tpsrhs_operator *h);          // tpsrhs_limiter_configure has set one
bool limiter_replaces_clamp(const tpsrhs_operator *h);  // ... which lists the species rows: the stages' clamp range is empty
void limiter_apply(tpsrhs_operator *h, double *x);      // k_limit on the operator's stream; needs limiter_active
// the weights W_n (DEVICE [NDofs]) the operator owns, computed at the first use: the modal filter's mean correction reads them
const double *limiter_weights_device(tpsrhs_operator *h);

// ---- modal.hip: the modal filter the time loop applies after the stages of every step, before the limiter (modal.hpp)
bool modal_filter_active(const tpsrhs_operator *h);       // tpsrhs_modal_filter_configure has set one
void modal_filter_apply(tpsrhs_operator *h, double *x);   // k_modal_filter on the operator's stream; needs modal_filter_active

// ---- sampling.hip
// h is being destroyed: tpsrhs_transfer forgets it as a source and drops every cached sampler at its nodes (the cache is
// keyed by the address of the destination, which the next tpsrhs_create may hand out again)
void transfer_forget(tpsrhs_operator *h);

// {dt, time, max speed} of the time loop in device memory; the probe and monitor records copy the time from there
inline double *loop_ctl(tpsrhs_operator *h) {
  if (!h->loop.d_ctl) h->loop.d_ctl = DevBuf<double>(3);
  return h->loop.d_ctl.get();
}

// the entry points that take no operator: there is no CPU path
inline void require_device(const char *what = "no HIP device visible") {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw NoDevice(what);
}

// f(std::integral_constant<int, DIM>, std::integral_constant<int, P>) for the operator's dim and order: the (dim, order) pairs
// the post-processing kernels are built for, listed once
template <int N>
using int_c = std::integral_constant<int, N>;
template <class F>
void with_dim_order(const tpsrhs_operator *h, const char *who, F &&f) {
  switch (h->dim * 10 + h->order) {
    case 21: f(int_c<2>(), int_c<1>()); break;
    case 22: f(int_c<2>(), int_c<2>()); break;
    case 23: f(int_c<2>(), int_c<3>()); break;
    case 24: f(int_c<2>(), int_c<4>()); break;
    case 25: f(int_c<2>(), int_c<5>()); break;
    case 31: f(int_c<3>(), int_c<1>()); break;
    case 32: f(int_c<3>(), int_c<2>()); break;
    case 33: f(int_c<3>(), int_c<3>()); break;
    case 34: f(int_c<3>(), int_c<4>()); break;
    case 35: f(int_c<3>(), int_c<5>()); break;
    default: throw Unsupported(std::string(who) + ": dim 2 or 3 and polynomial orders 1..5 are built");
  }
}

// What reading the probe records and reading the monitor records share.  The first n rows of one column of a log (`width`
// doubles a row) to the host, on the operator's stream ...
inline void fetch_rows(tpsrhs_operator *h, double *dst, const DevBuf<double> &col, int64_t n, int64_t width) {
  if (dst && n * width) HIP_CHECK(hipMemcpyAsync(dst, col.get(), sizeof(double) * n * width, hipMemcpyDeviceToHost, h->stream));
}
// ... and, once the stream has been synchronised, the host half: the counters, the step of every record, the optional restart
inline void read_index(RecordIndex &ix, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, int reset) {
  if (nrecords) *nrecords = ix.nrecords;
  if (ndropped) *ndropped = ix.ndropped;
  if (iters_out && ix.nrecords) std::memcpy(iters_out, ix.iters.data(), sizeof(int64_t) * ix.nrecords);
  if (reset) ix.reset();  // the buffer starts again; the step counter goes on
}

#endif
