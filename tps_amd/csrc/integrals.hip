// Volume integrals, nodal extrema and the monitor records of libtpsrhs.so (quadrature_points.hpp, integrals.hpp):
// tpsrhs_quadrature_points, tpsrhs_integrate, tpsrhs_nodal_stats and the monitor -- an observer of the device time loop
// (abi_support.hpp: monitor_cadence, monitor_record).
#include "abi_support.hpp"
#include "integrals.hpp"

namespace {
void monitor_off(tpsrhs_operator *h) {
  tpsrhs_integrals_state *is = h->integrals.get();
  if (!is || !is->monitor.cadence.interval) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);  // a record may still be running
  is->monitor = tpsrhs_monitor_log();
}

// a grid of at most INTEG_MAXBLOCKS blocks over ne elements in batches of eb: -> (blocks, elements per block)
void reduction_grid(int ne, int eb, int *blocks, int *run) {
  const int batches = (ne + eb - 1) / eb;
  const int per = std::max(1, (batches + INTEG_MAXBLOCKS - 1) / INTEG_MAXBLOCKS);
  *run = per * eb;
  *blocks = std::max(1, (batches + per - 1) / per);
}

// the state with its scratch, sized once: the grids depend on the mesh and the order only
tpsrhs_integrals_state *integrals_of(tpsrhs_operator *h) {
  if (h->integrals) return h->integrals.get();
  int eb = 0;
  with_dim_order(h, "tpsrhs_integrate", [&](auto dim, auto p) { eb = IntegCfg<decltype(dim)::value, decltype(p)::value>::EB; });
  std::unique_ptr<tpsrhs_integrals_state> is(new tpsrhs_integrals_state());
  is->integ_eb = eb;
  reduction_grid(h->ne, eb, &is->integ_blocks, &is->integ_run);
  const int npe = static_cast<int>(h->ndofs / std::max(h->ne, 1));
  is->stat_lpe = lanes_per_element(npe);
  reduction_grid(h->ne, 64 / is->stat_lpe, &is->stat_blocks, &is->stat_run);
  const int64_t per_row = std::max<int64_t>(2 * static_cast<int64_t>(is->integ_blocks) * eb,
                                             3 * static_cast<int64_t>(is->stat_blocks) * (64 / is->stat_lpe));
  is->d_partial = DevBuf<double>(INTEG_ROWS * per_row);
  h->integrals = owned_state(std::move(is));
  return h->integrals.get();
}

template <int DIM, int P>
void launch_integrate(tpsrhs_operator *h, const tpsrhs_integrals_state *is, const QuadTab &tab, int nrows, const double *field,
                      const double *exact, int radial, double *partial) {
  typedef IntegCfg<DIM, P> C;
  hipLaunchKernelGGL((k_integrate<DIM, P>), dim3(is->integ_blocks), dim3(64), 0, h->stream, h->ne, is->integ_run, nrows, h->ndofs,
                     static_cast<int64_t>(h->ne) * C::NQD, radial, tab, h->d_verts.get(), field, exact, partial);
  HIP_CHECK(hipGetLastError());
}

// sum_out[nrows], sumsq_out[nrows] (either may be NULL) of field[nrows][NDofs] - exact[nrows][npts], on the operator's stream
void integrate_field(tpsrhs_operator *h, int nrows, const double *field, const double *exact, int radial, double *sum_out,
                     double *sumsq_out) {
  tpsrhs_integrals_state *is = integrals_of(h);
  if (h->ne == 0) {
    if (sum_out) HIP_CHECK(hipMemsetAsync(sum_out, 0, sizeof(double) * nrows, h->stream));
    if (sumsq_out) HIP_CHECK(hipMemsetAsync(sumsq_out, 0, sizeof(double) * nrows, h->stream));
    return;
  }
  QuadTab tab = {};
  const int n1 = h->order + 1, nq = quad_points_1d(h->order);
  double nodes[TPSRHS_MAXORDER + 1], wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, n1, nodes, wts);  // the nodes of the operator's basis, as make_tables places them
  gauss_legendre01(nq, tab.g, tab.w);
  for (int q = 0; q < nq; q++)
    for (int a = 0; a < n1; a++) tab.B[q * n1 + a] = lagrange(nodes, n1, a, tab.g[q]);
  const int64_t npts = static_cast<int64_t>(h->ne) * (h->dim == 3 ? nq * nq * nq : nq * nq);
  const int64_t np = static_cast<int64_t>(is->integ_blocks) * is->integ_eb;
  for (int r0 = 0; r0 < nrows; r0 += INTEG_ROWS) {  // the stream orders the launches: one scratch serves every slab of rows
    const int nr = std::min(INTEG_ROWS, nrows - r0);
    const double *f = field + r0 * h->ndofs, *ex = exact ? exact + r0 * npts : nullptr;
    with_dim_order(h, "tpsrhs_integrate", [&](auto dim, auto p) {
      launch_integrate<decltype(dim)::value, decltype(p)::value>(h, is, tab, nr, f, ex, radial, is->d_partial.get());
    });
    hipLaunchKernelGGL(k_integrate_final<1024>, dim3(1), dim3(1024), 0, h->stream, nr, np, is->d_partial.get(),
                       sum_out ? sum_out + r0 : nullptr, sumsq_out ? sumsq_out + r0 : nullptr);
    HIP_CHECK(hipGetLastError());
  }
}

void nodal_stats_field(tpsrhs_operator *h, int nrows, const double *field, double *min_out, double *max_out, double *meanabs_out) {
  tpsrhs_integrals_state *is = integrals_of(h);
  const int npe = static_cast<int>(h->ndofs / std::max(h->ne, 1));
  const int64_t np = static_cast<int64_t>(is->stat_blocks) * (64 / is->stat_lpe);
  for (int r0 = 0; r0 < nrows; r0 += INTEG_ROWS) {
    const int nr = std::min(INTEG_ROWS, nrows - r0);
    // (ne == 0: one block without elements writes the empty partials +inf, -inf, 0)
    hipLaunchKernelGGL(k_nodal_stats, dim3(is->stat_blocks, nr), dim3(64), 0, h->stream, h->ne, is->stat_run, npe, is->stat_lpe,
                       h->ndofs, field + r0 * h->ndofs, is->d_partial.get());
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_nodal_stats_final<1024>, dim3(1), dim3(1024), 0, h->stream, nr, np, h->ndofs, is->d_partial.get(),
                       min_out ? min_out + r0 : nullptr, max_out ? max_out + r0 : nullptr,
                       meanabs_out ? meanabs_out + r0 : nullptr);
    HIP_CHECK(hipGetLastError());
  }
}
}  // namespace

StepCadence *monitor_cadence(tpsrhs_operator *h) { return h->integrals ? &h->integrals->monitor.cadence : nullptr; }

// One monitor record of the device vector x, stream-ordered, or one more dropped record when the buffer is full.
void monitor_record(tpsrhs_operator *h, const double *x) {
  tpsrhs_monitor_log &log = h->integrals->monitor;
  const int64_t r = log.index.claim(log.cadence.count);
  if (r < 0) return;
  const int axisym = h->dim == 2 && h->nvel == 3;
  integrate_field(h, h->neq, x, nullptr, axisym, log.d_totals.get() + r * h->neq, nullptr);
  nodal_stats_field(h, h->neq, x, log.d_mins.get() + r * h->neq, log.d_maxs.get() + r * h->neq, nullptr);
  // {dt of the next step, time}: the loop's control block, which the variable-dt loop never has on the host
  HIP_CHECK(hipMemcpyAsync(log.d_dts.get() + r, h->loop.d_ctl.get(), sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIP_CHECK(hipMemcpyAsync(log.d_times.get() + r, h->loop.d_ctl.get() + 1, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

extern "C" {

int tpsrhs_quadrature_points(const tpsrhs_mesh *mesh, int order, double *xyz_out, double *w_out, int64_t *npts_out) {
  const int st = quadrature_points(mesh, order, xyz_out, w_out, npts_out);
  if (st != TPSRHS_OK)
    return fail(st, "tpsrhs_quadrature_points: needs a mesh of dim 2 or 3 with elem_coords, an order in 1..5 and npts_out");
  return st;
}

int tpsrhs_integrate(tpsrhs_handle h, int nrows, const double *field, const double *exact_q, int radial_weight,
                     double *sum_out, double *sumsq_out) {
  if (!h || !field || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_integrate: needs a handle, nrows >= 1 and the device field");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    integrate_field(h, nrows, field, exact_q, radial_weight ? 1 : 0, sum_out, sumsq_out);
  });
}

int tpsrhs_nodal_stats(tpsrhs_handle h, int nrows, const double *field, double *min_out, double *max_out, double *meanabs_out) {
  if (!h || !field || nrows < 1)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_nodal_stats: needs a handle, nrows >= 1 and the device field");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    nodal_stats_field(h, nrows, field, min_out, max_out, meanabs_out);
  });
}

int tpsrhs_monitor_configure(tpsrhs_handle h, int64_t interval, int64_t capacity) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: NULL handle");
  if (interval < 0 || capacity < 0)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: needs interval >= 0 (0: off) and capacity >= 0");
  if (interval > 0 && capacity < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_configure: needs capacity >= 1");
  return guarded([&] {
    monitor_off(h);
    if (interval == 0) return;
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_integrals_state *is = integrals_of(h);  // with the scratch: a record allocates nothing
    tpsrhs_monitor_log log;
    log.cadence.interval = interval;
    log.index.capacity = capacity;
    log.d_times = DevBuf<double>(capacity);
    log.d_dts = DevBuf<double>(capacity);
    log.d_totals = DevBuf<double>(capacity * h->neq);
    log.d_mins = DevBuf<double>(capacity * h->neq);
    log.d_maxs = DevBuf<double>(capacity * h->neq);
    loop_ctl(h);  // a record copies dt and the time from there
    is->monitor = std::move(log);  // complete: a call that throws above leaves the monitor off
  });
}

int tpsrhs_monitor_read(tpsrhs_handle h, int64_t *nrecords, int64_t *ndropped, int64_t *iters_out, double *times_out,
                        double *dts_out, double *totals_out, double *mins_out, double *maxs_out, int reset) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_read: NULL handle");
  tpsrhs_integrals_state *is = h->integrals.get();
  if (!is || !is->monitor.cadence.interval)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_monitor_read: the monitor is not configured (tpsrhs_monitor_configure)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_monitor_log &log = is->monitor;
    const int64_t n = log.index.nrecords;
    fetch_rows(h, times_out, log.d_times, n, 1);
    fetch_rows(h, dts_out, log.d_dts, n, 1);
    fetch_rows(h, totals_out, log.d_totals, n, h->neq);
    fetch_rows(h, mins_out, log.d_mins, n, h->neq);
    fetch_rows(h, maxs_out, log.d_maxs, n, h->neq);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    read_index(log.index, nrecords, ndropped, iters_out, reset);
  });
}

}  // extern "C"
