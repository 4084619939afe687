// The device time loop of libtpsrhs.so: tpsrhs_rk4_step, tpsrhs_step, tpsrhs_advance and tpsrhs_advance_with.  Its state
// is tpsrhs_operator::loop; the rules of the trace chain are in trace_chain.hpp, the stage kernels in time_integrators.hpp.
// No kernel of the sweeps in here: a Mult is h->launch.  Whatever reads x between two steps -- the statistics, the probe
// records, the monitor -- is an observer (abi_support.hpp): the loop knows its StepCadence and one function.
#include "abi_support.hpp"
#include "time_integrators.hpp"

#include <algorithm>

namespace {
// The stage vectors in loop.d_rk (3 n doubles, with loop.d_nan allocated at the first step): k | y | z, or k | y with y on
// an even offset, so that an odd n keeps the 16-byte accesses (y then ends at or before 2 n + 1 <= 3 n).
struct StageScratch {
  double *k, *y, *z;
};
StageScratch stage_scratch(tpsrhs_operator *h, int64_t n, bool even_offsets) {
  tpsrhs_operator::TimeLoop &lp = h->loop;
  if (!lp.d_rk) {
    lp.d_rk = DevBuf<double>(3 * n);
    lp.d_nan = DevBuf<unsigned long long>(1);
    HIP_CHECK(hipMemsetAsync(lp.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
  }
  double *k = lp.d_rk.get();
  if (even_offsets) return {k, k + ((n + 1) & ~static_cast<int64_t>(1)), nullptr};
  return {k, k + n, k + 2 * n};
}

// the four stages of MFEM's RK4Solver::Step around Mult; dt by value or from device memory (dt_dev)
void rk4_stages(tpsrhs_operator *h, double *x, double dt, const double *dt_dev) {
  const int64_t n = static_cast<int64_t>(h->neq) * h->ndofs;
  const StageScratch sc = stage_scratch(h, n, false);
  double *k = sc.k, *y = sc.y, *z = sc.z;
  TraceChain &chain = h->loop.chain;
  chain.begin_step();
  ScopeExit step([&](bool) { chain.end_step(); });
  // Check_Undershoot's rows; none when the limiter has taken them over (limiter.hpp)
  const int sp_first = h->loop.sp_first, sp_last = limiter_replaces_clamp(h) ? sp_first : h->loop.sp_last;
  const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 8192));
  if (!h->forcing_active) {
    // The stage combinations in k_flux's epilogue (RkDev, kernel_args.hpp): k never goes to memory, the accumulator of
    // RK4Solver::Step is recovered from the stage states at the end.  (The optional forcing terms add to the residual in
    // a pass of their own after k_flux: with them the separate stage kernel below stays.)
    double *y2 = k, *y3 = y, *y4 = z;  // the three stage states
    const double *ins[4] = {x, y2, y3, y4};
    double *outs[4] = {y2, y3, y4, x};
    for (int stage = 1; stage <= 4; stage++) {
      RkDev r = {};
      r.mode = stage;
      r.sp_first = sp_first;
      r.sp_last = sp_last;
      r.dt_host = dt;
      r.dt_dev = dt_dev;
      r.x0 = x;
      r.y2 = y2;
      r.y3 = y3;
      r.y4 = y4;
      r.out = outs[stage - 1];
      r.nan_count = h->loop.d_nan.get();
      h->rk = r;  // in force for this launch only
      ScopeExit launched([&](bool failed) {
        h->rk = RkDev{};
        if (failed) chain.abandon();
      });
      h->launch(h, ins[stage - 1], outs[stage - 1], false);
    }
    return;
  }
  const double *in = x;
  for (int stage = 1; stage <= 4; stage++) {
    h->launch(h, in, k, false);  // k_s = f(stage input); SetTime is a no-op for this operator
    hipLaunchKernelGGL(k_rk4_stage<256>, dim3(grid), dim3(256), 0, h->stream, stage, n, h->ndofs, sp_first, sp_last, dt,
                       dt_dev, x, k, y, z, h->loop.d_nan.get());
    HIP_CHECK(hipGetLastError());
    in = y;
  }
}

// Forward Euler, RK2(a = 1) and RK3-SSP (time_integrators.hpp): the plain Mult (h->rk stays RkDev{}: k_flux writes the
// residual, nothing enters the trace chain) and one k_rk_stage pass per stage.  (Fusing these combinations into k_flux's
// epilogue, as RK4 has, is left out on purpose: DESIGN.md section 9.)
template <int OP>
void rk_stage(tpsrhs_operator *h, int64_t n, int64_t clamp_lo, int64_t clamp_hi, double dt, const double *dt_dev, double *x,
              const double *k, double *y) {
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int64_t items = vec ? (n + 1) / 2 : n;
  const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 8192));  // the grid cap of k_rk4_stage
  if (vec)
    hipLaunchKernelGGL((k_rk_stage<OP, true, 256>), dim3(grid), dim3(256), 0, h->stream, n, clamp_lo, clamp_hi, dt, dt_dev, x, k, y,
                       h->loop.d_nan.get());
  else
    hipLaunchKernelGGL((k_rk_stage<OP, false, 256>), dim3(grid), dim3(256), 0, h->stream, n, clamp_lo, clamp_hi, dt, dt_dev, x, k, y,
                       h->loop.d_nan.get());
  HIP_CHECK(hipGetLastError());
}

void rk_stages(tpsrhs_operator *h, int integrator, double *x, double dt, const double *dt_dev) {
  const int64_t n = static_cast<int64_t>(h->neq) * h->ndofs;
  const StageScratch sc = stage_scratch(h, n, true);
  double *k = sc.k, *y = sc.y;
  h->loop.chain.begin_step();  // every Mult of these schemes runs its own k_traces sweep
  ScopeExit step([h](bool) { h->loop.chain.end_step(); });
  // Check_Undershoot's rows, contiguous in [neq][ndofs]; none when the limiter has taken them over (limiter.hpp)
  const int64_t lo = h->loop.sp_first * h->ndofs, hi = limiter_replaces_clamp(h) ? lo : h->loop.sp_last * h->ndofs;
  h->launch(h, x, k, false);  // k = f(x); SetTime is a no-op for this operator
  if (integrator == TPSRHS_FORWARD_EULER) {
    rk_stage<RK_EULER>(h, n, lo, hi, dt, dt_dev, x, k, y);
  } else if (integrator == TPSRHS_RK2) {
    rk_stage<RK2_STAGE1>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK2_STAGE2>(h, n, lo, hi, dt, dt_dev, x, k, y);
  } else {
    rk_stage<RK3_STAGE1>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK3_STAGE2>(h, n, lo, hi, dt, dt_dev, x, k, y);
    h->launch(h, y, k, false);
    rk_stage<RK3_STAGE3>(h, n, lo, hi, dt, dt_dev, x, k, y);
  }
}

// TPSRHS_OK for the integrators that are built; the status of the others, before any device work
int check_integrator(int integrator, const char *who) {
  switch (integrator) {
    case TPSRHS_FORWARD_EULER:
    case TPSRHS_RK2:
    case TPSRHS_RK3_SSP:
    case TPSRHS_RK4: return TPSRHS_OK;
    case TPSRHS_RK6:
      return fail(TPSRHS_ERR_UNSUPPORTED, std::string(who) + ": the RK6 integrator (MFEM's eight-stage Verner scheme) is not built; "
                                              "forwardEuler, rk2, rk3 and rk4 are");
    default:
      return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown integrator " + std::to_string(integrator) +
                                                   " (the reference's timeIntegratorType: 1, 2, 3, 4 or 6)");
  }
}

// One step: the stage sequence, then the modal filter when one is configured (k_modal_filter), then the limiter when one
// is configured (k_limit, the last launch that writes x and the last word on the floors: the observers and the next step
// see the filtered, then limited state; the step size of the next step still comes from the last stage).
void step_stages(tpsrhs_operator *h, int integrator, double *x, double dt, const double *dt_dev) {
  if (integrator == TPSRHS_RK4)
    rk4_stages(h, x, dt, dt_dev);
  else
    rk_stages(h, integrator, x, dt, dt_dev);
  if (modal_filter_active(h)) modal_filter_apply(h, x);
  if (limiter_active(h)) limiter_apply(h, x);
}

// What the time loop does between two steps, and whether any of it falls after the first of the next two: everything that
// reads x between steps goes through these two, so that the loop itself knows nothing about statistics, probes, the
// monitor or the patch history.  Each observer has one StepCadence (record_log.hpp; interval 0: off), which answers both questions.
void after_step(tpsrhs_operator *h, const double *x) {
  if (StepCadence *c = stats_cadence(h); c && c->tick()) stats_sample(h, x);
  if (StepCadence *c = probe_cadence(h); c && c->tick()) probe_record(h, x);
  if (StepCadence *c = monitor_cadence(h); c && c->tick()) monitor_record(h, x);
  if (StepCadence *c = surface_cadence(h); c && c->tick()) surface_record(h, x);
}
bool work_due_after_next(tpsrhs_operator *h) {
  const StepCadence *s = stats_cadence(h), *p = probe_cadence(h), *m = monitor_cadence(h), *f = surface_cadence(h);
  return (s && s->due_after_next()) || (p && p->due_after_next()) || (m && m->due_after_next()) || (f && f->due_after_next());
}

int step_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double dt, double *max_char_speed,
              int64_t *nan_count) {
  if (!h || !x || !time) return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (const int st = check_integrator(integrator, who)) return st;
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    h->nr_dt = dt;  // the boundary conditions see M2ulPhyS::dt (src/BoundaryCondition.hpp:54)
    if (h->loop.d_nan) HIP_CHECK(hipMemsetAsync(h->loop.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
    step_stages(h, integrator, x, dt, nullptr);
    *time += dt;
    if (max_char_speed || nan_count) {
      hipLaunchKernelGGL(k_reduce_max<1024>, dim3(1), dim3(1024), 0, h->stream, h->flux_grid, h->d_block_speed.get(), h->d_speed.get());
      HIP_CHECK(hipGetLastError());
      double speed = 0.0;
      unsigned long long bad = 0;
      HIP_CHECK(hipMemcpyAsync(&speed, h->d_speed.get(), sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipMemcpyAsync(&bad, h->loop.d_nan.get(), sizeof(bad), hipMemcpyDeviceToHost, h->stream));
      HIP_CHECK(hipStreamSynchronize(h->stream));
      if (max_char_speed) *max_char_speed = speed;
      if (nan_count) *nan_count = static_cast<int64_t>(bad);
    }
  });
}

// The stage sequence (step_stages) is all that depends on the integrator: the end of the step, the MIN reduce, the graph,
// the error paths and the read-back are shared.
int advance_with(tpsrhs_handle h, int integrator, const char *who, double *x, double *time, double *dt, int num_steps,
                 int constant_dt, double cfl, double hmin, int64_t *nan_count) {
  TPSRHS_RECIPROCAL_DIVISION  // coef below: cfl * hmin * (1 / dim), as this function has always been compiled
  if (!h || !x || !time || !dt) return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (const int st = check_integrator(integrator, who)) return st;
  if (num_steps < 0 || !(*dt > 0.0) || (!constant_dt && !(cfl > 0.0 && hmin > 0.0)))
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, std::string(who) + ": needs num_steps >= 0, dt > 0 and (constant dt or cfl, hmin > 0)");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    if (!constant_dt && h->topo.num_shared > 0 && !h->reduce)
      throw HaloError("halo: a variable time step on a partitioned mesh needs runtime.reduce");
    double *const d_ctl = loop_ctl(h);
    const double ctl0[3] = {*dt, *time, 0.0};
    HIP_CHECK(hipMemcpyAsync(d_ctl, ctl0, sizeof(ctl0), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));  // ctl0 lives on this stack frame
    if (h->loop.d_nan) HIP_CHECK(hipMemsetAsync(h->loop.d_nan.get(), 0, sizeof(unsigned long long), h->stream));
    const double coef = cfl * hmin / static_cast<double>(h->dim);
    auto one_step = [&] {
      step_stages(h, integrator, x, 0.0, d_ctl);
      hipLaunchKernelGGL(k_step_end<1024>, dim3(1), dim3(1024), 0, h->stream, h->flux_grid, h->d_block_speed.get(), d_ctl,
                         constant_dt ? 1 : 0, coef);
      HIP_CHECK(hipGetLastError());
      if (!constant_dt && h->reduce && h->topo.num_shared > 0) {  // MPI_Allreduce(MIN) of src/M2ulPhyS.cpp:2015
        if (h->reduce(h->reduce_ctx, d_ctl, 1, TPSRHS_REDUCE_MIN, h->stream) != 0) throw HaloError("halo: reduce callback failed");
      }
    };
    // On one rank a step is a fixed sequence of launches (~17 for RK4) whose arguments do not change from step to step (dt
    // and the time are in device memory; the two boundary-state buffers swap four times per step): captured once
    // into a hipGraph and replayed -- the launch overhead matters on small meshes.  Needs a capturable stream (not
    // the NULL stream), no host callbacks in the step (partitioned meshes keep the plain loop), no timing events.
    const char *genv = std::getenv("TPSRHS_GRAPH");
    const bool use_graph = h->stream != nullptr && h->topo.num_shared == 0 && !h->timing && num_steps >= 3 &&
                           !(genv && genv[0] == '0');
    const int per_graph = steps_per_graph(integrator, h->n_nr_faces > 0);
    {
      // the session: the boundary conditions read dt from device memory, the steps are chained; put back however it ends
      h->nr_dt_dev = d_ctl;
      // (a limiter or a modal filter rewrites x after stage 4: the traces stage 4 would leave for the next step would be stale)
      h->loop.chain.begin_advance(integrator == TPSRHS_RK4 && !h->forcing_active && !limiter_active(h) && !modal_filter_active(h));
      ScopeExit session([&](bool) {
        h->nr_dt_dev = nullptr;
        h->loop.chain.end_advance();
      });
      // Running statistics and probe records: the host issues every step anyway and knows the iteration number, so it
      // enqueues the sample or the record between two steps -- never inside the captured graph, whose key knows about neither.
      int step = 0;
      if (use_graph) {
        one_step();  // first step outside the graph: allocations, initial boundary state, its own k_traces sweep
        after_step(h, x);
        step = 1;
        StepKey key;
        key.x = x;
        key.constant_dt = constant_dt ? 1 : 0;
        key.bstate_cur = h->bstate_cur;
        key.epoch = h->loop.config_epoch;
        key.integrator = integrator;
        key.coef = coef;
        h->loop.graph.ensure(key, h->stream, [&] {
          for (int i = 0; i < per_graph; i++) one_step();
        });
        for (; step + per_graph <= num_steps; step += per_graph) {
          // a sample or a record between the two steps of one graph: the pair runs as two plain steps (bit-equal to the
          // replay, as the odd remainder below is), which leave the boundary-state buffers as the graph does
          const bool split = per_graph == 2 && work_due_after_next(h);
          for (int i = 0; i < per_graph; i++) {
            if (split)
              one_step();
            else if (i == 0)
              h->loop.graph.launch(h->stream);
            after_step(h, x);
          }
        }
      }
      for (; step < num_steps; step++) {
        one_step();
        after_step(h, x);
      }
    }
    double ctl[3] = {0, 0, 0};
    unsigned long long bad = 0;
    HIP_CHECK(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, h->stream));
    if (h->loop.d_nan) HIP_CHECK(hipMemcpyAsync(&bad, h->loop.d_nan.get(), sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    *dt = ctl[0];
    *time = ctl[1];
    h->nr_dt = ctl[0];
    if (nan_count) *nan_count = static_cast<int64_t>(bad);
  });
}
}  // namespace

extern "C" {

int tpsrhs_rk4_step(tpsrhs_handle h, double *x, double *time, double dt, double *max_char_speed, int64_t *nan_count) {
  return step_with(h, TPSRHS_RK4, "tpsrhs_rk4_step", x, time, dt, max_char_speed, nan_count);
}

int tpsrhs_step(tpsrhs_handle h, int integrator, double *x, double *time, double dt, double *max_char_speed,
                int64_t *nan_count) {
  return step_with(h, integrator, "tpsrhs_step", x, time, dt, max_char_speed, nan_count);
}

int tpsrhs_advance(tpsrhs_handle h, double *x, double *time, double *dt, int num_steps, int constant_dt, double cfl,
                   double hmin, int64_t *nan_count) {
  return advance_with(h, TPSRHS_RK4, "tpsrhs_advance", x, time, dt, num_steps, constant_dt, cfl, hmin, nan_count);
}

int tpsrhs_advance_with(tpsrhs_handle h, int integrator, double *x, double *time, double *dt, int num_steps,
                        int constant_dt, double cfl, double hmin, int64_t *nan_count) {
  return advance_with(h, integrator, "tpsrhs_advance_with", x, time, dt, num_steps, constant_dt, cfl, hmin, nan_count);
}

}  // extern "C"
