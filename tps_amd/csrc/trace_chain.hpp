// The host state of the device time loop that can go stale without producing a NaN, and the rules that keep it right:
// the trace chain (which buffer holds the face-node traces of the next Mult's input), the key of the captured step graph,
// and the scope that puts loop state back when a step or an advance ends, whichever way.  Plain C++17, no HIP:
// tests/trace_chain_main.cpp drives it on the host.
//
// The trace chain.  k_flux of RK4 stages 1..3 forms the next stage's traces in its epilogue (RkDev::ta_out, kernels.hpp),
// so the next Mult starts at k_gradient; inside an advance stage 4 does the same for the next step's stage 1 (`chained`),
// because nothing touches x between two steps of one call.  There are two buffers, named by index: 0 is the operator's
// d_TA, 1 its d_TA2 (allocated at first use).  A Mult that reads one writes the other.  Only launch_all (launch.hpp) asks
// mult(); the stage functions and advance_with (time_loop.hip) make the transitions; nothing else writes the flags.
//   - Even number of swaps: a chained step hands over four times (stages 1..4), so it starts by reading buffer 0 and ends
//     by writing buffer 0 -- every step of an advance, and so every replay of a captured step, sees the buffers as the
//     captured one did.  A lone step hands over three times and leaves nothing valid.
//   - Anything that is not the next stage of the same step -- a plain Mult, gradients only, a kernel that cannot fuse, a
//     failed launch -- invalidates the chain: the Mult after it sweeps its own traces into buffer 0.
//
// Why StepKey = (x, constant_dt, bstate_cur, config_epoch, integrator, cfl hmin / dim) is enough to decide a replay -- what
// else could change what a replayed step launches, and why it cannot:
//   - chained is (RK4 and no forcing and no limiter and no modal filter), and forcing changes only in tpsrhs_set_forcing /
//     tpsrhs_set_joule_heating, which bump config_epoch.
//   - the modal filter (modal.hip): a configured filter adds one launch, k_modal_filter, after the stages and before
//     k_limit; it rewrites x after stage 4, so the advance is not chained, by the rule and for the reason stated for the
//     limiter below.  Whether it runs and everything it runs with (the matrix F, the rows, the sensor row and threshold,
//     the conservative flag: kernel arguments by value; the weights: a buffer the operator owns for its lifetime) change
//     only in tpsrhs_modal_filter_configure, which bumps config_epoch.  It leaves the clamp range of the stages alone.
//   - the limiter (limiter.hip): a configured limiter makes the last launch of a step k_limit, which rewrites x after stage
//     4 -- the traces stage 4 would leave for the next step would be stale, so the advance is not chained, the rule stated
//     for forcing terms.  Whether it runs, its rows and floors (kernel arguments by value) and the clamp range of the stage
//     kernels change only in tpsrhs_limiter_configure, which bumps config_epoch.
//   - validity and the buffers: the first step of every advance runs outside the graph, after begin_advance (a k_traces
//     sweep of its own), and the even number of swaps above does the rest.  Fusing is fixed when the operator is created.
//   - sweep_parity: only the order in which the workgroups walk the block list.  Every element's outputs depend on the
//     buffers of the previous sweep only, and the reductions over blocks (max char speed, NaN census) are a max and an
//     integer sum, so the direction cannot change a number.
//   - bstate_init: false only until the first Mult of an operator with non-reflecting faces.  The first step of every
//     advance runs outside the graph, so every captured step has it true, and nothing sets it back.
//   - nr_dt, which the dry-air parameter block carries by value: inside advance the boundary kernels read dt from device
//     memory (nr_dt_dev = d_ctl), never the block's copy.
// tests/test_gpu_time_loop.py crosses each of these on the device (fused against plain against the oracle).
#ifndef TPSRHS_TRACE_CHAIN_HPP_
#define TPSRHS_TRACE_CHAIN_HPP_

#include <exception>
#include <utility>

#include "../../include/tpsrhs.h"

namespace tpsrhs {

class TraceChain {
 public:
  // what one Mult does about traces: the buffer it reads, whether that buffer already holds them (no k_traces sweep), and
  // the buffer k_flux writes the next Mult's into (-1: none)
  struct Mult {
    int read = 0;
    bool have_traces = false;
    int write = -1;
  };
  // eligible: flux_fuses_traces<C, PH>() of the kernel; stage: RkDev::mode (0: a plain Mult)
  Mult mult(bool eligible, int stage, bool gradients_only, bool partitioned) {
    Mult m;
    // the previous stage of this step left them (its output is this input) -- or, chained, stage 4 of the previous step
    if (eligible && valid_ && (stage >= 2 || (stage == 1 && chained_))) {
      m.read = next_;
      m.have_traces = true;
    }
    valid_ = false;
    if (eligible && fuse_ && !gradients_only && !partitioned && stage >= 1 && (stage <= 3 || chained_)) {
      m.write = next_ = 1 - m.read;
      valid_ = true;
    }
    return m;
  }
  void set_fusing(bool on) { fuse_ = on; }  // TPSRHS_FUSE_TRACES, when the operator is created
  // a step starts with its own sweep unless an advance chains it to its predecessor: x may have been touched since the
  // last call; and it leaves nothing behind for whoever calls next
  void begin_step() {
    if (!chained_) valid_ = false;
  }
  void end_step() { begin_step(); }
  // chained: RK4 without forcing terms, without a limiter and without a modal filter (with forcing the stage kernel runs
  // and nothing is fused; a limiter or a filter rewrites x after stage 4; the other integrators never enter the chain)
  void begin_advance(bool chained) {
    valid_ = false;
    chained_ = chained;
  }
  void end_advance() { begin_advance(false); }  // the caller owns x again
  void abandon() { valid_ = false; }            // a launch failed: what it was to hand over does not exist

  bool valid() const { return valid_; }
  bool chained() const { return chained_; }

 private:
  bool fuse_ = true;
  bool valid_ = false;    // buffer next_ holds the traces of the input of the stage that runs next
  bool chained_ = false;  // inside an advance: stage 4 leaves the traces of the new solution for the next step
  int next_ = 0;
};

// One captured step (or pair of steps) of tpsrhs_advance / tpsrhs_advance_with is replayed when, and only when, its key
// matches (the argument is at the top of this file).  The key holds the integrator: a step captured for one scheme is
// never replayed for another.
struct StepKey {
  const void *x = nullptr;
  int constant_dt = 0, bstate_cur = 0, epoch = 0;
  int integrator = TPSRHS_RK4;
  double coef = 0.0;
  bool operator==(const StepKey &o) const {
    return x == o.x && constant_dt == o.constant_dt && bstate_cur == o.bstate_cur && epoch == o.epoch &&
           integrator == o.integrator && coef == o.coef;
  }
};
// (tpsrhs_integrator, the reference's timeIntegratorType, is the stage count of the four schemes that are built)
inline int mults_per_step(int integrator) { return integrator == TPSRHS_RK4 ? 4 : integrator; }
// A replayed graph must leave the boundary-state buffers as it found them, and they swap once per Mult: with
// non-reflecting faces a scheme with an odd number of Mults per step (Euler 1, RK3 3) is captured two steps at a time.
inline int steps_per_graph(int integrator, bool nr_faces) { return (nr_faces && (mults_per_step(integrator) & 1)) ? 2 : 1; }

// Runs f(failed) when the scope ends; failed: an exception is passing through it.  The time loop's state that is in force
// for one launch (RkDev) or one advance (dt in device memory, the chained mode) is put back here, once, instead of at the
// end of the normal path and again in a handler.
template <class F>
class ScopeExit {
 public:
  explicit ScopeExit(F f) : f_(std::move(f)) {}
  ~ScopeExit() { f_(std::uncaught_exceptions() > pending_); }
  ScopeExit(const ScopeExit &) = delete;
  ScopeExit &operator=(const ScopeExit &) = delete;

 private:
  F f_;
  int pending_ = std::uncaught_exceptions();
};

}  // namespace tpsrhs
#endif
