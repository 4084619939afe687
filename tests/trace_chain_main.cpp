// Stand-alone driver of tps_amd/csrc/trace_chain.hpp (tests/test_trace_chain.py builds it with plain g++, once without and
// once with -fsanitize=address,undefined, and runs it as a child process).  For every combination of fusing on / off,
// eligible / ineligible kernel and single rank / partitioned mesh it makes the calls a driver's time loop makes -- as
// launch_all, rk4_stages, rk_stages and advance_with of the library make them -- and prints what every Mult is told.  The
// expected lines are recomputed in Python from the rules.
#include <cstdio>
#include <stdexcept>

#include "../tps_amd/csrc/trace_chain.hpp"

using namespace tpsrhs;

namespace {

struct Driver {
  TraceChain chain;
  bool eligible, partitioned;
  int rk_mode = 0;  // the operator's RkDev::mode: a stage's block is in force for its own launch only

  void mult(bool gradients_only = false, bool launch_fails = false) {
    const TraceChain::Mult m = chain.mult(eligible, rk_mode, gradients_only, partitioned);
    std::printf("mult stage %d gradients_only %d read %d have_traces %d write %d valid %d\n", rk_mode, gradients_only ? 1 : 0, m.read,
                m.have_traces ? 1 : 0, m.write, chain.valid() ? 1 : 0);
    if (launch_fails) throw std::runtime_error("launch failed");
  }
  // rk4_stages without forcing terms; `between`, after stage 2: 1 a plain Mult, 2 gradients only, 3 stage 3's launch fails
  // and the step is taken again from stage 3 (what no driver does: it shows what the failure left)
  void rk4_step(int between = 0) {
    chain.begin_step();
    ScopeExit step([&](bool) { chain.end_step(); });
    for (int stage = 1; stage <= 4; stage++) {
      if (stage == 3 && between == 1) mult();
      if (stage == 3 && between == 2) mult(true);
      for (int attempt = 0; attempt < 2; attempt++) {
        const bool fails = stage == 3 && between == 3 && attempt == 0;
        try {
          rk_mode = stage;
          ScopeExit launched([&](bool failed) {
            rk_mode = 0;
            if (failed) chain.abandon();
          });
          mult(false, fails);
        } catch (const std::runtime_error &) {
          std::printf("failed valid %d rk_mode %d\n", chain.valid() ? 1 : 0, rk_mode);
        }
        if (!fails) break;
      }
    }
  }
  // rk_stages (forward Euler, RK2, RK3-SSP) and rk4_stages with forcing terms: plain Mults
  void plain_step(int mults) {
    chain.begin_step();
    ScopeExit step([&](bool) { chain.end_step(); });
    for (int i = 0; i < mults; i++) mult();
  }
  void state(const char *what) { std::printf("%s valid %d chained %d\n", what, chain.valid() ? 1 : 0, chain.chained() ? 1 : 0); }
};

}  // namespace

int main() {
  for (int fuse = 0; fuse < 2; fuse++)
    for (int eligible = 0; eligible < 2; eligible++)
      for (int partitioned = 0; partitioned < 2; partitioned++) {
        std::printf("case fuse %d eligible %d partitioned %d\n", fuse, eligible, partitioned);
        Driver d;
        d.eligible = eligible != 0;
        d.partitioned = partitioned != 0;
        d.chain.set_fusing(fuse != 0);
        std::printf("lone_rk4\n");
        d.rk4_step();
        d.state("end");
        std::printf("advance_rk4\n");
        {
          d.chain.begin_advance(true);
          ScopeExit session([&](bool) { d.chain.end_advance(); });
          for (int step = 0; step < 3; step++) d.rk4_step();
          d.state("inside");
        }
        d.state("end");
        for (int between = 1; between <= 3; between++) {
          std::printf("interrupted %d\n", between);
          d.rk4_step(between);
          d.state("end");
        }
        std::printf("advance_interrupted\n");
        try {
          d.chain.begin_advance(true);
          ScopeExit session([&](bool) { d.chain.end_advance(); });
          d.rk4_step();
          d.rk_mode = 1;
          d.mult(false, true);  // stage 1 of the second step fails and ends the advance
        } catch (const std::runtime_error &) {
          d.rk_mode = 0;
          d.state("failed");
        }
        d.rk4_step();
        d.state("end");
        for (int integrator : {TPSRHS_FORWARD_EULER, TPSRHS_RK2, TPSRHS_RK3_SSP, TPSRHS_RK4}) {
          std::printf("advance_plain %d\n", integrator);  // (RK4: with forcing terms)
          d.chain.begin_advance(false);
          ScopeExit session([&](bool) { d.chain.end_advance(); });
          for (int step = 0; step < 2; step++) d.plain_step(mults_per_step(integrator));
          d.state("inside");
        }
        d.state("end");
      }
  for (int integrator : {TPSRHS_FORWARD_EULER, TPSRHS_RK2, TPSRHS_RK3_SSP, TPSRHS_RK4})
    for (int nr = 0; nr < 2; nr++)
      std::printf("steps_per_graph integrator %d nr_faces %d mults %d steps %d\n", integrator, nr, mults_per_step(integrator),
                  steps_per_graph(integrator, nr != 0));
  StepKey a, b;
  b.integrator = TPSRHS_RK2;
  std::printf("step_key same %d other_integrator %d\n", a == StepKey() ? 1 : 0, a == b ? 1 : 0);
  std::printf("TRACE_CHAIN DONE\n");
  return 0;
}
