// Shared by the translation units of libtpsrhs.so: the operator object behind tpsrhs_handle, with what it owns.  No
// kernel in here: the launch sequence of one RHS evaluation is launch.hpp, for the units that instantiate the sweeps.
#ifndef TPSRHS_OPERATOR_HPP_
#define TPSRHS_OPERATOR_HPP_

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tpsrhs.h"
#include "basis.hpp"
#include "device_buffer.hpp"
#include "kernel_args.hpp"
#include "status.hpp"
#include "topology.hpp"
#include "trace_chain.hpp"

using namespace tpsrhs;

namespace {

constexpr int NKERN = 3;
const char *kKernelNames[NKERN] = {"k_traces", "k_gradient", "k_flux"};

}  // namespace

struct tpsrhs_stats_state;      // statistics.hpp: running mean and velocity covariances (statistics.hip)
struct tpsrhs_sampling_state;   // sampling.hpp: point samplers and probe records (sampling.hip)
struct tpsrhs_integrals_state;  // integrals.hpp: reduction scratch and monitor records (integrals.hip)
struct tpsrhs_surface_state;    // surface.hpp: face sets of boundary patches and their history (surface.hip)
struct tpsrhs_limiter_state;    // limiter.hip: weights, counters and the configured limiter of the time loop
struct tpsrhs_modal_state;      // modal.hip: counters and the configured modal filter of the time loop
// The owner of one of them: its type is complete in the one unit that creates it, which hands the deleter over with it
// (this struct's inline destructor is compiled in every unit, the kernel families included).
template <class T>
using OwnedState = std::unique_ptr<T, void (*)(T *)>;
template <class T>
OwnedState<T> owned_state(std::unique_ptr<T> p) {
  return OwnedState<T>(p.release(), [](T *q) { delete q; });
}

// One step (or pair of steps, steps_per_graph) of tpsrhs_advance / tpsrhs_advance_with as an executable graph: dt lives in
// device memory, so the step replays as is.  Owns the executable as DevBuf owns memory; whoever destroys it does so on the
// device that holds it.
class StepGraph {
 public:
  StepGraph() = default;
  StepGraph(const StepGraph &) = delete;
  StepGraph &operator=(const StepGraph &) = delete;
  ~StepGraph() { reset(); }
  // the graph for `key`: the one at hand, or what `capture` enqueues on `stream`, captured and instantiated in its place
  template <class F>
  void ensure(const StepKey &key, hipStream_t stream, F &&capture) {
    if (exec_ && key_ == key) return;
    reset();
    hipGraph_t g = nullptr;
    HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
      capture();
    } catch (...) {
      (void)hipStreamEndCapture(stream, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    HIP_CHECK(hipStreamEndCapture(stream, &g));
    const hipError_t ie = hipGraphInstantiate(&exec_, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIP_CHECK(ie);
    key_ = key;
  }
  void launch(hipStream_t stream) { HIP_CHECK(hipGraphLaunch(exec_, stream)); }

 private:
  void reset() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    exec_ = nullptr;
  }
  hipGraphExec_t exec_ = nullptr;
  StepKey key_;
};

struct tpsrhs_operator {
  int dim = 0, order = 0, neq = 0, nvel = 0;
  int nc = 0;  // 1: the non-collocated Gauss-Lobatto pair (basisType 1, integrationRule 1), 0: the collocated Gauss-Legendre pair
  DevBuf<double> d_minv;  // nc: [ne][npe][npe] inverse element mass matrices
  int ne = 0, nfaces = 0, nf = 0, nq = 0;
  int64_t ndofs = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  Topology topo;
  tpsrhs_physics phys;
  alignas(16) unsigned char params[4096];  // PH::Params of the selected physics, passed by value
  // device data: every buffer has its owner here (device_buffer.hpp), also those created at their first use
  DevBuf<void> d_chem;                // ChemDev block (plasma)
  DevBuf<void> d_params;              // device image of `params` for the physics that read it through a pointer (plasma)
  std::vector<DevBuf<void>> d_extra;  // what the parameter block points to: table coefficients, search aids, element sizes
  DevBuf<double> d_coulomb;           // coulomb_table.hpp: the Coulomb fits of the 3-D p = 3 argon-minimal sweeps (PlasmaParams::ctab)
  std::vector<DevBuf<void>> d_mixed_out;  // plane-node lists / sum buffers of the current forcing's mixed-out sponge zones
  DevBuf<double> d_verts;
  DevBuf<int2> d_face_info;
  DevBuf<double> d_Up, d_gradUp, d_TA, d_TB;
  // buffer 1 of loop.chain (d_TA is 0), allocated by the first hand-over: k_flux forms the next stage's traces in its epilogue.
  // Single-rank 3-D collocated kernels only (flux_fuses_traces); TPSRHS_FUSE_TRACES=0 keeps the separate sweep.
  DevBuf<double> d_TA2;
  DevBuf<double> d_speed, d_block_speed;
  int flux_grid = 0;
  DevBuf<double> d_xh, d_yh;  // staging for tpsrhs_mult_host
  RkDev rk = {};  // a stage's block is in force for its own launch only (rk4_stages); mode 0: k_flux writes the residual
  MixLenDev mixlen = {nullptr, 0.0, 1.0, 0.0};  // MixingLengthTransport (tpsrhs_set_mixing_length); distance NULL: off
  ForcingDev forcing = {};                  // host copy of the optional forcing terms (tpsrhs_set_forcing / _joule_heating)
  DevBuf<ForcingDev> d_forcing;
  bool forcing_terms = false;   // some term of `forcing` is set: k_forcing runs after the last k_flux launch
  bool forcing_active = false;  // forcing_terms, or reaction rates are set (ext.rates): some pass adds to the residual in memory
  // Reactions whose forward rate coefficient comes from outside (TPSRHS_GRIDFUNCTION_RXN; GridFunctionReaction,
  // src/reaction.cpp:85-117): the second chemistry block, which holds them alone (plasma_params_host.hpp::split_chemistry;
  // d_chem above holds the others), and the caller's rate array of tpsrhs_set_reaction_rates
  struct ExternalRates {
    DevBuf<void> d_chem;            // ChemDev of the external reactions; empty: the operator has none
    int num_reactions = 0;
    int num_components_needed = 0;  // 1 + the largest component index a reaction reads
    const double *rates = nullptr;  // [num_components][ndofs], the caller's; NULL: k_f = 0, no pass
    int num_components = 0;
  } ext;
  // non-reflecting inlet / outlet patches (dry air): their faces {slot, bc index}, slot -> ordinal, the
  // double-buffered boundary state, the patch sums of the primitives, the time step they integrate with
  bool has_nr = false;  // some boundary condition is of a non-reflecting type (possibly without local faces)
  int n_nr_faces = 0;
  DevBuf<int2> d_nr_faces;
  DevBuf<int> d_nr_ordinal;
  DevBuf<double> d_bstate[2];
  int bstate_cur = 0;
  bool bstate_init = false;
  DevBuf<double> d_bc_sums;
  double nr_dt = 0.0;
  const double *nr_dt_dev = nullptr;  // non-NULL while tpsrhs_advance runs: the boundary conditions read dt there
  tpsrhs_reduce_fn reduce = nullptr;
  void *reduce_ctx = nullptr;
  // The device time loop (tpsrhs_step / _rk4_step / _advance / _advance_with): what it keeps between stages, steps and
  // calls.  The rules are in trace_chain.hpp.
  struct TimeLoop {
    DevBuf<double> d_rk;               // k | y | z of the stages; stage_scratch (time_loop.hip) allocates both at the first step
    DevBuf<unsigned long long> d_nan;  // the NaN census: zeroed by step_with / advance_with per call, counted by the stages
    int sp_first = 0, sp_last = 0;     // the species rows Check_Undershoot clamps; setup, from the plan
    DevBuf<double> d_ctl;              // {dt, time, max speed}: loop_ctl allocates, advance_with and k_step_end write
    StepGraph graph;                   // advance_with, through ensure
    TraceChain chain;                  // launch_all asks mult(); rk4_stages, rk_stages and advance_with make the transitions
    int config_epoch = 0;              // bumped by whatever changes what a step launches: the forcing, mixing-length, limiter and modal-filter setters
    bool sweep_alt = true;             // alternate the direction of consecutive sweeps (launch_all); setup, TPSRHS_SWEEP_ALT
    int sweep_parity = 0;              // launch_all flips it once per Mult
  } loop;
  // halo
  tpsrhs_halo_fn halo = nullptr;
  void *halo_ctx = nullptr;
  hipStream_t comm_stream = nullptr;  // second stream: pack + exchange overlap the interior blocks
  hipEvent_t ev_halo[4] = {};         // traces of the halo blocks ready / TA received / TB ready / TB received
  DevBuf<int> d_blocks_halo, d_blocks_interior;
  int n_blocks_halo = 0, n_blocks_interior = 0;
  DevBuf<int32_t> d_shared_slot;
  DevBuf<uint8_t> d_shared_orient;
  DevBuf<double> d_send;
  std::vector<int64_t> send_off[2], recv_off[2];
  // timing
  // per-kernel timing: a ring of event sets so that a timed loop never synchronises
  static constexpr int MAXSETS = 128;
  bool timing = false;
  hipEvent_t evs[MAXSETS][NKERN + 1] = {};
  int64_t sets_recorded = 0;
  hipEvent_t *ev = evs[0];

  void (*launch)(tpsrhs_operator *, const double *, double *, bool) = nullptr;
  void (*point_eval)(tpsrhs_operator *, int, int64_t, const double *, double *) = nullptr;
  VsDev vs2d = {};  // viscous sponge of the 2-D heavy kernels (MeshDev::vs); enabled = 0: none
  // tpsrhs_visualization_fields: the post-processing passes of the plasma families (visualization.hpp); NULL for every other
  // physics
  void (*vis_fields)(tpsrhs_operator *, const VisRows &, const double *, double *) = nullptr;
  // external_rates.hpp, set with vis_fields from the same shared object: the pass of the external reactions (y += their
  // sources, after the last k_flux launch of a Mult: launch.hpp) and tpsrhs_boltzmann_fields
  void (*ext_reactions)(tpsrhs_operator *, const double *, double *) = nullptr;
  void (*boltzmann_fields)(tpsrhs_operator *, const double *, int, double *) = nullptr;
  // tpsrhs_stats_configure / tpsrhs_sampler_create, tpsrhs_probe_configure / tpsrhs_integrate, tpsrhs_monitor_configure /
  // tpsrhs_surface_create, tpsrhs_surface_monitor_configure;
  // NULL: none yet.  Last, and reset first in the destructor: they go while the events and the second stream still exist.
  // Whoever lets one go while its kernels may still run synchronises the stream first (tpsrhs_destroy, the configure calls).
  OwnedState<tpsrhs_stats_state> stats{nullptr, nullptr};
  OwnedState<tpsrhs_sampling_state> sampling{nullptr, nullptr};
  OwnedState<tpsrhs_integrals_state> integrals{nullptr, nullptr};
  OwnedState<tpsrhs_surface_state> surface{nullptr, nullptr};

  MeshDev mesh_dev() const {
    MeshDev m;
    m.blocks = nullptr;
    m.ne = ne;
    m.reverse = 0;
    m.ndofs = ndofs;
    m.verts = d_verts.get();
    m.face_info = d_face_info.get();
    m.minv = d_minv.get();
    m.ml = mixlen;
    m.vs = vs2d;
    return m;
  }
  // what is not memory; the buffers free themselves after this body, on the device set here
  ~tpsrhs_operator() {
    (void)hipSetDevice(device);
    stats.reset();
    sampling.reset();
    integrals.reset();
    surface.reset();
    limiter.reset();
    modal.reset();
    for (auto &e : ev_halo)
      if (e) (void)hipEventDestroy(e);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (auto &set : evs)
      for (auto &e : set)
        if (e) (void)hipEventDestroy(e);
  }
  // tpsrhs_get_flux (flux_fields.hpp): the pass of a plasma family, set with vis_fields from the same shared object; NULL for
  // every other physics, whose passes live in flux_fields.hip.  (part, x, out) on the operator's stream.  (It was
  // appended when the units of the sweeps could be older than the core; a full build compiles every unit against this header,
  // so the order of the members means nothing: state that comes later is appended below.)
  void (*flux_fields)(tpsrhs_operator *, int, const double *, double *) = nullptr;
  // tpsrhs_limiter_weights / tpsrhs_limit / tpsrhs_limiter_configure (limiter.hip): the weights W_n, the counters and the
  // limiter the time loop applies after every step; NULL: none yet.  Reset with the other states in the destructor.
  OwnedState<tpsrhs_limiter_state> limiter{nullptr, nullptr};
  // tpsrhs_modal_filter_apply / tpsrhs_modal_filter_configure / tpsrhs_modal_filter_read (modal.hip): the counters and the
  // filter the time loop applies after the stages of every step, before the limiter; NULL: none yet.
  OwnedState<tpsrhs_modal_state> modal{nullptr, nullptr};
};

#endif
