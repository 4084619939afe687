// Shared by the translation units of libtpsrhs.so: the operator object behind tpsrhs_handle and the
// templated launch sequence of one RHS evaluation.  Kernels are instantiated per physics family in
// separate .hip files (compiled in parallel); each has its own copy of the __constant__ tables.
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
#include "kernels.hpp"
#include "topology.hpp"
#include "trace_chain.hpp"
#include "unsupported.hpp"

using namespace tpsrhs;

namespace {

constexpr int NKERN = 3;
const char *kKernelNames[NKERN] = {"k_traces", "k_gradient", "k_flux"};

}  // namespace

struct tpsrhs_stats_state;  // statistics.hpp: running mean and velocity covariances (tpsrhs.hip only)
struct tpsrhs_sampling_state;  // sampling.hpp: point samplers and probe records (tpsrhs.hip only)
struct tpsrhs_integrals_state;  // integrals.hpp: reduction scratch and monitor records (tpsrhs.hip only)

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
  bool forcing_active = false;
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
    DevBuf<double> d_rk;               // k | y | z of the stages; stage_scratch (tpsrhs.hip) allocates both at the first step
    DevBuf<unsigned long long> d_nan;  // the NaN census: zeroed by step_with / advance_with per call, counted by the stages
    int sp_first = 0, sp_last = 0;     // the species rows Check_Undershoot clamps; setup, from the plan
    DevBuf<double> d_ctl;              // {dt, time, max speed}: loop_ctl allocates, advance_with and k_step_end write
    StepGraph graph;                   // advance_with, through ensure
    TraceChain chain;                  // launch_all asks mult(); rk4_stages, rk_stages and advance_with make the transitions
    int config_epoch = 0;              // bumped by whatever changes what a step launches: the forcing and mixing-length setters
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
  // tpsrhs_stats_configure / tpsrhs_sampler_create, tpsrhs_probe_configure / tpsrhs_integrate, tpsrhs_monitor_configure;
  // NULL: none yet.  Created, used and released (tpsrhs_destroy) by tpsrhs.hip.  Raw pointers because their types are
  // incomplete in the kernel families, where this struct's inline destructor is compiled as well.
  tpsrhs_stats_state *stats = nullptr;
  tpsrhs_sampling_state *sampling = nullptr;
  tpsrhs_integrals_state *integrals = nullptr;
  // tpsrhs_visualization_fields: the post-processing passes of the plasma families (visualization.hpp); NULL for every other
  // physics
  void (*vis_fields)(tpsrhs_operator *, const VisRows &, const double *, double *) = nullptr;

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
    for (auto &e : ev_halo)
      if (e) (void)hipEventDestroy(e);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    for (auto &set : evs)
      for (auto &e : set)
        if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// The parameter block as the kernels of physics PH take it: by value (dry air) or as a pointer to its device image
// (plasma: PlasmaPhys::KArg), uploaded once -- the block is complete when the first kernel is launched and nothing
// changes it afterwards (the dry-air block, which the non-reflecting conditions update per Mult, travels by value).
template <class PH>
typename PH::KArg kernel_params(tpsrhs_operator *op) {
  if constexpr (std::is_pointer<typename PH::KArg>::value) {
    if (!op->d_params) {
      op->d_params = DevBuf<unsigned char>(sizeof(op->params));
      HIP_CHECK(hipMemcpy(op->d_params.get(), op->params, sizeof(op->params), hipMemcpyHostToDevice));
    }
    return reinterpret_cast<typename PH::KArg>(op->d_params.get());
  } else {
    return *reinterpret_cast<const typename PH::Params *>(op->params);
  }
}

inline void exchange(tpsrhs_operator *op, int phase, double *T, int nfld, int per, hipStream_t stream) {
  const Topology &tp = op->topo;
  if (tp.num_shared == 0) return;
  const int n1 = (phase == 0) ? op->order + 1 : rule_points(op->nc, (op->dim - 1) + 2 * op->order);
  const int64_t total = static_cast<int64_t>(tp.num_shared) * nfld * per;
  const int grid = static_cast<int>(std::min<int64_t>((total + 255) / 256, 2048));
  if (op->dim == 3)
    hipLaunchKernelGGL(k_pack<3>, dim3(grid), dim3(256), 0, stream, tp.num_shared, nfld, n1, op->d_shared_slot.get(),
                       op->d_shared_orient.get(), T, op->d_send.get());
  else
    hipLaunchKernelGGL(k_pack<2>, dim3(grid), dim3(256), 0, stream, tp.num_shared, nfld, n1, op->d_shared_slot.get(),
                       op->d_shared_orient.get(), T, op->d_send.get());
  HIP_CHECK(hipGetLastError());
  double *recv = T + static_cast<int64_t>(op->ne) * op->nfaces * nfld * per;
  const int st = op->halo(op->halo_ctx, phase, op->d_send.get(), recv, static_cast<int>(tp.nbr_ranks.size()),
                          tp.nbr_ranks.data(), op->send_off[phase].data(), op->recv_off[phase].data(), stream);
  if (st != 0) throw std::runtime_error("halo callback failed in phase " + std::to_string(phase));
}

template <int DIM, int P, class PH, int NC = 0>
void launch_all(tpsrhs_operator *op, const double *x, double *y, bool gradients_only) {
  typedef Cfg<DIM, P, NC> C;
  static_assert(sizeof(typename PH::Params) <= sizeof(op->params), "parameter block too large");
  const typename PH::Params &prm = *reinterpret_cast<const typename PH::Params *>(op->params);  // host copy
  const int nblocks = (op->ne + C::EPB - 1) / C::EPB;
  hipStream_t s = op->stream;
  if constexpr (PH::HAS_NR_BC) {  // this Mult's view of the non-reflecting boundary state
    typename PH::Params &w = *reinterpret_cast<typename PH::Params *>(op->params);
    w.bstate = op->d_bstate[op->bstate_cur].get();
    w.nr_ordinal = op->d_nr_ordinal.get();
    w.nr_dt = op->nr_dt;
  }
  const typename PH::KArg prm_k = kernel_params<PH>(op);  // after the update above: what the kernels of this Mult get
  if (!op->d_block_speed && !gradients_only) {
    op->d_block_speed = DevBuf<double>(nblocks);
    op->flux_grid = nblocks;
  }
  // Alternating sweep direction (TPSRHS_SWEEP_ALT): k_traces and k_flux of a Mult walk the block list one way, k_gradient
  // the other, and the next Mult starts the other way round -- every sweep begins with what its predecessor wrote last
  // (xcd_block).  The direction is per sweep, the same for its halo and interior launches.
  const int dir0 = op->loop.sweep_alt ? op->loop.sweep_parity : 0;
  // which trace buffer this Mult reads, whether its k_traces sweep is already done, and where k_flux puts the next one's
  const TraceChain::Mult tc = op->loop.chain.mult(flux_fuses_traces<C, PH>(), op->rk.mode, gradients_only, op->topo.num_shared > 0);
  if (tc.write >= 0 && !op->d_TA2) op->d_TA2 = DevBuf<double>(static_cast<int64_t>(op->ne) * op->nfaces * 2 * PH::NEQ * C::NF);
  double *const tbuf[2] = {op->d_TA.get(), op->d_TA2.get()};
  double *const ta = tbuf[tc.read];
  const bool have_traces = tc.have_traces;
  if (tc.write >= 0) op->rk.ta_out = tbuf[tc.write];
  auto traces = [&](MeshDev m, int grid) {
    if (have_traces) return;
    m.reverse = dir0;
    hipLaunchKernelGGL((k_traces<C, PH>), dim3(grid), dim3(C::BLOCK), 0, s, m, prm_k, x, ta);
    HIP_CHECK(hipGetLastError());
  };
  auto gradient = [&](MeshDev m, int grid) {
    m.reverse = op->loop.sweep_alt ? 1 - dir0 : 0;
    hipLaunchKernelGGL((k_gradient<C, PH>), dim3(grid), dim3(C::BLOCK), 0, s, m, prm_k, x, ta, op->d_Up.get(), op->d_gradUp.get(),
                       op->d_TB.get());
    HIP_CHECK(hipGetLastError());
  };
  auto flux = [&](MeshDev m, int grid) {
    m.reverse = dir0;
    hipLaunchKernelGGL((k_flux<C, PH>), dim3(grid), dim3(C::BLOCK), 0, s, m, prm_k, x, op->d_gradUp.get(), ta, op->d_TB.get(), y,
                       op->d_block_speed.get(), op->rk);
    HIP_CHECK(hipGetLastError());
  };
  // non-reflecting patches: mean of the primitives (+ sum over the ranks), then the boundary-state update;
  // after the last k_gradient launch, before the first k_flux launch
  auto nr_update = [&](const MeshDev &m) {
    if constexpr (PH::HAS_NR_BC) {
      if (!op->has_nr) return;
      const int nbc = prm.num_bcs;
      hipLaunchKernelGGL((k_bc_mean<C, PH>), dim3(nbc), dim3(256), 0, s, op->n_nr_faces, op->d_nr_faces.get(), ta,
                         op->d_bc_sums.get());
      HIP_CHECK(hipGetLastError());
      if (op->reduce && op->topo.num_shared > 0) {
        const int st = op->reduce(op->reduce_ctx, op->d_bc_sums.get(), nbc * (TPSRHS_MAXEQUATIONS + 1), TPSRHS_REDUCE_SUM, s);
        if (st != 0) throw std::runtime_error("halo: reduce callback failed");
      }
      if (op->n_nr_faces > 0) {
        hipLaunchKernelGGL((k_bc_nr<C, PH>), dim3(op->n_nr_faces), dim3(C::BLOCK), 0, s, m, prm_k, op->d_nr_faces.get(), op->d_bc_sums.get(), x,
                           op->d_Up.get(), op->d_gradUp.get(), op->d_bstate[op->bstate_cur].get(), op->d_bstate[1 - op->bstate_cur].get(),
                           op->bstate_init ? 0 : 1, op->nr_dt_dev);
        HIP_CHECK(hipGetLastError());
      }
    }
  };
  // ConstantPressureGradient / SpongeZone / HeatSource / JouleHeating, after the last k_flux launch
  auto forcing = [&](const MeshDev &m) {
    if (!op->forcing_active) return;
    if constexpr (PH::HAS_MIXED_OUT) {  // SpongeZone::updateTerms: computeMixedOutValues first (src/forcing_terms.cpp:631-635)
      for (int z = 0; z < op->forcing.nsponge; z++) {
        if (!op->forcing.sponge[z].mixed_out) continue;
        hipLaunchKernelGGL((k_mixed_out_sum<C, PH>), dim3(1), dim3(256), 0, s, op->ndofs, prm_k, op->d_forcing.get(), z, x);
        HIP_CHECK(hipGetLastError());
        if (op->reduce && op->topo.num_shared > 0) {  // MPI_Allreduce of meanNormalFluxes, :732-735
          const int st = op->reduce(op->reduce_ctx, op->forcing.sponge[z].msum, PH::NEQ + 1, TPSRHS_REDUCE_SUM, s);
          if (st != 0) throw std::runtime_error("mixed-out sponge: reduce callback failed");
        }
        hipLaunchKernelGGL((k_mixed_out_finish<C, PH>), dim3(1), dim3(1), 0, s, prm_k, op->d_forcing.get(), z);
        HIP_CHECK(hipGetLastError());
      }
    }
    const int grid = static_cast<int>((op->ndofs + 255) / 256);
    hipLaunchKernelGGL((k_forcing<C, PH>), dim3(grid), dim3(256), 0, s, m, prm_k, op->d_forcing.get(), x, op->d_gradUp.get(), y);
    HIP_CHECK(hipGetLastError());
  };
  if (op->timing) {
    op->ev = op->evs[op->sets_recorded % tpsrhs_operator::MAXSETS];
    HIP_CHECK(hipEventRecord(op->ev[0], s));
  }
  const MeshDev all = op->mesh_dev();
  if (op->loop.sweep_alt) op->loop.sweep_parity ^= 1;  // (read into dir0 above: the next Mult starts from the other end)
  if (op->topo.num_shared == 0) {
    traces(all, nblocks);
    if (op->timing) HIP_CHECK(hipEventRecord(op->ev[1], s));
    gradient(all, nblocks);
    if (op->timing) HIP_CHECK(hipEventRecord(op->ev[2], s));
    if (gradients_only) return;
    nr_update(all);
    flux(all, nblocks);
  } else {
    // Partitioned mesh.  Blocks that touch a shared face ("halo blocks") run first in the producing
    // sweeps and last in the consuming ones; packing and the neighbour exchange run on the second
    // stream while the interior blocks compute (the reference overlaps its MPI exchange with the
    // volume work the same way, src/rhs_operator.cpp:361-372,775-831).
    if (!op->d_blocks_halo) {
      std::vector<int> halo, interior;
      std::vector<char> is_halo(nblocks, 0);
      for (int i = 0; i < op->topo.num_shared; i++) is_halo[(op->topo.shared_slot[i] / op->nfaces) / C::EPB] = 1;
      for (int b = 0; b < nblocks; b++) (is_halo[b] ? halo : interior).push_back(b);
      op->n_blocks_halo = static_cast<int>(halo.size());
      op->n_blocks_interior = static_cast<int>(interior.size());
      op->d_blocks_halo = DevBuf<int>(halo);
      op->d_blocks_interior = DevBuf<int>(interior);
      HIP_CHECK(hipStreamCreateWithFlags(&op->comm_stream, hipStreamNonBlocking));
      for (auto &e : op->ev_halo) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    MeshDev mh = all, mi = all;
    mh.blocks = op->d_blocks_halo.get();
    mi.blocks = op->d_blocks_interior.get();
    const int nh = op->n_blocks_halo, ni = op->n_blocks_interior;
    hipStream_t c = op->comm_stream;
    // host order: the interior launches are enqueued BEFORE the (host-side, slow) exchange callback, so
    // the compute stream never waits for the host
    traces(mh, nh);
    HIP_CHECK(hipEventRecord(op->ev_halo[0], s));
    if (ni) traces(mi, ni);
    if (op->timing) HIP_CHECK(hipEventRecord(op->ev[1], s));
    if (ni) gradient(mi, ni);
    HIP_CHECK(hipStreamWaitEvent(c, op->ev_halo[0], 0));
    exchange(op, 0, op->d_TA.get(), 2 * PH::NEQ, C::NF, c);  // overlaps the two interior launches above
    HIP_CHECK(hipEventRecord(op->ev_halo[1], c));
    HIP_CHECK(hipStreamWaitEvent(s, op->ev_halo[1], 0));
    gradient(mh, nh);
    if (op->timing) HIP_CHECK(hipEventRecord(op->ev[2], s));
    if (gradients_only) return;
    HIP_CHECK(hipEventRecord(op->ev_halo[2], s));
    nr_update(all);
    if (ni) flux(mi, ni);
    HIP_CHECK(hipStreamWaitEvent(c, op->ev_halo[2], 0));
    exchange(op, 1, op->d_TB.get(), PH::NEQ - 1, C::NQ, c);  // overlaps the interior flux launch
    HIP_CHECK(hipEventRecord(op->ev_halo[3], c));
    HIP_CHECK(hipStreamWaitEvent(s, op->ev_halo[3], 0));
    flux(mh, nh);
  }
  forcing(all);
  if constexpr (PH::HAS_NR_BC) {
    if (op->n_nr_faces > 0) {  // the updated states are what the next Mult's Riemann solver sees
      op->bstate_cur = 1 - op->bstate_cur;
      op->bstate_init = true;
    }
  }
  if (op->timing) {
    HIP_CHECK(hipEventRecord(op->ev[3], s));
    op->sets_recorded++;
  }
}

template <class PH>
void launch_point_eval(tpsrhs_operator *op, int quantity, int64_t n, const double *U, double *out) {
  const int grid = static_cast<int>((n + 255) / 256);
  if (grid == 0) return;
  hipLaunchKernelGGL((k_point_eval<PH>), dim3(grid), dim3(256), 0, op->stream, kernel_params<PH>(op), quantity, n, U, out);
  HIP_CHECK(hipGetLastError());
}

// 1-D operator tables -> this translation unit's __constant__ copy; a function of (dim, order) only
inline void upload_tables(int dim, int order, int nc = 0) {
  const Tables1D tabs = make_tables(order, dim, nc, nc);
  const size_t off = ((static_cast<size_t>(nc) * 2 + (dim - 2)) * (TPSRHS_MAXORDER + 1) + order) * sizeof(Tables1D);
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &tabs, sizeof(Tables1D), off, hipMemcpyHostToDevice));
}

// non-collocated (Gauss-Lobatto / Gauss-Lobatto) kernels: orders 1..3
template <int DIM, class PH>
void pick_order_nc(tpsrhs_operator *op) {
  upload_tables(DIM, op->order, 1);
  op->point_eval = &launch_point_eval<PH>;
  if constexpr (PH::AXISYM) {
    throw Unsupported("the Gauss-Lobatto pair is built for the planar 2-D and the 3-D formulation");
  } else {
    switch (op->order) {
      case 1: op->launch = &launch_all<DIM, 1, PH, 1>; break;
      case 2: op->launch = &launch_all<DIM, 2, PH, 1>; break;
      case 3: op->launch = &launch_all<DIM, 3, PH, 1>; break;
      default: throw Unsupported("Gauss-Lobatto basis + rule: polynomial orders 1..3 are built");
    }
  }
}

template <int DIM, class PH>
void pick_order(tpsrhs_operator *op) {
  if (op->nc) {
    pick_order_nc<DIM, PH>(op);
    return;
  }
  upload_tables(DIM, op->order);
  op->point_eval = &launch_point_eval<PH>;
  switch (op->order) {
    case 1: op->launch = &launch_all<DIM, 1, PH>; break;
    case 2: op->launch = &launch_all<DIM, 2, PH>; break;
    case 3: op->launch = &launch_all<DIM, 3, PH>; break;
    case 4: op->launch = &launch_all<DIM, 4, PH>; break;
    case 5:  // MAXDOFS = 216 of the reference (src/dataStructures.hpp:41-65): light physics only
      if constexpr (PH::MAX_ORDER >= 5) {
        op->launch = &launch_all<DIM, 5, PH>;
        break;
      }
      [[fallthrough]];
    default:
      throw Unsupported("polynomial order " + std::to_string(op->order) + " is not built for this physics (1.." +
                        std::to_string(PH::MAX_ORDER) + ")");
  }
}

// the four passes of tpsrhs_visualization_fields on the operator's stream: U = x, Up / gradUp the operator's own (just
// refreshed by the caller), out [nrows][NDofs].  Instantiated in the units of plasma_vis_family.hpp only: a unit that does
// not ask for it gets no kernel from it.
template <class PH>
void launch_vis_fields(tpsrhs_operator *op, const VisRows &rows, const double *x, double *out) {
  const int64_t n = op->ndofs;
  const int grid = static_cast<int>((n + 255) / 256);
  if (grid == 0) return;
  const typename PH::KArg prm_k = kernel_params<PH>(op);
  hipLaunchKernelGGL((k_vis_fields<PH, VIS_SPECIES>), dim3(grid), dim3(256), 0, op->stream, prm_k, rows, n, x, op->d_Up.get(), op->d_gradUp.get(), out);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_vis_fields<PH, VIS_FLUX>), dim3(grid), dim3(256), 0, op->stream, prm_k, rows, n, x, op->d_Up.get(), op->d_gradUp.get(), out);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_vis_fields<PH, VIS_SIGMA>), dim3(grid), dim3(256), 0, op->stream, prm_k, rows, n, x, op->d_Up.get(), op->d_gradUp.get(), out);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_vis_fields<PH, VIS_SOURCE>), dim3(grid), dim3(256), 0, op->stream, prm_k, rows, n, x, op->d_Up.get(), op->d_gradUp.get(), out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

#endif
