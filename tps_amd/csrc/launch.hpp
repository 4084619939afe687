// The launch sequence of one RHS evaluation over the operator object (operator.hpp): the parameter block as a physics takes
// it, the halo exchange, the three sweeps of kernels.hpp in their order, the point-wise closures and the visualization
// passes.  Included by the units that instantiate kernels of the sweeps -- tpsrhs.hip (dry air), dryair_axisym.hip,
// dryair_les.hip, lte_axisym.hip, the plasma families -- and by nothing else.  c_tab is static __constant__, a copy per
// unit: pick_order and the launch_all it selects are instantiated in one unit, and upload_tables fills that unit's copy.
#ifndef TPSRHS_LAUNCH_HPP_
#define TPSRHS_LAUNCH_HPP_

#include <type_traits>

#include "kernels.hpp"
#include "operator.hpp"

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
  if (st != 0) throw HaloError("halo callback failed in phase " + std::to_string(phase));
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
        if (st != 0) throw HaloError("halo: reduce callback failed");
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
    if (!op->forcing_terms) return;
    if constexpr (PH::HAS_MIXED_OUT) {  // SpongeZone::updateTerms: computeMixedOutValues first (src/forcing_terms.cpp:631-635)
      for (int z = 0; z < op->forcing.nsponge; z++) {
        if (!op->forcing.sponge[z].mixed_out) continue;
        hipLaunchKernelGGL((k_mixed_out_sum<C, PH>), dim3(1), dim3(256), 0, s, op->ndofs, prm_k, op->d_forcing.get(), z, x);
        HIP_CHECK(hipGetLastError());
        if (op->reduce && op->topo.num_shared > 0) {  // MPI_Allreduce of meanNormalFluxes, :732-735
          const int st = op->reduce(op->reduce_ctx, op->forcing.sponge[z].msum, PH::NEQ + 1, TPSRHS_REDUCE_SUM, s);
          if (st != 0) throw std::runtime_error("mixed-out sponge: reduce callback failed");  // (plain: TPSRHS_ERR_MESH)
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
  // the reactions with an external rate coefficient (tpsrhs_set_reaction_rates): y += their sources, a streaming pass of its
  // own from the family's post-processing unit (external_rates.hpp); the sweeps above saw the other reactions only
  if (op->ext.rates) op->ext_reactions(op, x, y);
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
  // ... and the packed image that the kernels with the staged prologue copy to LDS as it stands (kernels.hpp::stage_issue)
  if (dim == StagedCfg::DIM && order == StagedCfg::P && nc == StagedCfg::NC) {
    const Tab<StagedCfg> image = make_tab_image<StagedCfg>(tabs);
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_tab_image), &image, sizeof(image), 0, hipMemcpyHostToDevice));
  }
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
