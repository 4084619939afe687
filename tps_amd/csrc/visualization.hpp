// Post-processing fields of a plasma run on the device: M2ulPhyS::updateVisualizationVariables
// (src/M2ulPhyS.cpp:4156-4263), which the reference computes on the CPU only (:4157-4160 exits in its device build).
//
// One lane per node, byNODES loads and stores like k_point_eval; out is [nrows][n] with the rows of VisRows
// (tpsrhs_visualization_layout).  The GROUP is a template parameter: every pass carries the registers of its own
// closure only, and re-reads U (a pass per output file: the extra traffic does not matter, a spill would).
//   VIS_SPECIES    computeSpeciesPrimitives                                   -> X_sp, Y_sp, n_sp
//   VIS_FLUX       ComputeFluxTransportProperties(state, gradUp, E = 0)       -> the four coefficients, diff_vel_<sp>
//   VIS_SIGMA      ComputeSourceTransportProperties(state, Up, ...)           -> electric_cond
//   VIS_SOURCE     the rest of it, then Chemistry                             -> momentum-transfer frequencies, progress rates
// The state is the UNCLAMPED U (the reference calls no clamp here); the temperatures of VIS_FLUX come from the state
// (GetPrimitivesFromConservatives inside the transport), those of VIS_SOURCE and of the rates from Up, as in the reference.
#ifndef TPSRHS_VISUALIZATION_HPP_
#define TPSRHS_VISUALIZATION_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernel_args.hpp"

namespace tpsrhs {

enum { VIS_SPECIES = 0, VIS_FLUX = 1, VIS_SIGMA = 2, VIS_SOURCE = 3, VIS_NUM_GROUPS = 4 };

template <class PH, int GROUP>
__global__ __launch_bounds__(256) void k_vis_fields(typename PH::KArg prm_k, VisRows rows, int64_t n,
                                                    const double *__restrict__ U, const double *__restrict__ Up,
                                                    const double *__restrict__ gradUp, double *__restrict__ out) {
  typename PH::PRef prm = PH::pref(prm_k);
  constexpr int NEQ = PH::NEQ, NSP = PH::NSP, NVEL = PH::NVEL, DIM = PH::DIM;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double u[NEQ];
#pragma unroll
  for (int eq = 0; eq < NEQ; eq++) u[eq] = U[eq * n + i];
  if constexpr (GROUP == VIS_SPECIES) {
    const typename PH::Species q = PH::species(prm, u);
#pragma unroll
    for (int sp = 0; sp < NSP; sp++) {
      out[(rows.Xsp + sp) * n + i] = q.X[sp];
      out[(rows.Ysp + sp) * n + i] = q.Y[sp];
      out[(rows.nsp + sp) * n + i] = q.n[sp];
    }
  } else if constexpr (GROUP == VIS_FLUX) {
    const typename PH::State s = PH::make_state(prm, u);
    typename PH::TCoef c;
    PH::transport_coeffs(prm, u, s.Th, s.Te, true, c);
    out[(rows.FluxTrns + 0) * n + i] = c.visc;
    out[(rows.FluxTrns + 1) * n + i] = c.bulk;
    out[(rows.FluxTrns + 2) * n + i] = c.k;
    out[(rows.FluxTrns + 3) * n + i] = c.ke;
    // diff_vel_<sp>: NVEL rows per species, species-major (a grid function on nvelfes); the directions past DIM
    // (the azimuthal one of the axisymmetric formulation) stay zero as the transport leaves them
#pragma unroll
    for (int d = 0; d < NVEL; d++) {
      double V[NSP];
      if (d < DIM) {
        double gs[NEQ];  // diffusion_velocity reads the density and the species rows only
#pragma unroll
        for (int eq = 0; eq < NEQ; eq++) gs[eq] = (eq == 0 || (eq >= NVEL + 2 && eq < NVEL + 2 + PH::NACTIVE)) ? gradUp[(eq + d * NEQ) * n + i] : 0.0;
        PH::diffusion_velocity(prm, c, gs, V);
      } else {
#pragma unroll
        for (int sp = 0; sp < NSP; sp++) V[sp] = 0.0;
      }
#pragma unroll
      for (int sp = 0; sp < NSP; sp++) out[(rows.diffVel + sp * NVEL + d) * n + i] = V[sp];
    }
  } else if constexpr (GROUP == VIS_SIGMA) {
    const double Th = Up[PH::ITH * n + i], Te = PH::TWO_TEMPERATURE ? Up[PH::ITE * n + i] : Th;
    out[rows.SrcTrns * n + i] = PH::source_conductivity(prm, u, Th, Te);
  } else {
    const double Th = Up[PH::ITH * n + i], Te = PH::TWO_TEMPERATURE ? Up[PH::ITE * n + i] : Th;
    double nsp[NSP];
    {
      double mtfreq[NSP];
      PH::source_props_full(prm, u, Th, Te, nsp, mtfreq);
#pragma unroll
      for (int sp = 0; sp < NSP; sp++) out[(rows.SpeciesTrns + sp) * n + i] = mtfreq[sp];
    }
    PH::progress_rates(prm, nsp, Th, Te, [&](int r, double q) { out[(rows.rxn + r) * n + i] = q; });
  }
}

}  // namespace tpsrhs
#endif
