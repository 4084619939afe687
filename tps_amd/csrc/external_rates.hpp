// The flow side of the coupling to an electron Boltzmann solver (src/M2ulPhyS2Boltzmann.cpp), on the device:
//   k_external_reactions  the reactions with model = bte (GridFunctionReaction, src/reaction.cpp:85-117): their forward rate
//                         coefficient is read per node from the array of tpsrhs_set_reaction_rates -- M2ulPhyS::fetch
//   k_boltzmann_fields    species number densities and the two temperatures for the solver -- M2ulPhyS::push (:40-87)
// One lane per node, 256 per block, byNODES loads and stores like k_point_eval and k_vis_fields: every load and store of a
// wave is one contiguous run of 64 doubles.
//
// Why a pass of its own: the reference adds the chemical source nodally to y after the inverse mass, and the source is a sum
// over the reactions.  The sweeps keep the reactions with a closed form (the first chemistry block of the operator); this
// pass adds the others (the second block) to y after the last k_flux launch, where k_forcing adds the forcing terms.  It is
// instantiated in the units of plasma_vis_family.hpp only, so the sweeps' units gain no kernel and their device code stays
// what it was.
//
// Traffic per node: NEQ rows of U, one row per rate component read, NACTIVE (+ 1 for two temperatures) rows of y read and
// written.  No array is indexed by the run-time reaction number: creation[] is indexed by the unrolled species loop.
#ifndef TPSRHS_EXTERNAL_RATES_HPP_
#define TPSRHS_EXTERNAL_RATES_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "physics_plasma.hpp"

namespace tpsrhs {

template <class PH>
__global__ __launch_bounds__(256) void k_external_reactions(typename PH::KArg prm_k, const ChemDev *__restrict__ ext_k, int64_t n,
                                                            const double *__restrict__ U, const double *__restrict__ rates,
                                                            double *__restrict__ Y) {
  typename PH::PRef prm = PH::pref(prm_k);
  // the block of the external reactions like the parameter block: wave-uniform addresses, scalar loads
  const ChemDev __attribute__((address_space(4))) &ext = *(const ChemDev __attribute__((address_space(4))) *)ext_k;
  constexpr int NEQ = PH::NEQ, NSP = PH::NSP, NVEL = PH::NVEL;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double u[NEQ], up[NEQ];
#pragma unroll
  for (int eq = 0; eq < NEQ; eq++) u[eq] = U[eq * n + i];
  PH::prim(prm, u, up);  // as k_flux does before `source`: the primitives of the unclamped state
  double creation[NSP], e_loss;
  // GridFunctionReaction::setGridFunction: component c of the array starts at data + c * size
  PH::external_source(prm, ext, u, up, [&](int comp) { return rates[comp * n + i]; }, creation, e_loss);
  // y += the source, where it is not zero: a zero rate coefficient (the reference's null data_) leaves y as the sweeps wrote
  // it, bit for bit (-0 + 0 would be +0)
#pragma unroll
  for (int sp = 0; sp < PH::NACTIVE; sp++) {
    const double add = creation[sp] * prm.mw[sp];
    if (add != 0.0) Y[(NVEL + 2 + sp) * n + i] += add;
  }
  if constexpr (PH::TWO_TEMPERATURE) {
    if (e_loss != 0.0) Y[PH::ITE * n + i] -= e_loss;
  }
}

// out [num_species + 2][n]: AVOGADRONUMBER n_sp of computeNumberDensities (the UNCLAMPED state, as push reads U), then T_h and
// T_e of computeTemperaturesBase (equal for one temperature)
template <class PH>
__global__ __launch_bounds__(256) void k_boltzmann_fields(typename PH::KArg prm_k, int64_t n, int num_species,
                                                          const double *__restrict__ U, double *__restrict__ out) {
  typename PH::PRef prm = PH::pref(prm_k);
  constexpr int NEQ = PH::NEQ, NSP = PH::NSP;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double u[NEQ];
#pragma unroll
  for (int eq = 0; eq < NEQ; eq++) u[eq] = U[eq * n + i];
  const typename PH::State s = PH::make_state(prm, u);
#pragma unroll
  for (int sp = 0; sp < NSP; sp++)
    if (sp < num_species) out[sp * n + i] = kAvogadro * s.n[sp];
  out[num_species * n + i] = s.Th;
  out[(num_species + 1) * n + i] = s.Te;
}

}  // namespace tpsrhs

namespace {

template <class PH>
void launch_external_reactions(tpsrhs_operator *op, const double *x, double *y) {
  const int64_t n = op->ndofs;
  const int grid = static_cast<int>((n + 255) / 256);
  if (grid == 0 || op->ext.num_reactions == 0) return;
  hipLaunchKernelGGL((k_external_reactions<PH>), dim3(grid), dim3(256), 0, op->stream, kernel_params<PH>(op),
                     static_cast<const ChemDev *>(op->ext.d_chem.get()), n, x, op->ext.rates, y);
  HIP_CHECK(hipGetLastError());
}

template <class PH>
void launch_boltzmann_fields(tpsrhs_operator *op, const double *x, int num_species, double *out) {
  const int64_t n = op->ndofs;
  const int grid = static_cast<int>((n + 255) / 256);
  if (grid == 0) return;
  hipLaunchKernelGGL((k_boltzmann_fields<PH>), dim3(grid), dim3(256), 0, op->stream, kernel_params<PH>(op), n, num_species, x, out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

#endif
