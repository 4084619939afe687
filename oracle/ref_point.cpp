// TEST INFRASTRUCTURE -- the driver of oracle/_ref/libtpsref_point.so (oracle/ref.mk): the REFERENCE's own compiled
// point physics behind a C interface that takes this project's parameter structs (include/tpsrhs.h).
//
// The rule for this file: it MARSHALS and CALLS.  It copies the fields of tpsrhs_physics / tpsrhs_disc into the
// reference's input structs, constructs the reference's classes through the plain-data constructors its own GPU path
// uses, and calls their member functions on arrays of points.  It restates no formula.  A quantity that could only
// be had by re-implementing lines of the reference here is NOT covered:
//   * the per-node body of SourceTerm::updateTerms (src/source_term.cpp) lives in a class bound to the finite-element
//     spaces; its pieces are covered one by one (source transport, rate coefficients, equilibrium constants, progress
//     and creation rates, the net-emission sink), its assembly (clamps, electron-energy exchange) is not;
//   * the boundary-condition classes (WallBC / InletBC / OutletBC) need the mesh; only the mixture's state modifiers
//     they are built from are covered;
//   * the non-reflecting patches.
//
// Restriction of the stand-in headers: ref_stub/mfem.hpp's Vector(double *, int) COPIES where MFEM's aliases.  A
// reference function that wraps an OUTPUT pointer in a Vector and writes through it would lose its result here; every
// function below either takes the reference's `double *` interface or passes Vectors this file owns and copies out.
//
// Layout of every array: point-major, `n` points, the per-point block exactly what the reference's `double *`
// interface takes (state[eq], gradUp[eq + d * num_equation], flux[eq + d * num_equation], normals dim entries).
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "tpsrhs.h"

#include "chemistry.hpp"
#include "dataStructures.hpp"
#include "equation_of_state.hpp"
#include "fluxes.hpp"
#include "gas_transport.hpp"
#include "radiation.hpp"
#include "riemann_solver.hpp"
#include "transport_properties.hpp"

static_assert(TPSRHS_MAXSPECIES == gpudata::MAXSPECIES, "parameter blocks were laid out after the reference's");
static_assert(TPSRHS_MAXREACTIONS == gpudata::MAXREACTIONS, "");
static_assert(TPSRHS_MAXCHEMPARAMS == gpudata::MAXCHEMPARAMS, "");
static_assert(TPSRHS_MAXEQUATIONS == gpudata::MAXEQUATIONS, "");

// The one MPI call of the compiled units sits on an error path of reaction.cpp; no MPI library is linked.
extern "C" int MPI_Barrier(MPI_Comm) { return 0; }

namespace {

struct Ref {
  int dim = 0, nvel = 0, neq = 0, nsp = 0, nreact = 0;
  bool axisym = false, plasma = false;
  tpsrhs_physics phys;  // keeps the rate parameters and table pointers the reference's inputs point into
  std::unique_ptr<GasMixture> mixture;
  std::unique_ptr<TransportProperties> transport;
  std::unique_ptr<Fluxes> fluxes;
  std::unique_ptr<RiemannSolverTPS> lf, roe;
  std::unique_ptr<Chemistry> chemistry;
  std::unique_ptr<NetEmission> nec;
};

std::string g_err;

TableInput table_input(const tpsrhs_table &t) {
  TableInput in;
  in.Ndata = t.n_data;
  in.xdata = t.x_data;
  in.fdata = t.f_data;
  in.xLogScale = t.x_log_scale != 0;
  in.fLogScale = t.f_log_scale != 0;
  in.order = 1;
  return in;
}

constantTransportData constant_input(const tpsrhs_constant_transport &c) {
  constantTransportData d;
  d.viscosity = c.viscosity;
  d.bulkViscosity = c.bulk_viscosity;
  d.thermalConductivity = c.thermal_conductivity;
  d.electronThermalConductivity = c.electron_thermal_conductivity;
  for (int sp = 0; sp < gpudata::MAXSPECIES; sp++) {
    d.diffusivity[sp] = c.diffusivity[sp];
    d.mtFreq[sp] = c.mt_freq[sp];
  }
  d.electronIndex = c.electron_index;
  return d;
}

BoundaryViscousFluxData bdr_flux_data(int dim, const double *normal, const double *primFlux, const int *primFluxIdxs) {
  BoundaryViscousFluxData bc;
  for (int d = 0; d < gpudata::MAXDIM; d++) bc.normal[d] = (normal && d < dim) ? normal[d] : 0.0;
  for (int i = 0; i < gpudata::MAXEQUATIONS; i++) {
    bc.primFlux[i] = primFlux ? primFlux[i] : 0.0;
    bc.primFluxIdxs[i] = primFluxIdxs ? primFluxIdxs[i] != 0 : false;
  }
  return bc;
}

}  // namespace

extern "C" {

const char *tpsref_last_error() { return g_err.c_str(); }

// dim: 2 or 3; disc->axisymmetric: three velocity components in two dimensions
int tpsref_create(const tpsrhs_physics *p, const tpsrhs_disc *d, int dim, void **out) {
  std::unique_ptr<Ref> r(new Ref);
  r->phys = *p;
  p = &r->phys;
  r->dim = dim;
  r->axisym = d->axisymmetric != 0;
  r->nvel = r->axisym ? 3 : dim;
  const Equations eq = static_cast<Equations>(p->eq_system);
  if (p->working_fluid == TPSRHS_DRY_AIR) {
    DryAirInput in;
    in.f = DRY_AIR;
    in.eq_sys = eq;
    in.specific_heat_ratio = p->dry_air.specific_heat_ratio;
    in.gas_constant = p->dry_air.gas_constant;
    r->mixture.reset(new DryAir(in, dim, r->nvel));
    r->transport.reset(new DryAirTransport(r->mixture.get(), p->dry_air.visc_mult, p->dry_air.bulk_visc_mult,
                                           p->dry_air.sutherland_C1, p->dry_air.sutherland_S0, p->dry_air.sutherland_Pr));
  } else if (p->working_fluid == TPSRHS_USER_DEFINED) {
    r->plasma = true;
    PerfectMixtureInput in;
    in.f = USER_DEFINED;
    in.numSpecies = p->mixture.num_species;
    in.isElectronIncluded = p->mixture.is_electron_included != 0;
    in.ambipolar = p->mixture.ambipolar != 0;
    in.twoTemperature = p->mixture.two_temperature != 0;
    for (int i = 0; i < gpudata::MAXSPECIES * GasParams::NUM_GASPARAMS; i++) in.gasParams[i] = p->mixture.gas_params[i];
    for (int i = 0; i < gpudata::MAXSPECIES; i++) in.molarCV[i] = p->mixture.molar_cv[i];
    r->mixture.reset(new PerfectMixture(in, dim, r->nvel));
    if (p->transport_model == TPSRHS_CONSTANT) {
      r->transport.reset(new ConstantTransport(r->mixture.get(), constant_input(p->constant_transport)));
    } else if (p->transport_model == TPSRHS_ARGON_MINIMAL || p->transport_model == TPSRHS_ARGON_MIXTURE) {
      const tpsrhs_gas_transport &g = p->gas_transport;
      GasTransportInput in;
      in.neutralIndex = g.neutral_index;
      in.ionIndex = g.ion_index;
      in.neutralIndex2 = -1;
      in.ionIndex2 = -1;
      in.electronIndex = g.electron_index;
      in.thirdOrderkElectron = g.third_order_k_electron != 0;
      for (int i = 0; i < gpudata::MAXSPECIES * gpudata::MAXSPECIES; i++)
        in.collisionIndex[i] = static_cast<GasColl>(g.collision_index[i]);
      in.gas = Ar;
      in.multiply = g.multiply != 0;
      for (int i = 0; i < FluxTrns::NUM_FLUX_TRANS; i++) in.fluxTrnsMultiplier[i] = g.flux_trns_multiplier[i];
      for (int i = 0; i < SpeciesTrns::NUM_SPECIES_COEFFS; i++) in.spcsTrnsMultiplier[i] = g.spcs_trns_multiplier[i];
      in.diffMult = g.diff_mult;
      in.mobilMult = g.mobil_mult;
      in.constantActive = false;
      in.constantTransport = constant_input(p->constant_transport);
      if (p->transport_model == TPSRHS_ARGON_MINIMAL)
        r->transport.reset(new GasMinimalTransport(r->mixture.get(), in));
      else
        r->transport.reset(new GasMixtureTransport(r->mixture.get(), in));
    } else {
      g_err = "transport model outside the scope of the checker";
      return 1;
    }
    const tpsrhs_chemistry &c = p->chemistry;
    ChemistryInput ci;
    ci.model = NUM_CHEMISTRYMODEL;
    ci.electronIndex = c.electron_index;
    ci.numReactions = c.num_reactions;
    ci.minimumTemperature = c.minimum_temperature;
    for (int k = 0; k < gpudata::MAXREACTIONS; k++) {
      ci.reactionEnergies[k] = c.reaction_energies[k];
      ci.detailedBalance[k] = c.detailed_balance[k] != 0;
      ci.reactionModels[k] = static_cast<ReactionModel>(c.reaction_models[k]);
      ci.reactionInputs[k].modelParams = &c.rate_params[k * TPSRHS_MAXCHEMPARAMS];
      ci.reactionInputs[k].indexInput = 0;
      ci.reactionInputs[k].tableInput = table_input(c.rate_tables[k]);
      if (k < c.num_reactions && c.reaction_models[k] > TPSRHS_TABULATED_RXN) {
        g_err = "reaction model outside the scope of the checker";
        return 1;
      }
    }
    for (int i = 0; i < gpudata::MAXSPECIES * gpudata::MAXREACTIONS; i++) {
      ci.reactantStoich[i] = c.reactant_stoich[i];
      ci.productStoich[i] = c.product_stoich[i];
    }
    for (int i = 0; i < gpudata::MAXCHEMPARAMS * gpudata::MAXREACTIONS; i++)
      ci.equilibriumConstantParams[i] = c.equilibrium_constant_params[i];
    r->chemistry.reset(new Chemistry(r->mixture.get(), ci));
    r->nreact = c.num_reactions;
    if (p->radiation.model == TPSRHS_NET_EMISSION) {
      RadiationInput ri;
      ri.model = NET_EMISSION;
      ri.necModel = TABULATED_NEC;
      ri.necTableInput = table_input(p->radiation.nec_table);
      r->nec.reset(new NetEmission(ri));
    }
  } else {
    g_err = "working fluid outside the scope of the checker";
    return 1;
  }
  r->neq = r->mixture->GetNumEquations();
  r->nsp = r->mixture->GetNumSpecies();
  viscositySpongeData vsd;
  vsd.enabled = false;
  vsd.n[0] = vsd.n[1] = vsd.n[2] = 0.0;
  vsd.p[0] = vsd.p[1] = vsd.p[2] = 0.0;
  vsd.ratio = 1.0;
  vsd.width = 1.0;
  r->fluxes.reset(new Fluxes(r->mixture.get(), eq, r->transport.get(), r->neq, dim, r->axisym, 0, 0.0, 0.0, vsd));
  r->lf.reset(new RiemannSolverTPS(r->neq, r->mixture.get(), eq, r->fluxes.get(), false, r->axisym));
  r->roe.reset(new RiemannSolverTPS(r->neq, r->mixture.get(), eq, r->fluxes.get(), true, r->axisym));
  *out = r.release();
  return 0;
}

void tpsref_destroy(void *h) { delete static_cast<Ref *>(h); }
int tpsref_num_equation(void *h) { return static_cast<Ref *>(h)->neq; }
int tpsref_num_species(void *h) { return static_cast<Ref *>(h)->nsp; }
int tpsref_num_reactions(void *h) { return static_cast<Ref *>(h)->nreact; }

#define REF Ref *r = static_cast<Ref *>(h)

// GasMixture::GetPrimitivesFromConservatives / GetConservativesFromPrimitives
void tpsref_prim(void *h, int n, const double *U, double *Up) {
  REF;
  for (int i = 0; i < n; i++) r->mixture->GetPrimitivesFromConservatives(U + i * r->neq, Up + i * r->neq);
}
void tpsref_cons(void *h, int n, const double *Up, double *U) {
  REF;
  for (int i = 0; i < n; i++) r->mixture->GetConservativesFromPrimitives(Up + i * r->neq, U + i * r->neq);
}
// GasMixture::ComputePressure: out[2 i] total, out[2 i + 1] electron pressure
void tpsref_pressure(void *h, int n, const double *U, double *out) {
  REF;
  for (int i = 0; i < n; i++) {
    double pe = 0.0;
    out[2 * i] = r->mixture->ComputePressure(U + i * r->neq, &pe);
    out[2 * i + 1] = pe;
  }
}
void tpsref_max_char_speed(void *h, int n, const double *U, double *out) {
  REF;
  for (int i = 0; i < n; i++) out[i] = r->mixture->ComputeMaxCharSpeed(U + i * r->neq);
}
// GasMixture::computeSpeciesPrimitives: X, Y, n [i][MAXSPECIES] (mole fractions, mass fractions, number densities)
void tpsref_species_primitives(void *h, int n, const double *U, double *X, double *Y, double *n_sp) {
  REF;
  for (int i = 0; i < n; i++)
    r->mixture->computeSpeciesPrimitives(U + i * r->neq, X + i * gpudata::MAXSPECIES, Y + i * gpudata::MAXSPECIES,
                                         n_sp + i * gpudata::MAXSPECIES);
}
// GasMixture::computeSpeciesEnthalpies: out[i][sp]
void tpsref_species_enthalpies(void *h, int n, const double *U, double *out) {
  REF;
  for (int i = 0; i < n; i++) r->mixture->computeSpeciesEnthalpies(U + i * r->neq, out + i * r->nsp);
}
// the state modifiers the boundary conditions are built from
void tpsref_stagnation_state(void *h, int n, const double *U, double *out) {
  REF;
  for (int i = 0; i < n; i++) {
    Vector s(const_cast<double *>(U + i * r->neq), r->neq), o(r->neq);
    r->mixture->computeStagnationState(s, o);
    for (int eq = 0; eq < r->neq; eq++) out[i * r->neq + eq] = o(eq);
  }
}
void tpsref_stagnant_state_with_temp(void *h, int n, const double *U, double temp, double *out) {
  REF;
  for (int i = 0; i < n; i++) {
    Vector s(const_cast<double *>(U + i * r->neq), r->neq), o(r->neq);
    r->mixture->computeStagnantStateWithTemp(s, temp, o);
    for (int eq = 0; eq < r->neq; eq++) out[i * r->neq + eq] = o(eq);
  }
}
void tpsref_modify_energy_for_pressure(void *h, int n, const double *U, double p, int modifyElectronEnergy, double *out) {
  REF;
  for (int i = 0; i < n; i++)
    r->mixture->modifyEnergyForPressure(U + i * r->neq, out + i * r->neq, p, modifyElectronEnergy != 0);
}
// prim / primIdxs: one BoundaryPrimitiveData (MAXEQUATIONS entries) for all points
void tpsref_modify_state_from_primitive(void *h, int n, const double *U, const double *prim, const int *primIdxs,
                                        double *out) {
  REF;
  BoundaryPrimitiveData bc;
  for (int i = 0; i < gpudata::MAXEQUATIONS; i++) {
    bc.prim[i] = prim[i];
    bc.primIdxs[i] = primIdxs[i] != 0;
  }
  for (int i = 0; i < n; i++) r->mixture->modifyStateFromPrimitive(U + i * r->neq, bc, out + i * r->neq);
}
// GasMixture::computeSheathBdrFlux: primFlux[i][MAXEQUATIONS]
void tpsref_sheath_bdr_flux(void *h, int n, const double *U, double *primFlux) {
  REF;
  for (int i = 0; i < n; i++) {
    BoundaryViscousFluxData bc = bdr_flux_data(r->dim, nullptr, nullptr, nullptr);
    r->mixture->computeSheathBdrFlux(U + i * r->neq, bc);
    for (int k = 0; k < gpudata::MAXEQUATIONS; k++) primFlux[i * gpudata::MAXEQUATIONS + k] = bc.primFlux[k];
  }
}

// TransportProperties::ComputeFluxTransportProperties: buffer[i][4], diffVel[i][3 * MAXSPECIES] ([sp + d * nsp])
void tpsref_flux_transport(void *h, int n, const double *U, const double *gradUp, double *buffer, double *diffVel) {
  REF;
  const double E[3] = {0, 0, 0};
  for (int i = 0; i < n; i++)
    r->transport->ComputeFluxTransportProperties(U + i * r->neq, gradUp + i * r->neq * r->dim, E, -1.0, 0.0,
                                                 buffer + i * FluxTrns::NUM_FLUX_TRANS, diffVel + i * 3 * gpudata::MAXSPECIES);
}
// TransportProperties::ComputeSourceTransportProperties: global[i][1], species[i][MAXSPECIES], diffVel as above, n_sp[i][MAXSPECIES]
void tpsref_source_transport(void *h, int n, const double *U, const double *Up, const double *gradUp, double *global,
                             double *species, double *diffVel, double *n_sp) {
  REF;
  const double E[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    // The argon branch of GasMinimalTransport::ComputeSourceMolecularTransport stores a second neutral's frequency at
    // speciesTransport[neutralIndex2_ + ...] with neutralIndex2_ = -1 (src/gas_transport.cpp:717, a nitrogen-only
    // member): one double BEFORE the array.  The call therefore gets a scratch array with one double of padding in front.
    double sp[1 + gpudata::MAXSPECIES] = {0};
    r->transport->ComputeSourceTransportProperties(U + i * r->neq, Up + i * r->neq, gradUp + i * r->neq * r->dim, E, 0.0,
                                                   global + i * SrcTrns::NUM_SRC_TRANS, sp + 1,
                                                   diffVel + i * 3 * gpudata::MAXSPECIES, n_sp + i * gpudata::MAXSPECIES);
    for (int k = 0; k < gpudata::MAXSPECIES; k++) species[i * gpudata::MAXSPECIES + k] = sp[1 + k];
  }
}

void tpsref_convective_flux(void *h, int n, const double *U, double *flux) {
  REF;
  for (int i = 0; i < n; i++) r->fluxes->ComputeConvectiveFluxes(U + i * r->neq, flux + i * r->neq * r->dim);
}
// radius[i]: transip[0] of the axisymmetric formulation (NULL: planar)
void tpsref_viscous_flux(void *h, int n, const double *U, const double *gradUp, const double *radius, double *flux) {
  REF;
  for (int i = 0; i < n; i++) {
    double transip[3] = {radius ? radius[i] : -1.0, 0, 0};
    r->fluxes->ComputeViscousFluxes(U + i * r->neq, gradUp + i * r->neq * r->dim, transip, 0.0, 0.0,
                                    flux + i * r->neq * r->dim);
  }
}
// normals[i][dim]; primFlux / primFluxIdxs: one BoundaryViscousFluxData (MAXEQUATIONS entries) for all points, or per
// point when perPoint != 0 (the sheath)
void tpsref_bdr_viscous_flux(void *h, int n, const double *U, const double *gradUp, const double *radius,
                             const double *normals, const double *primFlux, const int *primFluxIdxs, int perPoint,
                             double *normalFlux) {
  REF;
  for (int i = 0; i < n; i++) {
    double transip[3] = {radius ? radius[i] : -1.0, 0, 0};
    const BoundaryViscousFluxData bc =
        bdr_flux_data(r->dim, normals + i * r->dim, primFlux + (perPoint ? i * gpudata::MAXEQUATIONS : 0), primFluxIdxs);
    r->fluxes->ComputeBdrViscousFluxes(U + i * r->neq, gradUp + i * r->neq * r->dim, transip, 0.0, 0.0, bc,
                                       normalFlux + i * r->neq);
  }
}
void tpsref_lf(void *h, int n, const double *U1, const double *U2, const double *normals, double *flux) {
  REF;
  for (int i = 0; i < n; i++)
    r->lf->Eval_LF(U1 + i * r->neq, U2 + i * r->neq, normals + i * r->dim, flux + i * r->neq);
}
// RiemannSolverTPS::Eval with useRoe (Eval_Roe itself is private): the Vector interface only
void tpsref_roe(void *h, int n, const double *U1, const double *U2, const double *normals, double *flux) {
  REF;
  for (int i = 0; i < n; i++) {
    Vector a(const_cast<double *>(U1 + i * r->neq), r->neq), b(const_cast<double *>(U2 + i * r->neq), r->neq);
    Vector nor(const_cast<double *>(normals + i * r->dim), r->dim), f(r->neq);
    r->roe->Eval(a, b, nor, f, false);
    for (int eq = 0; eq < r->neq; eq++) flux[i * r->neq + eq] = f(eq);
  }
}

// Chemistry: n_sp[i][MAXSPECIES], Th[i], Te[i] -> kfwd, keq, progress [i][MAXREACTIONS], creation [i][MAXSPECIES]
int tpsref_chemistry(void *h, int n, const double *n_sp, const double *Th, const double *Te, double *kfwd, double *keq,
                     double *progress, double *creation) {
  REF;
  if (!r->chemistry) return 1;
  for (int i = 0; i < n; i++) {
    double emission[gpudata::MAXSPECIES];
    double *kf = kfwd + i * gpudata::MAXREACTIONS, *kc = keq + i * gpudata::MAXREACTIONS;
    double *pr = progress + i * gpudata::MAXREACTIONS;
    r->chemistry->computeForwardRateCoeffs(n_sp + i * gpudata::MAXSPECIES, Th[i], Te[i], 0, kf);
    r->chemistry->computeEquilibriumConstants(Th[i], Te[i], kc);
    r->chemistry->computeProgressRate(n_sp + i * gpudata::MAXSPECIES, kf, kc, pr);
    r->chemistry->computeCreationRate(pr, creation + i * gpudata::MAXSPECIES, emission);
  }
  return 0;
}
// NetEmission::computeEnergySink
int tpsref_energy_sink(void *h, int n, const double *Th, double *out) {
  REF;
  if (!r->nec) return 1;
  for (int i = 0; i < n; i++) out[i] = r->nec->computeEnergySink(Th[i]);
  return 0;
}
}
