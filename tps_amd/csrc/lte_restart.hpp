// Restart of a species plasma from an LTE solution (`io/restartFromLTE = True`): PerfectMixture::GetSpeciesFromLTE of the
// reference, both forms -- the composition at (T, p) from the Saha equation and the Boltzmann distribution
// (src/equation_of_state.cpp:2096-2187) and the state of a node rebuilt from its rho, rho u, rho E through the tables of the
// table gas (:1944-2094), which M2ulPhyS::initilizeSpeciesFromLTE runs over the nodes in a serial host loop
// (src/M2ulPhyS.cpp:2388-2461; compiled out of the reference's CUDA and HIP builds).
//
// One text for the kernels of lte_restart.hip and for the stand-alone program tests/lte_restart_main.cpp, in the way of
// table2d.hpp: TPSRHS_T2_HD is __host__ __device__ under hipcc and nothing for a plain C++ compiler, everything is read
// through plain pointers.  The order of operations is the reference's, the cancellation in n_e = -s + sqrt(s^2 + n_0 s)
// included: parity with its arithmetic is the contract.  The loops over the species run to the constant LTE_MAXSP under a
// guard, so that every index into a local array is a constant after unrolling (registers, no scratch memory) while the
// species count stays a run-time number: one kernel for every mixture.
//
// Index convention of the routine (:1967-1970, :2112-2115): the ion at numSpecies - 3, the electron at numSpecies - 2, the
// neutral background at numSpecies - 1; the species 0 .. numSpecies - 4 are excited levels of the neutral.
#ifndef TPSRHS_LTE_RESTART_HPP_
#define TPSRHS_LTE_RESTART_HPP_

#include <cmath>
#include <string>

#include "../../include/tpsrhs.h"
#include "division_mode.hpp"
#include "operator_plan.hpp"
#include "table2d.hpp"

namespace tpsrhs {

constexpr int LTE_MAXSP = TPSRHS_MAXSPECIES;
// src/equation_of_state.hpp:55-67
constexpr double LTE_RGAS = 8.3144598;
constexpr double LTE_AVOGADRO = 6.0221409e+23;
constexpr double LTE_BOLTZMANN = LTE_RGAS / LTE_AVOGADRO;
constexpr double LTE_PLANCK = 6.62607015e-34;
constexpr double LTE_ELECTRONMASS = 9.1093837015e-31;
constexpr double LTE_PI = 3.14159265358979323846;

// what the routine reads of the mixture; cv = molar_cv * R (molarCV_, src/equation_of_state.cpp:486-489)
struct LteRestartParams {
  int num_species, num_active, nvel, ambipolar, two_temperature;
  double mw[LTE_MAXSP], eform[LTE_MAXSP], degen[LTE_MAXSP], cv[LTE_MAXSP];
};
// energy and gas constant on the (T, rho) grid of the thermo file, the first guess T(e, rho) on that of the e_rev file
struct LteRestartTables {
  Grid2Dev g_th;
  const BilinearCell *c_e, *c_R;
  Grid2Dev g_rev;
  const BilinearCell *c_T;
};

// per-node flags: where the reference prints its warning (:2024-2027), and where it would have hit one of its asserts
// (:2014, :2181-2186)
enum { LTE_NOT_CONVERGED = 1, LTE_INVALID = 2 };

struct LteComposition {
  double n_e, n_B;
  int flags;
};
struct LteNode {
  double T, density_change;  // |rho_update / rho - 1|, the quantity the comment at :2048-2057 tells the user to watch
  int flags;
};

inline LteRestartParams lte_restart_params(const tpsrhs_perfect_mixture &mx, int nvel) {
  LteRestartParams p = {};
  const int ns = mx.num_species;
  p.num_species = ns;
  p.ambipolar = mx.ambipolar != 0;
  p.two_temperature = mx.two_temperature != 0;
  p.num_active = p.ambipolar ? ns - 2 : ns - 1;
  p.nvel = nvel;
  for (int sp = 0; sp < ns && sp < LTE_MAXSP; sp++) {
    p.mw[sp] = mx.gas_params[sp + TPSRHS_SPECIES_MW * ns];
    p.eform[sp] = mx.gas_params[sp + TPSRHS_FORMATION_ENERGY * ns];
    p.degen[sp] = mx.gas_params[sp + TPSRHS_SPECIES_DEGENERACY * ns];
    p.cv[sp] = mx.molar_cv[sp] * LTE_RGAS;
  }
  return p;
}

// The assumptions the routine states (:1952-1963): one charged heavy species, a positive ion of charge +e, where the
// routine looks for it; everything below it a level of the neutral; electrons in the mixture.
inline void check_lte_restart_mixture(const tpsrhs_physics &phys, const std::string &who) {
  if (phys.working_fluid == TPSRHS_DRY_AIR) throw Unsupported(who + ": dry air has no species to restart");
  if (phys.working_fluid != TPSRHS_USER_DEFINED)
    throw Unsupported(who + ": built for the species mixtures (fluid = user_defined), not for the table gas");
  const tpsrhs_perfect_mixture &mx = phys.mixture;
  const int ns = mx.num_species;
  if (!mx.is_electron_included) throw Unsupported(who + ": the mixture has no electron (species " + std::to_string(ns - 2) + ")");
  auto charge = [&](int sp) { return mx.gas_params[sp + TPSRHS_SPECIES_CHARGES * ns]; };
  for (int sp = 0; sp < ns - 3; sp++)
    if (charge(sp) != 0.0)
      throw Unsupported(who + ": species " + std::to_string(sp) + " carries a charge; the species below numSpecies - 3 = " +
                        std::to_string(ns - 3) + " must be excited levels of the neutral");
  if (charge(ns - 3) != 1.0)
    throw Unsupported(who + ": species " + std::to_string(ns - 3) + " (numSpecies - 3) must be the ion of charge +1");
  if (charge(ns - 2) != -1.0) throw Unsupported(who + ": species " + std::to_string(ns - 2) + " (numSpecies - 2) must be the electron");
}
inline void check_lte_restart_tables(const tpsrhs_lte_restart &in) {
  check_table2d(in.energy, "lte_restart.energy");
  check_table2d(in.gas_constant, "lte_restart.gas_constant");
  check_table2d(in.temperature, "lte_restart.temperature");
  for (int j = 0; j < in.energy.ny; j++)  // the Newton iteration divides by de/dT
    for (int i = 1; i < in.energy.nx; i++)
      if (!(in.energy.f[j * in.energy.nx + i] > in.energy.f[j * in.energy.nx + i - 1]))
        throw std::invalid_argument("lte_restart.energy: e(T, rho) must increase with T on every density line");
  if (!same_grid2d(in.energy, in.gas_constant))
    throw Unsupported("lte_restart: energy and gas_constant must share their axes (the columns of one thermo file)");
}
// place(src, bytes): as for make_lte2d_tables (table2d.hpp)
template <class Place>
inline LteRestartTables make_lte_restart_tables(const tpsrhs_lte_restart &in, Place &&place) {
  LteRestartTables lt;
  lt.g_th = make_grid2d(in.energy, place);
  lt.c_e = place_cells(in.energy, place);
  lt.c_R = place_cells(in.gas_constant, place);
  lt.g_rev = make_grid2d(in.temperature, place);
  lt.c_T = place_cells(in.temperature, place);
  return lt;
}

// PerfectMixture::GetSpeciesFromLTE(T, p, n_sp), src/equation_of_state.cpp:2096-2187: n_sp[numSpecies] in mol/m^3
TPSRHS_T2_HD inline LteComposition lte_composition(const LteRestartParams &P, double T, double p, double *n_sp) {
  TPSRHS_IEEE_DIVISION
  const int ns = P.num_species, nPop = ns - 3, iIon1 = ns - 3, iBackground = ns - 1;  // (the electron: ns - 2)
  const double n_0 = p / T / LTE_RGAS;
  double ex[LTE_MAXSP - 3] = {};
  double Q_n = 1.0;  // the ground state
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP - 3; sp++)
    if (sp < nPop) {
      ex[sp] = exp(-P.eform[sp] / LTE_RGAS / T);
      Q_n += P.degen[sp] * ex[sp];
    }
  double Q_i = 0.0, mw_ion = 0.0, mw_neu = 0.0, EF_ion = 0.0;
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP; sp++) {
    if (sp == iIon1) {
      Q_i = P.degen[sp];
      mw_ion = P.mw[sp];
      EF_ion = P.eform[sp];
    }
    if (sp == iBackground) mw_neu = P.mw[sp];
  }
  const double Q_e = 2.0;
  const double massratio = mw_ion / mw_neu;
  const double mr32 = massratio * sqrt(massratio);
  const double lame = LTE_PLANCK / (sqrt(2 * LTE_PI * LTE_ELECTRONMASS * LTE_BOLTZMANN * T));
  const double lame3 = lame * lame * lame;
  const double Qrat = Q_e * Q_i / Q_n;
  const double tempSaha = mr32 * (Qrat / lame3) * exp(-EF_ion / LTE_RGAS / T) / LTE_AVOGADRO;
  const double n_e = -tempSaha + sqrt(tempSaha * tempSaha + n_0 * tempSaha);
  const double n_neutral = n_0 - 2 * n_e;  // charge neutrality
  const double n_B = n_neutral / Q_n;
  double n_0_check = 0.0;
  bool negative = false;
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP; sp++)
    if (sp < ns) {
      double v;
      if (sp < nPop)
        v = n_neutral * P.degen[sp] * ex[sp < LTE_MAXSP - 3 ? sp : 0] / Q_n;
      else if (sp == iBackground)
        v = n_B;
      else
        v = n_e;  // iIon1, iElectron
      n_sp[sp] = v;
      n_0_check += v;
      negative = negative || !(v >= 0.0);
    }
  LteComposition c;
  c.n_e = n_e;
  c.n_B = n_B;
  c.flags = (negative || !(n_e >= 0.0) || !(fabs(n_0 - n_0_check) / n_0 < 1e-14)) ? LTE_INVALID : 0;
  return c;
}

// PerfectMixture::GetSpeciesFromLTE(conserv, primit, tables), src/equation_of_state.cpp:1944-2094.  U and Up are the node's
// rows of the state and of the primitives, anything with operator[] (a plain array on the host, a strided view of the byNODES
// vectors in the kernel).  Read: U[0 .. nvel + 1].  Written: every row of both.  The Newton iteration is that of
// lte2d_temperature (table2d.hpp) with the reference's other ending: a node that has not converged goes on with its last
// iterate.
template <class RowsU, class RowsUp>
TPSRHS_T2_HD inline LteNode species_from_lte(const LteRestartParams &P, const LteRestartTables &LT, RowsU &&U, RowsUp &&Up) {
  TPSRHS_IEEE_DIVISION
  const int ns = P.num_species, nvel = P.nvel, iTh = nvel + 1, iElectron = ns - 2, iBackground = ns - 1;
  const int iTe = nvel + 2 + P.num_active;
  LteNode out;
  out.flags = 0;
  const double rho = U[0];
  double vel[3] = {0.0, 0.0, 0.0};
  double den_vel2 = 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++)
    if (d < nvel) {
      const double m = U[d + 1];
      vel[d] = m / rho;
      den_vel2 += m * m;
    }
  den_vel2 /= rho;
  const double energy = (U[iTh] - 0.5 * den_vel2) / rho;

  // the temperature from the tables
  double T = table2d_at(LT.g_rev, LT.c_T, energy, rho);
  const AxisCell cy = cell_y(LT.g_th, rho);
  const int row = cy.i * (LT.g_th.nx - 1);
  AxisCell cx = cell_x(LT.g_th, T);
  BilinearCell c = LT.c_e[row + cx.i];
  double dedT = cell_dx(c, cy.d);
  double res = energy - ((c.z + c.zy * cy.d) + dedT * cx.d);
  const double res0 = fabs(res);
  const double atol = 1e-18, rtol = 1e-12, dT_atol = 1e-12, dT_rtol = 1e-8;
  bool converged = (fabs(res) < atol) || (fabs(res) / fabs(res0) < rtol);
  int niter = 0;
  while (!converged && niter < 20) {
    const double dT = res / dedT;
    T += dT;
    if (!(T > 0.0)) out.flags |= LTE_INVALID;  // assert(T > 0)
    cx = cell_x(LT.g_th, T);
    c = LT.c_e[row + cx.i];
    dedT = cell_dx(c, cy.d);
    res = energy - ((c.z + c.zy * cy.d) + dedT * cx.d);
    converged = (fabs(res) < atol) || (fabs(res) / res0 < rtol) || (fabs(dT) < dT_atol) || (fabs(dT) / T < dT_rtol);
    niter++;
  }
  if (!converged) out.flags |= LTE_NOT_CONVERGED;

  // the pressure, then the number densities at (T, p)
  c = LT.c_R[row + cx.i];
  const double R = (c.z + c.zy * cy.d) + cell_dx(c, cy.d) * cx.d;
  const double p_0 = rho * R * T;
  double n_sp[LTE_MAXSP] = {};
  const LteComposition comp = lte_composition(P, T, p_0, n_sp);
  out.flags |= comp.flags;
  const double n_e = comp.n_e;

  // the state: temperature and pressure are kept, the density follows from the composition
  double rho_update = 0.0;
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP; sp++)
    if (sp < ns) rho_update += n_sp[sp] * P.mw[sp];
  U[0] = rho_update;
  Up[0] = rho_update;
#pragma unroll
  for (int d = 0; d < 3; d++)
    if (d < nvel) {
      U[d + 1] = rho_update * vel[d];
      Up[d + 1] = vel[d];
    }
  double cv_e = 0.0, cv_B = 0.0;
  double totalHeatCapacity = 0.0;  // computeHeaviesHeatCapacity, :576-584
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP; sp++) {
    if (sp < P.num_active) {
      U[nvel + 2 + sp] = n_sp[sp] * P.mw[sp];
      Up[nvel + 2 + sp] = n_sp[sp];
      if (sp != iElectron) totalHeatCapacity += n_sp[sp] * P.cv[sp];
    }
    if (sp == iElectron) cv_e = P.cv[sp];
    if (sp == iBackground) cv_B = P.cv[sp];
  }
  totalHeatCapacity += comp.n_B * cv_B;
  double rhoE_e = 0.0;
  if (P.two_temperature) {
    rhoE_e = n_e * cv_e * T;
    U[iTe] = rhoE_e;
    Up[iTe] = T;  // the electron temperature is the primitive
  } else {
    totalHeatCapacity += n_e * cv_e;
  }
  double totalEnergy = 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++)
    if (d < nvel) totalEnergy += vel[d] * vel[d];
  totalEnergy *= 0.5 * rho_update;
  totalEnergy += totalHeatCapacity * T;
  if (P.two_temperature) totalEnergy += rhoE_e;
#pragma unroll
  for (int sp = 0; sp < LTE_MAXSP; sp++)
    if (sp < ns - 2) totalEnergy += n_sp[sp] * P.eform[sp];
  U[iTh] = totalEnergy;
  Up[iTh] = T;
  out.T = T;
  out.density_change = fabs(rho_update / rho - 1.0);
  return out;
}

}  // namespace tpsrhs
#endif
