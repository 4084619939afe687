// What tpsrhs_create decides before it touches a device or the mesh connectivity: every refusal that follows from the
// discretisation, the physics and the boundary conditions alone, and the handful of derived facts the build phase
// (tpsrhs.hip::setup) then acts on.  Plain C++17, no HIP: tests/operator_plan_main.cpp drives it on the host.
//
// The numbers and the two predicates below are host copies of what the device headers define (physics_dryair.hpp,
// physics_plasma.hpp); tpsrhs.hip checks that they agree.
#ifndef TPSRHS_OPERATOR_PLAN_HPP_
#define TPSRHS_OPERATOR_PLAN_HPP_

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/tpsrhs.h"
#include "unsupported.hpp"

namespace tpsrhs {

constexpr int PLAN_MAXBC = 16, PLAN_PLASMA_MAXBC = 8;
enum { PLAN_TRANSPORT_CONSTANT = 0, PLAN_TRANSPORT_ARGON_MINIMAL = 1, PLAN_TRANSPORT_ARGON_MIXTURE = 2 };

inline bool plan_is_face_inlet(int category, int type) {
  return category == TPSRHS_INLET && type >= TPSRHS_SUB_DENS_VEL_FACE_X && type <= TPSRHS_SUB_DENS_VEL_FACE_Z;
}
inline bool plan_is_non_reflecting(int category, int type) {
  return (category == TPSRHS_INLET && (type == TPSRHS_SUB_DENS_VEL_NR || type == TPSRHS_SUB_VEL_CONST_ENT)) ||
         (category == TPSRHS_OUTLET && (type == TPSRHS_SUB_P_NR || type == TPSRHS_SUB_MF_NR || type == TPSRHS_SUB_MF_NR_PW));
}

// a two-dimensional table as tpsrhs_table2d states it: both axes strictly increasing, at least one cell, finite data
inline void check_table2d(const tpsrhs_table2d &t, const std::string &name) {
  if (!t.x || !t.y || !t.f) throw std::invalid_argument(name + ": NULL pointer");
  if (t.nx < 2 || t.ny < 2) throw std::invalid_argument(name + ": nx >= 2 and ny >= 2 (one cell at least)");
  for (int i = 0; i < t.nx; i++)
    if (!std::isfinite(t.x[i]) || (i > 0 && !(t.x[i] > t.x[i - 1]))) throw std::invalid_argument(name + ": x must be finite and strictly increasing");
  for (int j = 0; j < t.ny; j++)
    if (!std::isfinite(t.y[j]) || (j > 0 && !(t.y[j] > t.y[j - 1]))) throw std::invalid_argument(name + ": y must be finite and strictly increasing");
  for (int64_t k = 0; k < static_cast<int64_t>(t.nx) * t.ny; k++)
    if (!std::isfinite(t.f[k])) throw std::invalid_argument(name + ": non-finite value");
}
inline bool same_grid2d(const tpsrhs_table2d &a, const tpsrhs_table2d &b) {
  if (a.nx != b.nx || a.ny != b.ny) return false;
  for (int i = 0; i < a.nx; i++)
    if (a.x[i] != b.x[i]) return false;
  for (int j = 0; j < a.ny; j++)
    if (a.y[j] != b.y[j]) return false;
  return true;
}
// the tables of the two-dimensional table gas (tpsrhs_lte2d)
inline void check_lte2d(const tpsrhs_lte2d &in) {
  check_table2d(in.energy, "lte2d.energy");
  check_table2d(in.gas_constant, "lte2d.gas_constant");
  check_table2d(in.sound_speed, "lte2d.sound_speed");
  check_table2d(in.temperature, "lte2d.temperature");
  check_table2d(in.viscosity, "lte2d.viscosity");
  check_table2d(in.conductivity, "lte2d.conductivity");
  check_table2d(in.electric_conductivity, "lte2d.electric_conductivity");
  for (int j = 0; j < in.energy.ny; j++)  // the Newton iteration of the temperature divides by de/dT
    for (int i = 1; i < in.energy.nx; i++)
      if (!(in.energy.f[j * in.energy.nx + i] > in.energy.f[j * in.energy.nx + i - 1]))
        throw std::invalid_argument("lte2d.energy: e(T, rho) must increase with T on every density line");
  // the reference reads e, R, c from the columns of one file and mu, kappa from those of another: one cell search serves
  // the tables of a file
  if (!same_grid2d(in.energy, in.gas_constant) || !same_grid2d(in.energy, in.sound_speed))
    throw Unsupported("lte2d: energy, gas_constant and sound_speed must share their axes (the columns of one thermo file)");
  if (!same_grid2d(in.viscosity, in.conductivity))
    throw Unsupported("lte2d: viscosity and conductivity must share their axes (the columns of one transport file)");
}

struct OperatorPlan {
  int nc = 0;  // 1: the non-collocated Gauss-Lobatto pair, 0: the collocated Gauss-Legendre pair
  int dim = 0, order = 0, nvel = 0, neq = 0;
  int sp_first = 0, sp_last = 0;  // the species rows [sp_first, sp_last) of the state, which Check_Undershoot clamps; empty without a mixture
  bool plasma = false, lte = false;  // the working fluid; neither: dry air
  bool lte2d = false;                // lte with the two-dimensional (T, rho) tables of tpsrhs_physics::lte2d
  bool heavy2d = false;              // 2-D kernels with the heavy closure interface: mixtures, axisymmetric dry air / table gas
  bool les = false;                  // dry air with a sub-grid scale model or a viscous sponge: the LES flavour of the kernels
  bool any_nr = false;               // some boundary condition is of a non-reflecting type
  // the viscous sponge plane, normal normalised over the first `dim` components (src/fluxes.cpp:77-90), the rest 0; width
  // and ratio 1 when there is none.  Read by the 2-D heavy form (VsDev, two components) and the LES form (DryAirParams).
  int sponge = 0;
  double sponge_n[3] = {0, 0, 0}, sponge_p[3] = {0, 0, 0}, sponge_width = 1.0, sponge_ratio = 1.0;
  double sgs_const = 0.0;  // les: sgs.model_const or the reference's default for the model
  int transport = 0;       // plasma: PLAN_TRANSPORT_*
  // plasma: the sweeps of this operator read the Coulomb fits from the polynomial table (kernels.hpp::coulomb_tab: 3-D,
  // p = 3, collocated, single-temperature argon-minimal ternary mixture), which the build then uploads
  bool coulomb_table = false;
  std::string unit;        // plasma: the kernel family, plasma_<geo>_n<species>[a][_hi]
};

inline OperatorPlan plan_operator(int mesh_dim, const tpsrhs_disc &disc, const tpsrhs_physics &phys, int num_bcs, const tpsrhs_bc *bcs) {
  OperatorPlan pl;
  // basisType / integrationRule (src/M2ulPhyS.cpp:557-572): the collocated Gauss-Legendre pair (0, 0) of the
  // cylinder / wedge / torch inputs, or the Gauss-Lobatto pair (1, 1), the reference's defaults (:2671-2672)
  if (disc.basis_type == TPSRHS_BASIS_GAUSS_LEGENDRE && disc.int_rule_type == 0)
    pl.nc = 0;
  else if (disc.basis_type == TPSRHS_BASIS_GAUSS_LOBATTO && disc.int_rule_type == 1)
    pl.nc = 1;
  else
    throw Unsupported("basisType / integrationRule: built pairs are (0, 0) Gauss-Legendre and (1, 1) Gauss-Lobatto");
  const bool axi = disc.axisymmetric != 0;
  if (phys.working_fluid == TPSRHS_LTE_FLUID && phys.lte2d.enabled != 0 && (!axi || pl.nc))
    throw Unsupported("WorkingFluid::LTE_FLUID (two-dimensional tables): built for the axisymmetric formulation, Gauss-Legendre pair");
  if (pl.nc && axi) throw Unsupported("the Gauss-Lobatto pair is built for the planar 2-D and the 3-D formulation");
  const bool plasma = pl.plasma = phys.working_fluid == TPSRHS_USER_DEFINED;
  if (axi && mesh_dim != 2) throw std::invalid_argument("the axisymmetric formulation needs a 2-D mesh");
  const bool lte = pl.lte = phys.working_fluid == TPSRHS_LTE_FLUID;
  if (phys.working_fluid != TPSRHS_DRY_AIR && !plasma && !lte) throw std::invalid_argument("unknown working_fluid");
  const bool lte2d = pl.lte2d = lte && phys.lte2d.enabled != 0;  // (its scope: checked above, ahead of the general refusals)
  if (lte && (!axi || pl.nc))
    throw Unsupported("WorkingFluid::LTE_FLUID (one-dimensional tables): built for the axisymmetric formulation, Gauss-Legendre pair");
  if (disc.use_roe && (mesh_dim != 2 || axi || plasma || lte))
    throw Unsupported("flow/useRoe: Eval_Roe of the reference is 2-D, single-species, not axisymmetric "
                      "(src/riemann_solver.cpp:117-206)");
  if (phys.eq_system != TPSRHS_EULER && phys.eq_system != TPSRHS_NS) throw Unsupported("NS_PASSIVE is out of scope");
  if (num_bcs > (plasma ? PLAN_PLASMA_MAXBC : PLAN_MAXBC)) throw Unsupported("too many boundary conditions");
  for (int i = 0; i < num_bcs; i++) {
    const tpsrhs_bc &b = bcs[i];
    const bool nr = plan_is_non_reflecting(b.category, b.type);
    pl.any_nr = pl.any_nr || nr;
    if (nr && (plasma || lte || axi))
      throw Unsupported("non-reflecting inlet/outlet types: perfect gas (dry air), not axisymmetric -- the reference's "
                        "characteristic algebra (src/outletBC.cpp:573-1027)");
    if (nr && (b.type == TPSRHS_SUB_MF_NR || b.type == TPSRHS_SUB_MF_NR_PW) && !(b.data[7] > 0.0))
      throw std::invalid_argument("mass-flow outlet: data[7] must hold the total patch area");
    const bool face_inlet = plan_is_face_inlet(b.category, b.type);
    if (face_inlet && (mesh_dim != 3 || axi))
      throw Unsupported("face-relative inlets (subsonicFaceBasedX/Y/Z): 3-D (the reference's face frame has three components)");
    const bool ok = nr || face_inlet || (b.category == TPSRHS_INLET && b.type == TPSRHS_SUB_DENS_VEL) ||
                    (b.category == TPSRHS_OUTLET && b.type == TPSRHS_SUB_P) ||
                    (b.category == TPSRHS_WALL &&
                     (b.type == TPSRHS_INV || b.type == TPSRHS_SLIP || b.type == TPSRHS_VISC_ADIAB || b.type == TPSRHS_VISC_ISOTH ||
                      (b.type == TPSRHS_VISC_GNRL && plasma)));
    if (!ok) throw Unsupported("boundary condition type outside the hot-path scope (attribute " + std::to_string(b.attribute) + ")");
    if (b.category == TPSRHS_WALL && b.type == TPSRHS_VISC_GNRL) {
      // the combinations the reference's input parser lets through (src/M2ulPhyS.cpp:3515-3582)
      const int hc = static_cast<int>(b.data[2]), ec = static_cast<int>(b.data[3]);
      const bool two_t = phys.mixture.two_temperature != 0;
      const bool hvy_ok = (hc == TPSRHS_ISOTH || hc == TPSRHS_ADIAB);
      const bool elec_ok = two_t ? (ec == TPSRHS_ISOTH || ec == TPSRHS_ADIAB || ec == TPSRHS_SHTH) : (ec == TPSRHS_SHTH);
      if (!hvy_ok) throw std::invalid_argument("viscous_general wall: heavy thermal condition must be isothermal or adiabatic");
      if (!elec_ok)
        throw std::invalid_argument("viscous_general wall: electron thermal condition not understood "
                                    "(single-temperature plasmas accept the sheath condition only)");
      if (ec == TPSRHS_SHTH && !phys.mixture.ambipolar)
        throw std::invalid_argument("viscous_general wall: plasma must be ambipolar for the sheath condition");
    }
  }
  pl.dim = mesh_dim;
  pl.order = disc.order;
  pl.nvel = axi ? 3 : pl.dim;
  pl.neq = pl.nvel + 2;
  pl.sp_first = pl.sp_last = pl.nvel + 2;
  if (plasma) {
    const tpsrhs_perfect_mixture &mx = phys.mixture;
    if (!mx.is_electron_included) throw Unsupported("USER_DEFINED fluids without electrons are not built");
    if (mx.num_species < 3 || mx.num_species > TPSRHS_MAXSPECIES)
      throw Unsupported("USER_DEFINED fluids: 3 to 8 species (electron, background and 1 to 6 others)");
    if (mx.num_species > 7 && phys.transport_model == TPSRHS_ARGON_MIXTURE)  // the reference asserts, src/gas_transport.cpp:905-911
      throw Unsupported("argon_mixture transport supports at most 7 species (Ar, Ar.+1, Ar_m, Ar_r, Ar_p, Ar_h, E)");
    if (mx.num_species != 3 && phys.transport_model == TPSRHS_ARGON_MINIMAL)
      throw Unsupported("argon_minimal transport is the ternary (Ar, Ar.+1, E) model");
    if (phys.transport_model != TPSRHS_CONSTANT && phys.transport_model != TPSRHS_ARGON_MINIMAL &&
        phys.transport_model != TPSRHS_ARGON_MIXTURE)
      throw Unsupported("transport model outside the built scope (constant, argon_minimal, argon_mixture)");
    pl.sp_last = pl.sp_first + (mx.ambipolar ? mx.num_species - 2 : mx.num_species - 1);
    pl.neq = pl.sp_last + (mx.two_temperature ? 1 : 0);
    pl.transport = (phys.transport_model == TPSRHS_CONSTANT)
                       ? PLAN_TRANSPORT_CONSTANT
                       : (phys.transport_model == TPSRHS_ARGON_MINIMAL ? PLAN_TRANSPORT_ARGON_MINIMAL : PLAN_TRANSPORT_ARGON_MIXTURE);
    // one shared object per (geometry, species count, ambipolar) family, and a second one for the polynomial orders
    // 4 and 5: every species count up to MAXSPECIES = 8 (MAXEQUATIONS = 13) of the reference's device build
    // (src/dataStructures.hpp:41-65), ambipolar or not
    const char *geo = (pl.dim == 3) ? "3d" : (axi ? "axi" : "2d");
    pl.unit = std::string("plasma_") + geo + "_n" + std::to_string(mx.num_species) + (mx.ambipolar ? "a" : "") +
              ((pl.order >= 4 && !pl.nc) ? "_hi" : "");
    pl.coulomb_table = pl.dim == 3 && pl.order == 3 && !pl.nc && mx.num_species == 3 && !mx.two_temperature &&
                       phys.transport_model == TPSRHS_ARGON_MINIMAL;
  }
  // Fluxes: sub-grid scale model and viscous sponge (src/fluxes.cpp:223-246).  The 2-D kernels with the heavy interface
  // take the sponge plane in MeshDev and scale their coefficients (:232-246); dry air, planar and 3-D, takes both in the
  // LES flavour of its kernels.
  const bool heavy = plasma || lte || axi;
  pl.heavy2d = pl.dim == 2 && (plasma || axi);
  const tpsrhs_visc_sponge &v = phys.visc_sponge;
  auto sponge_plane = [&] {
    // "ensure normal is actually a unit normal": the constructor every CPU build of the reference uses, and its host
    // fluxClass, normalise vsd_.n (src/fluxes.cpp:77-90, src/M2ulPhyS.cpp:612-616); the device constructor
    // (:98-125) copies it as given.  The CPU path is this library's referent.
    if (v.enabled && !(v.width > 0.0)) throw std::invalid_argument("visc_sponge.width must be positive");
    double nmag = 0.0;
    for (int k = 0; k < pl.dim && k < 3; k++) nmag += v.normal[k] * v.normal[k];
    nmag = std::sqrt(nmag);
    if (v.enabled && !(nmag > 0.0)) throw std::invalid_argument("visc_sponge.normal is zero");
    pl.sponge = v.enabled ? 1 : 0;
    for (int k = 0; k < pl.dim && k < 3; k++) {  // vsd.n / vsd.p: dim entries
      pl.sponge_n[k] = nmag > 0.0 ? v.normal[k] / nmag : 0.0;
      pl.sponge_p[k] = v.point[k];
    }
    pl.sponge_width = v.enabled ? v.width : 1.0;
    pl.sponge_ratio = v.enabled ? v.ratio : 1.0;
  };
  if (heavy && phys.sgs.model_type != TPSRHS_SGS_NONE) throw Unsupported("sub-grid scale models: built for dry air in 3-D");
  if (heavy && v.enabled && (!pl.heavy2d || pl.nc))
    throw Unsupported("viscous sponge for mixtures: built for the planar 2-D and the axisymmetric formulation, Gauss-Legendre pair");
  if (pl.heavy2d && v.enabled) sponge_plane();
  if (lte2d) {
    check_lte2d(phys.lte2d);
  } else if (lte) {
    const tpsrhs_lte &in = phys.lte;
    // LinearTable with xLogScale = fLogScale = false, as the reference hard-codes for these tables (src/M2ulPhyS.cpp:176-255);
    // the inverse table T(e) and its search aid assume linear axes
    for (const tpsrhs_table *t : {&in.energy_table, &in.gas_constant_table, &in.sound_speed_table, &in.viscosity_table,
                                  &in.conductivity_table, &in.electric_conductivity_table})
      if (t->x_log_scale || t->f_log_scale) throw std::invalid_argument("lte tables: linear scales only (x_log_scale = f_log_scale = 0)");
    for (int k = 1; k < in.energy_table.n_data && in.energy_table.f_data; k++)
      if (!(in.energy_table.f_data[k] > in.energy_table.f_data[k - 1]))
        throw std::invalid_argument("lte.energy_table: e(T) must increase (the inverse table T(e) is its transpose)");
  }
  pl.les = !heavy && (phys.sgs.model_type != TPSRHS_SGS_NONE || v.enabled);
  if (pl.les) {
    if (phys.sgs.model_type < 0 || phys.sgs.model_type > TPSRHS_SGS_SIGMA) throw std::invalid_argument("unknown sgs.model_type");
    if (axi || pl.nc || pl.any_nr)
      throw Unsupported("sub-grid scale model / viscous sponge: built for dry air, planar 2-D and 3-D, Gauss-Legendre pair, "
                        "reflecting boundary types");
    if (phys.sgs.model_type != TPSRHS_SGS_NONE && pl.dim != 3)
      throw Unsupported("sub-grid scale models need dim == 3 (the reference's strain tensor indexes three directions)");
    pl.sgs_const = phys.sgs.model_const > 0.0 ? phys.sgs.model_const  // defaults of src/M2ulPhyS.cpp:2693-2698
                                              : (phys.sgs.model_type == TPSRHS_SGS_SMAGORINSKY ? 0.12 : (phys.sgs.model_type == TPSRHS_SGS_SIGMA ? 0.135 : 0.0));
    sponge_plane();
  }
  // the 1-D operator tables are indexed by the order (basis.hpp::make_tables, c_tab): nothing outside the declared range
  // reaches them
  if (pl.order < 1 || pl.order > TPSRHS_MAXORDER)
    throw Unsupported("polynomial order " + std::to_string(pl.order) + " is not built (1.." + std::to_string(TPSRHS_MAXORDER) + ")");
  return pl;
}

}  // namespace tpsrhs
#endif
