// TEST INFRASTRUCTURE (tests/test_flux_fields_host.py): the per-node body of tpsrhs_get_flux -- flux_fields.hpp::flux_parts,
// the very header of tps_amd/csrc -- compiled for the HOST through tests/host_physics/hip/hip_runtime.h, as a stand-alone
// program, plain and under AddressSanitizer / UndefinedBehaviorSanitizer.  Three instantiations: dry air 3-D, axisymmetric
// dry air, the ternary ambipolar argon plasma in planar 2-D with argon-minimal transport.
//
// usage: flux_fields_main <disc.bin> <physics.bin> <dry3d.bin> <axi.bin> <plasma2d.bin>
// The two struct images and the states are written by the test (a state file: n, neq, dim as doubles, then U[neq][n],
// G[dim*neq][n], radius[n]).  Checked per node:
//   CONVECTIVE - VISCOUS against the physics' own total_flux, entrywise within K eps (|C| + |V|);
//   the density row of VISCOUS exactly 0;  VISCOUS exactly 0 for TPSRHS_EULER (dry air 3-D, run a second time).
// K = the rounding-carrying terms behind one entry, counted from flux_fields.hpp::conv_tensor and the closures' visc_flux:
//   density    1                                           (C is a copy, V is zero)
//   momentum   2 + 3 + (NVEL + 1)                           C: product, + p;  V: sum of two gradients, x mu, + bulk x div u
//                                                           (div u: DIM gradients and u_r / r)
//   energy     2 + NVEL (K_momentum - 2 + 1) + 2 + 2 + 2 NSP  C: sum, product;  V: each stress times its velocity, heavy and
//                                                           electron conduction (2 + 2), species enthalpy times velocity (2 NSP)
//   species    1 + 2                                        C: product;  V: density times diffusion velocity
//   electron energy  2 + 2 + 2                              C: sum, product;  V: conduction, enthalpy times velocity
// Exit status 0: every check held.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/tpsrhs.h"
#include "flux_fields.hpp"
#include "physics_dryair_axisym.hpp"
#include "plasma_params_host.hpp"

using namespace tpsrhs;

namespace {

std::vector<double> read_doubles(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(3);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> v(static_cast<size_t>(bytes) / sizeof(double));
  if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(3);
  std::fclose(f);
  return v;
}

template <class T>
void read_struct(const char *path, T *out) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f || std::fread(out, sizeof(T), 1, f) != 1) {
    std::fprintf(stderr, "cannot read %zu bytes of %s\n", sizeof(T), path);
    std::exit(3);
  }
  std::fclose(f);
}

template <class PH>
int term_count(int eq) {
  constexpr int NVEL = PH::NVEL, NSP = PH::NACTIVE > 0 ? PH::NACTIVE + 2 : 0;
  const int kmom = 2 + 3 + (NVEL + 1);
  if (eq == 0) return 1;
  if (eq <= NVEL) return kmom;
  if (eq == NVEL + 1) return 2 + NVEL * (kmom - 2 + 1) + 2 + 2 + 2 * NSP;
  if (eq < NVEL + 2 + PH::NACTIVE) return 1 + 2;
  return 2 + 2 + 2;
}

// the physics' own F_c - F_v with the context k_flux gives it
template <class PH>
void own_total(typename PH::PRef p, const double *uc, const double *g, double radius, double *F) {
  const typename PH::State st = PH::make_state(p, uc);
  if constexpr (PH::TWO_STEP) {
    typename PH::FluxCoef fc;
    PH::template flux_coeffs<false>(p, uc, st, fc);
    PH::total_flux(p, uc, st, fc, g, PH::AXISYM ? radius : -1.0, F);
  } else if constexpr (PH::AXISYM) {
    PH::total_flux(p, uc, st, g, radius, F);
  } else {
    PH::total_flux(p, uc, st, g, F);
  }
}

template <class PH>
int check(const char *name, typename PH::PRef p, const std::vector<double> &data, bool euler) {
  constexpr int NEQ = PH::NEQ, DIM = PH::DIM;
  const long n = static_cast<long>(data[0]);
  if (static_cast<int>(data[1]) != NEQ || static_cast<int>(data[2]) != DIM ||
      data.size() != static_cast<size_t>(3 + n * (NEQ + NEQ * DIM + 1))) {
    std::fprintf(stderr, "%s: the state file does not fit (neq %d, dim %d)\n", name, NEQ, DIM);
    return 3;
  }
  const double *U = data.data() + 3, *G = U + NEQ * n, *R = G + NEQ * DIM * n;
  double worst[NEQ] = {};
  long bad = 0;
  for (long i = 0; i < n; i++) {
    double u[NEQ], g[NEQ * DIM];
    for (int eq = 0; eq < NEQ; eq++) u[eq] = U[eq * n + i];
    for (int k = 0; k < NEQ * DIM; k++) g[k] = G[k * n + i];
    FluxPoint pt;
    pt.radius = PH::AXISYM ? R[i] : 1.0;
    pt.pc.delta = 0.0;
    pt.pc.X[0] = pt.pc.X[1] = pt.pc.X[2] = 0.0;
    pt.ec = eddy_off();
    // the three parts as the kernel asks for them: each call writes only what its part needs
    double Fc[NEQ * DIM], Fv[NEQ * DIM], Fc2[NEQ * DIM], Fv2[NEQ * DIM], T[NEQ * DIM];
    flux_parts<PH>(p, FLUX_TOTAL, u, g, pt, Fc, Fv);
    flux_parts<PH>(p, FLUX_CONVECTIVE, u, g, pt, Fc2, nullptr);
    flux_parts<PH>(p, FLUX_VISCOUS, u, g, pt, nullptr, Fv2);
    double uc[NEQ];
    for (int eq = 0; eq < NEQ; eq++) uc[eq] = u[eq];
    PH::clamp_species(uc);
    own_total<PH>(p, uc, g, pt.radius, T);
    for (int k = 0; k < NEQ * DIM; k++) {
      const int eq = k % NEQ;
      if (Fc[k] != Fc2[k] || Fv[k] != Fv2[k]) bad++;  // a part does not depend on which parts were asked for
      if (!std::isfinite(Fc[k]) || !std::isfinite(Fv[k])) bad++;
      if (eq == 0 && Fv[k] != 0.0) bad++;
      if (euler && Fv[k] != 0.0) bad++;
      const double err = std::fabs((Fc[k] - Fv[k]) - T[k]), scale = DBL_EPSILON * (std::fabs(Fc[k]) + std::fabs(Fv[k]));
      const double ratio = scale > 0.0 ? err / scale : (err > 0.0 ? HUGE_VAL : 0.0);
      if (ratio > worst[eq]) worst[eq] = ratio;
      if (ratio > term_count<PH>(eq)) bad++;
    }
  }
  std::printf("%s%s: %ld nodes, per row K / worst |C - V - total_flux| in eps (|C| + |V|):", name, euler ? " (Euler)" : "", n);
  for (int eq = 0; eq < NEQ; eq++) std::printf(" %d/%.3g", term_count<PH>(eq), worst[eq]);
  std::printf("  -> %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

DryAirParams dry_air_params(int eq_system) {  // tpsrhs.hip::fill_single_fluid_params with the reference's defaults
  DryAirParams d;
  std::memset(&d, 0, sizeof(d));
  d.gamma = 1.4;
  d.Rg = 287.058;
  d.inv_Rg = 1.0 / d.Rg;
  d.visc_mult = 1.0;
  d.bulk_mult = 0.6;
  d.C1 = 1.458e-6;
  d.S0 = 110.4;
  d.cp_div_pr = d.gamma * d.Rg / (0.71 * (d.gamma - 1.0));
  d.eq_system = eq_system;
  d.ref_length = 1.0;
  return d;
}

std::vector<std::vector<double>> g_tables;

}  // namespace

int main(int argc, char **argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s disc.bin physics.bin dry3d.bin axi.bin plasma2d.bin\n", argv[0]);
    return 3;
  }
  int rc = 0;
  {
    typedef DryAirPhys<3> PH;
    const std::vector<double> data = read_doubles(argv[3]);
    const DryAirParams ns = dry_air_params(TPSRHS_NS), eu = dry_air_params(TPSRHS_EULER);
    rc |= check<PH>("dry air 3-D", PH::pref(ns), data, false);
    rc |= check<PH>("dry air 3-D", PH::pref(eu), data, true);
  }
  {
    typedef DryAirAxiPhys PH;
    const std::vector<double> data = read_doubles(argv[4]);
    const DryAirParams ns = dry_air_params(TPSRHS_NS);
    rc |= check<PH>("axisymmetric dry air", PH::pref(ns), data, false);
  }
  {
    typedef PlasmaPhys<2, 2, 3, true, false, TRANSPORT_ARGON_MINIMAL> PH;
    tpsrhs_disc disc;
    static tpsrhs_physics phys;
    read_struct(argv[1], &disc);
    read_struct(argv[2], &phys);
    const std::vector<double> data = read_doubles(argv[5]);
    static PH::Params prm;
    static ChemDev chem;
    g_tables.reserve(64);
    fill_plasma_params<PH::NSP>(prm, chem, &disc, &phys, 0, nullptr, [](const tpsrhs_table &t) {
      g_tables.emplace_back();
      TableDev td = table_coeffs(t, g_tables.back());
      td.x = g_tables.back().data();
      td.a = td.x + td.n;
      td.b = td.x + 2 * td.n;
      return td;
    });
    prm.chem = &chem;
    rc |= check<PH>("argon ternary 2-D, argon-minimal", PH::pref(&prm), data, false);
  }
  return rc;
}
