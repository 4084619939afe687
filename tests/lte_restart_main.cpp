// Stand-alone driver of the restart from an LTE solution on the host (tests/test_lte_restart_host.py builds it with plain g++,
// once without and once with -fsanitize=address,undefined, and runs it as a child process; nothing is loaded into Python):
// tps_amd/csrc/lte_restart.hpp, the text the kernels of lte_restart.hip run, on plain arrays.
// stdin:  num_species ambipolar two_temperature nvel
//         mass, charge, formation energy, degeneracy, molar c_v / R: one line of num_species numbers each
//         the tables energy, gas_constant, temperature: `nx ny`, then x, y and f row by row
//         n, then n states of nvel + 2 numbers (rho, rho u, rho E)
//         m, then m pairs (T, p)
// stdout: per state `S flags T density_change | U ... | Up ...`, per pair `C flags | n_sp ...`, %.17g; then LTE_RESTART DONE
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/tpsrhs.h"
#include "../tps_amd/csrc/lte_restart.hpp"

namespace {

using namespace tpsrhs;

struct HostTable {
  int nx = 0, ny = 0;
  std::vector<double> x, y, f;
  tpsrhs_table2d view() const { return {nx, ny, x.data(), y.data(), f.data()}; }
};

bool read_table(HostTable &h) {
  if (std::scanf("%d %d", &h.nx, &h.ny) != 2 || h.nx < 1 || h.ny < 1) return false;
  h.x.resize(h.nx);
  h.y.resize(h.ny);
  h.f.resize(static_cast<size_t>(h.nx) * h.ny);
  bool ok = true;
  for (double &v : h.x) ok = ok && std::scanf("%lf", &v) == 1;
  for (double &v : h.y) ok = ok && std::scanf("%lf", &v) == 1;
  for (double &v : h.f) ok = ok && std::scanf("%lf", &v) == 1;
  return ok;
}

}  // namespace

int main() {
  tpsrhs_physics phys;
  std::memset(&phys, 0, sizeof phys);
  phys.working_fluid = TPSRHS_USER_DEFINED;
  tpsrhs_perfect_mixture &mx = phys.mixture;
  int nvel = 0;
  if (std::scanf("%d %d %d %d", &mx.num_species, &mx.ambipolar, &mx.two_temperature, &nvel) != 4 || mx.num_species < 3 ||
      mx.num_species > TPSRHS_MAXSPECIES || nvel < 1 || nvel > 3) {
    std::fprintf(stderr, "lte_restart: malformed mixture line\n");
    return 2;
  }
  mx.is_electron_included = 1;
  const int ns = mx.num_species;
  const int param[4] = {TPSRHS_SPECIES_MW, TPSRHS_SPECIES_CHARGES, TPSRHS_FORMATION_ENERGY, TPSRHS_SPECIES_DEGENERACY};
  bool ok = true;
  for (int k = 0; k < 4; k++)
    for (int sp = 0; sp < ns; sp++) ok = ok && std::scanf("%lf", &mx.gas_params[sp + param[k] * ns]) == 1;
  for (int sp = 0; sp < ns; sp++) ok = ok && std::scanf("%lf", &mx.molar_cv[sp]) == 1;
  HostTable t[3];
  for (HostTable &h : t) ok = ok && read_table(h);
  if (!ok) {
    std::fprintf(stderr, "lte_restart: malformed parameters or tables\n");
    return 2;
  }
  const tpsrhs_lte_restart in = {t[0].view(), t[1].view(), t[2].view()};
  try {
    check_lte_restart_mixture(phys, "lte_restart");
    check_lte_restart_tables(in);
  } catch (const std::exception &e) {
    std::printf("refused: %s\n", e.what());
    return 3;
  }
  const LteRestartParams P = lte_restart_params(mx, nvel);
  std::vector<std::vector<BilinearCell>> homes;  // (storage of the records' own alignment, for the axes as well)
  const LteRestartTables LT = make_lte_restart_tables(in, [&homes](const void *src, size_t bytes) {
    homes.emplace_back((bytes + sizeof(BilinearCell) - 1) / sizeof(BilinearCell));
    std::memcpy(static_cast<void *>(homes.back().data()), src, bytes);
    return static_cast<const void *>(homes.back().data());
  });
  const int neq = nvel + 2 + P.num_active + (P.two_temperature ? 1 : 0);
  long n = 0;
  if (std::scanf("%ld", &n) != 1 || n < 0) return 2;
  for (long i = 0; i < n; i++) {
    // the rows the routine does not read start as NaN: it must write every one of them
    std::vector<double> U(neq, std::nan("")), Up(neq, std::nan(""));
    for (int k = 0; k < nvel + 2; k++)
      if (std::scanf("%lf", &U[k]) != 1) return 2;
    const LteNode nd = species_from_lte(P, LT, U.data(), Up.data());
    std::printf("S %d %.17g %.17g |", nd.flags, nd.T, nd.density_change);
    for (int k = 0; k < neq; k++) std::printf(" %.17g", U[k]);
    std::printf(" |");
    for (int k = 0; k < neq; k++) std::printf(" %.17g", Up[k]);
    std::printf("\n");
  }
  long m = 0;
  if (std::scanf("%ld", &m) != 1 || m < 0) return 2;
  for (long i = 0; i < m; i++) {
    double T, p;
    if (std::scanf("%lf %lf", &T, &p) != 2) return 2;
    std::vector<double> n_sp(TPSRHS_MAXSPECIES, 0.0);
    const LteComposition c = lte_composition(P, T, p, n_sp.data());
    std::printf("C %d |", c.flags);
    for (int sp = 0; sp < ns; sp++) std::printf(" %.17g", n_sp[sp]);
    std::printf("\n");
  }
  std::printf("LTE_RESTART DONE\n");
  return 0;
}
