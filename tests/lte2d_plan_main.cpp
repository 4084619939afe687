// Stand-alone driver of the two-dimensional table gas on the host (tests/test_lte2d_plan.py builds it with plain g++, once
// without and once with -fsanitize=address,undefined, and runs it as a child process; nothing is loaded into Python):
//   * tps_amd/csrc/operator_plan.hpp: the plan accepts the tables of the fixture, refuses each malformed table with
//     INVALID_ARGUMENT and the two-dimensional gas outside its scope with UNSUPPORTED;
//   * tps_amd/csrc/table2d.hpp: the temperature round trip T -> e(T, rho) -> T of the closure the kernels run, over a grid
//     of (T, rho) that visits every cell of the thermodynamic tables once.
// argv[1]: the seven tables as text (per table: `nx ny`, then x, y and f row by row), written by the test from
// tests/golden/tables/lte_tables_2d.npz in the order of tpsrhs_lte2d.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../include/tpsrhs.h"
#include "../tps_amd/csrc/operator_plan.hpp"
#include "../tps_amd/csrc/table2d.hpp"

namespace {

using namespace tpsrhs;

struct HostTable {
  int nx = 0, ny = 0;
  std::vector<double> x, y, f;
  tpsrhs_table2d view() const { return {nx, ny, x.data(), y.data(), f.data()}; }
};

bool read_tables(const char *path, HostTable (&t)[7]) {
  std::FILE *fp = std::fopen(path, "r");
  if (!fp) return false;
  bool ok = true;
  for (HostTable &h : t) {
    ok = ok && std::fscanf(fp, "%d %d", &h.nx, &h.ny) == 2 && h.nx > 0 && h.ny > 0;
    if (!ok) break;
    h.x.resize(h.nx);
    h.y.resize(h.ny);
    h.f.resize(static_cast<size_t>(h.nx) * h.ny);
    for (double &v : h.x) ok = ok && std::fscanf(fp, "%lf", &v) == 1;
    for (double &v : h.y) ok = ok && std::fscanf(fp, "%lf", &v) == 1;
    for (double &v : h.f) ok = ok && std::fscanf(fp, "%lf", &v) == 1;
  }
  std::fclose(fp);
  return ok;
}

tpsrhs_physics physics(const HostTable (&t)[7]) {
  tpsrhs_physics p;
  std::memset(&p, 0, sizeof p);
  p.eq_system = TPSRHS_NS;
  p.working_fluid = TPSRHS_LTE_FLUID;
  p.lte2d.enabled = 1;
  tpsrhs_table2d *dst[7] = {&p.lte2d.energy,    &p.lte2d.gas_constant, &p.lte2d.sound_speed,          &p.lte2d.temperature,
                            &p.lte2d.viscosity, &p.lte2d.conductivity, &p.lte2d.electric_conductivity};
  for (int k = 0; k < 7; k++) *dst[k] = t[k].view();
  return p;
}

tpsrhs_disc disc(int order, int basis, int rule, int axi) {
  tpsrhs_disc d;
  std::memset(&d, 0, sizeof d);
  d.order = order;
  d.basis_type = basis;
  d.int_rule_type = rule;
  d.axisymmetric = axi;
  return d;
}

void run(const char *name, int dim, const tpsrhs_disc &d, const tpsrhs_physics &p) {
  std::printf("%s: ", name);
  try {
    const OperatorPlan pl = plan_operator(dim, d, p, 0, nullptr);
    std::printf("ok lte %d lte2d %d heavy2d %d nvel %d neq %d\n", pl.lte ? 1 : 0, pl.lte2d ? 1 : 0, pl.heavy2d ? 1 : 0, pl.nvel, pl.neq);
  } catch (const Unsupported &e) {
    std::printf("unsupported %s\n", e.what());
  } catch (const std::invalid_argument &e) {
    std::printf("invalid %s\n", e.what());
  }
}

}  // namespace

int main(int argc, char **argv) {
  HostTable t[7];
  if (argc < 2 || !read_tables(argv[1], t)) {
    std::fprintf(stderr, "usage: lte2d_plan <tables.txt>\n");
    return 2;
  }
  const tpsrhs_disc axi = disc(3, 0, 0, 1);
  const tpsrhs_physics good = physics(t);
  run("fixture", 2, axi, good);
  {  // enabled = 0: the one-dimensional gas is asked for (its tables here are empty, which its own checks accept)
    tpsrhs_physics p = good;
    p.lte2d.enabled = 0;
    run("disabled", 2, axi, p);
  }
  // ---- malformed tables
  {
    tpsrhs_physics p = good;
    p.lte2d.sound_speed.nx = 1;
    run("nx_1", 2, axi, p);
  }
  {
    tpsrhs_physics p = good;
    p.lte2d.viscosity.ny = 1;
    run("ny_1", 2, axi, p);
  }
  {
    HostTable h = t[1];
    h.x[5] = h.x[4];
    tpsrhs_physics p = good;
    p.lte2d.gas_constant = h.view();
    run("x_repeats", 2, axi, p);
  }
  {
    HostTable h = t[3];
    std::swap(h.y[2], h.y[3]);
    tpsrhs_physics p = good;
    p.lte2d.temperature = h.view();
    run("y_decreases", 2, axi, p);
  }
  {
    HostTable h = t[5];
    h.f[h.f.size() - 1] = std::nan("");
    tpsrhs_physics p = good;
    p.lte2d.conductivity = h.view();
    run("nan_value", 2, axi, p);
  }
  {
    HostTable h = t[6];
    h.x[h.nx - 1] = std::numeric_limits<double>::infinity();
    tpsrhs_physics p = good;
    p.lte2d.electric_conductivity = h.view();
    run("inf_abscissa", 2, axi, p);
  }
  {
    tpsrhs_physics p = good;
    p.lte2d.energy.f = nullptr;
    run("null_values", 2, axi, p);
  }
  {
    tpsrhs_physics p = good;
    p.lte2d.temperature.y = nullptr;
    run("null_axis", 2, axi, p);
  }
  {
    HostTable h = t[0];  // e falls with T in one interval of the LAST density line only
    const size_t k = static_cast<size_t>(h.ny - 1) * h.nx + 40;
    h.f[k + 1] = h.f[k];
    tpsrhs_physics p = good;
    p.lte2d.energy = h.view();
    run("energy_not_increasing", 2, axi, p);
  }
  {
    HostTable h = t[2];  // c on another temperature grid than e and R
    h.x[7] += 1.0;
    tpsrhs_physics p = good;
    p.lte2d.sound_speed = h.view();
    run("thermo_grids_differ", 2, axi, p);
  }
  // ---- outside the built scope
  run("planar_2d", 2, disc(3, 0, 0, 0), good);
  run("3d", 3, disc(2, 0, 0, 0), good);
  run("gauss_lobatto", 2, disc(2, 1, 1, 1), good);
  {
    tpsrhs_physics p = good;
    p.sgs.model_type = TPSRHS_SGS_SMAGORINSKY;
    run("sgs", 2, axi, p);
  }
  {
    tpsrhs_disc d = axi;
    d.use_roe = 1;
    run("roe", 2, d, good);
  }
  {
    tpsrhs_bc b;
    std::memset(&b, 0, sizeof b);
    b.attribute = 2;
    b.category = TPSRHS_OUTLET;
    b.type = TPSRHS_SUB_P_NR;
    std::printf("non_reflecting: ");
    try {
      plan_operator(2, axi, good, 1, &b);
      std::printf("ok\n");
    } catch (const Unsupported &e) {
      std::printf("unsupported %s\n", e.what());
    } catch (const std::invalid_argument &e) {
      std::printf("invalid %s\n", e.what());
    }
  }

  // ---- the closure: T -> e(T, rho) -> T, one point in every cell of the thermodynamic grid (not at its centre)
  std::vector<std::vector<BilinearCell>> homes;  // (storage of the records' own alignment, for the axes as well)
  const Lte2dTables lt = make_lte2d_tables(good.lte2d, [&homes](const void *src, size_t bytes) {
    homes.emplace_back((bytes + sizeof(BilinearCell) - 1) / sizeof(BilinearCell));
    std::memcpy(static_cast<void *>(homes.back().data()), src, bytes);
    return static_cast<const void *>(homes.back().data());
  });
  std::printf("axes: T uniform %d rho uniform %d e uniform %d transport rho uniform %d\n", lt.g_th.inv_dx > 0.0, lt.g_th.inv_dy > 0.0,
              lt.g_rev.inv_dx > 0.0, lt.g_tr.inv_dy > 0.0);
  const HostTable &th = t[0];
  double worst = 0.0;
  int cells = 0, failed = 0;
  for (int j = 0; j + 1 < th.ny; j++)
    for (int i = 0; i + 1 < th.nx; i++) {
      const double T = th.x[i] + 0.37 * (th.x[i + 1] - th.x[i]), rho = th.y[j] + 0.61 * (th.y[j + 1] - th.y[j]);
      const double e = table2d_at(lt.g_th, lt.c_e, T, rho);
      ThermoCell tc;
      const double back = lte2d_temperature(lt, e, rho, cell_y(lt.g_th, rho), tc);
      if (!(back == back) || tc.k != j * (th.nx - 1) + i) failed++;
      worst = std::fmax(worst, std::fabs(back - T) / T);
      cells++;
    }
  std::printf("round_trip: cells %d failed %d worst_rel_err %.3e\n", cells, failed, worst);
  std::printf("LTE2D_PLAN DONE\n");
  return 0;
}
