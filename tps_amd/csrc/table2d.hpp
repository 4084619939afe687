// Two-dimensional tables on a tensor grid, bilinear: GslTableInterpolator2D with gsl_interp2d_bilinear
// (src/table.cpp:170-260), and the closures of LteMixture / LteTransport that look them up at (T, rho)
// (src/lte_mixture.cpp:119-470, src/lte_transport_properties.cpp:84-136; `flow/lte/table_dim = 2`).
//
// One text for the kernels of the two-dimensional table gas (physics_dryair_axisym.hpp, GAS = 2), for tpsrhs_table2d_eval
// and for the stand-alone program tests/lte2d_plan_main.cpp: everything here is TPSRHS_T2_HD -- __host__ __device__ under
// hipcc, nothing for a plain C++ compiler -- and reads its tables through plain pointers.
//
// The cell of an abscissa is GSL's (gsl_interp_bsearch): cell i holds x[i] <= x < x[i+1], the last abscissa belongs to the
// last cell.  ONE DEPARTURE from the reference: outside the table GSL raises a domain error, which aborts; here the cell
// index is clamped to the end cell, which extrapolates linearly from it -- what the reference's one-dimensional tables do
// (src/table.cpp:69-72).
#ifndef TPSRHS_TABLE2D_HPP_
#define TPSRHS_TABLE2D_HPP_

#include <cmath>
#include <stdexcept>
#include <vector>

#include "../../include/tpsrhs.h"

#if defined(__HIPCC__)
#define TPSRHS_T2_HD __host__ __device__
#else
#define TPSRHS_T2_HD
#endif

namespace tpsrhs {

// The axes of a table.  inv_dx / inv_dy > 0: that axis is uniformly spaced (checked on the host, axis_spacing) and the
// cell is a multiply and a floor; 0: bisection.
struct Grid2Dev {
  int nx, ny;
  const double *x, *y;
  double x0, inv_dx, y0, inv_dy;
};
// the cell of one abscissa on one axis and the offset x - x_i in it
struct AxisCell {
  int i;
  double d;
};
// One cell of a table, corner (i, j), at record j * (nx - 1) + i: the bilinear interpolant in the offsets from that corner,
//   z = z00 + zx dx + zy dy + zxy dx dy,  zx = (z10 - z00) / hx,  zy = (z01 - z00) / hy,  zxy = (z11 - z10 - z01 + z00) / (hx hy)
// -- the interpolant of tpsrhs_table2d in another order of operations (no weights, no division, one 32-byte record per
// look-up, and z_x = zx + zxy dy comes with the value).  Built once on the host (make_cells).
struct alignas(32) BilinearCell {
  double z, zx, zy, zxy;
};

// 1 / spacing of an axis whose abscissae lie within 1e-6 of a spacing of the uniform ones, else 0: the floor below is then
// off by one cell at the most, which the comparison with the two neighbouring abscissae corrects
inline double axis_spacing(int n, const double *x) {
  const double d = (x[n - 1] - x[0]) / (n - 1);
  for (int i = 0; i < n; i++)
    if (!(std::fabs(x[i] - (x[0] + i * d)) <= 1e-6 * d)) return 0.0;
  return 1.0 / d;
}

TPSRHS_T2_HD inline AxisCell axis_cell(const double *x, int n, double x0, double inv_d, double xe) {
  int i;
  if (inv_d > 0.0) {
    const double g = fmin(fmax(floor((xe - x0) * inv_d), 0.0), static_cast<double>(n - 2));  // (NaN -> 0)
    i = static_cast<int>(g);
    if (i > 0 && xe < x[i])
      i--;
    else if (i < n - 2 && xe >= x[i + 1])
      i++;
  } else {
    int hi = n - 1;
    i = 0;
    while (hi > i + 1) {
      const int mid = (i + hi) >> 1;
      if (x[mid] > xe)
        hi = mid;
      else
        i = mid;
    }
  }
  AxisCell c;
  c.i = i;
  c.d = xe - x[i];
  return c;
}
template <class G>
TPSRHS_T2_HD inline AxisCell cell_x(const G &g, double xe) { return axis_cell(g.x, g.nx, g.x0, g.inv_dx, xe); }
template <class G>
TPSRHS_T2_HD inline AxisCell cell_y(const G &g, double ye) { return axis_cell(g.y, g.ny, g.y0, g.inv_dy, ye); }

TPSRHS_T2_HD inline double cell_value(const BilinearCell &c, double dx, double dy) { return (c.z + c.zy * dy) + (c.zx + c.zxy * dy) * dx; }
TPSRHS_T2_HD inline double cell_dx(const BilinearCell &c, double dy) { return c.zx + c.zxy * dy; }
TPSRHS_T2_HD inline double cell_dy(const BilinearCell &c, double dx) { return c.zy + c.zxy * dx; }
// one table at one point: both searches, then the cell (what = 0 the value, 1 d/dx, 2 d/dy)
template <class G>
TPSRHS_T2_HD inline double table2d_at(const G &g, const BilinearCell *cells, double xe, double ye, int what = 0) {
  const AxisCell cx = cell_x(g, xe), cy = cell_y(g, ye);
  const BilinearCell c = cells[cy.i * (g.nx - 1) + cx.i];
  if (what == 1) return cell_dx(c, cy.d);
  if (what == 2) return cell_dy(c, cx.d);
  return cell_value(c, cx.d, cy.d);
}

// The tables of the gas.  e, R and c come from one file of the reference and share their grid, mu and kappa likewise
// (operator_plan.hpp refuses anything else): one pair of cells and offsets serves the tables of a grid.
struct Lte2dTables {
  Grid2Dev g_th;  // (T, rho) of e, R, c
  const BilinearCell *c_e, *c_R, *c_c;
  Grid2Dev g_rev;  // (e, rho) of the first guess T(e, rho), the reference's e_rev_table
  const BilinearCell *c_T;
  Grid2Dev g_tr;  // (T, rho) of mu, kappa
  const BilinearCell *c_mu, *c_k;
  Grid2Dev g_sig;  // (T, rho) of sigma
  const BilinearCell *c_sigma;
};

// where a state sits in the grid of the thermodynamic tables: the record of its cell and the two offsets in it
struct ThermoCell {
  int k;
  double dx, dy;
};

// LteMixture::ComputeTemperatureInternal, src/lte_mixture.cpp:161-223: the guess from T(e, rho), then Newton on e(T, rho) at
// the density of the state, whose cell `cy` in the thermodynamic grid the caller has found.  The reference asserts
// convergence; a state that does not converge returns NaN here and is caught like any other.
template <class LT>
TPSRHS_T2_HD inline double lte2d_temperature(const LT &p, double energy, double rho, const AxisCell &cy, ThermoCell &tc) {
  double T = table2d_at(p.g_rev, p.c_T, energy, rho);
  const int row = cy.i * (p.g_th.nx - 1);
  AxisCell cx = cell_x(p.g_th, T);
  BilinearCell c = p.c_e[row + cx.i];
  double dedT = cell_dx(c, cy.d);
  double res = energy - ((c.z + c.zy * cy.d) + dedT * cx.d);
  const double res0 = fabs(res);
  const double atol = 1e-18, rtol = 1e-12, dT_atol = 1e-12, dT_rtol = 1e-8;
  bool converged = (fabs(res) < atol) || (fabs(res) / fabs(res0) < rtol);
  int niter = 0;
  while (!converged && niter < 20) {
    const double dT = res / dedT;
    T += dT;
    cx = cell_x(p.g_th, T);
    c = p.c_e[row + cx.i];
    dedT = cell_dx(c, cy.d);
    res = energy - ((c.z + c.zy * cy.d) + dedT * cx.d);
    converged = (fabs(res) < atol) || (fabs(res) / res0 < rtol) || (fabs(dT) < dT_atol) || (fabs(dT) / T < dT_rtol);
    niter++;
  }
  tc.k = row + cx.i;
  tc.dx = cx.d;
  tc.dy = cy.d;
  return converged ? T : __builtin_nan("");
}
// LteMixture::ComputeTemperatureFromDensityPressure, src/lte_mixture.cpp:241-304: Newton on p = rho R(T, rho) T (the reference
// goes on with the last iterate when the iteration has not converged)
template <class LT>
TPSRHS_T2_HD inline double lte2d_temperature_rho_p(const LT &p, double rho, double pres, ThermoCell &tc) {
  const AxisCell cy = cell_y(p.g_th, rho);
  const int row = cy.i * (p.g_th.nx - 1);
  double T = pres / (rho * 208.);
  AxisCell cx = cell_x(p.g_th, T);
  BilinearCell c = p.c_R[row + cx.i];
  double R_T = cell_dx(c, cy.d);
  double R = (c.z + c.zy * cy.d) + R_T * cx.d;
  double res = pres - rho * R * T;
  const double res0 = fabs(res);
  const double atol = 1e-18, rtol = 1e-12, dT_atol = 1e-12, dT_rtol = 1e-8;
  bool converged = (fabs(res) < atol) || (fabs(res) / fabs(res0) < rtol);
  int niter = 0;
  while (!converged && niter < 20) {
    const double dpdT = rho * R + rho * R_T * T;
    const double dT = res / dpdT;
    T += dT;
    cx = cell_x(p.g_th, T);
    c = p.c_R[row + cx.i];
    R_T = cell_dx(c, cy.d);
    R = (c.z + c.zy * cy.d) + R_T * cx.d;
    res = pres - rho * R * T;
    converged = (fabs(res) < atol) || (fabs(res) / res0 < rtol) || (fabs(dT) < dT_atol) || (fabs(dT) / T < dT_rtol);
    niter++;
  }
  tc.k = row + cx.i;
  tc.dx = cx.d;
  tc.dy = cy.d;
  return T;
}

// The cell records of a table, row by row
inline std::vector<BilinearCell> make_cells(const tpsrhs_table2d &t) {
  std::vector<BilinearCell> cells(static_cast<size_t>(t.nx - 1) * (t.ny - 1));
  for (int j = 0; j + 1 < t.ny; j++)
    for (int i = 0; i + 1 < t.nx; i++) {
      const double hx = t.x[i + 1] - t.x[i], hy = t.y[j + 1] - t.y[j];
      const double z00 = t.f[j * t.nx + i], z10 = t.f[j * t.nx + i + 1], z01 = t.f[(j + 1) * t.nx + i], z11 = t.f[(j + 1) * t.nx + i + 1];
      BilinearCell &c = cells[static_cast<size_t>(j) * (t.nx - 1) + i];
      c.z = z00;
      c.zx = (z10 - z00) / hx;
      c.zy = (z01 - z00) / hy;
      c.zxy = ((z11 - z10) - (z01 - z00)) / (hx * hy);
    }
  return cells;
}
// The table records from the caller's tables.  place(src, bytes) returns where the kernels (or the host program) read a COPY
// of the bytes at src, which it owns (src is a temporary).  The plan (operator_plan.hpp::check_lte2d) has validated the
// tables and that the grids are shared.
template <class Place>
inline Grid2Dev make_grid2d(const tpsrhs_table2d &t, Place &&place) {
  Grid2Dev g;
  g.nx = t.nx;
  g.ny = t.ny;
  g.x0 = t.x[0];
  g.y0 = t.y[0];
  g.inv_dx = axis_spacing(t.nx, t.x);
  g.inv_dy = axis_spacing(t.ny, t.y);
  g.x = static_cast<const double *>(place(t.x, sizeof(double) * t.nx));
  g.y = static_cast<const double *>(place(t.y, sizeof(double) * t.ny));
  return g;
}
template <class Place>
inline const BilinearCell *place_cells(const tpsrhs_table2d &t, Place &&place) {
  const std::vector<BilinearCell> cells = make_cells(t);
  return static_cast<const BilinearCell *>(place(cells.data(), sizeof(BilinearCell) * cells.size()));
}
template <class Place>
inline Lte2dTables make_lte2d_tables(const tpsrhs_lte2d &in, Place &&place) {
  Lte2dTables lt;
  lt.g_th = make_grid2d(in.energy, place);
  lt.c_e = place_cells(in.energy, place);
  lt.c_R = place_cells(in.gas_constant, place);
  lt.c_c = place_cells(in.sound_speed, place);
  lt.g_rev = make_grid2d(in.temperature, place);
  lt.c_T = place_cells(in.temperature, place);
  lt.g_tr = make_grid2d(in.viscosity, place);
  lt.c_mu = place_cells(in.viscosity, place);
  lt.c_k = place_cells(in.conductivity, place);
  lt.g_sig = make_grid2d(in.electric_conductivity, place);
  lt.c_sigma = place_cells(in.electric_conductivity, place);
  return lt;
}

}  // namespace tpsrhs
#endif
