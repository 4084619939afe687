// The conservative positivity limiter (tpsrhs_limit, tpsrhs_limiter_configure; the contract is in include/tpsrhs.h): the
// Zhang-Shu linear scaling limiter, element by element, in place of the clamp of M2ulPhyS::Check_Undershoot
// (src/M2ulPhyS.cpp:2522-2548), which adds mass with every firing.  Plain C++17, no HIP, nothing but tpsrhs.h,
// division_mode.hpp and unsupported.hpp: the kernel of limiter.hip and the stand-alone program of tests/limiter_main.cpp use the same text.
//
// THE OPERATION.
//   Weights.  W_n = int_K l_n dV on the rule of tpsrhs_integrate (NQ = p + 2 Gauss-Legendre points per direction, order-1
//     geometry, the operator's Lagrange basis, |det J| at each point, times r_q when the operator is axisymmetric): sum_n
//     W_n f_n equals tpsrhs_integrate(f).sum up to rounding, for both basis / rule pairs.  On the Gauss-Lobatto pair they
//     are not the nodal quadrature weights.
//   Row step.  Element K with N nodes, a row v and a floor f: mean = sum W_n v_n / sum W_n; m = min_n v_n, kept with `<`,
//     so a NaN never wins.
//       1. mean is NaN: the element is left as it is and not counted (the NaN census of the loop reports it).
//       2. m >= f: untouched; nothing is written.
//       3. else mean > f: theta = (mean - f) / (mean - m); v_n <- mean + theta (v_n - mean); then v_n <- fmax(v_n, f),
//          which after the scaling can only move a value by rounding.  Counted in limited[row].
//       4. else the mean itself is inadmissible and no conservative fix exists: v_n <- fmax(v_n, f), the reference's
//          clamp, for this element only.  Counted in clamped[row].
//   Pressure step.  Dry air only, after the row steps, only when pressure_floor = f_p > 0.
//     p(U) = (gamma - 1)(U[nvel+1] - 1/2 sum_{d=1..nvel} U[d]^2 / U[0]); Ubar: the element means of all rows;
//     pbar = p(Ubar), p_min = min_n p(U_n).  p_min >= f_p: nothing.  Else pbar > f_p: theta = (pbar - f_p) / (pbar - p_min)
//     and every row of the element is scaled as v_n <- vbar + theta (v_n - vbar); counted in pressure_limited.  p is
//     concave in U for rho > 0, so p(U_n') >= (1 - theta) pbar + theta p(U_n) >= f_p up to rounding: no quadratic is
//     solved.  Else the element is left untouched and counted in pressure_unfixable.
//
// In the time loop one step is the stage sequence followed by the limiter.  The step size of the next step comes from the
// last stage's max_char_speed, as without a limiter: the limiter does not feed it.
//
// Two levels in here.  The decisions and the per-value updates (limiter_row_outcome, limiter_theta, limiter_row_value,
// limiter_pressure, ...) are what a lane of k_limit calls once the cross-lane reductions have given it the sums; the
// per-element functions over strided arrays (limit_row, limit_pressure) add the serial reductions around the same calls.
#ifndef TPSRHS_LIMITER_HPP_
#define TPSRHS_LIMITER_HPP_

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/tpsrhs.h"
#include "division_mode.hpp"
#include "unsupported.hpp"

#ifndef TPSRHS_HOST_DEVICE  // quadrature_points.hpp defines it too, the same way; a unit that needs both includes that one first
#if defined(__HIPCC__)
#define TPSRHS_HOST_DEVICE __host__ __device__
#else
#define TPSRHS_HOST_DEVICE
#endif
#endif

namespace tpsrhs {

enum LimiterOutcome { LIMITER_NAN = 0, LIMITER_UNTOUCHED = 1, LIMITER_SCALED = 2, LIMITER_CLAMPED = 3 };
enum LimiterPressureOutcome { LIMITER_P_UNTOUCHED = 0, LIMITER_P_SCALED = 1, LIMITER_P_UNFIXABLE = 2 };

// the counters of tpsrhs_limiter_report as one array of 64-bit integers
constexpr int LIMITER_CALLS = 0, LIMITER_LIMITED = 1, LIMITER_CLAMPED_AT = 1 + TPSRHS_MAXEQUATIONS,
              LIMITER_P_LIMITED = 1 + 2 * TPSRHS_MAXEQUATIONS, LIMITER_P_UNFIXABLE_AT = 2 + 2 * TPSRHS_MAXEQUATIONS,
              LIMITER_NCOUNTERS = 3 + 2 * TPSRHS_MAXEQUATIONS;

TPSRHS_HOST_DEVICE inline int limiter_row_outcome(double mean, double m, double f) {
  if (mean != mean) return LIMITER_NAN;
  if (m >= f) return LIMITER_UNTOUCHED;
  if (mean > f) return LIMITER_SCALED;
  return LIMITER_CLAMPED;
}
// (mean - f) / (mean - m) for mean > f > m: in (0, 1)
TPSRHS_HOST_DEVICE inline double limiter_theta(double mean, double m, double f) {
  TPSRHS_IEEE_DIVISION
  return (mean - f) / (mean - m);
}
TPSRHS_HOST_DEVICE inline double limiter_mean(double sum_wv, double sum_w) {
  TPSRHS_IEEE_DIVISION
  return sum_wv / sum_w;
}
TPSRHS_HOST_DEVICE inline double limiter_scale(double v, double mean, double theta) { return mean + theta * (v - mean); }
// the new value of one node for the outcomes that write (LIMITER_SCALED, LIMITER_CLAMPED)
TPSRHS_HOST_DEVICE inline double limiter_row_value(int outcome, double v, double mean, double theta, double f) {
  if (outcome == LIMITER_SCALED) v = limiter_scale(v, mean, theta);
  return fmax(v, f);
}

// p(U) of dry air; U: the rows 0 .. nvel + 1 of one node, `stride` apart
// (from scalars: a lane of k_limit holds the rows of a node in registers, which cannot be indexed; a momentum component
//  beyond nvel is passed as 0)
TPSRHS_HOST_DEVICE inline double limiter_pressure_of(double rho, double m1, double m2, double m3, double E, double gm1) {
  TPSRHS_IEEE_DIVISION
  double k = m1 * m1;
  k += m2 * m2;
  k += m3 * m3;
  return gm1 * (E - 0.5 * k / rho);
}
TPSRHS_HOST_DEVICE inline double limiter_pressure(const double *U, int64_t stride, int nvel, double gm1) {
  return limiter_pressure_of(U[0], U[stride], nvel >= 2 ? U[2 * stride] : 0.0, nvel >= 3 ? U[3 * stride] : 0.0,
                             U[(nvel + 1) * stride], gm1);
}
TPSRHS_HOST_DEVICE inline int limiter_pressure_outcome(double pbar, double pmin, double fp) {
  if (pmin >= fp) return LIMITER_P_UNTOUCHED;
  if (pbar > fp) return LIMITER_P_SCALED;
  return LIMITER_P_UNFIXABLE;
}

// The row step on one element: W and v are N values `ws` / `vs` apart.  -> LimiterOutcome.
TPSRHS_HOST_DEVICE inline int limit_row(int N, const double *W, int64_t ws, double *v, int64_t vs, double f) {
  double swv = 0.0, sw = 0.0, m = INFINITY;
  for (int n = 0; n < N; n++) {
    swv += W[n * ws] * v[n * vs];
    sw += W[n * ws];
    if (v[n * vs] < m) m = v[n * vs];
  }
  const double mean = limiter_mean(swv, sw);
  const int outcome = limiter_row_outcome(mean, m, f);
  if (outcome == LIMITER_SCALED || outcome == LIMITER_CLAMPED) {
    const double theta = outcome == LIMITER_SCALED ? limiter_theta(mean, m, f) : 0.0;
    for (int n = 0; n < N; n++) v[n * vs] = limiter_row_value(outcome, v[n * vs], mean, theta, f);
  }
  return outcome;
}

// The pressure step on one element: U[row * row_stride + n * node_stride], rows 0 .. neq - 1 (the first nvel + 2 enter p).
// -> LimiterPressureOutcome.
TPSRHS_HOST_DEVICE inline int limit_pressure(int N, const double *W, int64_t ws, double *U, int64_t node_stride, int64_t row_stride,
                                             int neq, int nvel, double gm1, double fp) {
  double ubar[TPSRHS_MAXEQUATIONS], sw = 0.0, pmin = INFINITY;
  for (int n = 0; n < N; n++) sw += W[n * ws];
  for (int r = 0; r < neq; r++) {
    double s = 0.0;
    for (int n = 0; n < N; n++) s += W[n * ws] * U[r * row_stride + n * node_stride];
    ubar[r] = limiter_mean(s, sw);
  }
  for (int n = 0; n < N; n++) {
    const double p = limiter_pressure(U + n * node_stride, row_stride, nvel, gm1);
    if (p < pmin) pmin = p;
  }
  const double pbar = limiter_pressure(ubar, 1, nvel, gm1);
  const int outcome = limiter_pressure_outcome(pbar, pmin, fp);
  if (outcome == LIMITER_P_SCALED) {
    const double theta = limiter_theta(pbar, pmin, fp);
    for (int r = 0; r < neq; r++)
      for (int n = 0; n < N; n++) {
        double &v = U[r * row_stride + n * node_stride];
        v = limiter_scale(v, ubar[r], theta);
      }
  }
  return outcome;
}

// What the plan needs to know of an operator.
struct LimiterFacts {
  int neq = 0, nvel = 0;
  int sp_first = 0, sp_last = 0;  // the species rows Check_Undershoot clamps (operator_plan.hpp); empty without a mixture
  bool dry_air = false;           // neither a mixture nor the table gas
  double gamma = 1.4;             // tpsrhs_dry_air::specific_heat_ratio
};

// A tpsrhs_limiter resolved against an operator; passed to k_limit by value.
struct LimiterPlan {
  int num_rows = 0;
  int rows[TPSRHS_MAXEQUATIONS] = {};
  double floors[TPSRHS_MAXEQUATIONS] = {};
  double pressure_floor = 0.0, gm1 = 0.0;
  int neq = 0, nvel = 0;
  bool covers_species = false;  // every row of a non-empty [sp_first, sp_last) is listed: the limiter replaces the clamp
};

// Resolves the rows and refuses what tpsrhs.h lists, before any device work: std::invalid_argument ->
// TPSRHS_ERR_INVALID_ARGUMENT, Unsupported -> TPSRHS_ERR_UNSUPPORTED.  in_loop: the limiter of the time loop, which must list
// all species rows or none (the clamp range of the stage kernels stays contiguous).
inline LimiterPlan plan_limiter(const tpsrhs_limiter &lim, const LimiterFacts &op, bool in_loop, const std::string &who) {
  LimiterPlan pl;
  pl.neq = op.neq;
  pl.nvel = op.nvel;
  if (lim.num_rows < -1 || lim.num_rows > op.neq || lim.num_rows > TPSRHS_MAXEQUATIONS)
    throw std::invalid_argument(who + ": num_rows must be -1 (the species rows) or in 0 .. num_equation = " + std::to_string(op.neq));
  if (lim.num_rows == -1) {
    for (int r = op.sp_first; r < op.sp_last; r++) {
      pl.rows[pl.num_rows] = r;
      pl.floors[pl.num_rows++] = 0.0;
    }
  } else {
    bool seen[TPSRHS_MAXEQUATIONS] = {};
    for (int i = 0; i < lim.num_rows; i++) {
      const int r = lim.rows[i];
      if (r < 0 || r >= op.neq)
        throw std::invalid_argument(who + ": row " + std::to_string(r) + " is outside [0, num_equation = " + std::to_string(op.neq) + ")");
      if (seen[r]) throw std::invalid_argument(who + ": row " + std::to_string(r) + " is listed twice");
      seen[r] = true;
      if (lim.floors[i] != lim.floors[i]) throw std::invalid_argument(who + ": the floor of row " + std::to_string(r) + " is NaN");
      pl.rows[pl.num_rows] = r;
      pl.floors[pl.num_rows++] = lim.floors[i];
    }
  }
  if (!(lim.pressure_floor >= 0.0)) throw std::invalid_argument(who + ": pressure_floor must be >= 0 (0: off)");
  if (lim.pressure_floor > 0.0) {
    if (!op.dry_air)
      throw Unsupported(who + ": pressure_floor > 0 is built for dry air (the energy of a mixture or of the table gas is not "
                              "one concave function of the state rows)");
    bool rho = false;
    for (int i = 0; i < pl.num_rows; i++) rho = rho || (pl.rows[i] == 0 && pl.floors[i] > 0.0);
    if (!rho) throw std::invalid_argument(who + ": pressure_floor > 0 needs row 0 (the density) listed with a floor > 0");
    pl.pressure_floor = lim.pressure_floor;
    pl.gm1 = op.gamma - 1.0;
  }
  int listed = 0;
  for (int i = 0; i < pl.num_rows; i++) listed += (pl.rows[i] >= op.sp_first && pl.rows[i] < op.sp_last) ? 1 : 0;
  const int nsp = op.sp_last - op.sp_first;
  if (in_loop && listed != 0 && listed != nsp)
    throw std::invalid_argument(who + ": lists " + std::to_string(listed) + " of the " + std::to_string(nsp) +
                                " species rows [" + std::to_string(op.sp_first) + ", " + std::to_string(op.sp_last) +
                                "); the limiter of the time loop replaces their clamp for all of them or for none");
  pl.covers_species = nsp > 0 && listed == nsp;
  return pl;
}

}  // namespace tpsrhs
#endif
