// The eight Coulomb collision fits of the third-order electron conductivity as ONE table of piecewise polynomials.
//
// Every fit is c0 log(1 + c1 Tp^c2)^c3 / Tp^2 (src/collision_integrals.cpp:53-115) with literal constants: a fixed function
// of x = ln Tp.  g_f(x) = c0 [log(1 + c1 e^(c2 x))]^c3 is smooth and slowly varying, so on intervals of width H a polynomial
// of degree DEG through the Chebyshev nodes reproduces it below rounding (worst relative truncation error 4.2e-17 for
// H = 0.25, DEG = 9 over x in [-8, 40]; tests/test_coulomb_table.py measures the whole evaluation against 40-digit
// arithmetic).  One Horner chain per fit replaces exp -> log -> log -> exp.  The factor 1 / Tp^2 stays with the caller.
//
// Plain C++17: no HIP type in here.  The host fills the table (fill), host and device evaluate it with the same routine
// (horner), FMA by FMA in the same order, so the two agree bit for bit.
//
// Layout: coef[interval][power][fit], interval i = [X0 + i H, X0 + (i + 1) H), power k = coefficient of t^k in the local
// variable t = (x - centre_i) * 2 / H in [-1, 1): one Horner step reads the NFIT contiguous doubles of its power.
#ifndef TPSRHS_COULOMB_TABLE_HPP_
#define TPSRHS_COULOMB_TABLE_HPP_

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define TPSRHS_CT_HD __host__ __device__
#else
#define TPSRHS_CT_HD
#endif

namespace tpsrhs {
namespace coulomb {

constexpr double X0 = -4.0;  // x = ln Tp: 1.1 .. 8.5 in a 3 000 - 12 000 K argon plasma at 1 atm, ~36 without electrons
constexpr double H = 0.25;
constexpr int NI = 176;  // [-4, 40)
constexpr int DEG = 9;
constexpr int NFIT = 8;
constexpr int STRIDE = (DEG + 1) * NFIT;  // doubles per interval
constexpr int SIZE = NI * STRIDE;         // 14 080 doubles, 110 KB
constexpr double XEND = X0 + NI * H;

// on the table?  (false for a NaN)
TPSRHS_CT_HD inline bool in_range(double x) { return X0 <= x && x < XEND; }
// interval of an x that is on the table.  x - X0 may round up across an interval's lower edge: the polynomial of the
// next interval then is evaluated a rounding error outside its interval, where it is as good as inside.
TPSRHS_CT_HD inline int interval(double x) {
  const int i = static_cast<int>((x - X0) * (1.0 / H));
  return i < NI - 1 ? i : NI - 1;
}
// the local variable of interval i (the centres are multiples of H / 2: exact, and so is the difference for |x| >= H / 2)
TPSRHS_CT_HD inline double local(double x, int i) { return (x - (X0 + 0.5 * H + H * i)) * (2.0 / H); }

// the first NF fits at local variable t from the coefficients c of one interval (a pointer into any address space)
template <int NF, class P>
TPSRHS_CT_HD inline void horner(P c, double t, double (&g)[NF]) {
  static_assert(NF >= 1 && NF <= NFIT, "fits of the table");
#pragma unroll
  for (int f = 0; f < NF; f++) g[f] = c[DEG * NFIT + f];
#pragma unroll
  for (int k = DEG - 1; k >= 0; k--)
#pragma unroll
    for (int f = 0; f < NF; f++) g[f] = __builtin_fma(g[f], t, c[k * NFIT + f]);
}
// host and probe: the first NF fits at x (which must be on the table)
template <int NF>
TPSRHS_CT_HD inline void eval(const double *table, double x, double (&g)[NF]) {
  const int i = interval(x);
  horner<NF>(table + i * STRIDE, local(x, i), g);
}

// table[SIZE] from the constants (c0, c1, c2, c3) of the NFIT fits: g sampled at the DEG + 1 Chebyshev nodes of every
// interval in long double, the interpolating polynomial converted from the Chebyshev to the monomial basis in t (degree
// 9 on [-1, 1]: the conversion amplifies by < 2^9, far below the 11 extra bits of long double), rounded once to double
inline void fill(const double (*c)[4], double *table) {
#if !defined(__HIP_DEVICE_COMPILE__)  // (host only: the device pass of a HIP unit parses this with its own long double)
  static_assert(LDBL_MANT_DIG >= 64, "the table is sampled in extended precision");
#endif
  constexpr int N = DEG + 1;
  const long double pi = 3.14159265358979323846264338327950288L;
  long double node[N], T[N][N];  // T[j][k] = T_j(node_k); mono[j][m] = coefficient of t^m in T_j
  long double mono[N][N] = {};
  for (int k = 0; k < N; k++) node[k] = std::cos(pi * (2 * k + 1) / (2 * N));
  for (int k = 0; k < N; k++) {
    T[0][k] = 1.0L;
    T[1][k] = node[k];
    for (int j = 2; j < N; j++) T[j][k] = 2.0L * node[k] * T[j - 1][k] - T[j - 2][k];
  }
  mono[0][0] = 1.0L;
  mono[1][1] = 1.0L;
  for (int j = 2; j < N; j++)
    for (int m = 0; m < N; m++) mono[j][m] = (m > 0 ? 2.0L * mono[j - 1][m - 1] : 0.0L) - mono[j - 2][m];
  for (int i = 0; i < NI; i++) {
    const long double centre = static_cast<long double>(X0) + H * (i + 0.5L);
    for (int f = 0; f < NFIT; f++) {
      const long double c0 = c[f][0], c1 = c[f][1], c2 = c[f][2], c3 = c[f][3];
      long double y[N], a[N], m[N] = {};
      for (int k = 0; k < N; k++) {
        const long double x = centre + 0.5L * H * node[k];
        y[k] = c0 * std::pow(std::log1p(c1 * std::exp(c2 * x)), c3);
      }
      for (int j = 0; j < N; j++) {
        long double s = 0.0L;
        for (int k = 0; k < N; k++) s += y[k] * T[j][k];
        a[j] = s * (j == 0 ? 1.0L : 2.0L) / N;
      }
      for (int j = 0; j < N; j++)
        for (int k = 0; k < N; k++) m[k] += a[j] * mono[j][k];
      for (int k = 0; k < N; k++) table[(i * N + k) * NFIT + f] = static_cast<double>(m[k]);
    }
  }
}

}  // namespace coulomb
}  // namespace tpsrhs
#endif
