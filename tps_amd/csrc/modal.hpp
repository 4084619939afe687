// The Legendre modal filter and the modal-decay smoothness sensor (tpsrhs_modal_transform, tpsrhs_modal_energy,
// tpsrhs_modal_filter_apply, tpsrhs_modal_filter_configure; the contract is in include/tpsrhs.h): the exponential filter of
// Hesthaven & Warburton and the sensor of Persson & Peraire, element by element.  Plain C++17, no HIP, nothing but tpsrhs.h
// and division_mode.hpp: the kernels of modal.hip and the stand-alone program of tests/modal_main.cpp use the same text.
//
// THE OPERATION, per element with N1 = p + 1 nodes xi_a in [0, 1] per direction (the operator's own: Gauss-Legendre or
// Gauss-Lobatto), lexicographic node order:
//   Modes.   V[a][k] = P_k(2 xi_a - 1);  u^ = (V^-1 x ... x V^-1) u.
//   Filter.  sigma_k = 1 (k <= k_c), exp(-alpha ((k - k_c) / (p - k_c))^s) (k > k_c);  F = V diag(sigma) V^-1;
//            u~ = (F x ... x F) u;  conservative: u~_n += sum W (u - u~) / sum W with the weights of tpsrhs_limiter_weights.
//   Shells.  gamma_k = 1 / (2k + 1);  E_m = sum_{max(i, j[, k]) = m} u^^2 gamma_i gamma_j [gamma_k];  S = E_p / sum_m E_m,
//            0 when the sum is 0, NaN when the element holds a NaN.
//   Selective filtering.  sensor_row >= 0: S of that row of the incoming state decides for all listed rows, S > threshold;
//            an element that is not filtered is not written.
//
// The matrices are formed here, on the host: the nodes handed in (doubles) are polished by Newton in long double, V is
// inverted by Gauss-Jordan with partial pivoting in long double (cond(V) < 4 for p <= 5 on both node sets), F is the long
// double product, and every entry is rounded to double once.  An entry therefore carries half an ulp, which is small
// against the (p + 1) ulps of the dot product it enters.
//
// Two levels in here, as in limiter.hpp.  The small decisions (modal_sensor, modal_filtered, modal_mode_weight,
// modal_correction) are what a lane of the kernels calls once the block has reduced the sums; the per-element functions
// (modal_apply_element, modal_energy_element, modal_filter_element) add plain serial loops around the same calls.
#ifndef TPSRHS_MODAL_HPP_
#define TPSRHS_MODAL_HPP_

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/tpsrhs.h"
#include "division_mode.hpp"

#ifndef TPSRHS_HOST_DEVICE  // quadrature_points.hpp and limiter.hpp define it too, the same way
#if defined(__HIPCC__)
#define TPSRHS_HOST_DEVICE __host__ __device__
#else
#define TPSRHS_HOST_DEVICE
#endif
#endif

namespace tpsrhs {

constexpr int MODAL_MAXN1 = TPSRHS_MAXORDER + 1;
constexpr int MODAL_MAXNPE = MODAL_MAXN1 * MODAL_MAXN1 * MODAL_MAXN1;

// the counters of tpsrhs_modal_filter_report as one array of 64-bit integers
constexpr int MODAL_CALLS = 0, MODAL_SEEN = 1, MODAL_FILTERED = 2, MODAL_NCOUNTERS = 3;

// One N1 x N1 matrix applied along every direction, m[a * N1 + i] (out_a = sum_i m[a][i] in_i); passed to the kernels by value.
struct ModalMatrix {
  double m[MODAL_MAXN1 * MODAL_MAXN1];
};
// What the host forms per operator.
struct ModalBasis {
  int n1 = 0;
  ModalMatrix V = {}, Vinv = {};
  double gamma[MODAL_MAXN1] = {};  // 1 / (2k + 1)
};

// ---- the 1-D matrices, on the host ------------------------------------------------------------------------------------
// P_k(z) and P_k'(z) by the three-term recurrence
inline long double modal_legendre(int k, long double z, long double *derivative = nullptr) {
  long double p1 = 1.0L, p2 = 0.0L;  // P_j, P_{j-1}
  for (int j = 1; j <= k; j++) {
    const long double p3 = p2;
    p2 = p1;
    p1 = ((2.0L * j - 1.0L) * z * p2 - (j - 1.0L) * p3) / j;
  }
  if (derivative) *derivative = k == 0 ? 0.0L : k * (z * p1 - p2) / (z * z - 1.0L);  // not at z = +-1
  return p1;
}

// the nodes on [-1, 1] in long double: the doubles of segment_rule01 (on [0, 1]) polished by Newton on P_n (Gauss-Legendre)
// or on P'_{n-1} (the interior Gauss-Lobatto nodes; the end points are exact)
inline void modal_polish_nodes(int lobatto, int n1, const double *nodes01, long double *z) {
  for (int a = 0; a < n1; a++) {
    z[a] = 2.0L * nodes01[a] - 1.0L;
    if (lobatto && (a == 0 || a == n1 - 1)) continue;
    for (int it = 0; it < 4; it++) {
      long double dp;
      if (!lobatto) {
        const long double pn = modal_legendre(n1, z[a], &dp);
        z[a] -= pn / dp;
      } else {
        const int m = n1 - 1;
        const long double pm = modal_legendre(m, z[a], &dp);
        const long double d2p = (2.0L * z[a] * dp - m * (m + 1.0L) * pm) / (1.0L - z[a] * z[a]);
        z[a] -= dp / d2p;
      }
    }
  }
}

// Gauss-Jordan with partial pivoting; false: singular
inline bool modal_invert(int n, const long double *A, long double *inv) {
  long double w[MODAL_MAXN1][2 * MODAL_MAXN1];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      w[i][j] = A[i * n + j];
      w[i][n + j] = i == j ? 1.0L : 0.0L;
    }
  for (int c = 0; c < n; c++) {
    int piv = c;
    for (int r = c + 1; r < n; r++)
      if (std::fabs(w[r][c]) > std::fabs(w[piv][c])) piv = r;
    if (w[piv][c] == 0.0L) return false;
    for (int j = 0; j < 2 * n; j++) {
      const long double t = w[c][j];
      w[c][j] = w[piv][j];
      w[piv][j] = t;
    }
    const long double d = w[c][c];
    for (int j = 0; j < 2 * n; j++) w[c][j] /= d;
    for (int r = 0; r < n; r++) {
      if (r == c) continue;
      const long double f = w[r][c];
      for (int j = 0; j < 2 * n; j++) w[r][j] -= f * w[c][j];
    }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) inv[i * n + j] = w[i][n + j];
  return true;
}

// V and V^-1 in long double for the nodes of the operator (nodes01: segment_rule01(lobatto, n1, ...))
inline void modal_vandermonde(int lobatto, int n1, const double *nodes01, long double *V, long double *Vinv) {
  long double z[MODAL_MAXN1];
  modal_polish_nodes(lobatto, n1, nodes01, z);
  for (int a = 0; a < n1; a++)
    for (int k = 0; k < n1; k++) V[a * n1 + k] = modal_legendre(k, z[a]);
  if (!modal_invert(n1, V, Vinv)) throw std::runtime_error("modal_vandermonde: singular Vandermonde matrix");
}

// sigma_k, k = 0 .. p
inline void modal_sigma(int p, int cutoff, double alpha, int exponent, long double *sigma) {
  for (int k = 0; k <= p; k++) {
    if (k <= cutoff) {
      sigma[k] = 1.0L;
      continue;
    }
    const long double eta = static_cast<long double>(k - cutoff) / static_cast<long double>(p - cutoff);
    long double e = 1.0L;
    for (int i = 0; i < exponent && e != 0.0L; i++) e *= eta;  // eta <= 1: an exponent of any size ends at 0 or stays at 1
    sigma[k] = std::exp(-static_cast<long double>(alpha) * e);
  }
}

inline ModalBasis modal_basis(int lobatto, int n1, const double *nodes01) {
  ModalBasis b;
  long double V[MODAL_MAXN1 * MODAL_MAXN1], Vi[MODAL_MAXN1 * MODAL_MAXN1];
  modal_vandermonde(lobatto, n1, nodes01, V, Vi);
  b.n1 = n1;
  for (int i = 0; i < n1 * n1; i++) {
    b.V.m[i] = static_cast<double>(V[i]);
    b.Vinv.m[i] = static_cast<double>(Vi[i]);
  }
  for (int k = 0; k < n1; k++) b.gamma[k] = 1.0 / (2.0 * k + 1.0);
  return b;
}

// F = V diag(sigma) V^-1
inline ModalMatrix modal_filter_matrix(int lobatto, int n1, const double *nodes01, int cutoff, double alpha, int exponent) {
  long double V[MODAL_MAXN1 * MODAL_MAXN1], Vi[MODAL_MAXN1 * MODAL_MAXN1], sigma[MODAL_MAXN1];
  modal_vandermonde(lobatto, n1, nodes01, V, Vi);
  modal_sigma(n1 - 1, cutoff, alpha, exponent, sigma);
  ModalMatrix F = {};
  for (int a = 0; a < n1; a++)
    for (int b = 0; b < n1; b++) {
      long double s = 0.0L;
      for (int k = 0; k < n1; k++) s += V[a * n1 + k] * sigma[k] * Vi[k * n1 + b];
      F.m[a * n1 + b] = static_cast<double>(s);
    }
  return F;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------
// A tpsrhs_modal_filter resolved against an operator; passed to k_modal_filter by value.
struct ModalPlan {
  int num_rows = 0;
  int rows[TPSRHS_MAXEQUATIONS] = {};
  int cutoff = 0, exponent = 1;
  double alpha = 0.0;
  int conservative = 0;
  int sensor_row = -1;
  double sensor_threshold = 0.0;
};

// Resolves the rows and refuses what tpsrhs.h lists, before any device work: std::invalid_argument ->
// TPSRHS_ERR_INVALID_ARGUMENT.  neq, order: the operator's.
inline ModalPlan plan_modal_filter(const tpsrhs_modal_filter &f, int neq, int order, const std::string &who) {
  ModalPlan pl;
  if (f.num_rows < -1 || f.num_rows > neq || f.num_rows > TPSRHS_MAXEQUATIONS)
    throw std::invalid_argument(who + ": num_rows must be -1 (every state row) or in 0 .. num_equation = " + std::to_string(neq));
  if (f.num_rows == -1) {
    for (int r = 0; r < neq; r++) pl.rows[pl.num_rows++] = r;
  } else {
    bool seen[TPSRHS_MAXEQUATIONS] = {};
    for (int i = 0; i < f.num_rows; i++) {
      const int r = f.rows[i];
      if (r < 0 || r >= neq)
        throw std::invalid_argument(who + ": row " + std::to_string(r) + " is outside [0, num_equation = " + std::to_string(neq) + ")");
      if (seen[r]) throw std::invalid_argument(who + ": row " + std::to_string(r) + " is listed twice");
      seen[r] = true;
      pl.rows[pl.num_rows++] = r;
    }
  }
  if (f.cutoff < 0 || f.cutoff > order - 1)
    throw std::invalid_argument(who + ": cutoff " + std::to_string(f.cutoff) + " is outside 0 .. p - 1 = " + std::to_string(order - 1));
  if (!(f.alpha > 0.0) || std::isinf(f.alpha)) throw std::invalid_argument(who + ": alpha must be > 0 and finite");
  if (f.exponent < 1) throw std::invalid_argument(who + ": exponent " + std::to_string(f.exponent) + " < 1");
  if (f.sensor_row < -1 || f.sensor_row >= neq)
    throw std::invalid_argument(who + ": sensor_row " + std::to_string(f.sensor_row) + " is outside [-1, num_equation = " +
                                std::to_string(neq) + ")");
  if (f.sensor_threshold != f.sensor_threshold) throw std::invalid_argument(who + ": sensor_threshold is NaN");
  pl.cutoff = f.cutoff;
  pl.exponent = f.exponent;
  pl.alpha = f.alpha;
  pl.conservative = f.conservative != 0 ? 1 : 0;
  pl.sensor_row = f.sensor_row;
  pl.sensor_threshold = f.sensor_threshold;
  return pl;
}

// ---- the decisions and per-value updates ----------------------------------------------------------------------------------
// gamma_i gamma_j [gamma_k]: the weight of one mode in the reference-space L2 norm
TPSRHS_HOST_DEVICE inline double modal_mode_weight(double gi, double gj, double gk) { return (gi * gj) * gk; }
TPSRHS_HOST_DEVICE inline double modal_mode_energy(double uhat, double weight) { return (uhat * uhat) * weight; }
// S = E_p / sum E: 0 for a zero element, NaN for one that holds a NaN (every mode of it is NaN then)
TPSRHS_HOST_DEVICE inline double modal_sensor(double ep, double esum) {
  TPSRHS_IEEE_DIVISION
  if (esum == 0.0) return 0.0;
  return ep / esum;
}
// a NaN sensor and a threshold of +inf: not filtered
TPSRHS_HOST_DEVICE inline bool modal_filtered(double sensor, double threshold) { return sensor > threshold; }
// what the conservative filter adds to every node of an element: sum W (u - u~) / sum W
TPSRHS_HOST_DEVICE inline double modal_correction(double sum_w_diff, double sum_w) {
  TPSRHS_IEEE_DIVISION
  return sum_w_diff / sum_w;
}

// ---- one element, serially ------------------------------------------------------------------------------------------------
// out = (M x ... x M) in on one element: n1^dim values `is` / `os` apart; in == out is allowed
inline void modal_apply_element(int dim, int n1, const double *M, const double *in, int64_t is, double *out, int64_t os) {
  double a[MODAL_MAXNPE], b[MODAL_MAXNPE];
  const int npe = dim == 3 ? n1 * n1 * n1 : n1 * n1;
  for (int n = 0; n < npe; n++) a[n] = in[n * is];
  int stride = 1;
  for (int d = 0; d < dim; d++) {  // direction d: the index with this stride is contracted
    for (int n = 0; n < npe; n++) {
      const int c = (n / stride) % n1, base = n - c * stride;
      double s = 0.0;
      for (int i = 0; i < n1; i++) s += M[c * n1 + i] * a[base + i * stride];
      b[n] = s;
    }
    for (int n = 0; n < npe; n++) a[n] = b[n];
    stride *= n1;
  }
  for (int n = 0; n < npe; n++) out[n * os] = a[n];
}

// the shell energies E[0 .. p] of one element of a scalar field; -> the sensor
inline double modal_energy_element(int dim, const ModalBasis &b, const double *u, int64_t us, double *E) {
  const int n1 = b.n1, npe = dim == 3 ? n1 * n1 * n1 : n1 * n1;
  double uh[MODAL_MAXNPE];
  modal_apply_element(dim, n1, b.Vinv.m, u, us, uh, 1);
  for (int m = 0; m < n1; m++) E[m] = 0.0;
  for (int n = 0; n < npe; n++) {
    const int i = n % n1, j = (n / n1) % n1, k = dim == 3 ? n / (n1 * n1) : 0;
    int m = i > j ? i : j;
    if (k > m) m = k;
    E[m] += modal_mode_energy(uh[n], modal_mode_weight(b.gamma[i], b.gamma[j], dim == 3 ? b.gamma[k] : 1.0));
  }
  double sum = 0.0;
  for (int m = 0; m < n1; m++) sum += E[m];
  return modal_sensor(E[n1 - 1], sum);
}

// The filter on one element: x[row * row_stride + n * node_stride], W[n * ws].  -> whether the element was filtered; one that
// is not is not written.  sensor_out (or NULL): S, NaN-free only where a sensor row is set.
inline bool modal_filter_element(int dim, const ModalBasis &b, const ModalMatrix &F, const ModalPlan &pl, const double *W, int64_t ws,
                                 double *x, int64_t node_stride, int64_t row_stride, double *sensor_out = nullptr) {
  const int n1 = b.n1, npe = dim == 3 ? n1 * n1 * n1 : n1 * n1;
  if (pl.sensor_row >= 0) {
    double E[MODAL_MAXN1];
    const double S = modal_energy_element(dim, b, x + pl.sensor_row * row_stride, node_stride, E);
    if (sensor_out) *sensor_out = S;
    if (!modal_filtered(S, pl.sensor_threshold)) return false;
  }
  double sw = 0.0;
  for (int n = 0; n < npe; n++) sw += W[n * ws];
  for (int i = 0; i < pl.num_rows; i++) {
    double *v = x + pl.rows[i] * row_stride;
    double t[MODAL_MAXNPE];
    modal_apply_element(dim, n1, F.m, v, node_stride, t, 1);
    double c = 0.0;
    if (pl.conservative) {
      double s = 0.0;
      for (int n = 0; n < npe; n++) s += W[n * ws] * (v[n * node_stride] - t[n]);
      c = modal_correction(s, sw);
    }
    for (int n = 0; n < npe; n++) v[n * node_stride] = pl.conservative ? t[n] + c : t[n];
  }
  return true;
}

}  // namespace tpsrhs
#endif
