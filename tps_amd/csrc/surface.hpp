// Integrals of a byNODES DG field over sets of element faces (tpsrhs_surface_integrate), and the patch history the device
// time loop keeps of them: the area the reference aggregates per inlet and outlet at start-up
// (BoundaryCondition::aggregateArea / aggregateBndryFaces, src/BoundaryCondition.cpp:59-92; OutletBC::computeParallelArea,
// src/outletBC.cpp:329-343), generalised to any array the caller hands over.  Included by surface.hip only: the kernel
// families do not see it.  The host half -- which faces make a patch -- is wall_faces.hpp::patch_faces.
//
// The rule and the summation structure are the contract of include/tpsrhs.h: the terms of one face are summed first; within
// a fixed run of the sorted faces of one patch, running sum k collects the face sums k, k + FB, ... in ascending order; and
// a last single-block kernel adds the running sums of a patch in a fixed order (stride 64, then a butterfly).  No floating-point atomics: two calls on the same input are bit-equal.
//
// Shape of the kernels, that of integrals.hpp.  A block is ONE wave.  The 64 lanes are cut into FB = 64 / LPF segments of
// LPF lanes (LPF: the power of two >= the NQ^(dim-1) points of a face); a segment owns one face of a batch of FB consecutive
// faces, a lane at most one point of it, and a block walks a fixed run of batches that lies inside ONE patch (the host
// lays the runs out: SurfaceRun).
//   k_surface<DIM, P>: per batch every lane forms the geometry of its point once, in registers (N_q w_q and |N_q| w_q, with
//   the radial factor); then, for each accumulator row and each component (FLUX: dim, else one), the nodal values of the
//   batch's elements are loaded into LDS (consecutive addresses per element: a value is read once, coalesced), reduced to the
//   trace along d with the vector l_a(s) (in LDS, both sides), interpolated along the tangential directions with the 1-D
//   matrix B (NQ x N1, in LDS), and every lane forms the term of its point; a butterfly over the segment's lanes gives the
//   face sums, which the segment's first lane adds to its running partial in LDS.  Rows beyond a pass are further launches.
//   k_surface_final: one block; a wave per output adds that patch's per-block partials in ascending order.
#ifndef TPSRHS_SURFACE_HPP_
#define TPSRHS_SURFACE_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/tpsrhs.h"
#include "device_buffer.hpp"
#include "quadrature_points.hpp"
#include "record_log.hpp"

struct tpsrhs_operator;

// one block's share of the sorted face list: faces [begin, end) of one patch
struct SurfaceRun {
  int32_t begin, end;
};

namespace tpsrhs {
// the rule and the 1-D tables of the operator's order and basis, passed to the kernel by value
struct SurfTab {
  double B[QUAD_MAXQ * (TPSRHS_MAXORDER + 1)];  // B[q * N1 + a] = l_a(g_q)
  double L[2 * (TPSRHS_MAXORDER + 1)];          // L[s * N1 + a] = l_a(s): the trace at xi_d = s
  double g[QUAD_MAXQ], w[QUAD_MAXQ];
};
}  // namespace tpsrhs

// behind tpsrhs_surface_handle; owned by its operator (tpsrhs_surface_state::surfaces)
struct tpsrhs_surface_s {
  tpsrhs_operator *owner = nullptr;
  int num_patches = 0;
  int64_t num_faces = 0;
  std::vector<int64_t> faces_per_patch;  // [num_patches]
  int fb = 1, nblocks = 0;               // segments of a block, blocks of the grid
  tpsrhs::SurfTab tab = {};              // filled once by tpsrhs_surface_create
  // device, SORTED by (patch, element, face)
  DevBuf<int32_t> d_elem, d_face;   // [num_faces]
  DevBuf<SurfaceRun> d_runs;        // [nblocks]
  DevBuf<int32_t> d_patch_block;    // [num_patches + 1] the first block of every patch
  DevBuf<double> d_partial;         // [SURF_ACC][nblocks * fb]
  DevBuf<double> d_flux;            // [dim][neq][NDofs]: the tensor of tpsrhs_surface_loads, allocated at its first call
};

// the patch history (tpsrhs_surface_monitor_configure); surface NULL: off
struct tpsrhs_surface_log {
  tpsrhs_surface_s *surface = nullptr;
  tpsrhs::StepCadence cadence;  // count: steps of tpsrhs_advance / tpsrhs_advance_with since the configure call
  tpsrhs::RecordIndex index;
  DevBuf<double> d_times;      // [capacity], copied from d_ctl[1] on the stream
  DevBuf<double> d_integrals;  // [capacity][num_patches][neq]
  DevBuf<double> d_mass_flow;  // [capacity][num_patches]
};

// behind tpsrhs_operator::surface; created by surface.hip at the first surface, owned by the operator
struct tpsrhs_surface_state {
  std::vector<std::unique_ptr<tpsrhs_surface_s>> surfaces;
  tpsrhs_surface_log history;
};

namespace tpsrhs {

constexpr int SURF_ACC = 16;          // accumulators per launch (rows, or rows x dim for NORMAL): their partials live in LDS
constexpr int SURF_MAXBLOCKS = 8192;  // 32 one-wave blocks on each of the 256 CUs (plus at most one short run per patch)

template <int DIM, int P>
struct SurfCfg {
  static constexpr int N1 = P + 1, NQ = P + 2;
  static constexpr int NPE = ipow(N1, DIM), NFN = ipow(N1, DIM - 1), NQF = ipow(NQ, DIM - 1);
  static constexpr int LPF = lanes_per_element(NQF), FB = 64 / LPF;
};

// x and the area-weighted outward normal N = (2s - 1) sgn(det J) cof(J) e_d at xi of one element; v: [2^DIM][DIM],
// lexicographic corners.  cof(J) e_d is the cross product of the other two columns of J in cyclic order (3-D) and the
// rotated other column (2-D); det J = (cof(J) e_d) . (J e_d).
template <int DIM>
__device__ inline void surface_geometry(const double *v, const double *xi, int d, int s, double *x, double *N) {
  double J[DIM * DIM];  // J[a * DIM + k] = dx_a / dxi_k
  if constexpr (DIM == 2) {
    const double a0 = 1.0 - xi[0], a1 = xi[0], b0 = 1.0 - xi[1], b1 = xi[1];
#pragma unroll
    for (int a = 0; a < 2; a++) {
      const double v00 = v[0 * 2 + a], v10 = v[1 * 2 + a], v01 = v[2 * 2 + a], v11 = v[3 * 2 + a];
      x[a] = (v00 * a0 + v10 * a1) * b0 + (v01 * a0 + v11 * a1) * b1;
      J[a * 2 + 0] = (v10 - v00) * b0 + (v11 - v01) * b1;
      J[a * 2 + 1] = (v01 - v00) * a0 + (v11 - v10) * a1;
    }
    double c[2], jd[2];
    if (d == 0) {
      c[0] = J[3], c[1] = -J[1];
      jd[0] = J[0], jd[1] = J[2];
    } else {
      c[0] = -J[2], c[1] = J[0];
      jd[0] = J[1], jd[1] = J[3];
    }
    const double det = c[0] * jd[0] + c[1] * jd[1];
    const double sg = ((s ? 1.0 : -1.0)) * (det < 0.0 ? -1.0 : 1.0);
    N[0] = sg * c[0];
    N[1] = sg * c[1];
  } else {
    const double a0 = 1.0 - xi[0], a1 = xi[0], b0 = 1.0 - xi[1], b1 = xi[1], c0 = 1.0 - xi[2], c1 = xi[2];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double v000 = v[0 * 3 + a], v100 = v[1 * 3 + a], v010 = v[2 * 3 + a], v110 = v[3 * 3 + a];
      const double v001 = v[4 * 3 + a], v101 = v[5 * 3 + a], v011 = v[6 * 3 + a], v111 = v[7 * 3 + a];
      const double e00 = v000 * a0 + v100 * a1, e10 = v010 * a0 + v110 * a1, e01 = v001 * a0 + v101 * a1,
                   e11 = v011 * a0 + v111 * a1;
      const double f0 = e00 * b0 + e10 * b1, f1 = e01 * b0 + e11 * b1;
      x[a] = f0 * c0 + f1 * c1;
      J[a * 3 + 0] = ((v100 - v000) * b0 + (v110 - v010) * b1) * c0 + ((v101 - v001) * b0 + (v111 - v011) * b1) * c1;
      J[a * 3 + 1] = (e10 - e00) * c0 + (e11 - e01) * c1;
      J[a * 3 + 2] = f1 - f0;
    }
    // columns d (jd), d + 1 (p) and d + 2 (q), cyclic
    double jd[3], p[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double j0 = J[a * 3 + 0], j1 = J[a * 3 + 1], j2 = J[a * 3 + 2];
      jd[a] = d == 0 ? j0 : (d == 1 ? j1 : j2);
      p[a] = d == 0 ? j1 : (d == 1 ? j2 : j0);
      q[a] = d == 0 ? j2 : (d == 1 ? j0 : j1);
    }
    const double c[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
    const double det = c[0] * jd[0] + c[1] * jd[1] + c[2] * jd[2];
    const double sg = ((s ? 1.0 : -1.0)) * (det < 0.0 ? -1.0 : 1.0);
    N[0] = sg * c[0];
    N[1] = sg * c[1];
    N[2] = sg * c[2];
  }
}

// partial: [nacc][gridDim.x * FB]; nacc = nrows (SCALAR, FLUX) or nrows * DIM (NORMAL), at most SURF_ACC
template <int DIM, int P>
__global__ void __launch_bounds__(64)
    k_surface(int form, int nrows, int64_t row_stride, int64_t comp_stride, int radial, SurfTab tab,
              const SurfaceRun *__restrict__ runs, const int32_t *__restrict__ elem, const int32_t *__restrict__ face,
              const double *__restrict__ verts, const double *__restrict__ field, double *__restrict__ partial) {
  typedef SurfCfg<DIM, P> C;
  constexpr int N1 = C::N1, NQ = C::NQ, NPE = C::NPE, NFN = C::NFN, NQF = C::NQF, LPF = C::LPF, FB = C::FB;
  constexpr int S1 = DIM == 3 ? NQ * N1 : 1;  // values of one face after the tangential direction a (3-D)
  __shared__ double sB[NQ * N1], sL[2 * N1], sg[NQ], sw[NQ];
  __shared__ double su[FB * NPE], st[FB * NFN], s1[FB * S1];
  __shared__ double sacc[SURF_ACC * FB];
  __shared__ int se[FB], sf[FB];
  const int lane = threadIdx.x, seg = lane / LPF, l = lane % LPF;
  const int ncomp = form == TPSRHS_SURFACE_FLUX ? DIM : 1, nout = form == TPSRHS_SURFACE_NORMAL ? DIM : 1;
  for (int i = lane; i < NQ * N1; i += 64) sB[i] = tab.B[i];
  if (lane < 2 * N1) sL[lane] = tab.L[lane];
  if (lane < NQ) {
    sg[lane] = tab.g[lane];
    sw[lane] = tab.w[lane];
  }
  if (l == 0)
    for (int j = 0; j < nrows * nout; j++) sacc[j * FB + seg] = 0.0;
  const SurfaceRun run = runs[blockIdx.x];
  for (int f0 = run.begin; f0 < run.end; f0 += FB) {
    const int nb = min(FB, run.end - f0);  // faces of this batch
    __syncthreads();                       // the tables are in place; the last batch has read se, sf, su, st, s1
    if (lane < nb) {
      se[lane] = elem[f0 + lane];
      sf[lane] = face[f0 + lane];
    }
    __syncthreads();
    // the geometry of this lane's point: Wn = w N (with the radial factor), Ws = |Wn|; lanes without a point keep zeros
    const bool has_point = seg < nb && l < NQF;
    double Wn[DIM] = {}, Ws = 0.0;
    const int fd = seg < nb ? sf[seg] >> 1 : 0, fs = seg < nb ? sf[seg] & 1 : 0;
    const int qa = l % NQ, qb = DIM == 3 ? (l / NQ) % NQ : 0;
    if (has_point) {
      // tangential directions a < b: the other reference directions in ascending order (selects: no register array is
      // indexed at run time)
      const double ta = sg[qa], tb = sg[qb], ts = fs;
      const double xi[3] = {fd == 0 ? ts : ta, fd == 1 ? ts : (fd == 0 ? ta : tb), fd == 2 ? ts : tb};
      double x[DIM], N[DIM];
      surface_geometry<DIM>(verts + static_cast<int64_t>(se[seg]) * (1 << DIM) * DIM, xi, fd, fs, x, N);
      double w = DIM == 3 ? sw[qa] * sw[qb] : sw[qa];
      if (radial) w *= x[0];
      double n2 = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; k++) {
        n2 += N[k] * N[k];
        Wn[k] = w * N[k];
      }
      Ws = w * sqrt(n2);
    }
    for (int r = 0; r < nrows; r++) {
      double term = 0.0;  // SCALAR, FLUX: the term of this lane's point
      double v = 0.0;
      for (int c = 0; c < ncomp; c++) {
        const double *u = field + r * row_stride + c * comp_stride;
        __syncthreads();  // the last interpolation has read su, st, s1
        for (int idx = lane; idx < nb * NPE; idx += 64) {
          const int el = idx / NPE, n = idx - el * NPE;
          su[idx] = u[static_cast<int64_t>(se[el]) * NPE + n];
        }
        __syncthreads();
        for (int idx = lane; idx < nb * NFN; idx += 64) {  // the trace: st[el][ja + N1 jb] = sum_i l_i(s) u[el][i along d]
          const int el = idx / NFN, m = idx - el * NFN;
          const int d = sf[el] >> 1, s = sf[el] & 1;
          const int ja = m % N1, jb = m / N1;
          int base, sd;
          if constexpr (DIM == 2) {
            sd = d == 0 ? 1 : N1;
            base = ja * (d == 0 ? N1 : 1);
          } else {
            sd = d == 0 ? 1 : (d == 1 ? N1 : N1 * N1);
            const int sa = d == 0 ? N1 : 1, sb = d == 2 ? N1 : N1 * N1;
            base = ja * sa + jb * sb;
          }
          double t = 0.0;
#pragma unroll
          for (int i = 0; i < N1; i++) t += sL[s * N1 + i] * su[el * NPE + base + i * sd];
          st[idx] = t;
        }
        __syncthreads();
        if constexpr (DIM == 3) {
          for (int idx = lane; idx < nb * S1; idx += 64) {  // direction a: s1[el][jb][qa] = sum_ja B[qa][ja] st[el][ja + N1 jb]
            const int q = idx % NQ, m = idx / NQ;           // m: face and line jb
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < N1; a++) t += sB[q * N1 + a] * st[m * N1 + a];
            s1[idx] = t;
          }
          __syncthreads();
        }
        v = 0.0;
        if (has_point) {
          if constexpr (DIM == 3) {
#pragma unroll
            for (int b = 0; b < N1; b++) v += sB[qb * N1 + b] * s1[(seg * N1 + b) * NQ + qa];
          } else {
#pragma unroll
            for (int a = 0; a < N1; a++) v += sB[qa * N1 + a] * st[seg * N1 + a];
          }
        }
        if (form == TPSRHS_SURFACE_FLUX) {
          // (a register array indexed by the loop counter of a runtime loop: select instead)
          const double wn = c == 0 ? Wn[0] : (c == 1 ? Wn[1] : Wn[DIM - 1]);
          term += wn * v;
        } else {
          term = Ws * v;
        }
      }
      if (form == TPSRHS_SURFACE_NORMAL) {
        double t[DIM];
#pragma unroll
        for (int k = 0; k < DIM; k++) t[k] = Wn[k] * v;
#pragma unroll
        for (int off = LPF / 2; off > 0; off >>= 1) {
#pragma unroll
          for (int k = 0; k < DIM; k++) t[k] += __shfl_xor(t[k], off, 64);
        }
        if (l == 0) {  // this lane alone touches its entries: no barrier
#pragma unroll
          for (int k = 0; k < DIM; k++) sacc[(r * DIM + k) * FB + seg] += t[k];
        }
      } else {
#pragma unroll
        for (int off = LPF / 2; off > 0; off >>= 1) term += __shfl_xor(term, off, 64);
        if (l == 0) sacc[r * FB + seg] += term;
      }
    }
  }
  if (l == 0) {
    const int64_t np = static_cast<int64_t>(gridDim.x) * FB, at = static_cast<int64_t>(blockIdx.x) * FB + seg;
    for (int j = 0; j < nrows * nout; j++) partial[j * np + at] = sacc[j * FB + seg];
  }
}

// One block: out[p * out_stride + j] = the sum of partial[j][patch_block[p] * fb .. patch_block[p + 1] * fb) for every patch p
// and accumulator j < nacc, in a fixed order -- a wave takes an output, lane t adds the entries t, t + 64, ... in ascending
// order and a butterfly adds the lanes.  An empty patch gives zero.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_surface_final(int num_patches, int nacc, int fb, int64_t np, const int32_t *__restrict__ patch_block,
                    const double *__restrict__ partial, int64_t out_stride, double *__restrict__ out) {
  constexpr int NW = BLOCK / 64;
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const int64_t nout = static_cast<int64_t>(num_patches) * nacc;
  for (int64_t o = wave; o < nout; o += NW) {
    const int p = static_cast<int>(o / nacc), j = static_cast<int>(o - static_cast<int64_t>(p) * nacc);
    const int64_t b = static_cast<int64_t>(patch_block[p]) * fb, e = static_cast<int64_t>(patch_block[p + 1]) * fb;
    const double *src = partial + j * np;
    double s = 0.0;
    for (int64_t i = b + lane; i < e; i += 64) s += src[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[p * out_stride + j] = s;
  }
}

}  // namespace tpsrhs
#endif
