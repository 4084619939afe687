// The nodal flux tensor of RHSoperator::GetFlux (src/rhs_operator.cpp:493-559) as an array of its own: tpsrhs_get_flux.
//
// k_flux (kernels.hpp, "nodal flux F_c - F_v") forms the tensor in registers and contracts it with the metric at once; this
// pass evaluates the same closures with the same context per node and WRITES the tensor -- the convective part, the viscous
// part, or their difference -- as out[d][eq][node], the layout of gradUp.  One lane per node, byNODES loads and stores like
// k_vis_fields; the position of a node (radius, viscous sponge, LES flavour) comes from the vertices of its element.
//
// The per-node body, flux_parts, is plain templated C++ over a physics PH: it compiles for the host through the stand-in
// of tests/host_physics (tests/flux_fields_main.cpp runs it under the sanitizers).  The kernel and its launcher follow
// under __HIPCC__.
//
// Rules (include/tpsrhs.h): F_v comes from the closure's own terms, F_c - F_v is ONE subtraction per entry, and the Coulomb
// fits of the argon-minimal transport come from their formulas (flux_coeffs<false>), never from the polynomial table of the
// 3-D p = 3 sweeps: no LDS window here.
#ifndef TPSRHS_FLUX_FIELDS_HPP_
#define TPSRHS_FLUX_FIELDS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "physics_dryair.hpp"

namespace tpsrhs {

enum { FLUX_TOTAL = 0, FLUX_CONVECTIVE = 1, FLUX_VISCOUS = 2 };

// what the closures take of a node besides its state and gradient
struct FluxPoint {
  double radius;  // axisymmetric / table gas: r of the node; 1 otherwise
  PointCtx pc;    // LES flavour: elSize and xyz (src/rhs_operator.cpp:526-539)
  EddyCtx ec;     // 2-D kernels with the heavy interface: mixing length and viscous sponge (kernels.hpp::closure_ctx)
};

// Fluxes::ComputeConvectiveFluxes (src/fluxes.cpp:135-170) as every total_flux of the device physics writes it; F[eq + d*NEQ].
// Terms per entry (K of tests/flux_fields_main.cpp): density 1 (a copy), momentum 2 (product, + p on the diagonal),
// energies 2 (sum, product), species 1.
template <class PH>
__device__ inline void conv_tensor(const double *U, const typename PH::State &s, double *F) {
  constexpr int NEQ = PH::NEQ, DIM = PH::DIM, NVEL = PH::NVEL, ITH = 1 + NVEL;
  const double H = U[ITH] + s.p;
#pragma unroll
  for (int d = 0; d < DIM; d++) {
    F[0 + d * NEQ] = U[1 + d];
#pragma unroll
    for (int i = 0; i < NVEL; i++) F[1 + i + d * NEQ] = U[1 + i] * s.vel[d] + (i == d ? s.p : 0.0);
    F[ITH + d * NEQ] = s.vel[d] * H;
#pragma unroll
    for (int sp = 0; sp < PH::NACTIVE; sp++) F[(NVEL + 2 + sp) + d * NEQ] = U[NVEL + 2 + sp] * s.vel[d];
    if constexpr (PH::TWO_TEMPERATURE) F[(NEQ - 1) + d * NEQ] = (U[NEQ - 1] + s.pe) * s.vel[d];
  }
}

// Fluxes::ComputeViscousFluxes (src/fluxes.cpp:178-335) through the closure of the physics, with the context k_flux gives
// it (kernels.hpp:2984-3031); Fv[eq + d*NEQ], all zeros for TPSRHS_EULER.  U: the clamped state.
template <class PH>
__device__ inline void visc_tensor(typename PH::PRef prm, const double *U, const typename PH::State &s, const double *g,
                                   const FluxPoint &pt, double *Fv) {
  constexpr int NEQ = PH::NEQ, DIM = PH::DIM;
  if constexpr (PH::TWO_STEP) {  // the mixtures: the state-only closure, then the terms linear in the gradient
    typename PH::FluxCoef fc;
    PH::template flux_coeffs<false>(prm, U, s, fc);
    if constexpr (DIM == 2)
      PH::visc_flux(prm, U, s, fc, g, PH::AXISYM ? pt.radius : -1.0, Fv, pt.ec);
    else
      PH::visc_flux(prm, U, s, fc, g, -1.0, Fv);
  } else if constexpr (PH::AXISYM) {  // axisymmetric dry air / table gas: the normal flux along each coordinate direction
#pragma unroll
    for (int i = 0; i < NEQ * DIM; i++) Fv[i] = 0.0;
    if (prm.eq_system == TPSRHS_EULER) return;
    double visc, bulkv, k;
    PH::transport(prm, s, visc, bulkv, k);
#pragma unroll
    for (int d = 0; d < DIM; d++) {
      const double nd[DIM] = {d == 0 ? 1.0 : 0.0, d == 1 ? 1.0 : 0.0};
      double fv[NEQ];
      PH::visc_normal_flux_of(s, visc, bulkv, k, U, g, nd, pt.radius, false, fv, pt.ec);
#pragma unroll
      for (int eq = 0; eq < NEQ; eq++) Fv[eq + d * NEQ] = fv[eq];
    }
  } else {  // dry air, planar and 3-D; the LES flavour reads elSize and xyz
    PH::visc_flux(prm, U, s, g, Fv, PH::LES ? &pt.pc : nullptr);
  }
}

// One node: u (as stored; the species rows are clamped here, src/rhs_operator.cpp:512-517), g = gradUp[eq + d*NEQ].  The
// parts asked for are written to Fc and Fv; `part` decides which closures run (wave-uniform).
template <class PH>
__device__ inline void flux_parts(typename PH::PRef prm, int part, const double *u, const double *g, const FluxPoint &pt,
                                  double *Fc, double *Fv) {
  constexpr int NEQ = PH::NEQ;
  double uc[NEQ];
#pragma unroll
  for (int eq = 0; eq < NEQ; eq++) uc[eq] = u[eq];
  PH::clamp_species(uc);
  const typename PH::State st = PH::make_state(prm, uc);
  if (part != FLUX_CONVECTIVE) visc_tensor<PH>(prm, uc, st, g, pt, Fv);
  if (part != FLUX_VISCOUS) conv_tensor<PH>(uc, st, Fc);
}

// element vertices -> position of reference point xi: the order-1 map of the sweeps (kernels.hpp::position), term for term
template <int DIM>
__device__ inline void flux_node_position(const double *V, const double *xi, double *X) {
  const double x = xi[0], y = xi[1];
  if constexpr (DIM == 2) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const double v00 = V[0 * 2 + i], v10 = V[1 * 2 + i], v01 = V[2 * 2 + i], v11 = V[3 * 2 + i];
      X[i] = (v00 * (1.0 - x) + v10 * x) * (1.0 - y) + (v01 * (1.0 - x) + v11 * x) * y;
    }
  } else {
    const double z = xi[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double v000 = V[0 * 3 + i], v100 = V[1 * 3 + i], v010 = V[2 * 3 + i], v110 = V[3 * 3 + i];
      const double v001 = V[4 * 3 + i], v101 = V[5 * 3 + i], v011 = V[6 * 3 + i], v111 = V[7 * 3 + i];
      const double lo = (v000 * (1.0 - x) + v100 * x) * (1.0 - y) + (v010 * (1.0 - x) + v110 * x) * y;
      const double hi = (v001 * (1.0 - x) + v101 * x) * (1.0 - y) + (v011 * (1.0 - x) + v111 * x) * y;
      X[i] = lo * (1.0 - z) + hi * z;
    }
  }
}

}  // namespace tpsrhs

#if defined(__HIPCC__)
#include "launch.hpp"

namespace tpsrhs {

// the mesh as the pass needs it: no element structure beyond node / NPE (the mixing-length block and the sponge plane,
// which MeshDev carries, are kernel arguments of their own)
struct FluxGeom {
  int64_t n;            // NDofs
  int n1, npe;          // nodes per direction and per element
  double x[MAXN1];      // the 1-D nodes of the operator's basis on [0,1]
  const double *verts;  // [ne][NV][DIM]
};

// ML: a mixing length is set (2-D kernels with the heavy interface only).  A template parameter, not a test of ml.distance:
// the closure holds the ADDRESS of the block, and an address that is `&ml or NULL` at run time keeps the block in scratch.
template <class PH, bool ML = false>
__global__ __launch_bounds__(256) void k_flux_fields(typename PH::KArg prm_k, const FluxGeom geo, const MixLenDev ml,
                                                     const VsDev vs, int part, const double *__restrict__ U, const double *__restrict__ gradUp,
                                                     double *__restrict__ out) {
  typename PH::PRef prm = PH::pref(prm_k);
  constexpr int NEQ = PH::NEQ, DIM = PH::DIM, NV = 1 << DIM;
  // the block's sponge weights, one word per lane (EddyCtx::vsw): a lane writes and reads its own word only
  __shared__ double sVsw[256];
  const int64_t n = geo.n;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double u[NEQ], g[NEQ * DIM];
#pragma unroll
  for (int eq = 0; eq < NEQ; eq++) u[eq] = U[eq * n + i];
  if (part != FLUX_CONVECTIVE) {
#pragma unroll
    for (int k = 0; k < NEQ * DIM; k++) g[k] = gradUp[k * n + i];
  }
  FluxPoint pt;
  pt.radius = 1.0;
  pt.ec = eddy_off();
  constexpr bool HEAVY2D = PH::HEAVY && DIM == 2;
  if constexpr (PH::AXISYM || HEAVY2D || PH::LES) {
    const int64_t e = i / geo.npe;
    const int nd = static_cast<int>(i - e * geo.npe);
    double X[3] = {0.0, 0.0, 0.0};
    if (PH::AXISYM || PH::LES || vs.enabled) {
      const int idx[3] = {nd % geo.n1, (nd / geo.n1) % geo.n1, nd / (geo.n1 * geo.n1)};
      double xi[DIM];
#pragma unroll
      for (int d = 0; d < DIM; d++) xi[d] = geo.x[idx[d]];
      flux_node_position<DIM>(geo.verts + e * (NV * DIM), xi, X);
    }
    if constexpr (PH::AXISYM) pt.radius = X[0];
    if constexpr (PH::LES) {
#pragma unroll
      for (int d = 0; d < 3; d++) pt.pc.X[d] = X[d];
      pt.pc.delta = prm.elem_delta[e];
    }
    if constexpr (HEAVY2D) {  // kernels.hpp::closure_ctx with the node's own distance
      if constexpr (ML) {
        pt.ec.ml = &ml;
        pt.ec.dist = ml.distance[i];
      }
      if (vs.enabled) {
        sVsw[threadIdx.x] = visc_sponge_weight_2d(vs, X);
        pt.ec.vsw = sVsw;
      }
    }
  }
  double Fc[NEQ * DIM], Fv[NEQ * DIM];
  flux_parts<PH>(prm, part, u, g, pt, Fc, Fv);
#pragma unroll
  for (int k = 0; k < NEQ * DIM; k++) {
    const int d = k / NEQ, eq = k - d * NEQ;
    const double v = (part == FLUX_CONVECTIVE) ? Fc[k] : (part == FLUX_VISCOUS ? Fv[k] : Fc[k] - Fv[k]);
    out[(static_cast<int64_t>(d) * NEQ + eq) * n + i] = v;
  }
}

}  // namespace tpsrhs

namespace {

// the pass of tpsrhs_get_flux on the operator's stream: U = x, gradUp the operator's own.  Instantiated in flux_fields.hip
// (dry air, the table gas) and in the units of plasma_vis_family.hpp, never in a unit of the sweeps.
template <class PH>
void launch_flux_fields(tpsrhs_operator *op, int part, const double *x, double *out) {
  using namespace tpsrhs;
  const int64_t n = op->ndofs;
  const int grid = static_cast<int>((n + 255) / 256);
  if (grid == 0) return;
  FluxGeom geo = {};
  geo.n = n;
  geo.n1 = op->order + 1;
  geo.npe = (op->dim == 3) ? geo.n1 * geo.n1 * geo.n1 : geo.n1 * geo.n1;
  double w[MAXN1];
  segment_rule01(op->nc, geo.n1, geo.x, w);
  geo.verts = op->d_verts.get();
  if constexpr (PH::HEAVY && PH::DIM == 2) {
    if (op->mixlen.distance != nullptr) {
      hipLaunchKernelGGL((k_flux_fields<PH, true>), dim3(grid), dim3(256), 0, op->stream, kernel_params<PH>(op), geo, op->mixlen,
                         op->vs2d, part, x, op->d_gradUp.get(), out);
      HIP_CHECK(hipGetLastError());
      return;
    }
  }
  hipLaunchKernelGGL((k_flux_fields<PH>), dim3(grid), dim3(256), 0, op->stream, kernel_params<PH>(op), geo, op->mixlen,
                     op->vs2d, part, x, op->d_gradUp.get(), out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
#endif

#endif
