// Point location on the device, and the node coordinates of an operator: the location half of what the reference delegates
// to gslib's FindPointsGSLIB when it carries a field from one mesh to another (utils/pfield_interpolate.cpp:114-142:
// the physical coordinates of every target node through ElementTransformation::Transform, then finder.Setup on the source
// mesh and finder.Interpolate; src/cycle_avg_joule_coupling.cpp:159-363 does the same in both directions at every coupling
// iteration).  Included by sampling.hip only: the kernel families do not see it.  The evaluation half is k_sample
// (sampling.hpp), unchanged.
//
// The location rule is point_locate.hpp's locate_one, the text the host locator runs: the point's one bin, its elements in
// ascending order, the box test, Newton from the element centre (at most 50 iterations, stop at a correction <= 1e-13), the
// first element whose reference coordinates all lie in [-tol, 1 + tol].  The device contracts a * b + c into an FMA and the
// host build does not: reference coordinates differ from the host's in the last bits, and the accepted element can differ
// only for a point whose coordinate lies within rounding of -tol or 1 + tol -- 1e-10 outside an element, not on a face.
#ifndef TPSRHS_LOCATE_DEVICE_HPP_
#define TPSRHS_LOCATE_DEVICE_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "point_locate.hpp"
#include "sampling.hpp"

namespace tpsrhs {

// One lane per point, in the caller's order; BLOCK = 64, one wave per block.  The lanes of a wave walk different numbers
// of candidates and Newton iterations, so a wave takes as long as its slowest lane: the kernel is meant for point sets
// that are spatially coherent (the nodes of another mesh arrive element by element), where the lanes of a wave share a
// bin and, mostly, the accepted element, and the vertex reads of neighbouring lanes hit the same cache lines.  A block of
// one wave keeps a slow wave from holding the registers of three finished ones.  No LDS: the Newton iterate, the Jacobian
// and the residual live in registers, the vertices are re-read from cache at every iteration.  Besides elem and ref the
// lane writes perm[i] = i (k_sample reads its output position there: no sort, identity).  The found count: a ballot over
// the wave and ONE integer atomic per block.
template <int DIM, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_locate(LocateGridView<DIM> g, const double *__restrict__ verts, int64_t npts, const double *__restrict__ xyz, double tol,
             int32_t *__restrict__ elem, double *__restrict__ ref, int64_t *__restrict__ perm,
             unsigned long long *__restrict__ nfound) {
#pragma clang fp reciprocal(off)  // Newton's corrections are IEEE divisions, whatever the unit switched on before
  static_assert(BLOCK == 64, "the found count is one ballot: one wave per block");
  const int64_t i = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
  bool found = false;
  if (i < npts) {
    double p[DIM], xi[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) p[d] = xyz[i + d * npts];
    const int32_t e = locate_one<DIM>(g, verts, p, tol, xi);
    elem[i] = e;
#pragma unroll
    for (int d = 0; d < DIM; d++) ref[i + d * npts] = xi[d];
    perm[i] = i;
    found = e >= 0;
  }
  const unsigned long long mask = __ballot(found);
  if (threadIdx.x == 0 && mask) atomicAdd(nfound, static_cast<unsigned long long>(__popcll(mask)));
}

// xyz[i + d * ndofs] of DG node i = e * n1^DIM + (a + b n1 + c n1^2): the order-1 vertex map at the operator's 1-D nodes.
// The node is picked with an unrolled select, not with a run-time index into the argument.
template <int DIM, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
    k_node_coordinates(int64_t ndofs, int n1, SampleNodes nodes, const double *__restrict__ verts, double *__restrict__ xyz) {
  constexpr int NV = 1 << DIM;
  const int64_t i = blockIdx.x * static_cast<int64_t>(BLOCK) + threadIdx.x;
  if (i >= ndofs) return;
  const int npe = DIM == 3 ? n1 * n1 * n1 : n1 * n1;
  const int64_t e = i / npe;
  int l = static_cast<int>(i - e * npe);
  double xi[DIM], x[DIM];
#pragma unroll
  for (int d = 0; d < DIM; d++) {
    const int a = l % n1;
    l /= n1;
    double t = nodes.x[0];
#pragma unroll
    for (int j = 1; j <= TPSRHS_MAXORDER; j++) t = j == a ? nodes.x[j] : t;
    xi[d] = t;
  }
  vertex_map<DIM>(verts + e * (NV * DIM), xi, x, nullptr);
#pragma unroll
  for (int d = 0; d < DIM; d++) xyz[i + d * ndofs] = x[d];
}

}  // namespace tpsrhs
#endif
