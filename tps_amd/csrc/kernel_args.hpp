// The plain blocks the host fills and the kernels take by value or through a pointer: what the operator object
// (operator.hpp) keeps of them needs no kernel, and the kernels (kernels.hpp) need no operator.  MixLenDev and VsDev, which
// MeshDev carries, stay in physics_dryair.hpp: the host builds of the point physics (tests/host_physics and its
// neighbours) compile that header from a directory that holds the physics headers alone, with a stand-in for HIP.
#ifndef TPSRHS_KERNEL_ARGS_HPP_
#define TPSRHS_KERNEL_ARGS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/tpsrhs.h"
#include "physics_dryair.hpp"

namespace tpsrhs {

// ConstantPressureGradient / HeatSource / SpongeZone / JouleHeating of RHSoperator's forcing array
// (src/rhs_operator.cpp:101-166), evaluated per node in k_flux next to the point sources.  One block in
// device memory; the address is wave-uniform, so its fields arrive through scalar loads.
struct ForcingDev {
  int has_pg, nheat, nsponge, pad;
  double pg[3];
  struct Heat {
    double value, radius, len;  // len = |point2 - point1|
    double p1[3], axis[3];      // axis = unit vector point1 -> point2
  } heat[TPSRHS_MAXHEATSOURCES];
  struct Sponge {
    int type, pad;
    double normal[3], p0[3], pinit[3];
    double r1, r2, mult;
    double target[TPSRHS_MAXEQUATIONS];
    // mixed-out target (SpongeZoneSolution::MIXEDOUT): nodes of the mix-out plane, and the sums over them
    int mixed_out, n_plane;
    const int *plane_nodes;  // [n_plane] device
    double *msum;            // [NEQ + 1] device: sum of F_c . n per equation, number of nodes
  } sponge[TPSRHS_MAXSPONGEZONES];
  const double *joule;  // [ndofs] or NULL
  int nps, pad2;
  struct Scalar {
    double x0[3], radius, value;
  } ps[TPSRHS_MAXPASSIVESCALARS];
};

// RK4 stage combination fused into the epilogue of k_flux inside tpsrhs_rk4_step / tpsrhs_advance (src/M2ulPhyS.cpp:
// 2004-2008 around MFEM's RK4Solver::Step): the residual k of a node never goes to memory, the lane that owns the node
// writes the next stage's state (or the new solution) instead.
//   mode 0  plain Mult: Y = k
//   mode 1  out = U + dt/2 k           (stage 1: the stage input is x itself, taken from LDS)
//   mode 2  out = x0 + dt/2 k          mode 3  out = x0 + dt k
//   mode 4  out = x0 + [(y2 - x0) + 2 (y3 - x0) + (y4 - x0)] / 3 + dt/6 k,  then the NaN census and the species clamp
//           (Check_NAN, Check_Undershoot).  With y2 = x0 + dt/2 k1, y3 = x0 + dt/2 k2, y4 = x0 + dt k3 this is
//           x0 + dt/6 (k1 + 2 k2 + 2 k3 + k4): the accumulator z of RK4Solver::Step is recovered from the stage states
//           instead of being streamed through memory at every stage (6 vector passes per step instead of 14); the
//           differences are exact, the result differs from the reference's order of operations by rounding only.
struct RkDev {
  int mode, sp_first, sp_last, pad;
  double dt_host;
  const double *dt_dev;  // tpsrhs_advance keeps dt in device memory
  const double *x0, *y2, *y3, *y4;
  double *out;
  unsigned long long *nan_count;
  double *ta_out;  // non-NULL (stages 1..3 of a step, launch_all): the face-node traces of `out` go here -- the NEXT stage's
                   // k_traces sweep done where the new state sits in registers (3-D collocated kernels, flux_fuses_traces)
};

struct MeshDev {
  const int *blocks;           // workgroup -> block of EPB consecutive elements (NULL: identity); lets one
                               // launch cover the interior and another the blocks that touch shared faces
  int ne;
  int reverse;                 // 1: the sweep walks each XCD's chunk of the block list backwards (xcd_block)
  int64_t ndofs;
  const double *verts;         // [ne][NV][DIM] lexicographic corners
  const int2 *face_info;       // [ne*NFACES] {neighbour slot | -(bc+1), orientation code}
  const double *minv;          // non-collocated variant: [ne][NPE][NPE] inverse element mass matrices (symmetric)
  MixLenDev ml;                // MixingLengthTransport (2-D kernels): wall-distance grid function, or distance = NULL
  VsDev vs;                    // viscous sponge of the 2-D kernels with the heavy interface (enabled = 0: none)
};

struct VisRows {  // first row of each group of tpsrhs_visualization_fields (AuxiliaryVisualizationIndexes, in rows)
  int Xsp, Ysp, nsp, FluxTrns, diffVel, SrcTrns, SpeciesTrns, rxn;
};

}  // namespace tpsrhs
#endif
