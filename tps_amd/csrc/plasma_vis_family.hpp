// The post-processing passes (visualization.hpp, k_vis_fields; external_rates.hpp) of the plasma kernel families, in translation units of
// their own: plasma_vis_<geo>_n<species>[a].hip -> libtpsrhs_plasma_vis_<...>.so, loaded by the core at the first
// tpsrhs_visualization_fields of an operator of that family (tpsrhs.hip::load_family), one per (geometry, species count,
// ambipolar or not) -- the passes do not depend on the polynomial order.
//
// Why not in the units of the sweeps, next to launch_point_eval: the compiler's decisions for a kernel depend on what else
// its unit holds.  With the passes instantiated in plasma_family.hpp -- after every sweep or not -- k_flux of some families
// came out with another register allocation (the closures it inlines had gained callers), which the byte-for-byte
// comparison of tools/device_asm_diff.py and the spill census both showed.  A unit of their own leaves the sweeps' units
// without a single new instantiation: their device code is what it was.
#ifndef TPSRHS_PLASMA_VIS_FAMILY_HPP_
#define TPSRHS_PLASMA_VIS_FAMILY_HPP_

#include "external_rates.hpp"
#include "flux_fields.hpp"
#include "launch.hpp"
#include "physics_plasma.hpp"

template <int DIM, int NVEL, int NSP, bool AMBI, bool TWOT, int TR>
static void pick_plasma_vis_of(tpsrhs_operator *op) {
  op->vis_fields = &launch_vis_fields<PlasmaPhys<DIM, NVEL, NSP, AMBI, TWOT, TR>>;
  // the per-node passes of the Boltzmann coupling (external_rates.hpp) need the same closures and live here for the same reason
  op->ext_reactions = &launch_external_reactions<PlasmaPhys<DIM, NVEL, NSP, AMBI, TWOT, TR>>;
  op->boltzmann_fields = &launch_boltzmann_fields<PlasmaPhys<DIM, NVEL, NSP, AMBI, TWOT, TR>>;
  // ... and the nodal flux tensor of tpsrhs_get_flux (flux_fields.hpp)
  op->flux_fields = &launch_flux_fields<PlasmaPhys<DIM, NVEL, NSP, AMBI, TWOT, TR>>;
}

// the transport models a family instantiates: those of plasma_family.hpp::pick_plasma_family
template <int DIM, int NVEL, int NSP, bool AMBI>
static void pick_plasma_vis(tpsrhs_operator *op, bool two_temperature, int transport) {
  if (transport == TRANSPORT_CONSTANT) {
    if (two_temperature)
      pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, true, TRANSPORT_CONSTANT>(op);
    else
      pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, false, TRANSPORT_CONSTANT>(op);
  } else if (transport == TRANSPORT_ARGON_MIXTURE) {
    if constexpr (NSP <= 7) {
      if (two_temperature)
        pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, true, TRANSPORT_ARGON_MIXTURE>(op);
      else
        pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, false, TRANSPORT_ARGON_MIXTURE>(op);
    } else {
      throw Unsupported("argon_mixture transport supports at most 7 species");
    }
  } else {
    if constexpr (NSP == 3) {
      if (two_temperature)
        pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, true, TRANSPORT_ARGON_MINIMAL>(op);
      else
        pick_plasma_vis_of<DIM, NVEL, NSP, AMBI, false, TRANSPORT_ARGON_MINIMAL>(op);
    } else {
      throw Unsupported("argon_minimal transport is the ternary (Ar, Ar.+1, E) model");
    }
  }
}

// The entry point is C, with the signature of the sweeps' families (and their <name>_operator_size): no exception crosses
// the boundary.
#define TPSRHS_PLASMA_VIS_FAMILY(name, DIM, NVEL, NSP, AMBI)                                                          \
  extern "C" { unsigned long name##_operator_size = sizeof(tpsrhs_operator); }                                        \
  extern "C" int name(tpsrhs_operator *op, int two_temperature, int transport, char *err, int errlen) {               \
    try {                                                                                                             \
      pick_plasma_vis<DIM, NVEL, NSP, AMBI>(op, two_temperature != 0, transport);                                     \
      return TPSRHS_OK;                                                                                               \
    } catch (const std::exception &e) {                                                                               \
      if (err && errlen > 0) {                                                                                        \
        std::strncpy(err, e.what(), static_cast<size_t>(errlen) - 1);                                                 \
        err[errlen - 1] = 0;                                                                                          \
      }                                                                                                               \
      return TPSRHS_ERR_UNSUPPORTED;                                                                                  \
    }                                                                                                                 \
  }
#endif
