// The nodal flux tensor of libtpsrhs.so (flux_fields.hpp): tpsrhs_get_flux, and the passes of the single-fluid physics -- dry
// air planar / 3-D with its LES flavour, axisymmetric dry air, the two table gases.  The passes of the mixtures live in the
// shared objects of their families (plasma_vis_family.hpp) and are reached through tpsrhs_operator::flux_fields.  No unit
// of the sweeps instantiates the pass: their device code does not know it exists.
#include "abi_support.hpp"
#include "flux_fields.hpp"
#include "physics_dryair_axisym.hpp"

namespace {

void pick_flux_fields(tpsrhs_operator *h) {
  if (h->flux_fields) return;
  if (h->phys.working_fluid == TPSRHS_USER_DEFINED) {
    load_plasma_vis_family(h, "tpsrhs_get_flux");
    if (!h->flux_fields) throw Unsupported("tpsrhs_get_flux: the kernel family of this mixture has no flux pass");
    return;
  }
  const bool axi = h->nvel > h->dim;
  if (h->phys.working_fluid == TPSRHS_LTE_FLUID) {
    h->flux_fields = (h->phys.lte2d.enabled != 0) ? &launch_flux_fields<Lte2dAxiPhys> : &launch_flux_fields<LteAxiPhys>;
  } else if (axi) {
    h->flux_fields = &launch_flux_fields<DryAirAxiPhys>;
  } else {
    // the LES flavour where a sub-grid scale model or the planar viscous sponge is on (operator_plan.hpp: OperatorPlan::les)
    const DryAirParams &d = *reinterpret_cast<const DryAirParams *>(h->params);
    const bool les = d.sgs_type > 0 || d.vs_enabled;
    if (h->dim == 3)
      h->flux_fields = les ? &launch_flux_fields<DryAirPhys<3, false, true>> : &launch_flux_fields<DryAirPhys<3>>;
    else
      h->flux_fields = les ? &launch_flux_fields<DryAirPhys<2, false, true>> : &launch_flux_fields<DryAirPhys<2>>;
  }
}

}  // namespace

void get_flux(tpsrhs_operator *h, const double *x, int part, int gradients_current, double *out) {
  pick_flux_fields(h);
  HIP_CHECK(hipSetDevice(h->device));
  if (!gradients_current) h->launch(h, x, nullptr, true);  // rhsOperator->updateGradients(*U, false): Up and gradUp of x
  h->flux_fields(h, part, x, out);
}

extern "C" {

int tpsrhs_get_flux(tpsrhs_handle h, const double *x, int part, int gradients_current, double *out) {
  if (!h || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_get_flux: NULL argument");
  if (part != TPSRHS_FLUX_TOTAL && part != TPSRHS_FLUX_CONVECTIVE && part != TPSRHS_FLUX_VISCOUS)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_get_flux: part " + std::to_string(part) + " is none of TOTAL, CONVECTIVE, VISCOUS");
  return guarded([&] { get_flux(h, x, part, gradients_current, out); });
}

}  // extern "C"
