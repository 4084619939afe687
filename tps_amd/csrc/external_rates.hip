// The C ABI of the coupling to an electron Boltzmann solver (include/tpsrhs.h; src/M2ulPhyS2Boltzmann.cpp):
// tpsrhs_set_reaction_rates (M2ulPhyS::fetch) and tpsrhs_boltzmann_fields (M2ulPhyS::push).  No kernel of this unit: the two
// per-node passes (external_rates.hpp) live in the post-processing units of the plasma families (plasma_vis_family.hpp),
// loaded on demand and reached through tpsrhs_operator::ext_reactions / boltzmann_fields.
#include "abi_support.hpp"

namespace {

void require_mixture(const tpsrhs_operator *h, const char *who) {
  if (h->phys.working_fluid == TPSRHS_DRY_AIR) throw Unsupported(std::string(who) + ": dry air has no species and no chemistry");
  if (h->phys.working_fluid != TPSRHS_USER_DEFINED)
    throw Unsupported(std::string(who) + ": built for the species mixtures (fluid = user_defined), not for the table gas");
}

}  // namespace

extern "C" {

int tpsrhs_set_reaction_rates(tpsrhs_handle h, const double *rates, int num_components, int64_t size) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_set_reaction_rates: NULL handle");
  return guarded([&] {
    if (rates) {
      if (h->ext.num_reactions == 0)
        throw std::invalid_argument("tpsrhs_set_reaction_rates: the operator has no reaction with an external rate coefficient");
      if (size != h->ndofs) throw std::invalid_argument("tpsrhs_set_reaction_rates: size must be the number of nodes (NDofs)");
      if (num_components < h->ext.num_components_needed)
        throw std::invalid_argument("tpsrhs_set_reaction_rates: a reaction reads component " +
                                    std::to_string(h->ext.num_components_needed - 1) + ", the array has " +
                                    std::to_string(num_components));
      HIP_CHECK(hipSetDevice(h->device));
      load_plasma_vis_family(h, "reaction rates");
    }
    // GridFunctionReaction::setGridFunction: component c at rates + c * size.  (setData offsets by the size_ of the call
    // BEFORE, src/reaction.cpp:90-93: not followed.)
    h->ext.rates = rates;
    h->ext.num_components = rates ? num_components : 0;
    // the pass adds to the residual in memory: the stage combinations of RK4 cannot stay in k_flux's epilogue
    h->forcing_active = h->forcing_terms || rates != nullptr;
    h->loop.config_epoch++;  // a captured time-loop graph holds the old pointer
  });
}

int tpsrhs_boltzmann_fields(tpsrhs_handle h, const double *x, int num_species, double *out) {
  if (!h || !x || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_boltzmann_fields: NULL argument");
  return guarded([&] {
    require_mixture(h, "boltzmann fields");
    if (num_species < 1 || num_species > h->phys.mixture.num_species)
      throw std::invalid_argument("tpsrhs_boltzmann_fields: 1 <= num_species <= the mixture's species count");
    HIP_CHECK(hipSetDevice(h->device));
    load_plasma_vis_family(h, "boltzmann fields");
    h->boltzmann_fields(h, x, num_species, out);
  });
}

}  // extern "C"
