// The refusal of a configuration outside the built scope (-> TPSRHS_ERR_UNSUPPORTED).  No HIP in here: thrown by the
// device-free plan (operator_plan.hpp) as well as by the library proper (status.hpp, which every unit of it includes).  plasma_params_host.hpp keeps a
// type of its own, UnsupportedConfig, which tpsrhs.hip translates: tests/host_physics builds that header from a copy, in a
// directory that holds the physics headers alone.
#ifndef TPSRHS_UNSUPPORTED_HPP_
#define TPSRHS_UNSUPPORTED_HPP_

#include <stdexcept>
#include <string>

namespace tpsrhs {

struct Unsupported : std::runtime_error {
  explicit Unsupported(const std::string &s) : std::runtime_error(s) {}
};

}  // namespace tpsrhs
#endif
