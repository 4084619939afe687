// From an exception to a status of tpsrhs.h: the types the library throws, the text tpsrhs_last_error returns, and the
// wrapper every entry point of the C ABI runs its body in.  The TYPE decides the status, never the message.  No HIP in
// here: tests/status_main.cpp drives it on the host.
#ifndef TPSRHS_STATUS_HPP_
#define TPSRHS_STATUS_HPP_

#include <stdexcept>
#include <string>

#include "../../include/tpsrhs.h"
#include "unsupported.hpp"

namespace tpsrhs {

struct DeviceError : std::runtime_error {  // a HIP call failed (HIP_CHECK, device_buffer.hpp) -> TPSRHS_ERR_DEVICE
  explicit DeviceError(const std::string &s) : std::runtime_error(s) {}
};
struct NoDevice : std::runtime_error {  // -> TPSRHS_ERR_NO_DEVICE
  explicit NoDevice(const std::string &s) : std::runtime_error(s) {}
};
struct HaloError : std::runtime_error {  // a callback of the caller's failed, or one a partitioned mesh needs is missing -> TPSRHS_ERR_HALO
  explicit HaloError(const std::string &s) : std::runtime_error(s) {}
};

// the text of the calling thread's last failure (tpsrhs_last_error): one object for every unit of the library
inline std::string &last_error() {
  static thread_local std::string text;
  return text;
}
inline int fail(int code, const std::string &msg) {
  last_error() = msg;
  return code;
}

// Any other std::runtime_error is the mesh's (topology.hpp and the geometry throw it plain), and whatever else derives from
// std::exception (std::logic_error, std::bad_alloc) is reported as an invalid argument.
template <class F>
int guarded(F &&f) {
  try {
    f();
    return TPSRHS_OK;
  } catch (const Unsupported &e) {
    return fail(TPSRHS_ERR_UNSUPPORTED, e.what());
  } catch (const DeviceError &e) {
    return fail(TPSRHS_ERR_DEVICE, e.what());
  } catch (const NoDevice &e) {
    return fail(TPSRHS_ERR_NO_DEVICE, e.what());
  } catch (const HaloError &e) {
    return fail(TPSRHS_ERR_HALO, e.what());
  } catch (const std::invalid_argument &e) {
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, e.what());
  } catch (const std::runtime_error &e) {
    return fail(TPSRHS_ERR_MESH, e.what());
  } catch (const std::exception &e) {
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, e.what());
  }
}

}  // namespace tpsrhs
#endif
