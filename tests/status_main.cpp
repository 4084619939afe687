// Stand-alone driver of tps_amd/csrc/status.hpp (tests/test_status_mapping.py builds it with plain g++, once without and
// once with -fsanitize=address,undefined, and runs it as a child process).  It throws one exception of each class the
// library throws through guarded() and prints the status and the text tpsrhs_last_error returns -- which the library
// defines over last_error() exactly as below.  A message never decides a status: the plain runtime_error here says "halo"
// and "no HIP device", and a HaloError and a NoDevice say neither.
#include <cstdio>
#include <new>
#include <stdexcept>

#include "../tps_amd/csrc/status.hpp"

using namespace tpsrhs;

extern "C" const char *tpsrhs_last_error(void) { return last_error().c_str(); }

namespace {
template <class F>
void show(const char *what, F &&f) {
  const int st = guarded(f);
  std::printf("%s status %d text %s\n", what, st, st == TPSRHS_OK ? "-" : tpsrhs_last_error());
}
}  // namespace

int main() {
  show("ok", [] {});
  show("Unsupported", [] { throw Unsupported("order 9 is not built"); });
  show("DeviceError", [] { throw DeviceError("hipMalloc: out of memory"); });
  show("NoDevice", [] { throw NoDevice("nothing to run on"); });
  show("HaloError", [] { throw HaloError("the exchange callback failed"); });
  show("invalid_argument", [] { throw std::invalid_argument("NULL mesh"); });
  show("runtime_error", [] { throw std::runtime_error("mesh: a halo face, and no HIP device, in the text only"); });
  show("logic_error", [] { throw std::logic_error("two predicates disagree"); });
  show("bad_alloc", [] { throw std::bad_alloc(); });
  show("ok_again", [] {});
  std::printf("last %s\n", tpsrhs_last_error());  // a success leaves the last failure's text in place
  std::printf("fail %d %s\n", fail(TPSRHS_ERR_MESH, "said directly"), tpsrhs_last_error());
  std::printf("STATUS DONE\n");
  return 0;
}
