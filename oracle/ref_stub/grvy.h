// TEST INFRASTRUCTURE, computes nothing but containers -- a stand-in for <grvy.h>, written from scratch: the point-physics
// units of the reference use GRVY for log levels and grvy_printf only (oracle/ref.mk).  Messages are dropped.
#ifndef TPSREF_STUB_GRVY_H_
#define TPSREF_STUB_GRVY_H_
#include <string>

namespace GRVY {
class GRVY_Timer_Class;
class GRVY_Input_Class;
}  // namespace GRVY

inline void grvy_printf(int, const char *, ...) {}

#define GRVY_ERROR 0
#define GRVY_INFO 1
#define GRVY_WARN 2
#define GRVY_DEBUG 3
#define GERROR 0
#define GINFO 1
#define GWARN 2
#define GDEBUG 3
#endif
