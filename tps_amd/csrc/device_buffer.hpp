// Device memory of the library: HIP_CHECK (which throws status.hpp's DeviceError), the one allocator (dev_alloc, which TPSRHS_POISON fills) and
// DevBuf<T>, device memory with an owner -- freed by the destructor, move-only.  A DevBuf knows neither its size nor a
// stream nor a device: whoever lets one go while a kernel may still read it synchronises first, on the device that holds
// it.  DevBuf<void> owns a buffer whose element type no longer matters (the operator's bags of tables and parameter
// images); it can only adopt a DevBuf<T> &&.  This file is the only place that calls hipFree.
#ifndef TPSRHS_DEVICE_BUFFER_HPP_
#define TPSRHS_DEVICE_BUFFER_HPP_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "status.hpp"

namespace {

#define HIP_CHECK(expr)                                                                                   \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess)                                                                                 \
      throw tpsrhs::DeviceError(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

// TPSRHS_POISON=1 (debug / tests/test_gpu_poison.py): every device allocation of the library starts as all-ones bytes
// (a NaN as a double, -1 as an index), so that a read of memory no kernel has written shows up as a NaN in the
// residual instead of depending on what the allocator happened to return.  Read at every call: cheap next to hipMalloc.
inline bool poison_allocations() {
  const char *e = std::getenv("TPSRHS_POISON");
  return e && e[0] == '1';
}
template <class T>
T *dev_alloc(size_t n) {
  T *p = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p), bytes));
  if (poison_allocations()) {
    HIP_CHECK(hipMemset(p, 0xFF, bytes));
    // the fill runs on the NULL stream, which is not ordered against a non-blocking stream (torch's side streams): it
    // must be complete before the operator's stream first writes p (else a freshly zeroed NaN counter reads -1)
    HIP_CHECK(hipDeviceSynchronize());
  }
  return p;
}

}  // namespace

template <class T>
class DevBuf;
template <>
class DevBuf<void>;

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(size_t n) : p_(dev_alloc<T>(n)) {}
  explicit DevBuf(const std::vector<T> &v) : DevBuf(v.size()) {  // (delegating: a throw below still frees the allocation)
    if (!v.empty()) HIP_CHECK(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { reset(); }

  T *get() const { return p_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  friend class DevBuf<void>;
  T *p_ = nullptr;
};

template <>
class DevBuf<void> {
 public:
  DevBuf() = default;
  template <class T>
  DevBuf(DevBuf<T> &&o) noexcept : p_(o.p_) {
    o.p_ = nullptr;
  }
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  void *get() const { return p_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void *p_ = nullptr;
};

#endif
