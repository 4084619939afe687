// DevBuf<T>: device memory with an owner.  Allocated through dev_alloc / dev_upload (operator.hpp, so TPSRHS_POISON fills
// it like every other allocation), freed by the destructor; move-only.  It knows neither its size nor a stream nor a
// device: whoever lets one go while a kernel may still read it synchronises first, on the device that holds it.
// Included by tpsrhs.hip only.
#ifndef TPSRHS_DEVICE_BUFFER_HPP_
#define TPSRHS_DEVICE_BUFFER_HPP_

#include <cstddef>
#include <vector>

#include "operator.hpp"

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(size_t n) : p_(dev_alloc<T>(n)) {}
  explicit DevBuf(const std::vector<T> &v) : p_(dev_upload(v)) {}
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
  T *p_ = nullptr;
};

#endif
