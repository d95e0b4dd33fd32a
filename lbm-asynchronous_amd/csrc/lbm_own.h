// lbm_own.h -- one move-only owning handle: a value (a pointer, a runtime handle) and the function that releases it,
// given as a template parameter.  The empty handle holds T() and releases nothing.  No HIP, no allocation: any C++17
// compiler builds it, and tests/own_check.cpp checks it on a machine without a GPU.  lbm_hip.hip defines the device
// buffer, pinned buffer, event, stream and graph handles on top of it; what a struct owns is then what it declares,
// released in reverse order of declaration after its destructor's body has run.
#pragma once

#include <utility>

namespace lbm_own {

template <class T, void (*Release)(T)>
class Own {
 public:
  Own() = default;
  explicit Own(T v) : v_(v) {}
  Own(Own&& o) noexcept : v_(o.release()) {}
  Own& operator=(Own&& o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Own(const Own&) = delete;
  Own& operator=(const Own&) = delete;
  ~Own() { reset(); }

  T get() const { return v_; }
  operator T() const { return v_; }  // reads as the raw value wherever one is expected (kernel arguments, runtime calls)
  explicit operator bool() const { return v_ != T(); }
  // releases what is held, then holds v (nothing by default)
  void reset(T v = T()) {
    const T old = std::exchange(v_, v);
    if (old != T()) Release(old);
  }
  // gives up ownership: the caller now holds the value, the handle is empty
  T release() { return std::exchange(v_, T()); }

 private:
  T v_ = T();
};

}  // namespace lbm_own
