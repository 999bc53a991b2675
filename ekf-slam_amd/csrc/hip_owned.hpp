// What the handles (ekf_ctx, ekf_sim, lm_ctx) own on the device: move-only buffers, events and
// streams that release themselves. Buf is written against an allocator policy (static alloc / free
// / clear_error), so tests/hip_owned_host_main.cpp runs the same template on the CPU with a
// counting allocator (HIP_OWNED_NO_HIP: the generic part alone, no HIP header).
#pragma once
#include <cstddef>

#include "ekf.h"

namespace ekfslam {

template <typename T>
constexpr size_t kOwnedSizeof = sizeof(T);
template <>
inline constexpr size_t kOwnedSizeof<void> = 1;  // Buf<void, …>: capacity in bytes

// T[capacity()], grown and never shrunk. Pointer and capacity agree after any outcome of reserve;
// growth keeps no contents. reserve does not synchronise: the caller makes sure nothing in flight
// reads the old block before a reserve that may free it.
template <typename T, typename Alloc>
class Buf {
 public:
  Buf() = default;
  explicit Buf(unsigned flags) : flags_(flags) {}  // (PinnedAlloc: hipHostMalloc's flags)
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_), flags_(o.flags_) { o.release(); }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_, flags_ = o.flags_;
      o.release();
    }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }

  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) Alloc::free(p_);
    release();
  }
  // Room for n elements: nothing happens while n fits; else the old block is freed and ONE block
  // of max(n, at_least) elements allocated. A failure leaves the buffer empty (EKF_E_NOMEM) and
  // the runtime's last error cleared (the launchers return hipGetLastError()).
  int reserve(size_t n, size_t at_least = 0) {
    if (n <= cap_) return EKF_OK;
    reset();
    const size_t cap = n > at_least ? n : at_least;
    p_ = static_cast<T*>(Alloc::alloc(cap * kOwnedSizeof<T>, flags_));
    if (!p_) {
      Alloc::clear_error();
      return EKF_E_NOMEM;
    }
    cap_ = cap;
    return EKF_OK;
  }

 private:
  void release() { p_ = nullptr, cap_ = 0; }
  T* p_ = nullptr;
  size_t cap_ = 0;
  unsigned flags_ = 0;
};

// All-or-nothing groups: `if (a.reserve(…) || b.reserve(…)) return reset_all(a, b);`
template <typename... Bufs>
int reset_all(Bufs&... bufs) {
  (bufs.reset(), ...);
  return EKF_E_NOMEM;
}

}  // namespace ekfslam

#ifndef HIP_OWNED_NO_HIP
#include <hip/hip_runtime.h>

namespace ekfslam {

struct DeviceAlloc {
  static void* alloc(size_t bytes, unsigned) {
    void* p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipFree(p); }
  static void clear_error() { (void)hipGetLastError(); }
};
struct PinnedAlloc {  // flags: hipHostMalloc's
  static void* alloc(size_t bytes, unsigned flags) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes, flags) == hipSuccess ? p : nullptr;
  }
  static void free(void* p) { (void)hipHostFree(p); }
  static void clear_error() { (void)hipGetLastError(); }
};
template <typename T>
using DeviceBuf = Buf<T, DeviceAlloc>;
template <typename T>
using PinnedBuf = Buf<T, PinnedAlloc>;

// An event with its creation flags (default: timing, as the profiling pool's); null until create().
class Event {
 public:
  Event() = default;
  explicit Event(unsigned flags) : flags_(flags) {}
  Event(Event&& o) noexcept : e_(o.e_), flags_(o.flags_) { o.e_ = nullptr; }
  Event(const Event&) = delete;
  Event& operator=(Event&&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  int create() {  // (once; an event that exists stays)
    if (e_ || hipEventCreateWithFlags(&e_, flags_) == hipSuccess) return EKF_OK;
    e_ = nullptr;
    (void)hipGetLastError();
    return EKF_E_HIP;
  }
  hipEvent_t get() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
  unsigned flags_ = hipEventDefault;
};

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }
  int create(unsigned flags = hipStreamDefault) {
    reset();
    if (hipStreamCreateWithFlags(&s_, flags) == hipSuccess) return EKF_OK;
    s_ = nullptr;
    (void)hipGetLastError();
    return EKF_E_HIP;
  }
  void adopt(hipStream_t s) {  // a stream made elsewhere (hipExtStreamCreateWithCUMask)
    reset();
    s_ = s;
  }
  void reset() {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }
  hipStream_t get() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace ekfslam
#endif  // HIP_OWNED_NO_HIP
