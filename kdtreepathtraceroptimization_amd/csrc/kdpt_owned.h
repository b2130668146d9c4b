// kdpt_owned.h -- the owners of the library's HIP resources (host only), and the only place that creates or
// releases one: device memory, pinned host memory, events, streams and host registrations.  Each handle is
// null by default, move-only, releases what it holds in its destructor, and releases its old value before it
// takes a new one.  get() is the raw view that goes into DevScene and kernel arguments.
// Two lifetimes: a DeviceBuf is for what is remade or dropped while its owner lives (a rebuilt mask table, a
// feature that can be turned off); an Arena is for buffers that live exactly as long as their owner (a scene's
// uploads, an iteration state's working set), freed in reverse order of allocation with no per-entry release.
// No handle synchronises: whoever drops one has drained the streams that use it.  A failed creation returns HIP's
// status for the caller's error channel (HIP_TRY / hip_fail, kdpt_error.h) and leaves the handle null.
// tests/native/owned_host.cpp compiles this header against a counting stub of HIP (KDPT_OWNED_HIP_STUB).
#pragma once
#ifndef KDPT_OWNED_HIP_STUB
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace kdpt {

// What the handles share: one value H, released with Release (which takes an Arg).
template <typename H, typename Arg, hipError_t (*Release)(Arg)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(o.detach()) {}
  Owned& operator=(Owned&& o) noexcept {
    reset(o.detach());  // (a self-move detaches first: nothing is released, the value stays)
    return *this;
  }
  ~Owned() { reset(); }  // (the move operations leave no copy)
  H get() const { return h_; }
  explicit operator bool() const { return h_ != H{}; }
  void reset(H h = H{}) {
    if (h_ != H{}) (void)Release(h_);
    h_ = h;
  }

 protected:
  H detach() {
    H h = h_;
    h_ = H{};
    return h;
  }
  H h_{};
};

inline hipError_t device_bytes(void** p, size_t n) { return hipMalloc(p, n); }
inline hipError_t pinned_bytes(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }

// n elements of memory from Alloc (a zero-length request allocates one element).
template <typename T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Release)(void*)>
class Buf : public Owned<T*, void*, Release> {
 public:
  hipError_t alloc(size_t n) {
    this->reset();
    void* q = nullptr;
    const hipError_t e = Alloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) this->h_ = static_cast<T*>(q);
    return e;
  }
};
template <typename T>
using DeviceBuf = Buf<T, device_bytes, hipFree>;
template <typename T>
using PinnedBuf = Buf<T, pinned_bytes, hipHostFree>;

// (An event or a stream converts to its raw handle, which is all a HIP call wants of it; a buffer is viewed through
// get() alone, so that what enters a kernel argument is spelled out.)
class Event : public Owned<hipEvent_t, hipEvent_t, hipEventDestroy> {
 public:
  operator hipEvent_t() const { return h_; }
  hipError_t create() {  // with timing
    reset();
    return hipEventCreate(&h_);
  }
  hipError_t create_untimed() {  // hipEventDisableTiming: ordering only
    reset();
    return hipEventCreateWithFlags(&h_, hipEventDisableTiming);
  }
};

// A non-blocking stream.  cus > 0: created with a mask of all `cus` compute units, which gives it a hardware
// queue of its own (kdpt_runtime.hip, create_stream); a failed masked creation falls back to a plain one.
class Stream : public Owned<hipStream_t, hipStream_t, hipStreamDestroy> {
 public:
  operator hipStream_t() const { return h_; }
  hipError_t create(int cus = 0) {
    reset();
    if (cus > 0) {
      std::vector<uint32_t> mask((cus + 31) / 32, 0xffffffffu);
      if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
      if (hipExtStreamCreateWithCUMask(&h_, (uint32_t)mask.size(), mask.data()) == hipSuccess) return hipSuccess;
      (void)hipGetLastError();
      h_ = nullptr;
    }
    return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
  }
};

// Device buffers that live as long as their owner, which stays where it is; freed last first.
class Arena {
 public:
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() {
    while (!p_.empty()) p_.pop_back();
  }
  template <typename T>
  hipError_t alloc(T** out, size_t n) {
    DeviceBuf<char> b;
    const hipError_t e = b.alloc(std::max<size_t>(n, 1) * sizeof(T));
    *out = reinterpret_cast<T*>(b.get());
    if (e == hipSuccess) p_.push_back(std::move(b));
    return e;
  }

 private:
  std::vector<DeviceBuf<char>> p_;
};

// Host ranges pinned in place (hipHostRegister) until clear() or the end of the scope.
class HostRegistrations {
 public:
  HostRegistrations() = default;
  HostRegistrations(const HostRegistrations&) = delete;
  HostRegistrations& operator=(const HostRegistrations&) = delete;
  ~HostRegistrations() { clear(); }
  hipError_t add(void* p, size_t bytes) {
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e == hipSuccess) p_.push_back(p);
    return e;
  }
  void clear() {
    for (; !p_.empty(); p_.pop_back()) (void)hipHostUnregister(p_.back());
  }

 private:
  std::vector<void*> p_;
};

}  // namespace kdpt
