// Host plumbing of the probe entry points: device buffers that free themselves, and error propagation.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "probe.h"

namespace pzkprobe {

#define PROBE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

struct DBuf {
  void* p = nullptr;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { if (p) (void)hipFree(p); }
  // allocate `bytes` (at least one) and fill from host `h`, or with zeros when h is null
  hipError_t up(const void* h, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) { p = nullptr; return e; }
    if (!bytes) return hipSuccess;
    return h ? hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
  }
  hipError_t down(void* h, size_t bytes) const { return bytes ? hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

inline bool bad_count(int n) { return n < 0 || n > PZK_PROBE_MAX_CASES; }
inline hipError_t finish() {
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : hipDeviceSynchronize();
}

}  // namespace pzkprobe
