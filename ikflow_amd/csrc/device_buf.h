// The two owning types behind every device and pinned-host allocation of the handle (struct ikf_model, ikf_model.h).  This header names
// hipMalloc, hipFree, hipHostMalloc, hipHostFree, hipError_t and hipSuccess and includes no HIP header itself: whoever includes it
// supplies those six (the API units through ikf_internal.h, tests/device_buf_host.cpp through a counting fake).
#pragma once
#include <cstddef>

#pragma GCC visibility push(hidden)  // (the members that are not inlined must not join the library's exports)

// A device array that only grows.  ensure(n): nothing when it already holds n elements; otherwise the old array is freed BEFORE the new
// one is allocated, and a failed hipMalloc leaves it empty - nothing leaked, no dangling pointer.  A site that must reallocate whatever
// it holds (a weight reload) calls release() first.  Reads as a plain T*.  The destructor frees: a handle's buffers go with `delete m`,
// which ikf_destroy and the error paths of ikf_create run inside their DeviceGuard's scope, i.e. on the handle's device.
template <class T>
struct DeviceBuf {
  T* p = nullptr;
  long long cap = 0;  // elements
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { release(); }
  operator T*() const { return p; }
  hipError_t ensure(long long n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, sizeof(T) * (size_t)n);
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// The same over pinned host memory (hipHostMalloc with `flags`, hipHostFree): the words a kernel or a copy hands back to the host.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  long long cap = 0;  // elements
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  operator T*() const { return p; }
  hipError_t alloc(long long n, unsigned flags = 0) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, sizeof(T) * (size_t)n, flags);
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};
#pragma GCC visibility pop
