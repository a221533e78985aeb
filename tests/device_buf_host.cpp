// Host test of ikflow_amd/csrc/device_buf.h: the header names six HIP symbols and includes no HIP header, so this program supplies counting
// fakes over malloc / free that can fail the N-th allocation, and is built with -fsanitize=address,undefined (tests/test_device_buf_host.py).
#include <cstdio>
#include <cstdlib>
#include <type_traits>

typedef int hipError_t;
static const hipError_t hipSuccess = 0;
static const hipError_t hipErrorOutOfMemory = 2;

static int g_live = 0;        // allocations made and not yet freed (device + pinned)
static int g_allocs = 0;      // successful + failed allocation calls
static int g_frees = 0;
static int g_fail_at = 0;     // fail the N-th allocation call from now (1 = the next one); 0 never
static size_t g_last_bytes = 0;
static unsigned g_last_flags = 0;
static int g_host_allocs = 0, g_host_frees = 0;

static hipError_t fake_alloc(void** p, size_t bytes) {
  ++g_allocs;
  g_last_bytes = bytes;
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *p = reinterpret_cast<void*>(0x10);  // a failing call may leave garbage behind: the owner must not keep it
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  ++g_live;
  return hipSuccess;
}
template <class T>
static hipError_t hipMalloc(T** p, size_t bytes) { return fake_alloc(reinterpret_cast<void**>(p), bytes); }
static hipError_t hipFree(void* p) {
  ++g_frees;
  --g_live;
  free(p);
  return hipSuccess;
}
template <class T>
static hipError_t hipHostMalloc(T** p, size_t bytes, unsigned flags) {
  ++g_host_allocs;
  g_last_flags = flags;
  return fake_alloc(reinterpret_cast<void**>(p), bytes);
}
static hipError_t hipHostFree(void* p) {
  ++g_host_frees;
  return hipFree(p);
}

#include "device_buf.h"

static_assert(!std::is_copy_constructible<DeviceBuf<float>>::value && !std::is_copy_assignable<DeviceBuf<float>>::value, "DeviceBuf must not copy");
static_assert(!std::is_copy_constructible<PinnedBuf<int>>::value && !std::is_copy_assignable<PinnedBuf<int>>::value, "PinnedBuf must not copy");
static_assert(std::is_convertible<const DeviceBuf<float>&, float*>::value && std::is_convertible<const PinnedBuf<int>&, int*>::value, "reads as T*");

static int g_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

static void test_ensure() {
  {
    DeviceBuf<float> b;
    CHECK(b.p == nullptr && b.cap == 0 && static_cast<float*>(b) == nullptr && !b);
    CHECK(b.ensure(0) == hipSuccess && g_allocs == 0);  // nothing asked, nothing done
    CHECK(b.ensure(10) == hipSuccess && b.p && b.cap == 10 && g_allocs == 1 && g_live == 1 && g_last_bytes == 40);
    b.p[9] = 1.f;  // (the sanitizer checks the size)
    float* const first = b.p;
    CHECK(b.ensure(10) == hipSuccess && b.p == first && g_allocs == 1 && g_frees == 0);  // equal: no call
    CHECK(b.ensure(3) == hipSuccess && b.p == first && b.cap == 10 && g_allocs == 1 && g_frees == 0);  // smaller: no call
    CHECK(b.ensure(11) == hipSuccess && b.cap == 11 && g_allocs == 2 && g_frees == 1 && g_live == 1 && g_last_bytes == 44);  // grows: freed, then allocated
    CHECK(static_cast<float*>(b) == b.p && b + 1 == b.p + 1 && b != nullptr);
    // a failed allocation: the old array is gone, nothing is kept, nothing is live
    g_fail_at = 1;
    CHECK(b.ensure(100) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && g_live == 0 && g_frees == 2);
    CHECK(b.ensure(5) == hipSuccess && b.cap == 5 && g_live == 1);  // and the next call retries
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && g_live == 0 && g_frees == 3);
    b.release();  // twice: no second free
    CHECK(g_frees == 3 && g_live == 0);
    // release, then ensure of the SAME size allocates again (a reload is never a reuse)
    CHECK(b.ensure(5) == hipSuccess);
    const int a0 = g_allocs;
    b.release();
    CHECK(b.ensure(5) == hipSuccess && g_allocs == a0 + 1 && g_live == 1);
  }  // destroyed with contents
  CHECK(g_live == 0 && g_frees == 5);
  {
    DeviceBuf<int> empty;
  }  // destroyed without
  CHECK(g_live == 0 && g_frees == 5);
  // byte-sized elements and a size beyond 32 bits of bytes are passed through unchanged (the fake fails the call: nothing is allocated)
  DeviceBuf<double> big;
  g_fail_at = 1;
  CHECK(big.ensure(1LL << 30) == hipErrorOutOfMemory && g_last_bytes == (size_t)8 << 30 && big.p == nullptr && big.cap == 0);
}

static void test_pinned() {
  const int f0 = g_frees;
  {
    PinnedBuf<int> h;
    CHECK(h.p == nullptr && h.cap == 0);
    CHECK(h.alloc(1) == hipSuccess && h.p && h.cap == 1 && g_host_allocs == 1 && g_last_flags == 0 && g_last_bytes == 4 && g_live == 1);
    *h = 7;
    CHECK(h[0] == 7);
    CHECK(h.alloc(1) == hipSuccess && g_host_allocs == 1);  // no call
    PinnedBuf<int> mapped;
    CHECK(mapped.alloc(2, 0x2u) == hipSuccess && g_last_flags == 0x2u && g_last_bytes == 8 && g_live == 2);
    g_fail_at = 1;
    CHECK(mapped.alloc(4, 0x2u) == hipErrorOutOfMemory && mapped.p == nullptr && mapped.cap == 0 && g_live == 1 && g_host_frees == 1);
    mapped.release();
    mapped.release();
    CHECK(g_host_frees == 1);
  }
  CHECK(g_live == 0 && g_host_frees == 2 && g_frees == f0 + 2);  // pinned memory goes through hipHostFree alone
}

// A group sized from one capacity (the handle's flow scratch, exact rows, exact poses, cluster buffers): every member released before any is
// allocated, members allocated in order, the gate 0 while the group is only partly there.
namespace {
struct Group {
  DeviceBuf<float> a, b, c;
  DeviceBuf<unsigned char> d;
  DeviceBuf<int> e;
  long long gate = 0;
  hipError_t ensure(long long n) {
    if (n <= gate) return hipSuccess;
    a.release(); b.release(); c.release(); d.release(); e.release();
    gate = 0;
    if (g_live != 0) return -1;  // (peak memory: nothing of the old group is left when the first new member is allocated)
    hipError_t r;
    if ((r = a.ensure(n * 7)) != hipSuccess) return r;
    if ((r = b.ensure(n * 1024)) != hipSuccess) return r;
    if ((r = c.ensure(n * 1024)) != hipSuccess) return r;
    if ((r = d.ensure(n)) != hipSuccess) return r;
    if ((r = e.ensure(2 * n)) != hipSuccess) return r;
    gate = n;
    return hipSuccess;
  }
  int members() const { return (a != nullptr) + (b != nullptr) + (c != nullptr) + (d != nullptr) + (e != nullptr); }
};
}  // namespace

static void test_group() {
  for (int fail_pos = 1; fail_pos <= 5; ++fail_pos) {
    {
      Group g;
      CHECK(g.ensure(128) == hipSuccess && g.gate == 128 && g_live == 5);
      const int a0 = g_allocs;
      CHECK(g.ensure(100) == hipSuccess && g_allocs == a0);  // inside the gate: no call
      g_fail_at = fail_pos;
      CHECK(g.ensure(256) == hipErrorOutOfMemory);
      CHECK(g.gate == 0 && g_live == fail_pos - 1 && g.members() == fail_pos - 1);  // the members allocated so far, and no others
      CHECK((g.a != nullptr) == (fail_pos > 1) && (g.d != nullptr) == (fail_pos > 4) && g.e == nullptr);  // ... in order
      // the next call retries the whole group, also for a size the partly-built group "has"
      CHECK(g.ensure(64) == hipSuccess && g.gate == 64 && g_live == 5 && g.a.cap == 64 * 7 && g.e.cap == 128);
      g_fail_at = fail_pos;
      CHECK(g.ensure(512) == hipErrorOutOfMemory && g_live == fail_pos - 1);
    }  // destroyed partly allocated
    CHECK(g_live == 0);
  }
}

int main() {
  test_ensure();
  test_pinned();
  test_group();
  CHECK(g_live == 0);
  if (g_failed) return 1;
  printf("device_buf_host ok: %d allocation calls, %d frees\n", g_allocs, g_frees);
  return 0;
}
