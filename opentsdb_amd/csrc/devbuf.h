// devbuf.h -- the buffers that own device and page-locked host memory (host code only).
//
// A buffer frees its memory when it goes out of scope or its owner is deleted, on the device that is
// current then; it moves but does not copy.  ensure() grows by freeing and allocating anew: it keeps
// no contents.  The live counters are process-wide and exist for the tests (tsdbhip_debug_buffers).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>

namespace tsdb {

struct BufCount {
  std::atomic<int64_t> n{0};        // live allocations
  std::atomic<uint64_t> bytes{0};   // ... and the bytes allocated for them
};
inline BufCount dev_live, host_live;

struct DevMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
  static BufCount& live() { return dev_live; }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
  static BufCount& live() { return host_live; }
};

template <class Mem>
struct OwnedBuf {
  void* p = nullptr;
  size_t n = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept { take(o); }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      take(o);
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= n && p) return hipSuccess;
    release();
    const size_t want = bytes ? bytes : 16;
    const hipError_t e = Mem::alloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = bytes;
    held = want;
    Mem::live().n.fetch_add(1, std::memory_order_relaxed);
    Mem::live().bytes.fetch_add(held, std::memory_order_relaxed);
    return e;
  }
  void release() {
    if (p) Mem::free(p);
    if (held) {
      Mem::live().n.fetch_sub(1, std::memory_order_relaxed);
      Mem::live().bytes.fetch_sub(held, std::memory_order_relaxed);
    }
    p = nullptr;
    n = held = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }

 private:
  // The bytes ensure() counted for this buffer.  A routine handed &p and &n (the scan wrappers'
  // temporary storage) frees and allocates behind the buffer's back: what it allocated is freed
  // here like anything else and is not counted.
  size_t held = 0;
  void take(OwnedBuf& o) {
    p = std::exchange(o.p, nullptr);
    n = std::exchange(o.n, 0);
    held = std::exchange(o.held, 0);
  }
};

using DevBuf = OwnedBuf<DevMem>;       // device memory
using HostBuf = OwnedBuf<PinnedMem>;   // page-locked host memory (staging of copies), grown on demand

}  // namespace tsdb
