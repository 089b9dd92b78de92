// DevBuf / PinBuf: the one way the library owns device and page-locked host memory.  Owning, move-only, grow-only:
// ensure(n, s) is the whole growth rule -- nothing within the capacity; else the stream that may still read the old
// block is synchronised (only when there is an old block), the block freed and exactly n elements allocated.  The
// growth POLICY (head room, doubling) is the caller's: it computes n.  A failed allocation leaves {nullptr, 0}.
// Reads like the pointer it holds (kernel arguments, copies, arithmetic); a capacity guard of a GROUP of buffers
// (max_q, DbStore::cap ...) is a fact about the group and stays with the group, written after every member has its size.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

namespace mh {

struct DeviceMem {
  static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t put(void* p) { return hipHostFree(p); }
};

template <typename T, typename Mem = DeviceMem>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  hipError_t ensure(size_t n, hipStream_t s) {
    if (n <= cap) return hipSuccess;
    if (p) {
      const hipError_t e = hipStreamSynchronize(s);   // work in flight may still read the old block
      if (e != hipSuccess) return e;
      reset();
    }
    void* q = nullptr;
    const hipError_t e = Mem::get(&q, n * sizeof(T));
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q);
    cap = n;
    return hipSuccess;
  }

  void reset() {
    if (p) (void)Mem::put(p);
    p = nullptr;
    cap = 0;
  }

  operator T*() const { return p; }
  T* operator->() const { return p; }
};

template <typename T>
using PinBuf = DevBuf<T, PinnedMem>;

}  // namespace mh
