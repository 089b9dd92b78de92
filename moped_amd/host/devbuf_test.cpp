// DevBuf / PinBuf (csrc/devbuf.h) on the CPU, under ASan + UBSan (`make devbuf_check`): the five runtime calls the
// type makes are defined HERE over malloc / free -- nothing of ROCm is linked -- so that every call is counted, a failure
// can be injected, and a double free or a leak is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "../csrc/devbuf.h"

namespace {

std::string g_log;      // one letter per call: M hipMalloc, F hipFree, H hipHostMalloc, h hipHostFree, S synchronise
long g_live = 0;        // blocks handed out and not yet returned
size_t g_last_bytes = 0;
int g_fail_next = 0;    // that many allocations fail from here on
hipStream_t g_last_stream = nullptr;

hipError_t stub_alloc(void** p, size_t bytes, char tag) {
  g_log += tag;
  if (g_fail_next > 0) {
    --g_fail_next;
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  g_last_bytes = bytes;
  ++g_live;
  return hipSuccess;
}

hipError_t stub_free(void* p, char tag) {
  g_log += tag;
  if (p) --g_live;
  std::free(p);
  return hipSuccess;
}

int g_failed = 0;
void check_at(bool ok, const char* what, int line) {
  if (ok) return;
  std::fprintf(stderr, "devbuf_test:%d: %s (calls so far: %s)\n", line, what, g_log.c_str());
  ++g_failed;
}
#define CHECK(cond) check_at((cond), #cond, __LINE__)

std::string take_log() {
  std::string s;
  s.swap(g_log);
  return s;
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, 'M'); }
hipError_t hipFree(void* p) { return stub_free(p, 'F'); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes, 'H'); }
hipError_t hipHostFree(void* p) { return stub_free(p, 'h'); }
hipError_t hipStreamSynchronize(hipStream_t s) {
  g_log += 'S';
  g_last_stream = s;
  return hipSuccess;
}
}

using mh::DevBuf;
using mh::PinBuf;

int main() {
  hipStream_t stream = reinterpret_cast<hipStream_t>(0x1000);   // (only ever handed back to the stub)

  {   // growth from empty: no synchronisation, exactly n elements; within the capacity: no call at all
    DevBuf<float> b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.ensure(0, stream) == hipSuccess && take_log() == "");
    CHECK(b.ensure(100, stream) == hipSuccess);
    CHECK(take_log() == "M" && g_last_bytes == 100 * sizeof(float) && b.p && b.cap == 100);
    float* const first = b.p;
    CHECK(b.ensure(100, stream) == hipSuccess && b.ensure(7, stream) == hipSuccess && take_log() == "");
    CHECK(b.p == first && b.cap == 100);
    first[99] = 1.f;   // (the whole block is ours)
    // growth of a held buffer: one synchronisation of the caller's stream, before the free
    CHECK(b.ensure(101, stream) == hipSuccess);
    CHECK(take_log() == "SFM" && g_last_stream == stream && g_last_bytes == 101 * sizeof(float) && b.cap == 101);
    float* q = b;   // reads like the pointer it holds
    CHECK(q == b.p && g_live == 1);
  }
  CHECK(take_log() == "F" && g_live == 0);

  {   // a failed allocation leaves {nullptr, 0} and returns the error; the next call succeeds
    DevBuf<int> b;
    g_fail_next = 1;
    CHECK(b.ensure(10, stream) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && take_log() == "M");
    CHECK(b.ensure(10, stream) == hipSuccess && b.cap == 10 && take_log() == "M");
    g_fail_next = 1;   // ... and of a held buffer: the old block is gone, nothing is held
    CHECK(b.ensure(20, stream) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && take_log() == "SFM");
    CHECK(g_live == 0);
    CHECK(b.ensure(5, stream) == hipSuccess && b.cap == 5 && take_log() == "M");
    b.reset();
    CHECK(b.p == nullptr && b.cap == 0 && take_log() == "F");
    b.reset();   // (of an empty buffer: no call)
    CHECK(take_log() == "");
  }
  CHECK(take_log() == "" && g_live == 0);

  {   // a move leaves the source empty, the memory is freed once
    DevBuf<unsigned char> a;
    CHECK(a.ensure(64, stream) == hipSuccess);
    unsigned char* const block = a.p;
    DevBuf<unsigned char> b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == block && b.cap == 64);
    DevBuf<unsigned char> c;
    CHECK(c.ensure(8, stream) == hipSuccess);
    c = std::move(b);   // (what c held goes first)
    CHECK(b.p == nullptr && b.cap == 0 && c.p == block && c.cap == 64 && take_log() == "MMF" && g_live == 1);
    DevBuf<unsigned char>& self = c;
    c = std::move(self);
    CHECK(c.p == block && c.cap == 64 && take_log() == "");
    CHECK(a.ensure(16, stream) == hipSuccess && take_log() == "M");   // a moved-from buffer is an empty one: no synchronisation
  }
  CHECK(take_log() == "FF" && g_live == 0);

  {   // the page-locked kind: the same rule through hipHostMalloc / hipHostFree
    struct Block {
      int head[4];
      double body[3];
    };
    PinBuf<Block> b;
    CHECK(b.ensure(1, stream) == hipSuccess && take_log() == "H" && g_last_bytes == sizeof(Block));
    b->head[3] = 7;
    CHECK(b.p[0].head[3] == 7);
    CHECK(b.ensure(2, stream) == hipSuccess && take_log() == "ShH" && b.cap == 2);
    g_fail_next = 1;
    CHECK(b.ensure(3, stream) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && take_log() == "ShH");
  }
  CHECK(take_log() == "" && g_live == 0);

  if (g_failed) return 1;
  std::printf("devbuf_test: no finding\n");
  return 0;
}
