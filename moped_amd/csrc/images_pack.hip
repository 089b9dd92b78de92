// Frames with several cameras from device images (mh_frame_enqueue_images[_batch]): the hand-over from FEAT to MATCH.
//
// FEAT_SIFT_CPU::process appends image 0's keypoints, then image 1's, ... to ONE list and files every one under its
// imageIdx (FEAT_SIFT_CPU.hpp:80-107).  On the device FEAT leaves every image's list at a fixed stride of `cap` rows with
// its count in a word of its own (sift_into_batch), because no launch knows the counts of the others.  This kernel packs
// them: frame f's list = the first min(count, cap) rows of its image 0, then of its image 1, ..., the image index of
// every row beside it, the total in a device word -- without the host ever reading a count.
//
// A pure mover.  One workgroup takes 64 rows of a frame's packed list: a row's 512 bytes are read and written by 32
// consecutive lanes, 16 bytes each, and all 8 loads of a thread are issued before its first store.  Every workgroup
// works out the frame's (at most 8) offsets for itself -- 8 count words, an exclusive scan in registers; no launch in
// front, no atomics.  Rows past an image's count are neither read nor written.
#include "context.h"

namespace mh {

namespace {

constexpr int PACK_THREADS = 256;
constexpr int PACK_ROWS = 64;                                              // rows of the packed list per workgroup
constexpr int ROW_F4 = DIM / 4;                                            // 16-byte pieces of a row (32)
constexpr int PACK_PER_THREAD = PACK_ROWS * ROW_F4 / PACK_THREADS;         // 8
static_assert(PACK_ROWS * ROW_F4 % PACK_THREADS == 0 && PACK_ROWS <= PACK_THREADS, "workgroup shape");
static_assert(sizeof(DevCam) % 4 == 0, "the camera table is copied word by word");

// The value is in its registers HERE: the compiler otherwise sinks a load whose only use is a conditional store into
// that store's branch, and the thread's loads go out one by one, each waited for.
__device__ __forceinline__ void loaded(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

__global__ __launch_bounds__(PACK_THREADS) void images_pack_kernel(const ImagesPackArgs a) {
  const int f = blockIdx.y, t = threadIdx.x;
  const int n = a.n_images, cap = a.cap;
  // exclusive scan of the frame's clamped counts: off[i] = first packed row of image i, off[MH_MAX_IMAGES] = the total
  // (uniform over the workgroup; fully unrolled, so it stays in registers)
  int off[MH_MAX_IMAGES + 1];
  off[0] = 0;
#pragma unroll
  for (int i = 0; i < MH_MAX_IMAGES; ++i) {
    const int c = i < n ? min(max(a.scount[f * n + i], 0), cap) : 0;
    off[i + 1] = off[i] + c;
  }
  const int total = off[MH_MAX_IMAGES];
  if (blockIdx.x == 0) {   // the frame's head: its total, its images' clamped counts; frame 0 also sets the rig's table
    if (t == 0) a.totals[f] = total;
#pragma unroll
    for (int i = 0; i < MH_MAX_IMAGES; ++i)
      if (t == i && i < n) a.counts[f * n + i] = off[i + 1] - off[i];
    if (f == 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.cams);
      uint32_t* dst = reinterpret_cast<uint32_t*>(a.cams_dev);
      for (int w = t; w < n * (int)(sizeof(DevCam) / 4); w += PACK_THREADS) dst[w] = src[w];
    }
  }
  const int row0 = blockIdx.x * PACK_ROWS;
  if (row0 >= total) return;
  // image and source row of packed row r < total: the last image whose first row is not past r (an empty image shares
  // its offset with the next one and loses to it)
  auto locate = [&](int r, int& img) {
    int start = 0;
    img = 0;
#pragma unroll
    for (int i = 1; i < MH_MAX_IMAGES; ++i)
      if (r >= off[i]) {
        img = i;
        start = off[i];
      }
    return (size_t)(f * n + img) * cap + (size_t)(r - start);
  };
  const size_t frame_row0 = (size_t)f * n * cap;
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(a.sdesc);
  float4* __restrict__ d4 = reinterpret_cast<float4*>(a.desc) + frame_row0 * ROW_F4;
  float4 v[PACK_PER_THREAD];
#pragma unroll
  for (int i = 0; i < PACK_PER_THREAD; ++i) {
    // (a piece past the list's end reads the list's last row again and is not stored: no branch around the loads, so
    // that all of them are in flight together)
    const int e = i * PACK_THREADS + t, r = min(row0 + (e >> 5), total - 1);
    int img;
    v[i] = s4[locate(r, img) * ROW_F4 + (e & 31)];
  }
  // the rows' coordinates and image indices (8 and 4 bytes a row: a packed row's offset from its source is any number of
  // rows, so wider pieces would straddle images), the first 64 threads one row each
  const int r1 = row0 + t;
  const bool mine = t < PACK_ROWS && r1 < total;
  int img1;
  float2 p = reinterpret_cast<const float2*>(a.sxy)[locate(min(r1, total - 1), img1)];
#pragma unroll
  for (int i = 0; i < PACK_PER_THREAD; ++i) loaded(v[i]);
  asm volatile("" : "+v"(p.x), "+v"(p.y));
#pragma unroll
  for (int i = 0; i < PACK_PER_THREAD; ++i) {
    const int e = i * PACK_THREADS + t, r = row0 + (e >> 5);
    if (r < total) d4[(size_t)r * ROW_F4 + (e & 31)] = v[i];
  }
  if (mine) {
    reinterpret_cast<float2*>(a.uv)[frame_row0 + r1] = p;
    a.q_img[frame_row0 + r1] = img1;
  }
}

}  // namespace

void launch_images_pack(const ImagesPackArgs& a, int n_frames, hipStream_t s) {
  if (n_frames <= 0 || a.n_images <= 0 || a.cap <= 0) return;
  const int blocks = (a.n_images * a.cap + PACK_ROWS - 1) / PACK_ROWS;   // for the capacity: workgroups past the total leave at once
  hipLaunchKernelGGL(images_pack_kernel, dim3(blocks, n_frames), dim3(PACK_THREADS), 0, s, a);
}

}  // namespace mh
