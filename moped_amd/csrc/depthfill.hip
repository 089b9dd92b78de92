// moped3d's DEPTHFILL step on the device: DEPTH_FILL_EXACT_CPU::fillInScaled
// (moped3d/libmoped/src/depthfill/DEPTH_FILL_EXACT_CPU.hpp:268-349; config.hpp:39 ships (8, false)).
// The depth map [h][w][4] stays in HBM: its holes (z < 0) get the depth of a nearby valid pixel, x / y / norm are
// recomputed for them (:249-273), and the step's second output, the distance map that DEPTHMAP_PROP and
// CLUSTER_LINKAGE read, is written beside it -- no trip through the host for a frame whose depth map is already on
// the device.
//
// The fill itself (:176-243) is a FIFO wavefront over the DOWNSCALED map (80 x 60 for a 640 x 480 map): a source is
// pushed on from a pixel whether or not the pixel still belongs to it, improvements are strict, ties go to the first
// arrival -- the result depends on the queue order, so the queue is replayed as it is: ONE wavefront pops the
// elements one at a time, nine lanes look at the popped pixel's 3 x 3 neighbourhood (nine different pixels: the
// updates of one element do not interact), the pushes of an element go to the tail in (dy, dx) order by ballot +
// prefix count.  Everything the loop touches lives in LDS (best distance, source, validity, a circular queue), one
// pop is ~3 dependent LDS round trips.  The rest -- downscale, seeds in raster order, upsampling (nearest neighbour
// with the reference's late row advance, :80-82, or bilinear, :93-168), normalisation -- is parallel.
//
// That is MH_DEPTH_FILL_REPLAY, the default mode (mh_depth_fill_set_mode): downscaled maps of up to 8192 pixels.
// MH_DEPTH_FILL_LEVELS, further down, runs the same queue generation by generation with all 1024 threads, its state in
// the context's scratch: the same bytes, downscaled maps of up to 2^21 pixels.
#include <climits>

#include "context.h"

namespace mh {

namespace {

constexpr int DF_THREADS = 1024;
constexpr int DF_MAX_PIX = 8192;      // pixels of the downscaled map (LDS resident)
constexpr int DF_QUEUE = 16384;       // live queue entries (circular)

struct DfLds {
  float best[DF_MAX_PIX];
  unsigned short src[DF_MAX_PIX];
  unsigned char valid[DF_MAX_PIX];
  unsigned int queue[DF_QUEUE];   // (source << 16) | pixel
  int head, tail, overflow;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The maps of a batch, by value (mh_depth_fill_batch: one per frame), and where a frame's downscaled maps lie in the
// context's scratch: zfill / fdist, [dh][dw] the filled downscaled depths and the fill's distance map (times `scale`),
// DF_MAX_PIX floats each, frame after frame.  mh_depth_fill launches the same bodies through entry points that take
// its one map's pointers directly: its launches are what they were before there were batches.
struct DfMaps {
  float4* depth[MH_MAX_BATCH] = {};
  float* dist[MH_MAX_BATCH] = {};
};
constexpr size_t DF_FRAME_FLOATS = 2 * (size_t)DF_MAX_PIX;

// One workgroup: one map.  zfill / fdist: [dh][dw] the filled downscaled depths and the fill's distance map.
__device__ __forceinline__ void depth_fill_body(const float4* __restrict__ depth, int w, int h, int scale, int dw, int dh,
                                                float* __restrict__ zfill, float* __restrict__ fdist,
                                                int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  DfLds& L = *reinterpret_cast<DfLds*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = dw * dh;
  // nearest-neighbour downsample (:317-323), validity (:190), best distance 0 / 1e30 (:205)
  for (int p = tid; p < n; p += DF_THREADS) {
    const int y = p / dw, x = p - y * dw;
    const float z = depth[(size_t)(y * scale) * w + x * scale].z;
    zfill[p] = z;
    const bool v = z >= 0.f;
    L.valid[p] = v ? 1 : 0;
    L.best[p] = v ? 0.f : 1e30f;
    L.src[p] = (unsigned short)p;
  }
  if (tid == 0) {
    L.head = 0;
    L.tail = 0;
    L.overflow = 0;
  }
  __syncthreads();
  if (tid < 64) {
    // seeds in raster order (:200-204): valid pixels with a hole among their in-image neighbours
    int tail = 0;
    for (int p0 = 0; p0 < n; p0 += 64) {
      const int p = p0 + lane;
      bool seed = false;
      if (p < n && L.valid[p]) {
        const int y = p / dw, x = p - y * dw;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if (xx >= 0 && xx < dw && yy >= 0 && yy < dh && !L.valid[yy * dw + xx]) seed = true;
          }
      }
      const unsigned long long m = __ballot(seed);
      if (seed) L.queue[(tail + __popcll(m & ((1ull << lane) - 1ull))) & (DF_QUEUE - 1)] = ((unsigned)p << 16) | (unsigned)p;
      tail += __popcll(m);
    }
    wave_sync();   // (tail <= n <= DF_MAX_PIX < DF_QUEUE)
    // the queue, one element at a time (:215-241)
    const int dy = lane / 3 - 1, dx = lane - (lane / 3) * 3 - 1;   // lanes 0..8: dy outer, dx inner
    const float dil = (float)scale;
    int head = 0;
    while (head < tail) {
      const unsigned e = L.queue[head & (DF_QUEUE - 1)];
      ++head;
      const int s = (int)(e >> 16), q = (int)(e & 0xffffu);
      const int sy = s / dw, sx = s - sy * dw;
      const int qy = q / dw, qx = q - qy * dw;
      const int xp = qx + dx, yp = qy + dy;
      const int pp = yp * dw + xp;
      bool upd = false;
      float d = 0.f;
      if (lane < 9 && xp >= 0 && xp < dw && yp >= 0 && yp < dh && !L.valid[pp]) {
        d = __fmul_rn(sqrtf((float)((xp - sx) * (xp - sx) + (yp - sy) * (yp - sy))), dil);   // :227
        upd = d < L.best[pp];
      }
      const unsigned long long m = __ballot(upd);
      if (tail + __popcll(m) - head > DF_QUEUE) {   // the live part would no longer fit the ring: stop, flagged
        if (lane == 0) L.overflow = 1;
        break;
      }
      if (upd) {
        L.best[pp] = d;
        L.src[pp] = (unsigned short)s;
        L.queue[(tail + __popcll(m & ((1ull << lane) - 1ull))) & (DF_QUEUE - 1)] = ((unsigned)s << 16) | (unsigned)pp;
      }
      tail += __popcll(m);
      wave_sync();
    }
  }
  __syncthreads();
  if (tid == 0 && L.overflow) atomicOr(err, 1);
  for (int p = tid; p < n; p += DF_THREADS) {
    fdist[p] = L.best[p];
    if (!L.valid[p] && L.src[p] != p) zfill[p] = zfill[L.src[p]];   // setDepth(xp, yp, getDepth(x0, y0)): sources are valid pixels, never rewritten
  }
}
__global__ __launch_bounds__(DF_THREADS) void depth_fill_kernel(const float4* __restrict__ depth, int w, int h, int scale,
                                                                int dw, int dh, float* __restrict__ zfill,
                                                                float* __restrict__ fdist, int32_t* __restrict__ err) {
  depth_fill_body(depth, w, h, scale, dw, dh, zfill, fdist, err);
}
// ... one workgroup per frame (blockIdx.x)
__global__ __launch_bounds__(DF_THREADS) void depth_fill_batch_kernel(DfMaps maps, int w, int h, int scale, int dw, int dh,
                                                                      float* __restrict__ scratch, int32_t* __restrict__ err) {
  float* zfill = scratch + blockIdx.x * DF_FRAME_FLOATS;
  depth_fill_body(maps.depth[blockIdx.x], w, h, scale, dw, dh, zfill, zfill + DF_MAX_PIX, err);
}

// Upsampling + normalisation, one thread per pixel of the full map.
__device__ __forceinline__ void depth_fill_upscale_body(float4* __restrict__ depth, int w, int h, int scale, int dw, int dh,
                                                        int bilinear, const float* __restrict__ zfill,
                                                        const float* __restrict__ fdist, float k0, float k1, float k2,
                                                        float k3, float* __restrict__ dist_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const int uy = i / w, ux = i - uy * w;
  float4 px = depth[i];
  if (px.z >= 0.f) {   // valid: left alone, distance 0 (:306-308)
    dist_out[i] = 0.f;
    return;
  }
  float z, fd;
  if (!bilinear) {
    // NNInterp (:69-85): lx advances before the pixel, ly after the row
    const int lx = min(ux / scale, dw - 1);
    const int ly = min(uy == 0 ? 0 : (uy - 1) / scale, dh - 1);
    z = zfill[ly * dw + lx];
    fd = fdist[ly * dw + lx];
  } else {
    // bilinearInterp (:93-168): the influences are doubles that lose `delta` per pixel since the last multiple
    const double delta = 1.0 / scale;
    double up = 1, left = 1;
    for (int k = uy % scale; k > 0; --k) up -= delta;
    for (int k = ux % scale; k > 0; --k) left -= delta;
    int x0 = ux / scale, y0 = uy / scale, x1 = x0 + 1, y1 = y0 + 1;
    float w00 = (float)(left * up), w01 = (float)(left * (1 - up)), w10 = (float)((1 - left) * up),
          w11 = (float)((1 - left) * (1 - up));
    if (x1 == dw) {
      w00 = __fadd_rn(w00, w01); w01 = 0.f;
      w01 = __fadd_rn(w01, w11); w11 = 0.f;
      x1 = x0;
    }
    if (y1 == dh) {
      w00 = __fadd_rn(w00, w10); w10 = 0.f;
      w10 = __fadd_rn(w10, w11); w11 = 0.f;
      y1 = y0;
    }
    x0 = min(x0, dw - 1); x1 = min(x1, dw - 1); y0 = min(y0, dh - 1); y1 = min(y1, dh - 1);
    auto mix = [&](const float* m) {
      float r = __fmul_rn(w00, m[y0 * dw + x0]);
      r = __fadd_rn(r, __fmul_rn(w01, m[y1 * dw + x0]));
      r = __fadd_rn(r, __fmul_rn(w10, m[y0 * dw + x1]));
      return __fadd_rn(r, __fmul_rn(w11, m[y1 * dw + x1]));
    };
    z = mix(zfill);
    fd = mix(fdist);
  }
  // normalizeDepthmap (:249-273)
  const float x = __fmul_rn(__fdiv_rn(__fsub_rn((float)ux, k2), k0), z);
  const float y = __fmul_rn(__fdiv_rn(__fsub_rn((float)uy, k3), k1), z);
  px.x = x;
  px.y = y;
  px.z = z;
  px.w = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
  depth[i] = px;
  dist_out[i] = fd;
}
__global__ void depth_fill_upscale_kernel(float4* __restrict__ depth, int w, int h, int scale, int dw, int dh, int bilinear,
                                          const float* __restrict__ zfill, const float* __restrict__ fdist, float k0, float k1,
                                          float k2, float k3, float* __restrict__ dist_out) {
  depth_fill_upscale_body(depth, w, h, scale, dw, dh, bilinear, zfill, fdist, k0, k1, k2, k3, dist_out);
}
// ... blockIdx.y = frame
__global__ void depth_fill_upscale_batch_kernel(DfMaps maps, int w, int h, int scale, int dw, int dh, int bilinear,
                                                const float* __restrict__ scratch, float k0, float k1, float k2, float k3) {
  const float* zfill = scratch + blockIdx.y * DF_FRAME_FLOATS;
  depth_fill_upscale_body(maps.depth[blockIdx.y], w, h, scale, dw, dh, bilinear, zfill, zfill + DF_MAX_PIX, k0, k1, k2, k3,
                          maps.dist[blockIdx.y]);
}

__global__ void depth_fill_scale1_kernel(const float* __restrict__ fdist, int n, float* __restrict__ dist_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dist_out[i] = fdist[i];
}
__global__ void depth_fill_scale1_batch_kernel(DfMaps maps, const float* __restrict__ scratch, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) maps.dist[blockIdx.y][i] = scratch[blockIdx.y * DF_FRAME_FLOATS + DF_MAX_PIX + i];
}

__global__ void depth_count_valid_kernel(const float4* __restrict__ depth, int n, int32_t* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool v = i < n && depth[i].z >= 0.f;
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

// ---- MH_DEPTH_FILL_LEVELS: the same queue, generation by generation ---------------------------------------------------
// The queue is FIFO: seeds are generation 0, what a generation-k element pushes is generation k + 1, and every element of
// generation k is popped before any of k + 1.  Within a generation best[t] / src[t] are touched only by the elements
// that target t, so ONE thread per target pixel t goes through t's candidates -- the elements on the (up to) nine pixels
// of its neighbourhood -- in the order of their queue positions i and finds the records (strictly below best[t] and below
// every earlier candidate): those are t's pushes.  The pushes of element i through neighbour slot j land at
// exscan_i(popcount(mask[i])) + popcount(mask[i] & ((1 << j) - 1)), the order of the serial loop, so the next generation
// is the same queue as the replay's and the results are its results bit for bit.
//
// Per frame, in the context's scratch (n = dw * dh, cap = DF_LV_CAP * n elements per generation):
//   zfill, best [n]              downscaled depths; the distance map (fdist of the upsampling)
//   src, tstamp [n]              the source of a filled hole; the last generation the pixel was listed as a target for
//   sstamp, sstart, scnt [2][n]  per parity of the generation: the pixel carries elements of generation sstamp, they are
//                                entries [sstart, sstart + scnt) of that parity's gpos / gsrc, ascending in position
//   act [2][n]                   the target pixels of the generation (any order)
//   gpos, gsrc [2][cap]          the elements, grouped by pixel: queue position within the generation, source
//   mb [cap]                     by queue position: the 9-bit mask of record slots, after the scan | (exclusive sum << 9)
// A generation of more than cap elements, or more than n generations, sets the sticky overflow word and ends the fill;
// nothing is written past cap.
constexpr int DF_LV_CAP = 4;                    // elements per generation, in downscaled pixels
constexpr long DF_LV_MAX_PIX = 1l << 21;        // (cap = 2^23 positions: position << 9 | mask is one word)
constexpr size_t DF_LV_HEAD = 64 + 16 * (size_t)MH_MAX_BATCH;   // [overflow word, valid count | int32[4] of stats per frame]
constexpr size_t df_lv_frame_words(size_t n) { return (12 + 5 * (size_t)DF_LV_CAP) * n; }

struct LvFrame {
  float *zfill, *best;
  int *src, *tstamp, *sstamp, *sstart, *scnt, *act, *gpos, *gsrc;
  unsigned* mb;
  int n, cap;
};
__device__ __forceinline__ LvFrame lv_frame(float* base, int n) {
  LvFrame F;
  F.n = n;
  F.cap = DF_LV_CAP * n;
  F.zfill = base;
  F.best = base + n;
  int* w = reinterpret_cast<int*>(base) + 2 * (size_t)n;
  F.src = w;
  F.tstamp = w + (size_t)n;
  F.sstamp = w + 2 * (size_t)n;
  F.sstart = w + 4 * (size_t)n;
  F.scnt = w + 6 * (size_t)n;
  F.act = w + 8 * (size_t)n;
  F.gpos = w + 10 * (size_t)n;
  F.gsrc = F.gpos + 2 * (size_t)F.cap;
  F.mb = reinterpret_cast<unsigned*>(F.gsrc + 2 * (size_t)F.cap);
  return F;
}

struct LvLds {
  int wsum[DF_THREADS / 64];
  int na_next, gtail;
};

// Exclusive sum of v over the workgroup's threads, `total` = the sum (two barriers).
__device__ __forceinline__ int lv_block_exscan(int v, LvLds& L, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();   // (the last call's readers are done with wsum)
  if (lane == 63) L.wsum[wv] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int k = 0; k < DF_THREADS / 64; ++k) {
    const int s = L.wsum[k];
    if (k < wv) off += s;
    tot += s;
  }
  total = tot;
  return off + inc - v;
}

// mb[0, m): mask -> mask | (exclusive sum of popcount(mask) << 9); -> the sum.  Every thread a contiguous chunk.
__device__ __forceinline__ int lv_scan_masks(unsigned* mb, int m, LvLds& L) {
  const int per = (m + DF_THREADS - 1) / DF_THREADS;
  const int lo = min((int)threadIdx.x * per, m), hi = min(lo + per, m);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += __popc(mb[i] & 0x1ffu);
  int total;
  unsigned run = (unsigned)lv_block_exscan(sum, L, total);
  for (int i = lo; i < hi; ++i) {
    const unsigned m9 = mb[i] & 0x1ffu;
    mb[i] = (run << 9) | m9;
    run += __popc(m9);
  }
  return total;
}

// Pixel u becomes a target of generation g (once: the first to raise its stamp lists it).  At most n distinct pixels.
__device__ __forceinline__ void lv_mark_targets(const LvFrame& F, int par, int g, int t, int dw, int dh, LvLds& L) {
  const int ty = t / dw, tx = t - ty * dw;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int ux = tx + dx, uy = ty + dy;
      if (ux < 0 || ux >= dw || uy < 0 || uy >= dh) continue;
      const int u = uy * dw + ux;
      if (F.zfill[u] >= 0.f) continue;   // valid pixels are never targets (:220)
      if (atomicMax(&F.tstamp[u], g) < g) {
        const int a = atomicAdd(&L.na_next, 1);
        if (a < F.n) F.act[(size_t)par * F.n + a] = u;
      }
    }
}

// The candidates of target t in generation k (parity par), in the order of their positions: a nine-way merge of the
// neighbourhood's element lists.  WRITE = false: marks the records in mb, -> their number.  WRITE = true (after the scan):
// writes them as t's elements of generation k + 1 from entry `out` on, and t's new best / src.
template <bool WRITE>
__device__ __forceinline__ int lv_walk(const LvFrame& F, int par, int k, int t, int dw, int dh, float dil, int out) {
  const int ty = t / dw, tx = t - ty * dw;
  const int* gpos = F.gpos + (size_t)par * F.cap;
  const int* gsrc = F.gsrc + (size_t)par * F.cap;
  int beg[9], end[9], hp[9];
  int todo = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int qx = tx - (j % 3 - 1), qy = ty - (j / 3 - 1);   // q + (dx, dy) = t through slot j = 3 (dy + 1) + (dx + 1)
    beg[j] = end[j] = 0;
    hp[j] = INT_MAX;
    if (qx >= 0 && qx < dw && qy >= 0 && qy < dh) {
      const size_t q = (size_t)par * F.n + (qy * dw + qx);
      if (F.sstamp[q] == k) {
        beg[j] = F.sstart[q];
        end[j] = min(beg[j] + F.scnt[q], F.cap);
        if (beg[j] < end[j]) hp[j] = gpos[beg[j]];
        todo += max(end[j] - beg[j], 0);
      }
    }
  }
  float cb = F.best[t];
  int cs = -1, rc = 0;
  for (int it = 0; it < todo; ++it) {
    int jm = 0, pm = hp[0], bm = beg[0];
#pragma unroll
    for (int j = 1; j < 9; ++j)
      if (hp[j] < pm) {
        pm = hp[j];
        jm = j;
        bm = beg[j];
      }
    if (pm == INT_MAX) break;
    const int s = gsrc[bm];
    const int sy = s / dw, sx = s - sy * dw;
    const long long ddx = tx - sx, ddy = ty - sy;
    const float d = __fmul_rn(sqrtf((float)(ddx * ddx + ddy * ddy)), dil);   // :224
    if (d < cb) {
      cb = d;
      cs = s;
      if (!WRITE) {
        if ((unsigned)pm < (unsigned)F.cap) atomicOr(&F.mb[pm], 1u << jm);
      } else {
        const unsigned w = (unsigned)pm < (unsigned)F.cap ? F.mb[pm] : 0u;
        const int e = out + rc;
        if ((unsigned)e < (unsigned)F.cap) {
          F.gpos[(size_t)(par ^ 1) * F.cap + e] = (int)(w >> 9) + __popc(w & ((1u << jm) - 1u));
          F.gsrc[(size_t)(par ^ 1) * F.cap + e] = s;
        }
      }
      ++rc;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (j == jm) {
        ++beg[j];
        hp[j] = beg[j] < end[j] ? gpos[beg[j]] : INT_MAX;
      }
  }
  if (WRITE && cs >= 0) {
    F.best[t] = cb;
    F.src[t] = cs;
  }
  return rc;
}

// One workgroup: the map of frame blockIdx.x.  stats[frame]: {non-empty generations, largest, elements, overflowed}.
__global__ __launch_bounds__(DF_THREADS) void depth_fill_levels_kernel(DfMaps maps, int w, int h, int scale, int dw, int dh,
                                                                       float* scratch, size_t frame_words, int32_t* err,
                                                                       int32_t* stats) {
  __shared__ LvLds L;
  const int tid = threadIdx.x;
  const int n = dw * dh;
  const float4* depth = maps.depth[blockIdx.x];
  const LvFrame F = lv_frame(scratch + blockIdx.x * frame_words, n);
  for (int p = tid; p < n; p += DF_THREADS) {
    const int y = p / dw, x = p - y * dw;
    const float z = depth[(size_t)(y * scale) * w + x * scale].z;
    F.zfill[p] = z;
    F.best[p] = z >= 0.f ? 0.f : 1e30f;
    F.src[p] = p;
    F.tstamp[p] = -1;
    F.sstamp[p] = -1;
    F.sstamp[n + p] = -1;
  }
  if (tid == 0) {
    L.na_next = 0;
    L.gtail = 0;
  }
  __syncthreads();
  // generation 0: the seeds in raster order (:194-198), valid pixels with a hole among their in-image neighbours
  for (int p = tid; p < n; p += DF_THREADS) {
    bool seed = false;
    if (F.zfill[p] >= 0.f) {
      const int y = p / dw, x = p - y * dw;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx, yy = y + dy;
          if (xx >= 0 && xx < dw && yy >= 0 && yy < dh && !(F.zfill[yy * dw + xx] >= 0.f)) seed = true;
        }
    }
    F.mb[p] = seed ? 1u : 0u;
  }
  __syncthreads();
  int n_k = lv_scan_masks(F.mb, n, L);
  __syncthreads();
  for (int p = tid; p < n; p += DF_THREADS) {
    const unsigned m = F.mb[p];
    if (m & 1u) {
      const int pos = (int)(m >> 9);
      F.gpos[pos] = pos;
      F.gsrc[pos] = p;
      F.sstart[p] = pos;
      F.scnt[p] = 1;
      F.sstamp[p] = 0;
      lv_mark_targets(F, 0, 0, p, dw, dh, L);
    }
  }
  __syncthreads();
  for (int p = tid; p < n; p += DF_THREADS) F.mb[p] = 0u;
  int na = min(L.na_next, n);
  __syncthreads();
  if (tid == 0) L.na_next = 0;
  __syncthreads();

  const float dil = (float)scale;
  int gens = 0, largest = 0, overflow = 0;
  long long elements = 0;
  for (int k = 0; n_k > 0; ++k) {
    if (k >= n) {   // (no map should come here: every generation improves a pixel)
      overflow = 1;
      break;
    }
    ++gens;
    largest = max(largest, n_k);
    elements += n_k;
    const int par = k & 1;
    const int* act = F.act + (size_t)par * n;
    // A: records of every target, marked by queue position and slot; room for them as the target's next elements
    for (int a = tid; a < na; a += DF_THREADS) {
      const int t = act[a];
      const int rc = lv_walk<false>(F, par, k, t, dw, dh, dil, 0);
      if (rc) {
        const size_t o = (size_t)(par ^ 1) * n + t;
        F.sstart[o] = atomicAdd(&L.gtail, rc);
        F.scnt[o] = rc;
        F.sstamp[o] = k + 1;
      }
    }
    __syncthreads();
    // B: positions in generation k + 1
    const int n_next = lv_scan_masks(F.mb, n_k, L);
    if (n_next > F.cap) {
      overflow = 1;
      break;
    }
    __syncthreads();
    // C: the records again, now with their positions; the targets of generation k + 1 are their neighbours
    for (int a = tid; a < na; a += DF_THREADS) {
      const int t = act[a];
      const size_t o = (size_t)(par ^ 1) * n + t;
      if (F.sstamp[o] != k + 1) continue;
      lv_walk<true>(F, par, k, t, dw, dh, dil, F.sstart[o]);
      lv_mark_targets(F, par ^ 1, k + 1, t, dw, dh, L);
    }
    __syncthreads();
    for (int i = tid; i < max(n_k, n_next); i += DF_THREADS) F.mb[i] = 0u;
    na = min(L.na_next, n);
    n_k = n_next;
    __syncthreads();
    if (tid == 0) {
      L.na_next = 0;
      L.gtail = 0;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    if (overflow) atomicOr(err, 1);
    int32_t* st = stats + 4 * blockIdx.x;
    st[0] = gens;
    st[1] = largest;
    st[2] = (int32_t)min(elements, (long long)INT_MAX);
    st[3] = overflow;
  }
  for (int p = tid; p < n; p += DF_THREADS)
    if (!(F.zfill[p] >= 0.f) && F.src[p] != p) F.zfill[p] = F.zfill[F.src[p]];   // (sources are valid pixels, never rewritten)
}

// Upsampling / the scale-1 copy from the LEVELS layout (blockIdx.y = frame; zfill, fdist = the frame's first 2 n words)
__global__ void depth_fill_upscale_levels_kernel(DfMaps maps, int w, int h, int scale, int dw, int dh, int bilinear,
                                                 const float* __restrict__ scratch, size_t frame_words, float k0, float k1,
                                                 float k2, float k3) {
  const float* zfill = scratch + blockIdx.y * frame_words;
  depth_fill_upscale_body(maps.depth[blockIdx.y], w, h, scale, dw, dh, bilinear, zfill, zfill + (size_t)dw * dh, k0, k1, k2, k3,
                          maps.dist[blockIdx.y]);
}
__global__ void depth_fill_scale1_levels_kernel(DfMaps maps, const float* __restrict__ scratch, size_t frame_words, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) maps.dist[blockIdx.y][i] = scratch[blockIdx.y * frame_words + n + i];
}

// The context's scratch, `bytes` behind its 64 bytes of status words.  Growing a held block synchronises the stream
// (DevBuf::ensure) and would lose the sticky overflow word: it is carried over.
int df_scratch_bytes(mh_ctx* ctx, size_t bytes);
// ... for `frames` frames of the replay: [overflow word, valid count | the frames' downscaled maps]
int df_scratch(mh_ctx* ctx, int frames) { return df_scratch_bytes(ctx, sizeof(float) * DF_FRAME_FLOATS * (size_t)frames); }
int df_scratch_bytes(mh_ctx* ctx, size_t bytes) {
  hipStream_t s = ctx->stream;
  const size_t need = 64 + bytes;
  if (ctx->df_buf.cap >= need) return MH_OK;
  int32_t word = 0;
  if (ctx->df_buf) {
    MH_HIP(ctx, hipMemcpyAsync(&word, ctx->df_buf, sizeof word, hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipStreamSynchronize(s));
  }
  MH_HIP(ctx, ctx->df_buf.ensure(need, s));
  MH_HIP(ctx, hipMemsetAsync(ctx->df_buf, 0, 64, s));
  if (word) {
    MH_HIP(ctx, hipMemcpyAsync(ctx->df_buf, &word, sizeof word, hipMemcpyHostToDevice, s));
    MH_HIP(ctx, hipStreamSynchronize(s));   // (`word` leaves scope)
  }
  return MH_OK;
}

// FILL + upsampling at a fixed scale >= 1, one launch per stage: of the one map (depth, dist), or -- batch != nullptr --
// of the table's n_frames maps of one size.
int df_launch(mh_ctx* ctx, const char* who, float4* depth, float* dist, const DfMaps* batch, int n_frames, int width, int height,
              int scale, int bilinear, const float K[4]) {
  const int dw = width / scale, dh = height / scale;
  if (dw < 1 || dh < 1) {
    ctx->err = std::string(who) + ": scale factor larger than the map";
    return MH_ERR_ARG;
  }
  if (ctx->df_mode == MH_DEPTH_FILL_LEVELS) {
    ctx->df_lv_frames = 0;   // (until the launches below are out: a refused or failed call leaves no stats to read)
    const long n = (long)dw * dh;
    if (n > DF_LV_MAX_PIX) {
      ctx->err = std::string(who) + ": the downscaled map has more than 2^21 pixels";
      return MH_ERR_CAPACITY;
    }
    // the scratch follows the map size and the frame count: it may grow here, before the launches (that synchronises)
    const size_t frame_words = df_lv_frame_words((size_t)n);
    if (int rc = df_scratch_bytes(ctx, DF_LV_HEAD - 64 + sizeof(float) * frame_words * (size_t)n_frames)) return rc;
    hipStream_t s = ctx->stream;
    const int n_full = width * height;
    int32_t* words = reinterpret_cast<int32_t*>(ctx->df_buf.p);
    int32_t* stats = reinterpret_cast<int32_t*>(ctx->df_buf + 64);
    float* scratch = reinterpret_cast<float*>(ctx->df_buf + DF_LV_HEAD);
    DfMaps one;
    if (!batch) {
      one.depth[0] = depth;
      one.dist[0] = dist;
      batch = &one;
    }
    hipLaunchKernelGGL(depth_fill_levels_kernel, dim3(n_frames), dim3(DF_THREADS), 0, s, *batch, width, height, scale, dw, dh,
                       scratch, frame_words, words, stats);
    const dim3 grid((n_full + 255) / 256, n_frames);
    if (scale == 1)
      hipLaunchKernelGGL(depth_fill_scale1_levels_kernel, grid, dim3(256), 0, s, *batch, scratch, frame_words, n_full);
    else
      hipLaunchKernelGGL(depth_fill_upscale_levels_kernel, grid, dim3(256), 0, s, *batch, width, height, scale, dw, dh,
                         bilinear ? 1 : 0, scratch, frame_words, K[0], K[1], K[2], K[3]);
    MH_HIP(ctx, hipGetLastError());
    ctx->df_lv_frames = n_frames;
    return MH_OK;
  }
  if ((long)dw * dh > DF_MAX_PIX) {
    ctx->err = std::string(who) + ": the downscaled map has more than 8192 pixels (the fill is LDS resident)";
    return MH_ERR_CAPACITY;
  }
  ctx->df_lv_frames = 0;   // (the replay's maps lie where the stats were)
  hipStream_t s = ctx->stream;
  const int n_full = width * height;
  int32_t* words = reinterpret_cast<int32_t*>(ctx->df_buf.p);
  float* scratch = reinterpret_cast<float*>(ctx->df_buf + 64);
  if (!batch) {
    float* zfill = scratch;
    float* fdist = zfill + DF_MAX_PIX;
    static DynLds attr;
    attr.ensure(depth_fill_kernel, sizeof(DfLds));
    hipLaunchKernelGGL(depth_fill_kernel, dim3(1), dim3(DF_THREADS), sizeof(DfLds), s, depth, width, height, scale, dw, dh, zfill,
                       fdist, words);
    if (scale == 1)   // :336-338: the filled map never reaches the frame, the distance map does
      hipLaunchKernelGGL(depth_fill_scale1_kernel, dim3((n_full + 255) / 256), dim3(256), 0, s, fdist, n_full, dist);
    else
      hipLaunchKernelGGL(depth_fill_upscale_kernel, dim3((n_full + 255) / 256), dim3(256), 0, s, depth, width, height, scale, dw,
                         dh, bilinear ? 1 : 0, zfill, fdist, K[0], K[1], K[2], K[3], dist);
  } else {
    static DynLds attr;
    attr.ensure(depth_fill_batch_kernel, sizeof(DfLds));
    hipLaunchKernelGGL(depth_fill_batch_kernel, dim3(n_frames), dim3(DF_THREADS), sizeof(DfLds), s, *batch, width, height, scale,
                       dw, dh, scratch, words);
    const dim3 grid((n_full + 255) / 256, n_frames);
    if (scale == 1)
      hipLaunchKernelGGL(depth_fill_scale1_batch_kernel, grid, dim3(256), 0, s, *batch, scratch, n_full);
    else
      hipLaunchKernelGGL(depth_fill_upscale_batch_kernel, grid, dim3(256), 0, s, *batch, width, height, scale, dw, dh,
                         bilinear ? 1 : 0, scratch, K[0], K[1], K[2], K[3]);
  }
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

}  // namespace

}  // namespace mh

using namespace mh;

extern "C" int mh_depth_fill(mh_ctx* ctx, float* depth_xyzn_dev, int width, int height, int scale_factor, int bilinear,
                             const float K[4], float* fill_distance_dev, int* scale_used) {
  if (!ctx) return MH_ERR_ARG;
  if (!depth_xyzn_dev || !fill_distance_dev || !K || width <= 0 || height <= 0 || (scale_factor < 1 && scale_factor != -1)) {
    ctx->err = "mh_depth_fill: bad arguments";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_stream(ctx)) return rc;
  hipStream_t s = ctx->stream;
  const int n_full = width * height;
  // the context's own scratch (the status outlives the call)
  if (int rc = df_scratch(ctx, 1)) return rc;
  int32_t* words = reinterpret_cast<int32_t*>(ctx->df_buf.p);
  int scale = scale_factor;   // (the overflow word words[0] is sticky until mh_depth_fill_status reads it)
  if (scale == -1) {   // :283-296: the factor follows the share of holes (one small reduction + a 4-byte read)
    MH_HIP(ctx, hipMemsetAsync(words + 1, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(depth_count_valid_kernel, dim3((n_full + 255) / 256), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(depth_xyzn_dev), n_full, words + 1);
    int32_t valid_count = 0;
    MH_HIP(ctx, hipMemcpyAsync(&valid_count, words + 1, sizeof valid_count, hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipStreamSynchronize(s));
    const float invalid_ratio = ((float)width * height - valid_count) / (width * height);
    scale = invalid_ratio < 0.1 ? 1 : invalid_ratio < 0.2 ? 2 : invalid_ratio < 0.4 ? 4 : invalid_ratio < 0.6 ? 8 : 16;
  }
  if (int rc = df_launch(ctx, "mh_depth_fill", reinterpret_cast<float4*>(depth_xyzn_dev), fill_distance_dev, nullptr, 1, width,
                         height, scale, bilinear, K))
    return rc;
  if (scale_used) *scale_used = scale;
  return MH_OK;
}

extern "C" int mh_depth_fill_batch(mh_ctx* ctx, float* const* depth_xyzn_dev, float* const* fill_distance_dev, int n_frames,
                                   int width, int height, int scale_factor, int bilinear, const float K[4]) {
  if (!ctx) return MH_ERR_ARG;
  if (scale_factor == -1) {
    ctx->err = "mh_depth_fill_batch: the automatic factor needs a read-back per map (mh_depth_fill takes -1, one map per call)";
    return MH_ERR_ARG;
  }
  bool ok = depth_xyzn_dev && fill_distance_dev && K && n_frames >= 1 && n_frames <= MH_MAX_BATCH && width > 0 && height > 0 &&
            scale_factor >= 1;
  for (int f = 0; ok && f < n_frames; ++f) ok = depth_xyzn_dev[f] && fill_distance_dev[f];
  if (!ok) {
    ctx->err = "mh_depth_fill_batch: bad arguments";
    return MH_ERR_ARG;
  }
  // the frames are filled in place side by side: a map handed in twice would have one frame read what the other has filled
  for (int f = 1; f < n_frames; ++f)
    for (int g = 0; g < f; ++g)
      if (depth_xyzn_dev[f] == depth_xyzn_dev[g] || fill_distance_dev[f] == fill_distance_dev[g]) {
        ctx->err = "mh_depth_fill_batch: the same depth or distance map for two frames (every frame needs buffers of its own)";
        return MH_ERR_ARG;
      }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_stream(ctx)) return rc;
  // the replay: room for MH_MAX_BATCH frames from the first batch on, so no later batch regrows the block behind one in
  // flight.  MH_DEPTH_FILL_LEVELS sizes the block in df_launch from the map and n_frames: a larger batch regrows it there.
  if (ctx->df_mode != MH_DEPTH_FILL_LEVELS)
    if (int rc = df_scratch(ctx, MH_MAX_BATCH)) return rc;
  DfMaps maps;
  for (int f = 0; f < n_frames; ++f) {
    maps.depth[f] = reinterpret_cast<float4*>(depth_xyzn_dev[f]);
    maps.dist[f] = fill_distance_dev[f];
  }
  return df_launch(ctx, "mh_depth_fill_batch", nullptr, nullptr, &maps, n_frames, width, height, scale_factor, bilinear, K);
}

extern "C" int mh_depth_fill_set_mode(mh_ctx* ctx, int mode) {
  if (!ctx || (mode != MH_DEPTH_FILL_REPLAY && mode != MH_DEPTH_FILL_LEVELS)) return MH_ERR_ARG;
  ctx->df_mode = mode;
  return MH_OK;
}

extern "C" int mh_depth_fill_get_mode(mh_ctx* ctx, int* mode) {
  if (!ctx || !mode) return MH_ERR_ARG;
  *mode = ctx->df_mode;
  return MH_OK;
}

extern "C" int mh_depth_fill_stats(mh_ctx* ctx, int frame, int32_t out[4]) {
  if (!ctx || !out) return MH_ERR_ARG;
  if (!ctx->df_buf || frame < 0 || frame >= ctx->df_lv_frames) {
    ctx->err = "mh_depth_fill_stats: no MH_DEPTH_FILL_LEVELS fill of that frame since the last fill of the other mode";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_stream(ctx)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(out, ctx->df_buf + 64 + 16 * (size_t)frame, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

extern "C" int mh_depth_fill_status(mh_ctx* ctx) {
  if (!ctx) return MH_ERR_ARG;
  if (!ctx->df_buf) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_stream(ctx)) return rc;
  int32_t word = 0;
  MH_HIP(ctx, hipMemcpyAsync(&word, ctx->df_buf, sizeof word, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (word) {
    MH_HIP(ctx, hipMemsetAsync(ctx->df_buf, 0, sizeof(int32_t), ctx->stream));
    // (df_lv_frames: the last fill was a MH_DEPTH_FILL_LEVELS one; the default mode keeps the text it always had)
    ctx->err = ctx->df_lv_frames
                   ? "mh_depth_fill: a generation of the fill outgrew 4 * dw * dh elements, or the fill dw * dh generations "
                     "(MH_DEPTH_FILL_LEVELS; the maps of that call are incomplete)"
                   : "mh_depth_fill: the fill's queue outgrew its ring (the maps of that call are incomplete)";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

extern "C" int mh_depth_fill_host(mh_ctx* ctx, float* depth_xyzn_host, int width, int height, int scale_factor, int bilinear,
                                  const float K[4], float* fill_distance_host, int* scale_used) {
  if (!ctx) return MH_ERR_ARG;
  if (!depth_xyzn_host || !fill_distance_host || width <= 0 || height <= 0) {
    ctx->err = "mh_depth_fill_host: bad arguments";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_stream(ctx)) return rc;
  const size_t px = (size_t)width * height;
  if (int rc = ensure_own_depth(ctx, px)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_depth, depth_xyzn_host, px * 4 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = mh_depth_fill(ctx, ctx->own_depth, width, height, scale_factor, bilinear, K, ctx->own_fill, scale_used)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(depth_xyzn_host, ctx->own_depth, px * 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(fill_distance_host, ctx->own_fill, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  return mh_depth_fill_status(ctx);   // (synchronises the stream)
}
