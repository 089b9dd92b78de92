// Two-stage MATCH (match_screen.hip): the f16 images the screen multiplies -- the DB's, made at upload with the rows'
// -dd/2 terms and the statistics the error model needs, and a frame's queries -- and the screen values themselves for tests.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "screen_int.h"

MH_TRACE_TU()

namespace mh {

namespace {

// DB: [n_pad][128] f16 (round to nearest), dneg[n_pad] = -dd/2, + statistics over the real rows: max dd, max |x|, any non-finite dd.
__global__ __launch_bounds__(256) void db_to_half_kernel(const float* __restrict__ db, const float* __restrict__ dnorm, int N,
                                                         size_t n_chunks, _Float16* __restrict__ dbh, float* __restrict__ dneg,
                                                         unsigned int* __restrict__ stats) {
  __shared__ unsigned int red[3];
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  __syncthreads();
  float x_max = 0.f, dd_max = 0.f;
  unsigned int bad = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_chunks; i += (size_t)gridDim.x * blockDim.x) {   // one 8-element chunk
    const float4 a = reinterpret_cast<const float4*>(db)[2 * i], b = reinterpret_cast<const float4*>(db)[2 * i + 1];
    half8 h;
    h[0] = (_Float16)a.x; h[1] = (_Float16)a.y; h[2] = (_Float16)a.z; h[3] = (_Float16)a.w;
    h[4] = (_Float16)b.x; h[5] = (_Float16)b.y; h[6] = (_Float16)b.z; h[7] = (_Float16)b.w;
    reinterpret_cast<half8*>(dbh)[i] = h;
    const int row = (int)(i >> 4);
    if ((i & 15) == 0) dneg[(size_t)(row >> 7) * SC_DD + (row & 127)] = -0.5f * dnorm[row];   // the rows' -dd/2; -inf on padding rows
    if (row < N) {
      // (fmaxf drops NaNs: a NaN coordinate shows in the row's norm term)
      x_max = fmaxf(x_max, fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                                 fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w)))));
      if ((i & 15) == 0) {
        const float dd = dnorm[row];
        if (!(dd >= 0.f) || dd == __builtin_inff()) bad = 1;
        else dd_max = fmaxf(dd_max, dd);
      }
    }
  }
  // non-negative floats order like their bit patterns
  atomicMax(&red[0], __float_as_uint(dd_max));
  atomicMax(&red[1], __float_as_uint(x_max));
  if (bad) atomicOr(&red[2], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMax(&stats[0], red[0]);
    atomicMax(&stats[1], red[1]);
    if (red[2]) atomicOr(&stats[2], 1u);
  }
}

// Per 32-row block the largest and the smallest of its rows' -dd/2 (entries 128..131 and 132..135 of the tile's part of
// the array): dot + largest >= every row's screen value >= dot + smallest.  Pass B works on the dots alone and
// decides with the block's largest term (a superset of the rows above the threshold: for the L2-normalised rows of a
// MOPED database the two differ in the last bit); pass C reads both to turn a record's value into bounds.
__global__ void db_block_bounds_kernel(const float* __restrict__ dnorm, int N, int n_tiles, float* __restrict__ dneg,
                                       unsigned int* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;   // 32-row block
  if (b >= n_tiles * 4) return;
  float hi = -__builtin_inff(), lo = __builtin_inff();
  for (int r = 0; r < 32; ++r) {
    const int row = b * 32 + r;
    const float v = row < N ? -0.5f * dnorm[row] : -__builtin_inff();
    if (row < N) hi = fmaxf(hi, v);
    lo = fminf(lo, v);
  }
  float* t = dneg + (size_t)(b >> 2) * SC_DD;
  t[128 + (b & 3)] = hi;
  t[132 + (b & 3)] = lo;
  // the largest spread of -dd/2 inside a block of real rows (stats[3]; non-negative floats order like their bits):
  // what a record's value can overstate its block's largest screen value by
  if (b * 32 + 32 <= N && hi - lo >= 0.f) atomicMax(&stats[3], __float_as_uint(hi - lo));
  if ((b & 3) == 0)
    for (int i = 136; i < SC_DD; ++i) t[i] = 0.f;
}

// The exact answer for an all-zero query: canonical distance max(0, fmaf(-2, 0, 0 + dd_r)) = dd_r, so the two smallest
// norm terms over the real rows, the lower row on a tie (what the exact kernels' top-2 gives).  One workgroup.
__global__ __launch_bounds__(1024) void db_zero_query_kernel(const float* __restrict__ dnorm, int N, unsigned int* __restrict__ stats) {
  __shared__ float s1[1024], s2[1024];
  __shared__ int si[1024];
  float b1 = __builtin_inff(), b2 = __builtin_inff();
  int i1 = -1;
  for (int r = threadIdx.x; r < N; r += 1024) {   // ascending rows: a strict < keeps the lower row on ties
    const float d = fmaxf(dnorm[r], 0.f);
    if (d < b1 || i1 < 0) {
      if (i1 >= 0) b2 = fminf(b2, b1);
      b1 = d;
      i1 = r;
    } else {
      b2 = fminf(b2, d);
    }
  }
  s1[threadIdx.x] = b1;
  s2[threadIdx.x] = b2;
  si[threadIdx.x] = i1;
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      const float o1 = s1[threadIdx.x + st], o2 = s2[threadIdx.x + st];
      const int oi = si[threadIdx.x + st];
      float a1 = s1[threadIdx.x], a2 = s2[threadIdx.x];
      int ai = si[threadIdx.x];
      if (oi >= 0) {
        const bool take = ai < 0 || o1 < a1 || (o1 == a1 && oi < ai);
        const float lose = take ? a1 : o1;
        a2 = fminf(fminf(a2, o2), ai >= 0 ? lose : __builtin_inff());
        if (take) {
          a1 = o1;
          ai = oi;
        }
      }
      s1[threadIdx.x] = a1;
      s2[threadIdx.x] = a2;
      si[threadIdx.x] = ai;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[4] = (unsigned int)si[0];
    stats[5] = __float_as_uint(s1[0]);
    stats[6] = __float_as_uint(s2[0]);
  }
}

// Queries of the frame: f16 rows (zero rows up to the padded count) + a flag for queries the screen
// cannot vouch for (non-finite norm term, or a coordinate outside f16's range).
__global__ void screen_prepare_kernel(const float* __restrict__ qn, const float* __restrict__ qnorm, int Q,
                                      const int32_t* __restrict__ q_count, int q_pad, _Float16* __restrict__ qh,
                                      uint8_t* __restrict__ qbad) {
  MH_TRACE_SCOPE(mh::TK_PREPARE);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // one 8-element chunk; 16 consecutive threads = one row
  if (i >= q_pad * 16) return;
  const int row = i >> 4;
  const int Qe = q_count ? min(Q, *q_count) : Q;
  half8 h = {0, 0, 0, 0, 0, 0, 0, 0};
  float m = 0.f;
  if (row < Qe) {
    const float4 a = reinterpret_cast<const float4*>(qn)[2 * (size_t)i], b = reinterpret_cast<const float4*>(qn)[2 * (size_t)i + 1];
    h[0] = (_Float16)a.x; h[1] = (_Float16)a.y; h[2] = (_Float16)a.z; h[3] = (_Float16)a.w;
    h[4] = (_Float16)b.x; h[5] = (_Float16)b.y; h[6] = (_Float16)b.z; h[7] = (_Float16)b.w;
    m = fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
              fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
  }
  reinterpret_cast<half8*>(qh)[i] = h;
  // row maximum over its 16 threads (fmaxf drops NaNs: a NaN coordinate shows in the norm term instead)
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((i & 15) == 0) {
    int bad = 0;
    if (row < Qe) {
      const float qq = qnorm[row];
      bad = (!(qq >= 0.f) || qq == __builtin_inff() || !(m < 60000.f)) ? 1 : 0;
      // norm term exactly -1 = "no such query" (the rows past an image's keypoint count in a batch of images,
      // mh_frame_enqueue_image_batch): no threshold, no records, no neighbour -- not a query the screen cannot vouch for
      if (qq == -1.f) bad = 2;
      else if (!bad && m == 0.f && qq == 0.f) bad = 3;   // an all-zero query: its answer is known per DB (ScreenDb::zero_*)
    }
    qbad[row] = (uint8_t)bad;
  }
}

// The screen value of every (query, row) pair of a small problem, by the arithmetic of pass A: one wavefront per
// (32 queries, 32 rows), operands straight from the f16 images, the accumulator seeded with the rows' -dd/2, the eight
// MFMAs of a block in ascending k.  Register r of lane (l32, half) = query l32, row (r & 3) + 8 (r >> 2) + 4 half.
__global__ __launch_bounds__(64) void screen_values_kernel(const _Float16* __restrict__ qh, const _Float16* __restrict__ dbh,
                                                           const float* __restrict__ dneg, int n_rows, float* __restrict__ out,
                                                           int shape16) {
  const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
  const int q0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  if (shape16) {   // screen16_kernel's arithmetic: 2 x 2 tiles of 16 x 16, four k-steps of 32, seeded with -dd/2
    const int quarter = lane >> 4, l16 = lane & 15;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        v4f acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + 16 * ti + 4 * quarter + r;
          acc[r] = dneg[(size_t)(row >> 7) * SC_DD + (row & 127)];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const half8 a = *reinterpret_cast<const half8*>(dbh + (size_t)(r0 + 16 * ti + l16) * DIM + 32 * s + 8 * quarter);
          const half8 b = *reinterpret_cast<const half8*>(qh + (size_t)(q0 + 16 * tj + l16) * DIM + 32 * s + 8 * quarter);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(q0 + 16 * tj + l16) * n_rows + r0 + 16 * ti + 4 * quarter + r] = acc[r];
      }
    return;
  }
  half8 a[8], b[8];
  const _Float16* arow = dbh + (size_t)(r0 + l32) * DIM + 8 * half;
  const _Float16* brow = qh + (size_t)(q0 + l32) * DIM + 8 * half;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    a[s] = *reinterpret_cast<const half8*>(arow + 16 * s);
    b[s] = *reinterpret_cast<const half8*>(brow + 16 * s);
  }
  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    acc[r] = dneg[(size_t)(row >> 7) * SC_DD + (row & 127)];
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], b[s], acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(size_t)(q0 + l32) * n_rows + r0 + (r & 3) + 8 * (r >> 2) + 4 * half] = acc[r];
}

}  // namespace

size_t screen_db_half_elems(int N) { return ((size_t)N + SC_TILE - 1) / SC_TILE * SC_TILE * DIM; }
size_t screen_dneg_elems(int N) { return ((size_t)N + SC_TILE - 1) / SC_TILE * SC_DD; }

void launch_db_to_half(const float* db, const float* dnorm, int N, _Float16* dbh, float* dneg, unsigned int* stats,
                       hipStream_t s) {
  const size_t n_chunks = screen_db_half_elems(N) / 8;
  if (n_chunks == 0) return;
  const unsigned blocks = (unsigned)std::min<size_t>((n_chunks + 255) / 256, 2048);
  hipLaunchKernelGGL(db_to_half_kernel, dim3(blocks), dim3(256), 0, s, db, dnorm, N, n_chunks, dbh, dneg, stats);
  launch_db_aggregates(dnorm, N, dneg, stats, s);
}

void launch_db_aggregates(const float* dnorm, int N, float* dneg, unsigned int* stats, hipStream_t s) {
  const int n_tiles = (N + SC_TILE - 1) / SC_TILE;
  if (n_tiles == 0) return;
  hipLaunchKernelGGL(db_block_bounds_kernel, dim3((n_tiles * 4 + 255) / 256), dim3(256), 0, s, dnorm, N, n_tiles, dneg, stats);
  hipLaunchKernelGGL(db_zero_query_kernel, dim3(1), dim3(1024), 0, s, dnorm, N, stats);
}

void launch_screen_values(const _Float16* qh, int Q, const ScreenDb& sdb, int n_rows, float* out, hipStream_t s, int shape) {
  if (Q <= 0 || n_rows <= 0) return;
  const int shape16 = shape == 2 || (shape == 0 && SC_SHAPE16_LARGE);
  hipLaunchKernelGGL(screen_values_kernel, dim3(Q / 32, n_rows / 32), dim3(64), 0, s, qh, sdb.dbh, sdb.dneg, n_rows, out, shape16);
}
void launch_screen_prepare(const float* qn, const float* qnorm, int Q, int q_pad, _Float16* qh, uint8_t* qbad, hipStream_t s,
                           const int32_t* q_count) {
  hipLaunchKernelGGL(screen_prepare_kernel, dim3((q_pad * 16 + 255) / 256), dim3(256), 0, s, qn, qnorm, Q, q_count, q_pad, qh, qbad);
}

int screen_q_pad(int Q) { return (Q + SC_QPAD - 1) / SC_QPAD * SC_QPAD; }
int screen_max_splits_a() { return 64; }
// per query: a float2 per pass A split (screen_kernel), or SC_PART5 floats per lane slot of a one-sweep launch
size_t screen_part_bytes(int q_pad) {
  return (size_t)q_pad * std::max<size_t>(screen_max_splits_a() * sizeof(float2), (size_t)SC_SA_SPLITS_MAX * 4 * SC_PART5 * sizeof(float));
}

}  // namespace mh
