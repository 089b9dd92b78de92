// MATCH in two stages: an f16 matrix-pipe SCREEN of all (query, row) pairs, then the canonical f32
// arithmetic only on the few rows per query that can still be one of its two nearest.  Results --
// (idx1, d1, d2) per query -- are bit for bit those of match.hip / match_mfma.hip (and of the oracle):
// the screen only decides WHICH rows get the exact treatment, and it errs on the side of too many.
//
// Replaces the kd-tree search of MATCH_ANN_CPU::process (moped2/libmoped/src/match/MATCH_ANN_CPU.hpp:
// 155-165) like the exact kernels do; what changes is the cost: 2*128*Q*N flops on
// v_mfma_f32_32x32x16_f16 (16x the f32 rate) instead of on v_mfma_f32_32x32x2_f32.
//
// Why it is exact.  Canonical distance (match.hip): a(q,r) = max(0, fmaf(-2, p, qq + dd_r)) with p the
// f32 fmaf chain of dot(q, d_r).  Ranking by a is ranking by w(q,r) = p - dd_r / 2 (a = qq - 2w up to
// f32 rounding).  The screen computes w~ = sum_k f16(q_k) f16(d_rk) - dd_r / 2 with f32 accumulation
// (the -dd_r/2 term is the accumulator's initial value, exact).  With u = 2^-11 (f16 unit roundoff)
//     |w~ - w| <= E(q) = (2u + u^2) |q| Dmax            rounding of both operands (Cauchy-Schwarz)
//                      + 2^-25 sqrt(128) (|q| + Dmax)    f16 subnormal range (absolute 2^-25 per element)
//                      + 3e-5 (|q| Dmax + Dmax^2 / 2)    136 f32 accumulations on either side + the chain's own rounding
// where Dmax = max_r |d_r| (taken at upload).  Let T be any value known to be <= the second largest w~
// over distinct rows (pass A: the second largest over a SAMPLE of the rows).  A row r that is one of the
// two nearest by a satisfies w_r >= (second largest w) - slack, hence w~_r >= T - 2E - slack.  Pass B emits
// every row above tau = T - (2E + slack); pass C evaluates the canonical distance of the emitted rows and
// folds the exact top-2 (ties -> lower row, second best = second smallest value), which is the global
// answer because every row it did not see is strictly farther than the two it reports.  A query whose
// candidate list overflows, or whose descriptor is not finite / too large for f16, is searched by brute
// force inside pass C: the screen can be slow, never wrong.  The bound is exercised by
// tests/test_gpu_screen.py (near-ties inside the bound, duplicates, zero rows, unnormalised rows) and
// its arithmetic by tests/test_screen_bound_cpu.py.
//
// Shape (gfx950).  A workgroup = 4 wavefronts, 2 workgroups per CU.  A wavefront keeps 64 queries in
// registers as the B operands of all 8 k-steps (2 blocks x 8 x 4 VGPRs); the f16 DB streams through
// LDS in 128-row tiles (32 KB, double buffered, filled by global_load_lds_dwordx4 with the 16-byte
// chunks of row r stored at chunk position c ^ (r & 15), so the A-operand ds_read_b128 of 16 lanes
// touch all 64 banks once).  Queries sit on the accumulator's lane axis, rows on its register axis:
// a lane's 16 values of a 32x32 block are 16 rows of ONE query, so the running maxima are lane-local
// v_max3_f32 (8 per block) and only a lane with a hit looks at individual values.
#include <type_traits>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "screen.h"

MH_TRACE_TU()

namespace mh {

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
#define MH_AS1 __attribute__((address_space(1)))
#define MH_AS3 __attribute__((address_space(3)))

// Wavefronts per workgroup (template parameter NW of the passes): 8 = one workgroup per CU, two of ITS wavefronts per
// SIMD; 4 = one wavefront per SIMD, so that TWO workgroups share a CU -- the two wavefronts of a SIMD then belong to
// different workgroups (no common barrier, phases drift apart: one's LDS waits and hit paths sit under the other's MFMAs),
// and a CU on which a small kernel of another frame holds a few wavefronts still takes one such workgroup (the 8-wavefront
// shape needs the whole register file of the CU: scripts/cu_trace.py found 21% of all CU time spent with only small
// workgroups resident and 16-20% with none).  Price: every tile is staged from L2 by twice as many workgroups.
constexpr int SC_QPAD = 3 * 1024;                  // the query image is padded to whole workgroups of every kernel width
constexpr int SC_TILE = 128;                       // DB rows per LDS tile (= the DB's row padding)
constexpr int SC_TILE_BYTES = SC_TILE * DIM * 2;   // 32 KB of f16
// hits a wavefront parks in LDS (80 bytes each: the block's 16 values go along) before they go to memory: 112 with eight
// wavefronts (the whole workgroup's hits, written out at its end), 40 with four (two workgroups' LDS must fit a CU:
// 2 x (64 KB tiles + 1.5 KB + 4 x 40 x 80 B) = 156 KB) -- written out whenever the buffer is three quarters full
constexpr bool SC_SHAPE16_LARGE = true;   // the four-query-block launches run on v_mfma_f32_16x16x32_f16 (screen16_kernel)
constexpr int SC_NW_LARGE = 8;   // wavefronts per workgroup of the four-query-block launches (4 or 8; MH_SCREEN_NW in experiment builds)
__host__ __device__ constexpr int sc_recbuf(int nw) { return nw >= 8 ? 112 : 40; }
constexpr int SC_GROUP = 1;                        // tiles per barrier: the wavefronts of a workgroup drift apart within a group
constexpr int SC_NBUF = 2 * SC_GROUP;              // (a hit costs its wavefront ~300 cycles), every barrier makes seven wait for the slowest
constexpr int SC_DD = 192;                         // floats per tile of the -dd/2 array: 128 rows, the 4 row blocks' maxima, their minima, padding
constexpr int SC_LDS_TILES = SC_NBUF * SC_TILE_BYTES + SC_NBUF * SC_DD * 4;   // the tiles + their -dd/2 terms
constexpr int SC_REC_BYTES = 80;                   // {slot, row0, thr, top, 16 dots}
__host__ __device__ constexpr int sc_lds_bytes(int nw) { return SC_LDS_TILES + nw * sc_recbuf(nw) * SC_REC_BYTES; }   // + the wavefronts' hit buffers
static_assert(SC_TILE == 128 && DIM == 128, "tile image and chunk swizzle assume 128 x 128");

// error model of the screen (see the header comment): E(q), the bound of ONE screen value's distance from w = p - dd / 2
__host__ __device__ inline float screen_value_err(float qq, float dmax) {
  const float nq = sqrtf(fmaxf(qq, 0.f));
  return 0.000978f * nq * dmax + 4e-7f * (nq + dmax) + 3e-5f * (nq * dmax + 0.5f * dmax * dmax);
}
__host__ __device__ inline float screen_margin(float qq, float dmax) {
  const float E = screen_value_err(qq, dmax);
  return 2.f * E + 2e-6f * (qq + dmax * dmax);
}

// Can the ratio test `fdiv(d1, d2) < ratio` (match_accepted, steps.h) still accept this query?  Pass C asks after its first
// round trip, when it holds of the query's records h1 = the largest upper bound and l2 = the second largest lower bound
// (over distinct records) of a block's largest screen value; true = no, whatever the exact arithmetic gives.
//   * Every row whose screen value exceeds tau_q is in a record (the caller sees to that: no overflowed list, no
//     incomplete query), so every row's screen value is <= top = max(h1, tau_q).
//   * Two different records hold different rows: two distinct rows have screen values >= l2.
//   * A row's canonical distance is a = max(0, fl(-2 p + fl(qq + dd))) and its screen value w~ lies within E of
//     w = p - dd / 2 (the header), so |x - (qq - 2 w~)| <= delta = 2 E + 2e-6 (qq + Dmax^2) for x = the value under the
//     max: 2 E from the screen, and the two roundings of x are worth <= 3 * 2^-24 (qq + Dmax^2) < 1.8e-7 (qq + Dmax^2) --
//     per value the same allowances screen_margin makes for a pair (the margin is delta in units of w~, which are half
//     those of a; tests/test_screen_bound_cpu.py).
//   * Hence d1 = the smallest a >= qq - 2 top - delta =: L1, and d2 = the second smallest a (over rows: equal values count
//     twice) <= max(0, qq - 2 l2 + delta) =: U2.
//   * If U2 > 0 and L1 >= ratio U2, then d1 >= ratio d2 with d2 > 0 or d1 = d2 = 0: the quotient is NaN or >= ratio, and
//     the correctly rounded division keeps it there (ratio is an f32, rounding is monotone).
// L1 and U2 are formed in f32, three roundings each of values below `mag`; `slack` = 1e-6 mag pays for them (and for a
// compiler that contracts the expressions differently on the host and on the device), the factor on the product for its
// own two roundings.  false for ratio <= 0, a non-finite input, l2 = -inf (fewer than two records) and U2 <= 0.
__host__ __device__ inline bool screen_reject_proved(float qq, float dmax, float h1, float l2, float tau_q, float ratio) {
  const float big = 1e30f;
  if (!(ratio > 0.f) || !(ratio < big) || !(fabsf(qq) < big) || !(fabsf(dmax) < big) || !(fabsf(tau_q) < big)) return false;
  if (!(fabsf(l2) < big) || !(h1 < big)) return false;   // (h1 = -inf cannot be, with l2 finite; it would do no harm)
  const float top = fmaxf(h1, tau_q);
  const float delta = 2.f * screen_value_err(qq, dmax) + 2e-6f * (qq + dmax * dmax);
  const float mag = fabsf(qq) + 2.f * fabsf(top) + 2.f * fabsf(l2) + delta;
  const float slack = 1e-6f * mag;
  const float lo_d1 = qq - 2.f * top - delta - slack;
  const float hi_d2 = qq - 2.f * l2 + delta + slack;
  if (!(hi_d2 > 0.f)) return false;
  return lo_d1 >= ratio * hi_d2 * 1.000001f;
}

// ---- f16 images ------------------------------------------------------------------------------
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

// ---- passes A and B ------------------------------------------------------------------------------
// MODE 0 (pass A): top-2 VALUES of w~ per (split, query) over the sampled tiles -> part[split][q].
// MODE 1 (pass B): every row with w~ > tau(q) -> the query's candidate records {row0, bits}: rows
//                  row0 + (r & 3) + 8 (r >> 2) for the set bits r.  A lane owns the sub-list (query, split, half)
//                  -- `sub_cap` slots nobody else writes, no atomics; a sub-list that is full spills into the
//                  query's overflow list (atomic append, rare).  bits = 0 marks an empty slot.
constexpr int SC_SLOTS_MAX = 256;   // pass B's record slots per query: 2 halves x splits x sub_cap <= this
// ... and behind them the slots of the records pass A's sampled tiles leave (screen_handover_kernel; the one-sweep launches)
constexpr int SC_SA_SLOTS = 32;
constexpr int SC_SLOT_PITCH = SC_SLOTS_MAX + SC_SA_SLOTS;
// The 16x16x32 launches (launch_passes16) use the same memory as ONE counted list per query instead: the records lie in
// recs[q * SC_SLOT_PITCH + 0 .. count), count = the query's word of `ovf_cnt` (those launches have no overflow list).
// screen_handover_kernel writes its records as the list's head and stores the count; pass B appends behind them with one
// atomic add per record, when a wavefront writes its parked hits out (screen16_kernel's flush_parked: outside the hit
// path).  A record that finds the list full is dropped and still counted: count > SC_SLOT_PITCH sends the query to pass
// C's brute-force search.  Pass C reads the count with its other scalars and 64 slots (one 512-byte line) in the same round
// trip, instead of every slot a sub-list might have used.  Between launches every slot is empty and every count zero, as
// the 32x32x16 launches -- which share a context's buffers with these -- need it: pass C re-empties what it consumed.

#ifdef SC_PROF   // experiment build (make EXTRA=-DSC_PROF ...): switch parts of passes A/B off (results are wrong then)
// and stamp a workgroup's time; scripts/screen_prof.py
__device__ unsigned long long g_sc_prof[8];
__device__ unsigned long long g_sc_trace[2][1024];   // (event << 56 | cycles since the workgroup's start) of wavefronts 0 and 4 of workgroup 3
static int g_sc_ablate = 0;
#define SC_ABL(bit) ((A.ablate >> (bit)) & 1)
#define SC_EV(e) do { if (tracing && n_ev < 1024) { g_sc_trace[wave >> 2][n_ev++] = ((unsigned long long)(e) << 56) | (__builtin_amdgcn_s_memtime() - t_start); } } while (0)
#else
#define SC_ABL(bit) 0
#define SC_EV(e) do { } while (0)
#endif
#ifdef MH_EXPERIMENTS
// hits of screen16_kernel's pass B that found their wavefront's park buffer full and were appended from the hit path
// (mh_debug_screen_direct_appends)
__device__ unsigned long long g_sc_direct_appends;
#endif

struct ScreenArgs {
  const _Float16* qh;
  const _Float16* dbh;
  const float* dneg;     // [padded rows] -dd/2, -inf on padding rows
  const float* qnorm;
  const uint8_t* qbad;
  const int32_t* q_count;
  float2* part;          // pass A's output, [n_splits_a][q_pad] (screen_kernel)
  float* part5;          // ... of screen16_kernel: [n_splits_a x 4 quarters][SC_TOPK + 1][q_pad], the same memory
  const float* tau;      // pass B's input, [q_pad] (screen_tau_kernel)
  uint2* recs;           // [q_pad][SC_SLOTS_MAX], empty (bits 0) on entry of pass B (pass C re-empties)
  int32_t* ovf_cnt;      // [q_pad], zero on entry (screen16_kernel: the records in the query's list, set by the hand-over)
  uint2* ovf;            // [q_pad][ovf_cap] (screen_kernel only)
  int Q, q_pad, ovf_cap, sub_cap;   // (ovf_cap, sub_cap: screen_kernel only)
  int n_sel, tile_first, tile_stride;   // the pass covers tiles tile_first + j * tile_stride, j < n_sel
  int tiles_base, tiles_rem, n_splits;  // split s takes tiles_base selected tiles, the first tiles_rem one more
  int n_splits_a;
  unsigned pack_keep;    // pass A (screen16_kernel): the bits of a block maximum that survive the packing of the block's number
  int skip_first, skip_stride;   // pass B (screen16_kernel): selected tile j = the j-th tile that is NOT skip_first + i * skip_stride; 0 = no tile is skipped
  float dmax;
  int ablate;            // SC_PROF builds only: 1 = no finish(), 2 = stage only the first tile, 4 = no MFMAs, 8 = no end-of-tile barrier
};

// Between the passes: a query's threshold from pass A's per-split top-2 values.  tau = +inf for queries that do not
// exist in this frame or that the screen cannot vouch for (pass B then leaves them no records; pass C searches the
// latter by brute force).  One thread per query; the splits' values of neighbouring queries are neighbours in memory.
__global__ void screen_tau_kernel(const float2* __restrict__ part, int n_splits_a, int q_pad, int Q,
                                  const int32_t* __restrict__ q_count, const float* __restrict__ qnorm,
                                  const uint8_t* __restrict__ qbad, float dmax, float* __restrict__ tau) {
  MH_TRACE_SCOPE(mh::TK_TAU);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= q_pad) return;
  const int Qe = q_count ? min(Q, *q_count) : Q;
  float t = __builtin_inff();
  if (q < Qe && !qbad[q]) {
    float B = -__builtin_inff(), S = -__builtin_inff();
    for (int s0 = 0; s0 < n_splits_a; s0 += 8) {
      float2 p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        p[j] = (s0 + j < n_splits_a) ? part[(size_t)(s0 + j) * q_pad + q] : make_float2(-__builtin_inff(), -__builtin_inff());
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        S = fmaxf(fminf(B, p[j].x), fmaxf(S, p[j].y));
        B = fmaxf(B, p[j].x);
      }
    }
    t = S - screen_margin(qnorm[q], dmax);
  }
  tau[q] = t;
}

// ---- pass A of the one-sweep launches: the sampled tiles' blocks that can matter, kept by identity -----------------
// screen16_kernel's pass A keeps, per LANE SLOT (split x quarter: the rows one lane sees of one query), the SC_TOPK
// largest block maxima with the block each belongs to, and the next largest value: the block's number inside the lane
// slot (local tile x 4 + row block) replaces the low `bits` mantissa bits of the maximum (screen_pack_value), so the
// insertion into the sorted list is branch-free (one v_max, SC_TOPK v_med3) and the packed values of a lane slot are
// all different.  screen_handover_kernel turns the lists into the query's threshold AND into the records of the sampled
// tiles, so that pass B need not multiply those tiles a second time.  Why that is exact (P = screen_pack_pert: a
// packed value lies within P of the block maximum it was made from; all lane slots hold different rows):
//   - T = (second largest packed value over all lists) - P <= the second largest block maximum of the sample <= the
//     second largest screen value over distinct rows: tau = T - screen_margin is a valid threshold (header);
//   - a block of a sampled tile whose maximum exceeds tau has a packed value v' > tau - P.  Either v' is among its lane
//     slot's SC_TOPK largest -- then it becomes a record (the block's 8 rows, not yet told apart; value v' - tau) -- or it is not, and
//     then the slot's (SC_TOPK + 1)-th value is >= v' > tau - P and the query is marked INCOMPLETE for that lane slot:
//     pass C runs the canonical chain over the slot's rows instead of its records (none is written for such a slot);
//   - a padding row's screen value is -inf and a block of padding rows would pack into a NaN: block maxima are floored
//     at SC_PACK_FLOOR, far below any real row's value, and anything that low counts as "no block" here.
//   - which rows of a handed-over block get the exact treatment (pass C): screen_handover_kernel knows the block's packed
//     maximum only, so its record's mask says "all 8 rows" (0xFF) and means "not evaluated".  For the records that
//     survive its thinning, pass C RECOMPUTES the block's 8 screen values with pass A's arithmetic (sample_pair_values:
//     the same v_mfma_f32_16x16x32_f16, accumulator seeded with the rows' -dd/2, four k-steps in ascending k, the same
//     f16 operands; an element of the product does not depend on which row or column of the operand tiles it sits in) and
//     keeps the rows with w~_r > tau.  These ARE the values pass A saw before it packed their maximum, i.e. values in an
//     arithmetic the header's E covers (pass A's accumulators): a row of the exact top-2 has w~_r >= T - 2E - slack, so it
//     is above tau -- the header's rule "every row above tau is emitted", applied to the sampled tiles as pass B applies it
//     to the others; no new bound.  The mask can be EMPTY (the record test used tau - P: a packed maximum in
//     (tau - P, tau] whose block has no row above tau): the record then leaves no candidate.
//     tests/test_gpu_sample_mask.py holds the recomputed values against mh_screen_values(shape 2) bit for bit.
// tests/test_screen_handover_cpu.py restates the lists and this kernel's decisions against the direct definition.
constexpr int SC_TOPK = 4;
constexpr int SC_PART5 = SC_TOPK + 1;           // floats per (lane slot, query) in `part5`
constexpr int SC_SA_SPLITS_MAX = 28;            // pass A splits of a one-sweep launch: bits 0..27 of a query's incomplete word (28..31: the quarters)
constexpr int SC_PACK_BITS_MAX = 10;            // block numbers up to 1024 per lane slot: P <= 2^-13 of the largest screen value, a tenth of the margin
constexpr float SC_PACK_FLOOR = -1e38f;
constexpr unsigned SC_REC_LAYOUT16 = 0x80000000u;   // in a record's row word: the rows of the 16x16x32 passes
constexpr unsigned SC_REC_SAMPLE = 0x40000000u; // in a record's row word: made by screen_handover_kernel (value = packed maximum - tau; mask 0xFF = pass C names the rows above tau)

// what pass C has to know about pass A's sweep to find a lane slot's rows again
struct SampleGeom {
  int sa_slots;          // 0: no hand-over (pass B swept every tile)
  int pack_bits;
  int tile_first, tile_stride, tiles_base, tiles_rem, n_sel;
};

// A workgroup = 64 queries along the lanes (the lane slots' values of neighbouring queries are neighbours in memory) x
// blockDim.y parts; a thread loads the lists of ITS HS lane slots -- HS x SC_PART5 values, all in flight at once, kept
// in registers -- and the parts of a query meet in LDS three times: the two largest packed values (-> tau), the
// incomplete lane slots (the fifth values against tau - P), and the parts' record counts (-> where a part's records go:
// in lane slot order, as one thread walking all lists would write them).
// tau = +inf for queries that do not exist in this frame or that the screen cannot vouch for (pass B then leaves them
// no records; pass C searches the latter by brute force).
constexpr int HO_PARTS_MAX = 16;
template <int HS>
__global__ __launch_bounds__(64 * HO_PARTS_MAX) void screen_handover_kernel(
    const float* __restrict__ part5, int n_lane_slots, int q_pad, int Q, const int32_t* __restrict__ q_count,
    const float* __restrict__ qnorm, const uint8_t* __restrict__ qbad, float dmax, SampleGeom g, float* __restrict__ tau,
    uint2* __restrict__ recs, int32_t* __restrict__ rec_cnt, unsigned int* __restrict__ inc) {
  MH_TRACE_SCOPE(mh::TK_TAU);
  __shared__ float s_b[HO_PARTS_MAX][64], s_s[HO_PARTS_MAX][64];
  __shared__ int s_cnt[HO_PARTS_MAX][64];
  __shared__ unsigned s_sm[64], s_qm[64];
  const int ql = threadIdx.x, part = threadIdx.y, n_parts = blockDim.y;
  const int q = blockIdx.x * 64 + ql;
  const int Qe = q_count ? min(Q, *q_count) : Q;
  const bool live = q < q_pad && q < Qe && !qbad[q];
  const int ls0 = part * HS;
  float v[HS][SC_PART5];
#pragma unroll
  for (int j = 0; j < HS; ++j)
#pragma unroll
    for (int k = 0; k < SC_PART5; ++k)
      v[j][k] = live && ls0 + j < n_lane_slots ? part5[((size_t)(ls0 + j) * SC_PART5 + k) * q_pad + q] : -__builtin_inff();
  const float qq = live ? qnorm[q] : 0.f;
  if (part == 0) {
    s_sm[ql] = 0u;
    s_qm[ql] = 0u;
  }
  float B = -__builtin_inff(), S = -__builtin_inff();
#pragma unroll
  for (int j = 0; j < HS; ++j) {
#pragma unroll
    for (int k = 0; k < SC_PART5; ++k) v[j][k] = v[j][k] < 0.5f * SC_PACK_FLOOR ? -__builtin_inff() : v[j][k];
    S = fmaxf(fminf(B, v[j][0]), fmaxf(S, v[j][1]));
    B = fmaxf(B, v[j][0]);
  }
  s_b[part][ql] = B;
  s_s[part][ql] = S;
  __syncthreads();
  // (the second largest of all the parts' values: max and min only, the same number in any order)
  B = S = -__builtin_inff();
  for (int p = 0; p < n_parts; ++p) {
    const float ob = s_b[p][ql], os = s_s[p][ql];
    S = fmaxf(fminf(B, ob), fmaxf(S, os));
    B = fmaxf(B, ob);
  }
  const float P = screen_pack_pert(qq, dmax, g.pack_bits);
  const float t = live ? S - P - screen_margin(qq, dmax) : __builtin_inff();
  const float thr = t - P;
  // (t = -inf: pass B's lists overflow and pass C searches by brute force)
  const bool hand = live && g.sa_slots > 0 && t > -__builtin_inff();
  unsigned sm = 0, qm = 0;   // the incomplete lane slots, as (splits) x (quarters): a superset
  if (hand) {
#pragma unroll
    for (int j = 0; j < HS; ++j)
      if (v[j][SC_TOPK] > thr) {   // (no list behind the last lane slot: -inf)
        sm |= 1u << ((ls0 + j) >> 2);
        qm |= 1u << ((ls0 + j) & 3);
      }
    if (sm) {
      atomicOr(&s_sm[ql], sm);
      atomicOr(&s_qm[ql], qm);
    }
  }
  __syncthreads();
  sm = s_sm[ql];
  qm = s_qm[ql];
  // this part's records: of every lane slot pass C does not sweep, the listed blocks above tau - P (the lists are sorted)
  int n_j[HS], cnt = 0;
#pragma unroll
  for (int j = 0; j < HS; ++j) {
    const int ls = ls0 + j;
    const bool swept = ((sm >> (ls >> 2)) & 1u) && ((qm >> (ls & 3)) & 1u);
    n_j[j] = 0;
    bool run = hand && !swept;
#pragma unroll
    for (int k = 0; k < SC_TOPK; ++k) {
      run = run && v[j][k] > thr;
      n_j[j] += run ? 1 : 0;
    }
    cnt += n_j[j];
  }
  s_cnt[part][ql] = cnt;
  __syncthreads();
  int before = 0, total = 0;
  for (int p = 0; p < n_parts; ++p) {
    const int c = s_cnt[p][ql];
    before += p < part ? c : 0;
    total += c;
  }
  // more records than slots (never seen): none is written, every lane slot's rows go to pass C's sweep instead
  const bool full = total > g.sa_slots;
  if (cnt && !full) {
    uint2* mine = recs + (size_t)q * SC_SLOT_PITCH + before;   // the head of the query's list; pass B appends behind `total`
    const unsigned id_mask = (1u << g.pack_bits) - 1u;
    int n = 0;
#pragma unroll
    for (int j = 0; j < HS; ++j) {
      const int split = (ls0 + j) >> 2, quarter = (ls0 + j) & 3;
#pragma unroll
      for (int k = 0; k < SC_TOPK; ++k)
        if (k < n_j[j]) {
          const unsigned id = __float_as_uint(v[j][k]) & id_mask;
          const int sel = split * g.tiles_base + min(split, g.tiles_rem) + (int)(id >> 2);
          const unsigned row0 = (unsigned)((g.tile_first + sel * g.tile_stride) * SC_TILE + (int)(id & 3u) * 32 + 4 * quarter);
          // (the mask says "all 8 rows": pass C names the rows above tau itself, for the records its thinning leaves)
          mine[n++] = make_uint2(row0 | SC_REC_LAYOUT16 | SC_REC_SAMPLE, 0xFFu | ((unsigned)screen_record_value(v[j][k], t) << 16));
        }
    }
  }
  if (part == 0 && q < q_pad) {
    if (full) {
      sm = (1u << (n_lane_slots >> 2)) - 1u;
      qm = 0xFu;
    }
    tau[q] = t;
    rec_cnt[q] = full ? 0 : total;
    if (inc) inc[q] = sm ? sm | (qm << 28) : 0u;
  }
}

// Four LDS-DMA pieces (1 KB each: 16 bytes per lane to lds_i + lane * 16) in one statement: the source of piece i
// is base_i + voff (the same per-lane offset for all four), M0 is saved once.  Issued as asm so that hipcc neither
// counts the transfers nor waits for them before the next ds_read (it would: vmcnt(0) at the first LDS read after a
// __builtin_amdgcn_global_load_lds).  Completion: the s_waitcnt vmcnt(0) + barrier that end every tile.
__device__ __forceinline__ void dma16x4(unsigned voff, const void* b0, const void* b1, const void* b2, const void* b3,
                                        unsigned l0, unsigned l1, unsigned l2, unsigned l3) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
      "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4\n\t"
      "s_mov_b32 m0, %9\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(b0), "s"(b1), "s"(b2), "s"(b3), "s"(l0), "s"(l1), "s"(l2), "s"(l3)
      : "memory");
}
__device__ __forceinline__ void dma4(unsigned voff, const void* base, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_dst) : "memory");
}

template <int MODE, int NQB, int NW>
__global__ __launch_bounds__(64 * NW, 2) void screen_kernel(const ScreenArgs A) {
  MH_TRACE_SCOPE(MODE == 0 ? mh::TK_PASS_A : mh::TK_PASS_B);
  constexpr int SC_WAVES = NW;
  constexpr int SC_RECBUF = sc_recbuf(NW);
  constexpr int QW = 32 * NQB;            // queries per wavefront
  constexpr int QB = QW * SC_WAVES;       // queries per workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const unsigned lds_base = (unsigned)(uintptr_t)(MH_AS3 unsigned char*)lds;
  // XCD-aware (query block, split) map as in match.hip: workgroups are dealt round-robin to the 8 XCDs, so
  // giving XCD x the splits x, x + 8, ... keeps a split's rows in one L2
  const int nqb = gridDim.x / A.n_splits;
  int qblock, split;
  {
    // workgroup L runs on XCD L % 8: XCD x takes the x-th eighth of the (split-major) unit list, so the rows of a
    // split -- read by all nqb query blocks -- pass through one or two of the eight L2s and not through all of them,
    // whatever the number of splits
    const int L = blockIdx.x, U = gridDim.x;
    const int x = L & 7, j = L >> 3;
    const int unit = x * (U >> 3) + min(x, U & 7) + j;
    split = unit / nqb;
    qblock = unit - split * nqb;
  }
  const int Qe = A.q_count ? min(A.Q, *A.q_count) : A.Q;
  if (qblock * QB >= Qe) return;   // uniform over the workgroup
  const int q0 = qblock * QB + wave * QW;
  const int sel_begin = split * A.tiles_base + min(split, A.tiles_rem);
  const int sel_end = min(sel_begin + A.tiles_base + (split < A.tiles_rem ? 1 : 0), A.n_sel);

  // ---- staging: one tile = 32 pieces of 1 KB (64 lanes x 16 B, lane-linear in LDS); wavefront w brings pieces
  // w, w + NW, w + 2 NW, ... (four of them with eight wavefronts, eight with four).  Chunk g = 64 piece + lane of the LDS
  // image is row g >> 4, position g & 15, and holds source chunk (g & 15) ^ (row & 15); row & 15 = (4 w + (lane >> 4)) & 15
  // for all pieces of a wavefront (they lie 4 NW rows apart: a multiple of 16), so one per-lane offset serves them and the
  // pieces differ by NW KB in a scalar base.  The rows' -dd/2 terms (512 B per tile) and the row blocks' extrema (768 B
  // per tile) come the same way: wavefronts 0..2, 4 bytes per lane.
  const unsigned voff = (unsigned)(wave * 1024 + (lane >> 4) * 256 + (((lane & 15) ^ ((wave * 4 + (lane >> 4)) & 15)) << 4));
  const unsigned voff_dd = (unsigned)((wave * 64 + lane) * 4);
  auto stage = [&](int sel, int buf) {
    const int tile = A.tile_first + sel * A.tile_stride;
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(A.dbh) + (size_t)tile * SC_TILE_BYTES;
    const unsigned l = lds_base + buf * SC_TILE_BYTES + wave * 1024;
    constexpr int STEP = NW * 1024;   // bytes between a wavefront's pieces (the same in the source tile and in LDS)
#pragma unroll
    for (int g = 0; g < 32 / NW; g += 4)
      dma16x4(voff, tb + g * STEP, tb + (g + 1) * STEP, tb + (g + 2) * STEP, tb + (g + 3) * STEP, l + g * STEP, l + (g + 1) * STEP,
              l + (g + 2) * STEP, l + (g + 3) * STEP);
    if (wave < 3)
      dma4(voff_dd, A.dneg + (size_t)tile * SC_DD, lds_base + SC_NBUF * SC_TILE_BYTES + buf * (SC_DD * 4) + wave * 256);
  };

#ifdef SC_PROF
  const unsigned long long t_start = __builtin_amdgcn_s_memtime(), r_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long t_wait = 0;
#endif
#pragma unroll
  for (int j = 0; j < SC_GROUP; ++j)
    if (sel_begin + j < sel_end) stage(sel_begin + j, j);
  // ---- B operands: this lane's query of each block, k = 16 s + 8 half .. + 7 of every k-step s ----
  half8 bq[NQB][8];
#pragma unroll
  for (int nb = 0; nb < NQB; ++nb) {
    const _Float16* row = A.qh + (size_t)(q0 + nb * 32 + l32) * DIM + 8 * half;
#pragma unroll
    for (int s = 0; s < 8; ++s) bq[nb][s] = *reinterpret_cast<const half8*>(row + 16 * s);
  }
  // ---- per-query state ----
  float b1[NQB], b2[NQB], tau[NQB];
  int n_rec[NQB];
#pragma unroll
  for (int nb = 0; nb < NQB; ++nb) {
    b1[nb] = -__builtin_inff();
    b2[nb] = -__builtin_inff();
    tau[nb] = __builtin_inff();
    n_rec[nb] = 0;
    if (MODE == 1) tau[nb] = A.tau[q0 + nb * 32 + l32];
  }
  // vmcnt(0) as a builtin, not asm: hipcc must KNOW that the B operands (and everything else) have arrived, or it
  // keeps counted vmcnt waits for them inside the tile loop -- where they would wait for the LDS-DMA of the next tile
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  // ---- what a lane does with one finished 32 x 32 block: 16 rows of one of its queries ----
  // pass A: running top-2 values
  // (the two largest BLOCK MAXIMA, not the two largest values: 10 instructions per block instead of 32.  Two blocks
  // are different rows, so the second largest block maximum is still some second row's value -- a lower bound of the
  // query's second best, weaker than the exact one only when a lane's two best rows sit in the same 16-row group)
  auto fold_a = [&](const v16f& acc, int nb) {
    float m = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) m = fmaxf(fmaxf(m, acc[r]), acc[r + 1]);
    m = fmaxf(m, acc[15]);
    b2[nb] = __builtin_amdgcn_fmed3f(b1[nb], b2[nb], m);
    b1[nb] = fmaxf(b1[nb], m);
  };
  // pass B, rare part: this lane has rows above its query's threshold -> one record.  The record does not go to
  // memory now: the s_waitcnt vmcnt(0) that ends every tile (it is there for the LDS-DMA) would wait for the store's
  // round trip too, and the tile's barrier would hand that wait to all eight wavefronts.  It is parked in the
  // wavefront's LDS buffer {destination slot, row0, bits} and written out when the workgroup is done.
  uint4* const recbuf = reinterpret_cast<uint4*>(lds + SC_LDS_TILES + wave * (SC_RECBUF * SC_REC_BYTES));
  int n_parked = 0;   // records parked so far: wave-uniform (advanced by the hit lanes' count outside the divergent part)
  // `acc` = the block's 16 DOT PRODUCTS (pass B's accumulators start at zero), `top` their maximum, `thr` = tau - the
  // row block's largest -dd/2: dot > thr holds for every row whose screen value dot - dd/2 exceeds tau, and for hardly
  // any other (a superset is all pass C needs).
  // A record from a block's 16 dots: which of them exceed thr (bit r = sign(thr - acc[r]), shifted in from r = 15
  // down), and the largest dot + the block's largest -dd/2 -- an upper bound of the block's largest screen value, at
  // most the block's spread of -dd/2 above it -- as an f16 of its distance above tau (a small positive number, so the
  // f16 costs ~1e-5 and not 5e-4): pass C ranks the records by it and runs the exact arithmetic only on those that can
  // still hold one of the two nearest rows.
  auto record_bits = [](const v16f& acc, float top, float thr) {
    unsigned bits = 0;
#pragma unroll
    for (int r = 15; r >= 0; --r) bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(thr - acc[r]), 31);
    return (bits & 0xFFFFu) | ((unsigned)screen_record_value(top, thr) << 16);
  };
  // The hit path proper is as short as it can be -- a wavefront meets four or five hit blocks per tile and every
  // cycle it spends here its MFMAs do not issue (a quarter of pass B before this): the lane takes a slot of its
  // sub-list and parks the block's raw values in the wavefront's LDS buffer; the record is made from them when the
  // workgroup is done, all lanes in parallel.  Only when the buffer or the sub-list is full is it made on the spot.
  auto emit = [&](const v16f& acc, int nb, int row0, float top, float thr, int pos) {
    const int q = q0 + nb * 32 + l32;
    if (n_rec[nb] < A.sub_cap) {
      const unsigned dst = (unsigned)q * SC_SLOT_PITCH + (2 * split + half) * A.sub_cap + n_rec[nb];
      ++n_rec[nb];
      if (pos < SC_RECBUF) {
        uint4* e = recbuf + 5 * pos;
        e[0] = make_uint4(dst, (unsigned)row0, __float_as_uint(thr), __float_as_uint(top));
#pragma unroll
        for (int g = 0; g < 4; ++g)
          e[1 + g] = make_uint4(__float_as_uint(acc[4 * g]), __float_as_uint(acc[4 * g + 1]), __float_as_uint(acc[4 * g + 2]),
                                __float_as_uint(acc[4 * g + 3]));
      } else {
        A.recs[dst] = make_uint2((unsigned)row0, record_bits(acc, top, thr));   // buffer full
      }
    } else {
      // the lane's sub-list is full: the query's overflow list (rare)
      const int opos = atomicAdd(&A.ovf_cnt[q], 1);
      if (opos < A.ovf_cap) A.ovf[(size_t)q * A.ovf_cap + opos] = make_uint2((unsigned)row0, record_bits(acc, top, thr));
      if (pos < SC_RECBUF) recbuf[5 * pos] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);   // its place in the buffer stays empty
    }
  };
  // the hit lanes of a block get consecutive places in the wavefront's buffer: ballot + prefix count, no LDS atomic
  // (its round trip was a quarter of the hit path)
  auto emit_hits = [&](bool hit, const v16f& acc, int nb, int row0, float top, float thr) {
    const unsigned long long hm = __ballot(hit);
    if (hm == 0ull) return;
    if (hit)
      emit(acc, nb, row0, top, thr,
           n_parked + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u)));
    n_parked += __popcll(hm);
  };

  // the parked records to their slots (all lanes in parallel); the buffer is empty afterwards
  auto flush_parked = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = min(n_parked, SC_RECBUF);
    for (int j = lane; j < n; j += 64) {
      const uint4 e = recbuf[5 * j];
      if (e.x == 0xFFFFFFFFu) continue;
      v16f v;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint4 x = recbuf[5 * j + 1 + g];
        v[4 * g] = __uint_as_float(x.x);
        v[4 * g + 1] = __uint_as_float(x.y);
        v[4 * g + 2] = __uint_as_float(x.z);
        v[4 * g + 3] = __uint_as_float(x.w);
      }
      A.recs[e.x] = make_uint2(e.y, record_bits(v, __uint_as_float(e.w), __uint_as_float(e.z)));
    }
    __builtin_amdgcn_wave_barrier();   // (everybody has read its entries before the next hit overwrites them)
    n_parked = 0;
  };

  const int swz = l32 & 15;
  // A operands of a row block: row rb * 32 + l32, k-step s -> chunk 2 s + half, stored at position chunk ^ (row & 15);
  // accumulator register r belongs to row (r & 3) + 8 (r >> 2) + 4 half of the block: its -dd/2 goes in as C
  auto load_rb = [&](const unsigned char* T, const float* ddp, int rb, half8 (&a)[8], v16f& init) {
    const unsigned char* rowp = T + (rb * 32 + l32) * 256;
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = *reinterpret_cast<const half8*>(rowp + (((2 * s + half) ^ swz) << 4));
    if (MODE == 1) return;   // pass B's accumulators start at zero
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(ddp + rb * 32 + 8 * g + 4 * half);
      init[4 * g] = v.x;
      init[4 * g + 1] = v.y;
      init[4 * g + 2] = v.z;
      init[4 * g + 3] = v.w;
    }
  };

#ifdef SC_PROF
  const unsigned long long t_loop = __builtin_amdgcn_s_memtime();
#endif
  int side = 0;         // which half of the LDS buffers holds the current group of tiles
  v16f pend;            // pass B: the block whose MFMAs were issued last; looked at behind the next block's MFMAs
  float pend_hi = 0.f;  // ... and the largest -dd/2 of its row block
  int pend_row0 = 0;    // (its query block is (nb + NQB - 1) % NQB when block nb is issued: a constant after unrolling --
  bool have_pend = false;   // a run-time index would put tau[] and n_rec[] into scratch memory)
  for (int grp = sel_begin; grp < sel_end; grp += SC_GROUP) {
    const bool more = grp + SC_GROUP < sel_end;
    if (!SC_ABL(1)) {
#pragma unroll
      for (int j = 0; j < SC_GROUP; ++j)
        if (grp + SC_GROUP + j < sel_end) stage(grp + SC_GROUP + j, (side ^ 1) * SC_GROUP + j);
    }
#pragma unroll 1
    for (int j = 0; j < SC_GROUP; ++j) {
    const int sel = grp + j;
    if (sel >= sel_end) break;
    const int buf = SC_ABL(1) ? 0 : side * SC_GROUP + j;
    const unsigned char* T = lds + buf * SC_TILE_BYTES;
    const float* ddp = reinterpret_cast<const float*>(lds + SC_NBUF * SC_TILE_BYTES + buf * (SC_DD * 4));
    const int row_tile = (A.tile_first + sel * A.tile_stride) * SC_TILE;
    if (MODE == 0) {
#pragma unroll 1   // (pass A unrolled: 123 spilled registers at three query blocks)
      for (int rb = 0; rb < SC_TILE / 32; ++rb) {
        half8 a[8];
        v16f init;
        load_rb(T, ddp, rb, a, init);
#pragma unroll
        for (int nb = 0; nb < NQB; ++nb) {
          v16f acc = init;
#pragma unroll
          for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], bq[nb][s], acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);   // (left alone, the scheduler overlaps several blocks' accumulators and spills)
          fold_a(acc, nb);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
      // Software pipeline: while the MFMAs of block b are issued, (1) the A operands of the NEXT row block arrive from
      // LDS and (2) the maximum over the 16 values of block b - 1 is taken, two values per MFMA -- vector instructions
      // in the shadow of the matrix pipe.  Only a lane whose maximum beats its threshold looks at single values.
      // (three and four query blocks per wavefront: no room for the prefetched copy of the next row block's operands;
      // the other wavefront of the SIMD covers the LDS latency at the head of a row block)
      constexpr bool PREF = NQB <= 2;
      half8 a_cur[8], a_nxt[PREF ? 8 : 1];
      v16f unused;
      const v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (PREF) load_rb(T, ddp, 0, a_cur, unused);
      const float4 hi4 = *reinterpret_cast<const float4*>(ddp + 128);   // the four row blocks' largest -dd/2 (the same for all lanes)
      const float hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
      for (int rb = 0; rb < SC_TILE / 32; ++rb) {
        if constexpr (PREF) {
          if (rb + 1 < SC_TILE / 32) load_rb(T, ddp, rb + 1, a_nxt, unused);
        } else {
          load_rb(T, ddp, rb, a_cur, unused);
        }
        const int row0 = row_tile + rb * 32 + 4 * half;
#pragma unroll
        for (int nb = 0; nb < NQB; ++nb) {
          const int pnb = (nb + NQB - 1) % NQB;
          v16f acc = zero;
          float m = -__builtin_inff();
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            if (!SC_ABL(2)) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_cur[s], bq[nb][s], acc, 0, 0, 0);
            // (nothing behind the first four MFMAs: the pending block's last values are still on their way out of the
            // matrix pipe, and a vector instruction that reads them stalls the wavefront -- and the MFMAs behind it)
            if (have_pend && s >= 4) {
              if (s == 4) m = fmaxf(fmaxf(fmaxf(fmaxf(pend[0], pend[1]), pend[2]), pend[3]), pend[4]);
              else if (s < 7) m = fmaxf(fmaxf(fmaxf(fmaxf(m, pend[4 * s - 15]), pend[4 * s - 14]), pend[4 * s - 13]), pend[4 * s - 12]);
              else m = fmaxf(fmaxf(fmaxf(m, pend[13]), pend[14]), pend[15]);
            }
          }
          // pin the interleave: four MFMAs, then one MFMA and the two vector instructions of its shadow, four times
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
#pragma unroll
          for (int s = 4; s < 8; ++s) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (have_pend && !SC_ABL(0)) emit_hits(m > tau[pnb] - pend_hi, pend, pnb, pend_row0, m, tau[pnb] - pend_hi);
          __builtin_amdgcn_sched_barrier(0);
          pend = acc;
          pend_row0 = row0;
          pend_hi = hi[rb];
          have_pend = true;
        }
        if constexpr (PREF) {
          if (rb + 1 < SC_TILE / 32) {
#pragma unroll
            for (int s = 0; s < 8; ++s) a_cur[s] = a_nxt[s];
          }
        }
      }
    }
    }   // tiles of the group
#ifdef SC_PROF
    const unsigned long long t_w0 = __builtin_amdgcn_s_memtime();
#endif
    // a small buffer (four-wavefront workgroups) is written out when three quarters full -- behind the tile's wait for the
    // next tile's pieces, so that the stores' round trip is not in it
    const bool flush_now = MODE == 1 && NW < 8 && n_parked > SC_RECBUF * 3 / 4;
    if (!SC_ABL(3)) {   // (experiment builds: 8 = no end-of-tile wait and barrier -- what the synchronisation costs)
    if (more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wavefront's pieces of the next group have landed
    __syncthreads();   // everybody's pieces have; nobody reads this group's buffers any more
    }
    if (flush_now) flush_parked();
#ifdef SC_PROF
    t_wait += __builtin_amdgcn_s_memtime() - t_w0;
#endif
    side ^= 1;
  }
  if (MODE == 1 && have_pend) {
    float m = pend[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, pend[r]);
    emit_hits(m > tau[NQB - 1] - pend_hi, pend, NQB - 1, pend_row0, m, tau[NQB - 1] - pend_hi);
  }
  if (MODE == 1) flush_parked();
#ifdef SC_PROF
  if (MODE == 1 && tid == 0) {
    atomicAdd(&g_sc_prof[0], __builtin_amdgcn_s_memtime() - t_start);       // shader cycles of the workgroup
    atomicAdd(&g_sc_prof[1], __builtin_amdgcn_s_memrealtime() - r_start);   // 100 MHz ticks
    atomicAdd(&g_sc_prof[2], t_wait);                                       // cycles in the end-of-tile wait + barrier
    atomicAdd(&g_sc_prof[3], (unsigned long long)(sel_end - sel_begin));
    atomicAdd(&g_sc_prof[4], 1ull);
    atomicAdd(&g_sc_prof[5], t_loop - t_start);                             // prologue
    if (SC_ABL(0)) A.part[0].x = b1[0] + pend[3];
  }
#endif

  if (MODE == 0) {
    // the two halves of the wavefront hold different rows of the same queries
#pragma unroll
    for (int nb = 0; nb < NQB; ++nb) {
      const float ob = __shfl_xor(b1[nb], 32), os = __shfl_xor(b2[nb], 32);
      const float S = fmaxf(fminf(b1[nb], ob), fmaxf(b2[nb], os));
      const float B = fmaxf(b1[nb], ob);
      const int q = q0 + nb * 32 + l32;
      if (half == 0 && q < A.q_pad) A.part[(size_t)split * A.q_pad + q] = make_float2(B, S);
    }
  }
}

// ---- passes A and B on v_mfma_f32_16x16x32_f16 ------------------------------------------------------------------
// The same passes with the other f16 MFMA shape.  On random operands out of registers, two wavefronts per SIMD, every
// CU busy, the 16x16x32 instruction sustains 1 842 TFLOP/s on this part and the 32x32x16 one 1 625 (the power budget's
// clock, not the issue rate: scripts/experiments/mfma_shapes_rate.hip, profiles/r03_mfma_shapes_rate.txt) -- pass B on
// 32x32x16 ran at 83% of what that instruction can deliver at all.
// A 32-query x 32-row block is 2 x 2 tiles of 16 x 16 and four k-steps of 32: 16 MFMAs of 16 cycles (the other shape: 8
// of 32).  Operands (cdna_hip_programming.md 3): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k][col l & 15];
// result register r of a tile: col = l & 15, row = 4 (l >> 4) + r.  Rows (A) = DB rows, columns (B) = queries, so a
// lane holds, of a block, TWO queries (l & 15 of either 16-query tile) x EIGHT rows (16 ti + 4 (l >> 4) + r): the four
// "quarters" l >> 4 of a wavefront see different rows of the same queries.  What follows from that:
//   - per-query state (thresholds, running maxima, record counts) is [query block][2] per lane;
//   - a record covers the 8 rows a lane holds of one query in a block: row0 = block + 4 quarter, bit 4 ti + r = row
//     row0 + r + 16 ti; bit 31 of the record's row word marks the layout for pass C (the 32x32x16 records: bit r = row
//     row0 + (r & 3) + 8 (r >> 2), 16 rows, all 16 mask bits in use);
//   - a query's records go to ONE counted list (SC_SLOT_PITCH's comment), appended when the parked hits are written out;
//   - pass A folds the lane's 8 rows of a block into ONE maximum per query (two blocks are still different rows).
// Staging, swizzle (chunk ^ (row & 15): a 16-lane group reads 16 rows at one chunk index -- all 64 banks once), the
// XCD-aware unit map, the parked records and the exactness argument are those of screen_kernel.
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int SC_REC16_BYTES = 48;                  // {slot, row0, thr, top, 8 dots}
// Parked hits per wavefront: what the 160 KB of a compute unit leave beside the tiles and the thresholds (the 256-register
// workgroup has the CU to itself whatever its LDS), 11.25 KB.  A hit that finds the buffer full appends from the hit path
// with an atomic add whose value it waits for, and seven wavefronts wait for it at the tile's barrier: with 170 places (8
// KB) 51 775 hits of a judged launch did; profiles/wave_sublists_ab.txt has what pass B costs without any.
constexpr int SC_RECBUF16 = 240;
constexpr int SC_LDS16_TAU = SC_LDS_TILES + 8 * SC_RECBUF16 * SC_REC16_BYTES;   // the wavefronts' thresholds: 8 x 128 floats
constexpr int SC_LDS16_BYTES = SC_LDS16_TAU + 8 * 128 * 4;
static_assert(SC_LDS16_BYTES <= 160 * 1024, "screen16_kernel's LDS fits a gfx950 compute unit");

// Experiment builds, PLACES (MH_SCREEN_PLACES; WRONG results, timing only -- what the places' atomic adds cost pass B,
// profiles/wave_sublists_ab.txt): 1 = flush_parked takes a record's place from lane arithmetic instead of the atomic add
// (the stores stay), 2 = so does the buffer-full branch of `emit` as well (no atomic left in the hit path), 3 = the product's
// kernel.  (0, this build's default, also counts the hits that find the buffer full -- g_sc_direct_appends, an atomic of
// its own in the hit path and four spilled registers more; 1, 2 and 3 do not.)
#ifdef MH_EXPERIMENTS
template <int MODE, int NQB, int PLACES = 0>
#else
template <int MODE, int NQB>
#endif
__global__ __launch_bounds__(512, 2) void screen16_kernel(const ScreenArgs A) {
#ifndef MH_EXPERIMENTS
  constexpr int PLACES = 0;
#endif
  MH_TRACE_SCOPE(MODE == 0 ? mh::TK_PASS_A : mh::TK_PASS_B);
  constexpr int NW = 8;
  constexpr int QW = 32 * NQB;            // queries per wavefront
  constexpr int QB = QW * NW;             // queries per workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quarter = lane >> 4, l16 = lane & 15;
  const unsigned lds_base = (unsigned)(uintptr_t)(MH_AS3 unsigned char*)lds;
  const int nqb = gridDim.x / A.n_splits;
  int qblock, split;
  {
    const int L = blockIdx.x, U = gridDim.x;
    const int x = L & 7, j = L >> 3;
    const int unit = x * (U >> 3) + min(x, U & 7) + j;
    split = unit / nqb;
    qblock = unit - split * nqb;
  }
  const int Qe = A.q_count ? min(A.Q, *A.q_count) : A.Q;
  if (qblock * QB >= Qe) return;   // uniform over the workgroup
  const int q0 = qblock * QB + wave * QW;
  const bool live = q0 < Qe;   // uniform over the wavefront
  const int sel_begin = split * A.tiles_base + min(split, A.tiles_rem);
  const int sel_end = min(sel_begin + A.tiles_base + (split < A.tiles_rem ? 1 : 0), A.n_sel);

  const unsigned voff = (unsigned)(wave * 1024 + (lane >> 4) * 256 + (((lane & 15) ^ ((wave * 4 + (lane >> 4)) & 15)) << 4));
  const unsigned voff_dd = (unsigned)((wave * 64 + lane) * 4);
  // The sweep's tiles.  Pass A: tile_first + sel * tile_stride.  Pass B of a one-sweep launch: the sel-th tile pass A did
  // NOT see (those are skip_first + i * skip_stride) -- the tile number runs along with `sel`, and `gap` counts the
  // tiles left before the next one to jump over; the one division is here, in front of the loop.
  int tile_cur = A.tile_first + sel_begin * A.tile_stride, gap_cur = 0x7FFFFFFF;
  if (MODE == 1 && A.skip_stride > 1) {
    const int d = A.skip_stride - 1;
    if (sel_begin < A.skip_first) {
      tile_cur = sel_begin;
      gap_cur = A.skip_first - sel_begin;
    } else {
      const int jj = sel_begin - A.skip_first;
      tile_cur = sel_begin + 1 + jj / d;
      gap_cur = d - jj % d;
    }
  }
  auto stage = [&](int tile, int buf) {
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(A.dbh) + (size_t)tile * SC_TILE_BYTES;
    const unsigned l = lds_base + buf * SC_TILE_BYTES + wave * 1024;
    dma16x4(voff, tb, tb + 8192, tb + 16384, tb + 24576, l, l + 8192, l + 16384, l + 24576);
    if (wave < 3)
      dma4(voff_dd, A.dneg + (size_t)tile * SC_DD, lds_base + SC_NBUF * SC_TILE_BYTES + buf * (SC_DD * 4) + wave * 256);
  };
  if (sel_begin < sel_end) stage(tile_cur, 0);
  // ---- B operands: the lane's query of either 16-query tile of each block, k = 32 s + 8 quarter .. + 7 ----
  half8 bq[NQB][2][4];
#pragma unroll
  for (int nb = 0; nb < NQB; ++nb)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const _Float16* row = A.qh + (size_t)(q0 + nb * 32 + 16 * tj + l16) * DIM + 8 * quarter;
#pragma unroll
      for (int s = 0; s < 4; ++s) bq[nb][tj][s] = *reinterpret_cast<const half8*>(row + 32 * s);
    }
  // per-query state of the lane's 2 NQB queries.  Pass B is at the register limit (128 for the queries' operands, 32 + 16
  // + 16 for a row block's fragments, the accumulators and the pending block): the thresholds wait in LDS (two ds_read_b32
  // per block, in the MFMAs' shadow), and nobody counts records here: the queries' counts live in memory (flush_parked).
  // pass A: the lane's SC_TOPK largest packed block maxima per query, sorted, and the next largest value
  float pk[NQB][2][SC_PART5];
  float* const tau_lds = reinterpret_cast<float*>(lds + SC_LDS16_TAU) + wave * 128;
#pragma unroll
  for (int nb = 0; nb < NQB; ++nb)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int k = 0; k < SC_PART5; ++k) pk[nb][tj][k] = -__builtin_inff();
  if (MODE == 1)
    for (int i = lane; i < QW; i += 64) tau_lds[i] = A.tau[q0 + i];
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  uint4* const recbuf = reinterpret_cast<uint4*>(lds + SC_LDS_TILES + wave * (SC_RECBUF16 * SC_REC16_BYTES));
  int n_parked = 0;
  // a record from the lane's 8 dots of one query: bit 4 ti + r = sign(thr - dot)
  auto record_bits8 = [](const v4f& d0, const v4f& d1, float top, float thr) {
    unsigned bits = 0;
#pragma unroll
    for (int r = 3; r >= 0; --r) bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(thr - d1[r]), 31);
#pragma unroll
    for (int r = 3; r >= 0; --r) bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(thr - d0[r]), 31);
    return (bits & 0xFFu) | ((unsigned)screen_record_value(top, thr) << 16);
  };
  // one more record into query q's list (the top of the file, "ONE counted list per query"): the place comes from the
  // query's count; a record past the list's end is dropped, the count says so to pass C
  auto append = [&](int q, int at, unsigned row0, unsigned bits) {
    if (at < SC_SLOT_PITCH) A.recs[(size_t)q * SC_SLOT_PITCH + at] = make_uint2(row0 | SC_REC_LAYOUT16, bits);
  };
  // a hit waits in the wavefront's LDS buffer {q, row0, thr, top, 8 dots} for flush_parked; nothing here touches memory
  // unless that buffer is full (an average sweep parks ~128 hits per wavefront against SC_RECBUF16 places)
  auto emit = [&](const v4f& d0, const v4f& d1, int q, int row0, float top, float thr, int pos) {
    if (pos < SC_RECBUF16) {
      uint4* e = recbuf + 3 * pos;
      e[0] = make_uint4((unsigned)q, (unsigned)row0, __float_as_uint(thr), __float_as_uint(top));
      e[1] = make_uint4(__float_as_uint(d0[0]), __float_as_uint(d0[1]), __float_as_uint(d0[2]), __float_as_uint(d0[3]));
      e[2] = make_uint4(__float_as_uint(d1[0]), __float_as_uint(d1[1]), __float_as_uint(d1[2]), __float_as_uint(d1[3]));
    } else {
#ifdef MH_EXPERIMENTS
      if (PLACES == 0) atomicAdd(&g_sc_direct_appends, 1ull);
#endif
      // buffer full.  (The list's address is worked out HERE: the lane's eight queries never change, and the compiler
      // would keep eight 64-bit addresses across the sweep for this branch alone -- 16 registers this kernel does not have.)
      const int at = PLACES == 2 ? SC_SA_SLOTS + (pos & 3) * A.n_splits + split : atomicAdd(&A.ovf_cnt[q], 1);
      int qa = q;
      asm volatile("" : "+v"(qa));
      append(qa, at, (unsigned)row0, record_bits8(d0, d1, top, thr));
    }
  };
  // the pending block: acc[ti][tj]; query tj of the lane = tiles (0, tj) and (1, tj)
  auto emit_block = [&](bool hit0, bool hit1, const v4f (&p)[2][2], int nb, int row0, float m0, float m1, float thr0, float thr1) {
    const unsigned long long h0 = __ballot(hit0), h1 = __ballot(hit1);
    if ((h0 | h1) == 0ull) return;
    if (hit0)
      emit(p[0][0], p[1][0], q0 + nb * 32 + l16, row0, m0, thr0,
           n_parked + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(h0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)h0, 0u)));
    n_parked += __popcll(h0);
    if (hit1)
      emit(p[0][1], p[1][1], q0 + nb * 32 + 16 + l16, row0, m1, thr1,
           n_parked + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(h1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)h1, 0u)));
    n_parked += __popcll(h1);
  };
  // The wavefront's parked hits go to their queries' lists: lane j takes the parked records j, j + 64, j + 128, j + 192.  Every
  // atomic add of the flush is issued before the first returned place is looked at -- one round trip, at the end of the
  // workgroup's sweep, outside the hit path.
  auto flush_parked = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int TRIPS = (SC_RECBUF16 + 63) / 64;
    const int n = min(n_parked, SC_RECBUF16);
    uint4 e[TRIPS];
    int at[TRIPS];
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
      e[i] = make_uint4(0u, 0u, 0u, 0u);
      if (lane + 64 * i < n) e[i] = recbuf[3 * (lane + 64 * i)];
    }
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
      at[i] = SC_SLOT_PITCH;
      if (lane + 64 * i < n) at[i] = PLACES == 1 || PLACES == 2 ? SC_SA_SLOTS + ((lane + i) & 3) * A.n_splits + split : atomicAdd(&A.ovf_cnt[e[i].x], 1);
    }
#pragma unroll
    for (int i = 0; i < TRIPS; ++i)
      if (at[i] < SC_SLOT_PITCH) {
        const int j = lane + 64 * i;
        const uint4 x0 = recbuf[3 * j + 1], x1 = recbuf[3 * j + 2];
        const v4f d0 = {__uint_as_float(x0.x), __uint_as_float(x0.y), __uint_as_float(x0.z), __uint_as_float(x0.w)};
        const v4f d1 = {__uint_as_float(x1.x), __uint_as_float(x1.y), __uint_as_float(x1.z), __uint_as_float(x1.w)};
        append((int)e[i].x, at[i], e[i].y, record_bits8(d0, d1, __uint_as_float(e[i].w), __uint_as_float(e[i].z)));
      }
    __builtin_amdgcn_wave_barrier();
    n_parked = 0;
  };

  // A operands of a row block: tile ti = rows rb 32 + 16 ti + l16, k-step s -> chunk 4 s + quarter at position
  // chunk ^ (row & 15) = chunk ^ l16
  auto load_rb = [&](const unsigned char* T, int rb, half8 (&a)[2][4]) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const unsigned char* rowp = T + (rb * 32 + 16 * ti + l16) * 256;
#pragma unroll
      for (int s = 0; s < 4; ++s) a[ti][s] = *reinterpret_cast<const half8*>(rowp + (((4 * s + quarter) ^ l16) << 4));
    }
  };
  // (as instructions: fmaxf() quiets every operand first -- a v_max_f32 x, x per value, 28 vector instructions per block
  // where 8 do; the dots of finite operands are never NaN)
  auto max3 = [](float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
  };
  auto max8 = [&](const v4f& x, const v4f& y) {
    return max3(max3(max3(x[0], x[1], x[2]), x[3], y[0]), max3(y[1], y[2], y[3]), -__builtin_inff());
  };
  // Pass A takes the maxima of a block whose MFMAs have JUST been issued (pass B looks at the block before): hipcc pads
  // no wait states between a matrix instruction and an asm statement that reads its result, and the last two
  // accumulators then read as what the registers held before (a block maximum that misses rows 17..19 of its lane's
  // eight: harmless for a threshold that only has to be low enough, fatal for a hand-over).  So both queries' maxima
  // are ONE statement that opens with the wait states of an 8-pass MFMA's result (11; 16 here), floored for the packing.
  auto max8x2_after_mfma = [](const v4f (&acc)[2][2], float floor, float& m0, float& m1) {
    float t0, t1;
    asm("s_nop 7\n\ts_nop 7\n\t"
        "v_max3_f32 %0, %4, %5, %6\n\t"
        "v_max3_f32 %1, %12, %13, %14\n\t"
        "v_max3_f32 %2, %9, %10, %11\n\t"
        "v_max3_f32 %3, %17, %18, %19\n\t"
        "v_max3_f32 %0, %0, %7, %8\n\t"
        "v_max3_f32 %1, %1, %15, %16\n\t"
        "v_max3_f32 %0, %0, %2, %20\n\t"
        "v_max3_f32 %1, %1, %3, %20"
        : "=&v"(m0), "=&v"(m1), "=&v"(t0), "=&v"(t1)
        : "v"(acc[0][0][0]), "v"(acc[0][0][1]), "v"(acc[0][0][2]), "v"(acc[0][0][3]), "v"(acc[1][0][0]), "v"(acc[1][0][1]),
          "v"(acc[1][0][2]), "v"(acc[1][0][3]), "v"(acc[0][1][0]), "v"(acc[0][1][1]), "v"(acc[0][1][2]), "v"(acc[0][1][3]),
          "v"(acc[1][1][0]), "v"(acc[1][1][1]), "v"(acc[1][1][2]), "v"(acc[1][1][3]), "v"(floor));
  };
  auto max2 = [](float a, float b) {   // (as an instruction, like max3: the packed values are never NaN)
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  };

  int side = 0;
  // the pending block starts as one no threshold lets through (its dots -inf): the loop needs no "is there one yet"
  const v4f ninf4 = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  v4f pend[2][2] = {{ninf4, ninf4}, {ninf4, ninf4}};
  float pend_hi = 0.f;
  int pend_row0 = 0;
  const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
  {
  MH_TRACE_PHASE(trace_loop_, MODE == 1 ? mh::TK_PASS_B_LOOP : mh::TK_PASS_A_LOOP);
  for (int sel = sel_begin; sel < sel_end; ++sel) {
    const bool more = sel + 1 < sel_end;
    int tile_nxt = tile_cur + (MODE == 0 ? A.tile_stride : 1), gap_nxt = gap_cur - 1;
    if (gap_nxt == 0) {   // the next tile is one of pass A's: over it
      tile_nxt += 1;
      gap_nxt = A.skip_stride - 1;
    }
    if (more) stage(tile_nxt, side ^ 1);
    const unsigned char* T = lds + side * SC_TILE_BYTES;
    const float* ddp = reinterpret_cast<const float*>(lds + SC_NBUF * SC_TILE_BYTES + side * (SC_DD * 4));
    const int row_tile = tile_cur * SC_TILE;
    tile_cur = tile_nxt;
    gap_cur = gap_nxt;
    // (a wavefront none of whose 128 queries exists -- the tail of the last query block -- only helps with the staging
    // and the barriers: the SIMD's matrix pipe is then its neighbour's alone)
    if (!live) {
    } else if (MODE == 0) {
#pragma unroll 1
      for (int rb = 0; rb < SC_TILE / 32; ++rb) {
        half8 a[2][4];
        load_rb(T, rb, a);
        const unsigned blk = (unsigned)((sel - sel_begin) * 4 + rb) & ~A.pack_keep;   // the block's number inside the lane slot
        v4f init[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
          const float4 v = *reinterpret_cast<const float4*>(ddp + rb * 32 + 16 * ti + 4 * quarter);
          init[ti] = v4f{v.x, v.y, v.z, v.w};
        }
#pragma unroll
        for (int nb = 0; nb < NQB; ++nb) {
          v4f acc[2][2] = {{init[0], init[0]}, {init[1], init[1]}};
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
              for (int tj = 0; tj < 2; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ti][s], bq[nb][tj][s], acc[ti][tj], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          float mx[2];
          max8x2_after_mfma(acc, SC_PACK_FLOOR, mx[0], mx[1]);
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) {
            // the block's maximum with its number in the low mantissa bits, into the sorted list: level k becomes the
            // median of (level k - 1, level k, new) -- from the bottom up, every level from the OLD level above it
            const float m = __uint_as_float((__float_as_uint(mx[tj]) & A.pack_keep) | blk);
            float(&p)[SC_PART5] = pk[nb][tj];
#pragma unroll
            for (int k = SC_PART5 - 1; k > 0; --k) p[k] = __builtin_amdgcn_fmed3f(p[k - 1], p[k], m);
            p[0] = max2(p[0], m);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
      const float4 hi4 = *reinterpret_cast<const float4*>(ddp + 128);
      const float hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
      for (int rb = 0; rb < SC_TILE / 32; ++rb) {
        half8 a[2][4];
        load_rb(T, rb, a);
        const int row0 = row_tile + rb * 32 + 4 * quarter;
#pragma unroll
        for (int nb = 0; nb < NQB; ++nb) {
          const int pnb = (nb + NQB - 1) % NQB;
          v4f acc[2][2] = {{zero4, zero4}, {zero4, zero4}};
          float m0 = -__builtin_inff(), m1 = -__builtin_inff();
          const float t0 = tau_lds[pnb * 32 + l16], t1 = tau_lds[pnb * 32 + 16 + l16];   // the pending block's thresholds
#pragma unroll
          for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
              for (int tj = 0; tj < 2; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ti][s], bq[nb][tj][s], acc[ti][tj], 0, 0, 0);
            // the pending block's maxima in the shadow of the second half of the MFMAs (its values have left the pipe by then)
            if (s == 2) m0 = max8(pend[0][0], pend[1][0]);
            if (s == 3) m1 = max8(pend[0][1], pend[1][1]);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          {
            const float thr0 = t0 - pend_hi, thr1 = t1 - pend_hi;
            emit_block(m0 > thr0, m1 > thr1, pend, pnb, pend_row0, m0, m1, thr0, thr1);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) pend[ti][tj] = acc[ti][tj];
          pend_row0 = row0;
          pend_hi = hi[rb];
        }
      }
    }
    if (more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    side ^= 1;
  }
  }
  if (MODE == 1) {
    {
      const float m0 = max8(pend[0][0], pend[1][0]), m1 = max8(pend[0][1], pend[1][1]);
      const float thr0 = tau_lds[(NQB - 1) * 32 + l16] - pend_hi, thr1 = tau_lds[(NQB - 1) * 32 + 16 + l16] - pend_hi;
      emit_block(m0 > thr0, m1 > thr1, pend, NQB - 1, pend_row0, m0, m1, thr0, thr1);
    }
    flush_parked();
  }
  if (MODE == 0) {
    // every lane its own lists (the four quarters of the wavefront hold different rows of the same queries: four lane
    // slots); 16 lanes = 16 neighbouring queries = one 64-byte line per store
#pragma unroll
    for (int nb = 0; nb < NQB; ++nb)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const int q = q0 + nb * 32 + 16 * tj + l16;
        if (q < A.q_pad) {
#pragma unroll
          for (int k = 0; k < SC_PART5; ++k) A.part5[((size_t)(split * 4 + quarter) * SC_PART5 + k) * A.q_pad + q] = pk[nb][tj][k];
        }
      }
  }
}

// ---- pass C: canonical arithmetic on the candidates ------------------------------------------------
struct Best {
  float b1, b2;
  int i1;
};
// one more row into a running top-2; rows arrive in any order: lower row wins a tie on the best distance,
// b2 = second smallest value.  A first row at distance +inf leaves "none" (i1 = -1) as the exact kernels do.
__device__ __forceinline__ void take(Best& a, float d, int row) {
  const bool better = d < a.b1 || (d == a.b1 && a.i1 >= 0 && row < a.i1);
  const float lose = better ? a.b1 : d;
  a.b2 = fminf(a.b2, lose);
  a.b1 = better ? d : a.b1;
  a.i1 = better ? row : a.i1;
}
__device__ __forceinline__ void merge(Best& a, float ob1, float ob2, int oi1) {   // match.hip's merge
  const bool take_o = (ob1 < a.b1) || (ob1 == a.b1 && (unsigned)oi1 < (unsigned)a.i1);
  const float lose1 = take_o ? a.b1 : ob1;
  const float s2 = fminf(a.b2, ob2);
  a.b2 = fminf(lose1, s2);
  a.b1 = take_o ? ob1 : a.b1;
  a.i1 = take_o ? oi1 : a.i1;
}

// One wavefront per query; every lane runs the canonical chain of one candidate row at a time:
// dot = fmaf chain over k = 0..127 from 0, dist = max(0, fmaf(-2, dot, qq + dd)).  The query's coordinates are
// wave-uniform (LDS broadcast reads), the row comes straight from HBM / the Infinity Cache, 16 bytes per load.
constexpr int RS_WAVES = 4;          // wavefronts per workgroup, one query each
// ... of the accepting kernel (rescore_query's ACCEPT): four fifths of its wavefronts leave after one round trip, and a
// workgroup holds its LDS until its slowest query is done -- one query per workgroup beat four in every round, two did not
// beat four by the rule (profiles/accept_reject_ab.txt)
constexpr int RS_WAVES_ACCEPT = 1;
#ifdef MH_EXPERIMENTS
constexpr int RS_WAVES_FAT = 16;     // ... of a chip-filling launch's fat workgroups, two of which hold a compute unit
constexpr int RS_FAT_K = 2;          // ... and that many of them per compute unit are the whole grid (their wavefronts walk the queries)
#endif
constexpr int RS_MAXC = 1024;        // candidate rows a query may have before it is searched by brute force
constexpr int RS_STAGE = 8;          // candidate rows staged through LDS (8 x 512 bytes = the candidate list's 4 KB)
static_assert(RS_STAGE * DIM * 4 <= RS_MAXC * 4 && RS_STAGE % 2 == 0 && RS_STAGE <= 32, "staged rows live in the candidate list's LDS");

__device__ __forceinline__ float exact_dist(const float* __restrict__ q_lds, const float* __restrict__ row, float nq, float dn) {
  // 64 bytes x 2 in flight per step: 48 VGPRs here (the kernel around it: 64, eight wavefronts per SIMD).  (Round 3: the whole 512-byte row in flight before
  // the chain -- one round trip per row instead of four -- takes 160 VGPRs, three wavefronts per SIMD, and pass C went
  // from 0.047 to 0.071 ms per 24 000 queries: it lives on the number of queries in flight, not on one query's latency.)
  float s = 0.f;
  const float4* r4 = reinterpret_cast<const float4*>(row);
#pragma unroll 2
  for (int c = 0; c < DIM / 16; ++c) {
    const float4 x0 = r4[4 * c], x1 = r4[4 * c + 1], x2 = r4[4 * c + 2], x3 = r4[4 * c + 3];
    const float4 y0 = *reinterpret_cast<const float4*>(q_lds + 16 * c), y1 = *reinterpret_cast<const float4*>(q_lds + 16 * c + 4);
    const float4 y2 = *reinterpret_cast<const float4*>(q_lds + 16 * c + 8), y3 = *reinterpret_cast<const float4*>(q_lds + 16 * c + 12);
    s = fmaf(y0.x, x0.x, s); s = fmaf(y0.y, x0.y, s); s = fmaf(y0.z, x0.z, s); s = fmaf(y0.w, x0.w, s);
    s = fmaf(y1.x, x1.x, s); s = fmaf(y1.y, x1.y, s); s = fmaf(y1.z, x1.z, s); s = fmaf(y1.w, x1.w, s);
    s = fmaf(y2.x, x2.x, s); s = fmaf(y2.y, x2.y, s); s = fmaf(y2.z, x2.z, s); s = fmaf(y2.w, x2.w, s);
    s = fmaf(y3.x, x3.x, s); s = fmaf(y3.y, x3.y, s); s = fmaf(y3.z, x3.z, s); s = fmaf(y3.w, x3.w, s);
  }
  return fmaxf(fmaf(-2.f, s, nq + dn), 0.f);
}

__device__ __forceinline__ void wave_lds_sync() {   // LDS written by some lanes of this wavefront, read by others
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The screen values of the 8 + 8 rows of two sampled blocks (records of screen_handover_kernel: rows row0 + r + 16 ti) for ONE
// query, by pass A's arithmetic: one v_mfma_f32_16x16x32_f16 set, accumulator seeded with the rows' -dd/2, the four k-steps
// in ascending k (screen16_kernel MODE 0, screen_values_kernel shape 2).  Operand row i = l & 15: block X's row bit i for
// i < 8, block Y's row bit i - 8 above; lane l holds k = 32 s + 8 (l >> 4) + j as in the passes; the query -- the f16 of its
// f32 coordinates, the conversion of screen_prepare_kernel -- sits in every column.  An element of the product depends on its
// own row and column only, so these are the values pass A folded into the block's maximum.  Result: lane group g = l >> 4
// holds operand rows 4 g .. 4 g + 3 = block g >> 1, mask bits 4 (g & 1) + r.
__device__ __forceinline__ v4f sample_pair_values(const float* __restrict__ q_lds, const _Float16* __restrict__ dbh,
                                                  const float* __restrict__ dneg, int row0x, int row0y, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int arow = (i < 8 ? row0x : row0y) + (i & 3) + 16 * ((i >> 2) & 1);
  const half8* ap = reinterpret_cast<const half8*>(dbh + (size_t)arow * DIM + 8 * g);
  half8 a[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) a[s] = ap[4 * s];
  const int crow = (g < 2 ? row0x : row0y) + 16 * (g & 1);
  const float4 c = *reinterpret_cast<const float4*>(dneg + (size_t)(crow >> 7) * SC_DD + (crow & 127));
  v4f acc = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float4 y0 = *reinterpret_cast<const float4*>(q_lds + 32 * s + 8 * g), y1 = *reinterpret_cast<const float4*>(q_lds + 32 * s + 8 * g + 4);
    half8 b;
    b[0] = (_Float16)y0.x; b[1] = (_Float16)y0.y; b[2] = (_Float16)y0.z; b[3] = (_Float16)y0.w;
    b[4] = (_Float16)y1.x; b[5] = (_Float16)y1.y; b[6] = (_Float16)y1.z; b[7] = (_Float16)y1.w;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b, acc, 0, 0, 0);
  }
  return acc;
}

// (eight wavefronts per SIMD -- what the kernel's LDS allows -- instead of the five its 82 VGPRs would; the kernel lives on
// queries in flight.  Config 1: 0.096 -> 0.085 ms)
//
// Launch shape.  WAVES wavefronts per workgroup, each with an LDS region of its own (no workgroup barrier anywhere: only
// wave_lds_sync).  Wavefront w of the grid's W = gridDim.x * WAVES takes the queries w, w + W, w + 2 W, ...  The product
// launches a wavefront per query in workgroups of four, so the loop runs once.  The other shapes exist in experiment
// builds (launch_match_screen's MH_PASSC_* switches): workgroups of 16 wavefronts, two per compute unit (or of 12 at six
// wavefronts per SIMD and 80 registers), a grid of RS_FAT_K such workgroups per compute unit whose wavefronts walk, and
// PF = what a walking wavefront asks for one query ahead, at the top of the iteration before (0 = nothing; 1 = the next
// query's record slots; 2 = the slots, the scalars and the row; a query's slots are written by its own wavefront alone,
// so reading them early races with nothing).  None of them paid on top of the product's shape (DESIGN.md 4,
// profiles/passc_persistent_ab.txt).  Where wavefronts walk the striding is static, no ticket: a query that is searched by
// brute force (an overflowed list, a query f16 cannot hold: the whole DB on one wavefront) delays the later queries of
// its own wavefront and nobody else's; tests/test_gpu_passc_persistent.py puts such queries into the first, second and
// third trip of the same wavefronts.
constexpr int RS_ITERS = (SC_SLOT_PITCH + SCREEN_OVF_CAP + 63) / 64;
struct RsScalars {   // what a query's wavefront reads besides its slots before it knows its candidates
  int bad;
  float nq, tau_q;
  int n_ovf;
  unsigned incw;
  float2 qv;
};
// the counters of the pre-rejected queries: query q adds to counter q % RS_PREREJ_WORDS, each on a cache line of its own
// (two thirds of a launch's wavefronts add one: a single word would queue them all in one L2 channel)
constexpr int RS_PREREJ_WORDS = 16, RS_PREREJ_PITCH = 64;
constexpr size_t rs_lds_bytes(int waves) { return (size_t)waves * (DIM * 4 + RS_MAXC * 4 + SC_SA_SLOTS * 4 + 8); }

struct RsArgs {
  const float* qn;
  const float* qnorm;
  const uint8_t* qbad;
  int Q;
  const int32_t* q_count;
  const float* db;
  const float* dnorm;
  int N;
  RowMap rmap;
  uint2* recs;
  int n_slots;
  int32_t* ovf_cnt;
  uint2* ovf;
  int ovf_cap;
  float dmax;
  const float* tau;
  float spread;
  int32_t* idx1;
  float* d1;
  float* d2;
  unsigned int* stats;
  int32_t zero_idx;
  float zero_d1, zero_d2;
  SampleGeom g;
  const unsigned int* inc;
  unsigned int* inc_count;
  const _Float16* dbh;
  const float* dneg;
  // (behind everything else: the kernels that do not ask read the same words at the same offsets as before)
  float accept_ratio;      // > 0: the caller keeps only queries that pass `d1 / d2 < accept_ratio` (screen_reject_proved)
  unsigned int* prerej;    // RS_PREREJ_WORDS counters, RS_PREREJ_PITCH words apart: queries that left by that proof
};
// The kernel's arguments as an iteration of the loop reads them: from the kernel argument segment (the one struct is all
// of it), through a pointer the compiler cannot see through.  Read once in front of the loop they would all live in scalar
// registers across it -- some sixty, with the loop's own more than a wavefront has: 74 of them spilled, and 46 vector
// registers after them -- where the kernel without a loop fetches each next to its use; so does every iteration now.
typedef const __attribute__((address_space(4))) RsArgs* RsArgsPtr;
__device__ __forceinline__ RsArgsPtr rs_args() {
  RsArgsPtr p = (RsArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// a query's slots in scan order: pass B's n_slots, then (one-sweep launches) the sa_slots of the sampled tiles' records,
// which lie behind pass B's SC_SLOTS_MAX; then the overflow list.  COMPACT (the counted list of the 16x16x32 launches):
// the list's first 64 slots, whatever the count -- the slots behind a list's end are empty -- so that they travel with
// the count and the other scalars; a longer list's remaining slots are fetched when the count is known (rescore_query)
constexpr int RS_ITERS_C = (SC_SLOT_PITCH + 63) / 64;   // registers of slots a counted list can fill
template <int COMPACT>
__device__ __forceinline__ void rs_load_slots(const uint2* recs, int n_slots, int sa_slots, int q, int lane, uint2 (&rv)[RS_ITERS]) {
  const uint2* theirs = recs + (size_t)q * SC_SLOT_PITCH;
  if (COMPACT) {
    rv[0] = theirs[lane];
#pragma unroll
    for (int it = 1; it < RS_ITERS; ++it) rv[it] = make_uint2(0u, 0u);
    return;
  }
  const int n_own = n_slots + sa_slots;
#pragma unroll
  for (int it = 0; it < RS_ITERS; ++it) {
    const int j = it * 64 + lane;
    rv[it] = j < n_own ? theirs[j < n_slots ? j : SC_SLOTS_MAX + (j - n_slots)] : make_uint2(0u, 0u);
  }
}
// (qbad, qnorm, tau, inc: written by the launches before this one, read-only here -- read as constant memory they come
// through the scalar unit, all in flight at once, where a global load of a wave-uniform address inside the loop is waited
// for on the spot.  So does the query's overflow count: its wavefront is the only one to write it, and does so after this
// read, so whichever state of the cache line the scalar cache holds has the query's own word right.  The compiler takes
// constant memory for never written: what keeps this read in front of the kernel's own `ovf_cnt[q] = 0` is not the address
// space but the data -- that store is made only `if (n_ovf ...)`, on the value read here -- and no word is read again after
// it was written.  `inc` may be absent.)
#define RS_CONST(T, p) ((const __attribute__((address_space(4))) T*)(p))
__device__ __forceinline__ RsScalars rs_load_scalars(const uint8_t* qbad, const float* qnorm, const float* tau, const int32_t* ovf_cnt,
                                                     const unsigned int* inc, const float* qn, int q, int lane) {
  RsScalars v;
  v.qv = reinterpret_cast<const float2*>(qn + (size_t)q * DIM)[lane];
  v.n_ovf = RS_CONST(int32_t, ovf_cnt)[q];
  const unsigned w = RS_CONST(unsigned int, inc ? inc : reinterpret_cast<const unsigned int*>(tau))[q];
  v.bad = (RS_CONST(unsigned int, qbad)[q >> 2] >> (8 * (q & 3))) & 0xFFu;   // (the byte's word: the scalar unit reads no bytes; [q_pad], q_pad % 256 == 0)
  v.nq = RS_CONST(float, qnorm)[q];
  v.tau_q = RS_CONST(float, tau)[q];
  v.incw = inc ? w : 0u;
  return v;
}

// One query on one wavefront: `recv` its slots and `sc` what else it reads first (asked for by the caller), the four LDS
// regions the wavefront's own.
// COMPACT: the query's records are one counted list (SC_SLOT_PITCH's comment), `sc.n_ovf` its count, `recv[0]` its first
// 64 slots.  Nothing below depends on the ORDER of a query's records, which the appends of concurrent wavefronts leave
// open: the thinning bound is the second largest of the records' lower bounds (max / min folds), the keep / drop test
// looks at one record at a time, candidates and surviving sampled records get their LDS places from counters (the
// sampled pairs are evaluated row by row whatever their pairing), and the exact top-2 breaks ties by row number.
static_assert(RS_ITERS_C <= RS_ITERS, "a counted list's slots fit the registers the scan has");
// ACCEPT: the caller applies the ratio test `accept_ratio` to the result and reads nothing of a query that fails it: a query
// the records' bounds already prove to fail (screen_reject_proved) is answered like an absent one, (-1, inf, inf), after the
// first round trip -- before the sampled records' evaluation, the candidate rows' gather and the chains.  Without ACCEPT
// the code is what it was.
template <int COMPACT, int ACCEPT = 0>
__device__ __forceinline__ void rescore_query(
    int q, int lane, float* q_sw, int* cand_sw, int* samp_sw, int* ncand_sw, int* nsamp_sw, uint2 (&recv)[RS_ITERS], const RsScalars sc, int Qe,
    const float* __restrict__ db, const float* __restrict__ dnorm, int N,
    RowMap rmap, uint2* __restrict__ recs, int n_slots, int32_t* __restrict__ ovf_cnt, uint2* __restrict__ ovf,
    int ovf_cap, float dmax, float spread, int32_t* __restrict__ idx1, float* __restrict__ d1, float* __restrict__ d2,
    unsigned int* __restrict__ stats, int32_t zero_idx, float zero_d1, float zero_d2, SampleGeom g,
    unsigned int* __restrict__ inc_count, const _Float16* __restrict__ dbh, const float* __restrict__ dneg,
    float accept_ratio = 0.f, unsigned int* __restrict__ prerej = nullptr) {
  uint2* mine = recs + (size_t)q * SC_SLOT_PITCH;
  // (COMPACT: the records the list holds; a count above the capacity = records were dropped = brute force)
  const int n_own = COMPACT ? min(sc.n_ovf, SC_SLOT_PITCH) : n_slots + g.sa_slots;
  auto slot_at = [&](int j) -> uint2& { return mine[COMPACT || j < n_slots ? j : SC_SLOTS_MAX + (j - n_slots)]; };
  const int bad = sc.bad;
  const float nq = sc.nq;
  const float tau_q = sc.tau_q;
  const int n_ovf = sc.n_ovf;
  const unsigned incw = sc.incw;
  const float2 qv = sc.qv;
  // (the values are wanted HERE: without this the compiler moves the loads behind the tests below, one round trip each)
  asm volatile("" ::"v"(bad), "v"(nq), "v"(tau_q), "v"(n_ovf), "v"(incw), "v"(qv.x), "v"(qv.y), "s"(Qe));
  if (q >= Qe) {   // no such query in this frame: "no neighbour", like combine_splits_kernel (pass B left it no records)
    if (lane == 0) {
      idx1[q] = -1;
      d1[q] = __builtin_inff();
      d2[q] = __builtin_inff();
    }
    return;
  }
  if (bad == 2) {   // an absent row inside the launch (see screen_prepare_kernel)
    if (lane == 0) {
      idx1[q] = -1;
      d1[q] = __builtin_inff();
      d2[q] = __builtin_inff();
    }
    return;
  }
  if (bad == 3) {   // an all-zero query: every row's distance is its norm term
    if (lane == 0) {
      idx1[q] = zero_idx >= 0 ? row_to_global(rmap, zero_idx) : -1;
      d1[q] = zero_d1;
      d2[q] = zero_d2;
      if (stats) stats[3 * q + 2] += 1u;   // a search, without candidates
    }
    return;
  }
  wave_lds_sync();   // the iteration before has read its query row and its staged rows
  if (lane == 0) {
    *ncand_sw = 0;
    *nsamp_sw = 0;
  }
  q_sw[2 * lane] = qv.x;
  q_sw[2 * lane + 1] = qv.y;
  // ---- records -> candidate row list in LDS; the slots read are emptied for the next frame ----
  bool brute = n_ovf > (COMPACT ? SC_SLOT_PITCH : ovf_cap) || bad == 1;
  int n_cand = 0;
  if (!brute) {
    // Every record carries the largest screen value of its rows (f16, nearest).  Two different records hold different
    // rows, so the second largest of these values (minus the f16 rounding) is a lower bound of the DB's second largest
    // screen value s2, and a row that belongs to the exact top-2 has a screen value >= s2 - 2 E (pass B's argument
    // with the exact s2 in the place of pass A's sampled one): records whose largest value (plus the rounding) lies
    // more than screen_margin below that bound cannot hold one.  Pass A's threshold comes from an eighth of the rows
    // and lets ~25 rows per query through; ~3 survive this one and get their 512-byte row fetched.
    float l1 = -__builtin_inff(), l2 = -__builtin_inff();   // the lane's two largest lower bounds
    float h1 = -__builtin_inff();                           // ACCEPT: and its largest upper bound
    const float pert = screen_pack_pert(nq, dmax, g.pack_bits);
    auto bounds = [tau_q, spread, N, dmax, pert](uint2 rec, float& lo, float& hi) {
      // the record's value: (largest dot of the block + the block's largest -dd/2) - tau, rounded to f16.  The block's
      // largest screen value is at most that, and at least that less the spread of -dd/2 inside a block (`spread`: the
      // largest over the DB's blocks of real rows, ~1e-7 for L2-normalised rows); a block with padding rows (their
      // dot is 0, their -dd/2 is -inf) gives no lower bound.  (screen.h; checked in host arithmetic by the CPU tests)
      // (a record of a sampled tile carries that block's own largest screen value, seen through pass A's packing)
      if (rec.x & SC_REC_SAMPLE) screen_sample_bounds((unsigned short)(rec.y >> 16), tau_q, pert, dmax, lo, hi);
      else screen_record_bounds((unsigned short)(rec.y >> 16), rec.x & 0x3FFFFFFFu, tau_q, spread, N, dmax, lo, hi);
    };
    // (COMPACT: a list of more than 64 records -- rare, and the same for the whole wavefront -- has the rest of its slots
    // fetched in a second trip, and both loops then run over those registers as well)
    const bool more = COMPACT && n_own > 64;
    if (more) {
#pragma unroll
      for (int it = 1; it < RS_ITERS_C; ++it) {
        const int j = it * 64 + lane;
        recv[it] = j < n_own ? mine[j] : make_uint2(0u, 0u);
      }
    }
    auto scan = [&](int it) {
      const int j = it * 64 + lane;
      uint2 rec = recv[it];
      if (COMPACT) {
        if (j < n_own) mine[j] = make_uint2(0u, 0u);
        else rec = make_uint2(0u, 0u);
      } else if (j < n_own) {
        if (rec.y) slot_at(j) = make_uint2(0u, 0u);
      } else if (j < n_own + n_ovf) {
        rec = ovf[(size_t)q * ovf_cap + (j - n_own)];
      }
      recv[it] = rec;
      if (rec.y & 0xFFFFu) {
        float lo, hi;
        bounds(rec, lo, hi);
        l2 = fmaxf(l2, fminf(l1, lo));
        l1 = fmaxf(l1, lo);
        if (ACCEPT) h1 = fmaxf(h1, hi);
      }
    };
    if (COMPACT) {
      scan(0);
      if (more) {
#pragma unroll
        for (int it = 1; it < RS_ITERS_C; ++it) scan(it);
      }
    } else {
#pragma unroll
      for (int it = 0; it < RS_ITERS; ++it) scan(it);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float o1 = __shfl_xor(l1, d), o2 = __shfl_xor(l2, d);
      l2 = fmaxf(fmaxf(l2, o2), fminf(l1, o1));
      l1 = fmaxf(l1, o1);
      if (ACCEPT) h1 = fmaxf(h1, __shfl_xor(h1, d));
    }
    // Every record the query has was read above (no list overflowed: !brute; no lane slot of pass A left its blocks out:
    // incw == 0), so screen_reject_proved's premises hold.  The slots read are empty again (scan), the count goes the way it
    // goes below; the LDS counters are reset by whichever query this wavefront takes next.
    if (ACCEPT && incw == 0u && accept_ratio > 0.f && screen_reject_proved(nq, dmax, h1, l2, tau_q, accept_ratio)) {
      if (lane == 0) {
        if (n_ovf) ovf_cnt[q] = 0;
        idx1[q] = -1;
        d1[q] = __builtin_inff();
        d2[q] = __builtin_inff();
        if (prerej) atomicAdd(prerej + (q % RS_PREREJ_WORDS) * RS_PREREJ_PITCH, 1u);
      }
      return;
    }
    const float keep_from = l2 - screen_margin(nq, dmax);   // -inf with fewer than two records: everything stays
    auto keep = [&](int it) {
      const uint2 rec = recv[it];
      unsigned bits = rec.y & 0xFFFFu;
      if (bits) {
        float lo, hi;
        bounds(rec, lo, hi);
        if (hi < keep_from) bits = 0;
      }
      // which rows a bit stands for: records of the 32x32x16 passes hold 16 rows, row0 + (r & 3) + 8 (r >> 2); those of
      // the 16x16x32 passes (bit 31 of the row word) 8 rows, row0 + (r & 3) + 16 (r >> 2)
      const int hi_stride = (rec.x & 0x80000000u) ? 16 : 8;
      const int row0 = (int)(rec.x & 0x3FFFFFFFu);
      // a sampled tile's record names no rows (its mask is all 8): which of them lie above tau is found below, for the
      // records that are still here
      if (bits && (rec.x & SC_REC_SAMPLE)) {
        const int w = atomicAdd(nsamp_sw, 1);
        if (w < SC_SA_SLOTS) samp_sw[w] = row0;
        bits = 0;
      }
      // candidates in any order (the exact top-2 below breaks ties by row number): an LDS counter hands out places
      while (bits) {
        const int r = __builtin_ctz(bits);
        bits &= bits - 1;
        const int w = atomicAdd(ncand_sw, 1);
        if (w < RS_MAXC) cand_sw[w] = row0 + (r & 3) + hi_stride * (r >> 2);
      }
    };
    if (COMPACT) {
      keep(0);
      if (more) {
#pragma unroll
        for (int it = 1; it < RS_ITERS_C; ++it) keep(it);
      }
    } else {
#pragma unroll
      for (int it = 0; it < RS_ITERS; ++it) keep(it);
    }
    wave_lds_sync();
    // The surviving sampled records, two per MFMA set: the rows whose screen value -- pass A's own, see sample_pair_values --
    // exceeds tau become candidates, as pass B's rule has it for every other tile; a record none of whose rows does (its
    // packed maximum lay between tau - P and tau) leaves none.
    const int n_samp = min(*nsamp_sw, SC_SA_SLOTS), n_pad_rows = (N + SC_TILE - 1) / SC_TILE * SC_TILE;
    for (int p = 0; p < n_samp; p += 2) {
      const bool pair = p + 1 < n_samp;
      const int rx = samp_sw[p], ry = samp_sw[pair ? p + 1 : p];
      if (rx + 19 >= n_pad_rows || ry + 19 >= n_pad_rows) continue;   // (not a block of the DB: never written)
      const v4f w = sample_pair_values(q_sw, dbh, dneg, rx, ry, lane);
      const int grp = lane >> 4;
      if ((lane & 15) == 0 && (grp < 2 || pair)) {
        const int base = (grp < 2 ? rx : ry) + 16 * (grp & 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (w[r] > tau_q) {
            const int at = atomicAdd(ncand_sw, 1);
            if (at < RS_MAXC) cand_sw[at] = base + r;
          }
      }
    }
    if (n_samp) wave_lds_sync();
    n_cand = *ncand_sw;
    if (n_cand > RS_MAXC) brute = true;
  } else if (COMPACT ? n_ovf > 0 : n_ovf > ovf_cap) {
    for (int j = lane; j < n_own; j += 64) slot_at(j) = make_uint2(0u, 0u);   // the lists overflowed: empty every slot
  }
  if (n_ovf && lane == 0) ovf_cnt[q] = 0;
  wave_lds_sync();

  Best best = {__builtin_inff(), __builtin_inff(), -1};
  const int n_rows = brute ? N : n_cand;
  if (!brute && n_cand <= 64) {
    // The usual query: a handful of candidates.  The first RS_STAGE rows come in as ONE round trip -- 32 lanes x 16 bytes
    // per row, all of them in flight at once -- into the LDS the candidate list lay in (chunk c of staged row r at
    // c ^ r: the lanes that run the chains read different banks), and lane r runs row r's chain from there: the same
    // fmaf chain in the same order as exact_dist, its 512 bytes read from LDS instead of in four dependent round trips.
    const int my_row = lane < n_cand ? cand_sw[lane] : -1;
    const bool my_ok = my_row >= 0 && my_row < N;
    const float my_dn = my_ok ? dnorm[my_row] : 0.f;
    wave_lds_sync();   // every lane holds its candidate: the list's memory is free
    float4* stage = reinterpret_cast<float4*>(cand_sw);
    const int n_st = min(n_cand, RS_STAGE);
    const int half = lane >> 5, c = lane & 31;
    float4 v[RS_STAGE / 2];
#pragma unroll
    for (int i = 0; i < RS_STAGE / 2; ++i) {
      const int r = 2 * i + half;
      const int row_r = __shfl(my_row, r);
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < n_st && row_r >= 0 && row_r < N) v[i] = reinterpret_cast<const float4*>(db + (size_t)row_r * DIM)[c];
    }
#pragma unroll
    for (int i = 0; i < RS_STAGE / 2; ++i) {
      const int r = 2 * i + half;
      if (r < n_st) stage[r * 32 + (c ^ r)] = v[i];
    }
    wave_lds_sync();
    if (lane < n_st) {
      if (my_ok) {
        float sdot = 0.f;
        const float4* qs4 = reinterpret_cast<const float4*>(q_sw);
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
          const float4 x = stage[lane * 32 + (k ^ lane)], y = qs4[k];
          sdot = fmaf(y.x, x.x, sdot); sdot = fmaf(y.y, x.y, sdot); sdot = fmaf(y.z, x.z, sdot); sdot = fmaf(y.w, x.w, sdot);
        }
        take(best, fmaxf(fmaf(-2.f, sdot, nq + my_dn), 0.f), my_row);
      }
    } else if (my_ok) {
      take(best, exact_dist(q_sw, db + (size_t)my_row * DIM, nq, my_dn), my_row);
    }
  } else {
    for (int k = lane; k < n_rows; k += 64) {
      const int row = brute ? k : cand_sw[k];
      if (row >= 0 && row < N) take(best, exact_dist(q_sw, db + (size_t)row * DIM, nq, dnorm[row]), row);
    }
  }
  if (incw && !brute) {
    // An incomplete query (screen_handover_kernel): some lane slots of pass A held more blocks above the threshold than
    // their lists keep, and left no records.  The canonical chain over those slots' rows -- the sampled tiles of the
    // marked splits, the rows 16 i + 4 quarter .. + 3 of the marked quarters -- takes their place: bounded (a lane
    // slot is 1 / (4 x pass A's splits) of an eighth of the DB), and none of these rows is in a record.
    for (unsigned sm = incw & 0x0FFFFFFFu; sm; sm &= sm - 1) {
      const int split = __builtin_ctz(sm);
      const int sel0 = split * g.tiles_base + min(split, g.tiles_rem);
      const int sel1 = min(sel0 + g.tiles_base + (split < g.tiles_rem ? 1 : 0), g.n_sel);
      for (int k = sel0 * SC_TILE + lane; k < sel1 * SC_TILE; k += 64) {
        const int row = (g.tile_first + (k >> 7) * g.tile_stride) * SC_TILE + (k & 127);
        if (((incw >> (28 + ((k & 15) >> 2))) & 1u) && row < N)
          take(best, exact_dist(q_sw, db + (size_t)row * DIM, nq, dnorm[row]), row);
      }
    }
    if (lane == 0 && inc_count) atomicAdd(inc_count, 1u);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float ob1 = __shfl_xor(best.b1, d), ob2 = __shfl_xor(best.b2, d);
    const int oi1 = __shfl_xor(best.i1, d);
    if (oi1 >= 0) merge(best, ob1, ob2, oi1);
  }
  if (lane == 0) {
    idx1[q] = best.i1 >= 0 ? row_to_global(rmap, best.i1) : -1;
    d1[q] = best.b1;
    d2[q] = best.b2;
    if (stats) {   // per-query tallies (this wavefront is the query's only writer; launches are stream ordered): no atomics
      stats[3 * q] += (unsigned)n_cand;
      stats[3 * q + 1] += brute ? 1u : 0u;
      stats[3 * q + 2] += 1u;
    }
  }
}

// RsArgs is the kernel's ONLY parameter: rs_args() reads it from offset 0 of the kernel argument segment (the assertion
// behind the kernel holds the signature to that).
// The product (<4, 0>, a wavefront per query) runs the loop once and keeps its form all the same: it is the form that was
// measured (profiles/passc_persistent_ab.txt, the row WAVES=4), its arguments fetched next to their uses inside the
// iteration and no scratch memory; the same per-query code without the loop around it was not measured.
template <int WAVES, int PF, int COMPACT, int ACCEPT = 0>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WAVES == 12 ? 6 : 8, WAVES == 12 ? 6 : 8))) void rescore_kernel(const RsArgs args) {
  MH_TRACE_SCOPE(mh::TK_PASS_C);
  // dynamic LDS (sixteen wavefronts' regions are more than the 64 KB a kernel may declare): [WAVES][DIM] query rows,
  // [WAVES][RS_MAXC] candidate lists (then RS_STAGE rows of them), [WAVES][SC_SA_SLOTS] row0 of the sampled tiles'
  // records that survive the thinning, the two counters
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  const int lane0 = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q_first = blockIdx.x * WAVES + wave0, q_stride = (int)gridDim.x * WAVES;
  if (q_first >= args.Q) return;
  const int Qe = args.q_count ? min(args.Q, *RS_CONST(int32_t, args.q_count)) : args.Q;   // (the one value an iteration does not read anew)
  uint2 recv_next[RS_ITERS];
  RsScalars sc_next = {};
  if (PF >= 1) rs_load_slots<COMPACT>(args.recs, args.n_slots, args.g.sa_slots, q_first, lane0, recv_next);
  if (PF >= 2) sc_next = rs_load_scalars(args.qbad, args.qnorm, args.tau, args.ovf_cnt, args.inc, args.qn, q_first, lane0);
  for (int q = q_first;; q += q_stride) {
    // (what an iteration derives from the lane and the wavefront's number -- addresses, masks -- it derives anew, as it
    // reads the arguments anew: kept in registers across the loop these values, too, end in scratch memory)
    int lane = lane0, wave = wave0;
    asm volatile("" : "+v"(lane), "+s"(wave));
    float* const q_sw = reinterpret_cast<float*>(rs_lds) + wave * DIM;
    int* const cand_sw = reinterpret_cast<int*>(rs_lds + (size_t)WAVES * DIM * 4) + wave * RS_MAXC;
    int* const samp_sw = reinterpret_cast<int*>(rs_lds + (size_t)WAVES * (DIM + RS_MAXC) * 4) + wave * SC_SA_SLOTS;
    int* const ncand_sw = reinterpret_cast<int*>(rs_lds + (size_t)WAVES * (DIM + RS_MAXC + SC_SA_SLOTS) * 4) + wave;
    int* const nsamp_sw = ncand_sw + WAVES;
    const RsArgsPtr A = rs_args();
    const int Q = A->Q;
    if (q >= Q) break;
    // Everything the query's wavefront reads before it knows its candidates is asked for HERE, in one go (or was, an
    // iteration ago): the kernel lives on round trips (a query is ~a dozen loads and ~400 fmaf), and loads issued behind
    // the branches of rescore_query each cost one.
    uint2 recv[RS_ITERS];
    if (PF >= 1) {
#pragma unroll
      for (int it = 0; it < RS_ITERS; ++it) recv[it] = recv_next[it];
    } else {
      rs_load_slots<COMPACT>(A->recs, A->n_slots, A->g.sa_slots, q, lane, recv);
    }
    const RsScalars sc = PF >= 2 ? sc_next : rs_load_scalars(A->qbad, A->qnorm, A->tau, A->ovf_cnt, A->inc, A->qn, q, lane);
    if (PF >= 1 && q + q_stride < Q) {   // the next query of this wavefront: consumed an iteration from here
      rs_load_slots<COMPACT>(A->recs, A->n_slots, A->g.sa_slots, q + q_stride, lane, recv_next);
      if (PF >= 2) sc_next = rs_load_scalars(A->qbad, A->qnorm, A->tau, A->ovf_cnt, A->inc, A->qn, q + q_stride, lane);
    }
    RowMap rmap;
    rmap.glo = A->rmap.glo;
    rmap.llo = A->rmap.llo;
    rmap.nb = A->rmap.nb;
    rmap.base = A->rmap.base;
    const SampleGeom g = {A->g.sa_slots, A->g.pack_bits, A->g.tile_first, A->g.tile_stride, A->g.tiles_base, A->g.tiles_rem, A->g.n_sel};
    if (ACCEPT)
      rescore_query<COMPACT, 1>(q, lane, q_sw, cand_sw, samp_sw, ncand_sw, nsamp_sw, recv, sc, Qe, A->db, A->dnorm, A->N, rmap, A->recs,
                    A->n_slots, A->ovf_cnt, A->ovf, A->ovf_cap, A->dmax, A->spread, A->idx1, A->d1, A->d2, A->stats, A->zero_idx,
                    A->zero_d1, A->zero_d2, g, A->inc_count, A->dbh, A->dneg, A->accept_ratio, A->prerej);
    else
    rescore_query<COMPACT>(q, lane, q_sw, cand_sw, samp_sw, ncand_sw, nsamp_sw, recv, sc, Qe, A->db, A->dnorm, A->N, rmap, A->recs,
                  A->n_slots, A->ovf_cnt, A->ovf, A->ovf_cap, A->dmax, A->spread, A->idx1, A->d1, A->d2, A->stats, A->zero_idx,
                  A->zero_d1, A->zero_d2, g, A->inc_count, A->dbh, A->dneg);
  }
}
static_assert(std::is_same<decltype(&rescore_kernel<RS_WAVES, 0, 0>), void (*)(RsArgs)>::value,
              "rs_args() reads RsArgs from offset 0 of the kernel argument segment: it must stay the only parameter");

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

// The values pass C names a sampled record's rows by (sample_pair_values, the function rescore_kernel calls): one wavefront
// per query and pair of blocks, out[q][8 block + bit].
__global__ __launch_bounds__(64) void screen_sample_values_kernel(const float* __restrict__ qn, const _Float16* __restrict__ dbh,
                                                                  const float* __restrict__ dneg, const int32_t* __restrict__ row0,
                                                                  float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float q_s[DIM];
  const int lane = threadIdx.x, q = blockIdx.x;
  const float2 qv = reinterpret_cast<const float2*>(qn + (size_t)q * DIM)[lane];
  q_s[2 * lane] = qv.x;
  q_s[2 * lane + 1] = qv.y;
  __syncthreads();
  const v4f w = sample_pair_values(q_s, dbh, dneg, row0[2 * q], row0[2 * q + 1], lane);
  if ((lane & 15) == 0)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(size_t)q * 16 + 4 * (lane >> 4) + r] = w[r];
}

}  // namespace

#ifdef SC_PROF
extern "C" int mh_debug_screen_trace(unsigned long long* out /* [2][1024] */) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sc_trace), 2 * 1024 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
extern "C" int mh_debug_screen_prof(unsigned long long out[8], int reset, int ablate) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sc_prof), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_sc_prof), z, sizeof z) != hipSuccess) return -1;
  }
  g_sc_ablate = ablate;
  return 0;
}
#endif
#ifdef MH_EXPERIMENTS
// the counter since the last reset, or -1 (synchronises the device)
extern "C" long long mh_debug_screen_direct_appends(int reset) {
  unsigned long long v = 0, z = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_sc_direct_appends), sizeof v) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_sc_direct_appends), &z, sizeof z) != hipSuccess) return -1;
  return (long long)v;
}
#endif

// ---- host side -----------------------------------------------------------------------------------
float screen_margin_host(float qq, float dmax) { return screen_margin(qq, dmax); }
bool screen_reject_proved_host(float qq, float dmax, float h1, float l2, float tau_q, float ratio) {
  return screen_reject_proved(qq, dmax, h1, l2, tau_q, ratio);
}
int screen_prerej_words() { return RS_PREREJ_WORDS * RS_PREREJ_PITCH; }
int screen_prerej_pitch() { return RS_PREREJ_PITCH; }

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
void launch_screen_sample_values(const float* qn, int Q, const ScreenDb& sdb, const int32_t* row0, float* out, hipStream_t s) {
  if (Q <= 0) return;
  hipLaunchKernelGGL(screen_sample_values_kernel, dim3(Q), dim3(64), 0, s, qn, sdb.dbh, sdb.dneg, row0, out);
}
void launch_screen_prepare(const float* qn, const float* qnorm, int Q, int q_pad, _Float16* qh, uint8_t* qbad, hipStream_t s) {
  hipLaunchKernelGGL(screen_prepare_kernel, dim3((q_pad * 16 + 255) / 256), dim3(256), 0, s, qn, qnorm, Q, (const int32_t*)nullptr,
                     q_pad, qh, qbad);
}

size_t screen_rec_slots() { return SC_SLOT_PITCH; }
int screen_park_places() { return SC_RECBUF16; }

int screen_q_pad(int Q) { return (Q + SC_QPAD - 1) / SC_QPAD * SC_QPAD; }
int screen_max_splits_a() { return 64; }
// per query: a float2 per pass A split (screen_kernel), or SC_PART5 floats per lane slot of a one-sweep launch
size_t screen_part_bytes(int q_pad) {
  return (size_t)q_pad * std::max<size_t>(screen_max_splits_a() * sizeof(float2), (size_t)SC_SA_SPLITS_MAX * 4 * SC_PART5 * sizeof(float));
}

// When the screen pays: enough (query, row) pairs to be bound by arithmetic rather than by its launches, and
// enough rows for pass A's sample to mean something.  MH_MATCH_SCREEN = 0 / 1 pins the choice for the process
// (A/B runs; bench.py records it), mh_match_set_mode for a context.
bool screen_wanted(int q_expected, int N, int mode) {
  static const int pinned = exp_int("MH_MATCH_SCREEN", -1);
  if (mode < 0) mode = pinned;
  if (mode == 0 || N < 4096) return false;
  if (mode == 1) return true;
  return (double)q_expected * (double)N >= 8e6;
}

namespace {

template <int NQB, int NW>
void launch_passes(ScreenArgs a, int Q, int qe, int n_tiles, int sample, int blocks_a, int blocks_b, int* n_slots_out,
                   hipEvent_t* ev, hipStream_t s, int cu_avail) {
  constexpr int QB = 32 * NQB * NW;
  constexpr int SC_THREADS = 64 * NW, SC_LDS_BYTES = sc_lds_bytes(NW);
  static DynLds attr0, attr1;
  attr0.ensure(screen_kernel<0, NQB, NW>, SC_LDS_BYTES);
  attr1.ensure(screen_kernel<1, NQB, NW>, SC_LDS_BYTES);
  // (the workgroup targets below are in units of eight wavefronts: a four-wavefront grid has twice the workgroups)
  blocks_a *= 8 / NW;
  (void)cu_avail;
  const int nqb = (Q + QB - 1) / QB;        // the grid covers the capacity ...
  const int nqb_e = (qe + QB - 1) / QB;     // ... the splits are sized for the queries expected
  auto splits_for = [&](int n_sel, int target, int s_max) {
    int S = std::max(1, target / nqb_e);
    S = std::min(std::min(S, n_sel), s_max);
    // whole splits per XCD (a split's rows stay in one L2) unless the rounding would leave CUs without a workgroup:
    // 24 query blocks x 8 splits fill 192 of 256 CUs, x 10 fill 240 (measured: 10% on the stage at Q = 12000)
    if (S >= 8 && (S / 8 * 8) * 33 >= S * 32) S = S / 8 * 8;
    return std::max(S, 1);
  };
  // pass A: every `stride`-th tile, starting in the middle of the first stride
  // (a shard of a few models: the records a query leaves do not shrink with the shard, the MFMA work beside them does --
  // every 4th tile there: half the records for 1/8 more of pass A's rows.  15 000 rows x 96 000 queries: pass B 0.38 ->
  // 0.34 ms, pass A 0.055 -> 0.09, the rank's frames/s +2.5%)
  const int every = sample == 8 && n_tiles < 256 ? 4 : sample;
  const int stride = n_tiles >= 4 * every ? every : 1;
  const int n_sel_a = (n_tiles + stride - 1) / stride;
  const int Sa = splits_for(n_sel_a, blocks_a, screen_max_splits_a());
  a.n_sel = n_sel_a;
  a.tile_first = std::min(stride / 2, n_tiles - 1 - (n_sel_a - 1) * stride);
  if (a.tile_first < 0) a.tile_first = 0;
  a.tile_stride = stride;
  a.n_splits = Sa;
  a.tiles_base = n_sel_a / Sa;
  a.tiles_rem = n_sel_a % Sa;
  a.n_splits_a = Sa;
  hipLaunchKernelGGL((screen_kernel<0, NQB, NW>), dim3(nqb * Sa), dim3(SC_THREADS), SC_LDS_BYTES, s, a);
  if (ev) hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(screen_tau_kernel, dim3((a.q_pad + 255) / 256), dim3(256), 0, s, a.part, Sa, a.q_pad, a.Q, a.q_count,
                     a.qnorm, a.qbad, a.dmax, const_cast<float*>(a.tau));
  if (ev) hipEventRecord(ev[3], s);
  // pass B: all tiles; a query's record slots are shared out over 2 x Sb lane-private sub-lists
  static const int sb_pin = exp_int("MH_SCREEN_SPLITS_B", 0);   // experiments
  // Twice as many workgroups as CUs when every one of them still sweeps >= 24 tiles: two rounds of half-length
  // workgroups finish more evenly than one round of ~240 (pass B alone 0.272 -> 0.261 ms at Q = 12000, N = 100k), and
  // under load a one-round grid stalls on every CU another frame's kernel holds (+5% frames/s at config 1, +3% at
  // config 2).  With fewer tiles per workgroup the query-operand prologue costs more than that (Q = 3000: 0.445 ->
  // 0.394 of peak), so small launches keep one workgroup per CU.
  if (blocks_b <= 0) blocks_b = (long)n_tiles * nqb_e * NW / 8 >= (NQB >= 4 ? 16L : 24L) * 512 ? 512 : 256;
  blocks_b *= 8 / NW;
  const int Sb = sb_pin > 0 ? std::min(std::min(sb_pin, n_tiles), SC_SLOTS_MAX / 2)
                            : splits_for(n_tiles, blocks_b, SC_SLOTS_MAX / 2);
  a.n_sel = n_tiles;
  a.tile_first = 0;
  a.tile_stride = 1;
  a.n_splits = Sb;
  a.tiles_base = n_tiles / Sb;
  a.tiles_rem = n_tiles % Sb;
  // (few splits = long sub-streams: a lane sees many of its query's candidates, its sub-list must hold them)
  a.sub_cap = std::max(1, std::min(48, SC_SLOTS_MAX / (2 * Sb)));
  hipLaunchKernelGGL((screen_kernel<1, NQB, NW>), dim3(nqb * Sb), dim3(SC_THREADS), SC_LDS_BYTES, s, a);
  if (ev) hipEventRecord(ev[4], s);
  *n_slots_out = 2 * Sb * a.sub_cap;
}

// The launch policy of the 16x16x32 kernels (eight wavefronts; a query's records in one counted list), as
// host arithmetic: launch_passes16 launches what this says, screen_launch_plan shows it to the tests.
struct Plan16 {
  bool onesweep;                                  // pass A hands its tiles' records over, pass B skips them
  int stride, tile_first, n_sel_a, Sa, pack_bits; // pass A
  int n_sel_b, Sb;                                // pass B
};
template <int NQB>
Plan16 plan_passes16(int qe, int n_tiles, int sample, int blocks_a, int blocks_b) {
  constexpr int QB = 32 * NQB * 8;
  const int nqb_e = (qe + QB - 1) / QB;
  auto splits_for = [&](int n_sel, int target, int s_max) {
    int S = std::max(1, target / nqb_e);
    S = std::min(std::min(S, n_sel), s_max);
    if (S >= 8 && (S / 8 * 8) * 33 >= S * 32) S = S / 8 * 8;
    return std::max(S, 1);
  };
  Plan16 p;
  // (a shard of a few models: the records a query leaves do not shrink with the shard, the MFMA work beside them does --
  // every 4th tile there: half the records for 1/8 more of pass A's rows.  15 000 rows x 96 000 queries: pass B 0.38 ->
  // 0.34 ms, pass A 0.055 -> 0.09, the rank's frames/s +2.5%)
  const int every = sample == 8 && n_tiles < 256 ? 4 : sample;
  p.stride = n_tiles >= 4 * every ? every : 1;
  p.n_sel_a = (n_tiles + p.stride - 1) / p.stride;
  p.Sa = splits_for(p.n_sel_a, blocks_a, SC_SA_SPLITS_MAX);   // (the lists of 4 x Sa lane slots per query: screen_part_bytes)
  p.tile_first = std::max(0, std::min(p.stride / 2, n_tiles - 1 - (p.n_sel_a - 1) * p.stride));
  // One sweep: pass A keeps the identity of its best blocks (the block's number inside a lane slot in the low mantissa
  // bits of the block's maximum) and pass B leaves the sampled tiles out.  Not when pass A sees every tile anyway, nor
  // when a lane slot would have more blocks than SC_PACK_BITS_MAX bits count even with all the splits pass A may have
  // (7 M rows): pass B then sweeps all tiles as before, and the block maxima stay as they are (0 bits).
  static const int onesweep_on = exp_int("MH_SCREEN_ONESWEEP", 1);   // experiment builds: 0 = pass B sweeps every tile (scripts/ab_env.sh)
  if (onesweep_on && p.stride > 1)   // (a long sweep: more, shorter splits rather than wider block numbers)
    while (4 * ((p.n_sel_a + p.Sa - 1) / p.Sa) > (1 << SC_PACK_BITS_MAX) && p.Sa < SC_SA_SPLITS_MAX) ++p.Sa;
  const int blocks_slot = 4 * ((p.n_sel_a + p.Sa - 1) / p.Sa);
  int bits = 2;
  while ((1 << bits) < blocks_slot) ++bits;
  p.onesweep = onesweep_on && p.stride > 1 && bits <= SC_PACK_BITS_MAX;
  p.pack_bits = p.onesweep ? bits : 0;
  // Pass B's splits.  Sb <= 21 dates from the lane-private layout (a query's 256 slots shared out over 4 x Sb sub-lists,
  // each with room for three records: 12 000 queries x 250 000 rows ran 42 splits with ONE slot per sub-list for a while,
  // 42 brute-force queries per launch, pass C 10 ms instead of 0.03); the counted lists do not need it, and it stays
  // because the launch geometry was not to change with them.  One workgroup per compute unit, so the
  // launch takes ceil(workgroups / 256) rounds of tiles / Sb tiles each: the Sb with the least rounds x tiles, the
  // larger of equals.  (blocks_b > 0: an experiment's request, capped the same way.)
  constexpr int SB16_MAX = SC_SLOTS_MAX / 12;
  p.n_sel_b = p.onesweep ? n_tiles - p.n_sel_a : n_tiles;
  p.Sb = 1;
  if (blocks_b > 0) {
    p.Sb = std::min(splits_for(p.n_sel_b, blocks_b, SC_SLOTS_MAX / 4), SB16_MAX);
  } else {
    double best = 1e30;
    for (int c = 1; c <= std::min(SB16_MAX, std::max(1, p.n_sel_b / 8)); ++c) {
      const double cost = (double)((nqb_e * c + 255) / 256) * (double)((p.n_sel_b + c - 1) / c);
      if (cost <= best) {
        best = cost;
        p.Sb = c;
      }
    }
  }
  // (No slots per sub-list and no slot target per query any more -- `sub_cap`, `slots_target` of the lane-private layout:
  // a query's records go to one counted list of SC_SLOT_PITCH places whatever Sb is, and pass C reads by the count.  Sb's
  // cap above is kept as it was: this plan's eight outputs are what the launches were measured with.)
  return p;
}

template <int NQB>
void launch_passes16(ScreenArgs a, int Q, int qe, int n_tiles, int sample, int blocks_a, int blocks_b, int* n_slots_out,
                     SampleGeom* geom_out, unsigned int* inc, hipEvent_t* ev, hipStream_t s) {
  constexpr int QB = 32 * NQB * 8;
  static DynLds attr0, attr1;
  attr0.ensure(screen16_kernel<0, NQB>, SC_LDS16_BYTES);
  attr1.ensure(screen16_kernel<1, NQB>, SC_LDS16_BYTES);
  const int nqb = (Q + QB - 1) / QB;
  const Plan16 p = plan_passes16<NQB>(qe, n_tiles, sample, blocks_a, blocks_b);
  // pass A: every `stride`-th tile, starting in the middle of the first stride
  a.n_sel = p.n_sel_a;
  a.tile_first = p.tile_first;
  a.tile_stride = p.stride;
  a.n_splits = p.Sa;
  a.tiles_base = p.n_sel_a / p.Sa;
  a.tiles_rem = p.n_sel_a % p.Sa;
  a.n_splits_a = p.Sa;
  a.pack_keep = ~((1u << p.pack_bits) - 1u);
  a.skip_first = a.skip_stride = 0;
  hipLaunchKernelGGL((screen16_kernel<0, NQB>), dim3(nqb * p.Sa), dim3(512), SC_LDS16_BYTES, s, a);
  if (ev) hipEventRecord(ev[2], s);
  SampleGeom g = {p.onesweep ? SC_SA_SLOTS : 0, p.pack_bits, a.tile_first, a.tile_stride, a.tiles_base, a.tiles_rem, a.n_sel};
  // 64 queries per workgroup, one wavefront per split of pass A (its four lane slots) -- or per two splits when pass A has
  // more than HO_PARTS_MAX
  static_assert(SC_SA_SPLITS_MAX <= 2 * HO_PARTS_MAX, "a thread of screen_handover_kernel holds at most 8 lane slots");
  if (p.Sa <= HO_PARTS_MAX)
    hipLaunchKernelGGL(screen_handover_kernel<4>, dim3((a.q_pad + 63) / 64), dim3(64, p.Sa), 0, s, (const float*)a.part5, 4 * p.Sa,
                       a.q_pad, a.Q, a.q_count, a.qnorm, a.qbad, a.dmax, g, const_cast<float*>(a.tau), a.recs, a.ovf_cnt, inc);
  else
    hipLaunchKernelGGL(screen_handover_kernel<8>, dim3((a.q_pad + 63) / 64), dim3(64, (p.Sa + 1) / 2), 0, s, (const float*)a.part5,
                       4 * p.Sa, a.q_pad, a.Q, a.q_count, a.qnorm, a.qbad, a.dmax, g, const_cast<float*>(a.tau), a.recs, a.ovf_cnt, inc);
#ifdef MH_EXPERIMENTS
  // what the records cost pass B: thresholds no value reaches (WRONG results: timing only)
  if (exp_int("MH_SCREEN_NO_HITS", 0)) hipMemsetAsync(const_cast<float*>(a.tau), 0x7f, (size_t)a.q_pad * sizeof(float), s);
#endif
  if (ev) hipEventRecord(ev[3], s);
  // pass B: the tiles pass A did not see (all tiles when there is no hand-over)
  a.n_sel = p.n_sel_b;
  a.tile_first = 0;
  a.tile_stride = 1;
  a.skip_first = p.onesweep ? p.tile_first : 0;
  a.skip_stride = p.onesweep ? p.stride : 0;
  a.n_splits = p.Sb;
  a.tiles_base = p.n_sel_b / p.Sb;
  a.tiles_rem = p.n_sel_b % p.Sb;
  // (no sub_cap: a query's records go to its one counted list, and pass C finds them by the count)
#ifdef MH_EXPERIMENTS
  // what the places' atomic adds cost pass B (screen16_kernel's PLACES; WRONG results: timing only)
  static const int places = exp_int("MH_SCREEN_PLACES", 0);
  static DynLds attr_p1, attr_p2, attr_p3;
  if (places == 3) {
    attr_p3.ensure(screen16_kernel<1, NQB, 3>, SC_LDS16_BYTES);
    hipLaunchKernelGGL((screen16_kernel<1, NQB, 3>), dim3(nqb * p.Sb), dim3(512), SC_LDS16_BYTES, s, a);
  } else if (places == 1) {
    attr_p1.ensure(screen16_kernel<1, NQB, 1>, SC_LDS16_BYTES);
    hipLaunchKernelGGL((screen16_kernel<1, NQB, 1>), dim3(nqb * p.Sb), dim3(512), SC_LDS16_BYTES, s, a);
  } else if (places == 2) {
    attr_p2.ensure(screen16_kernel<1, NQB, 2>, SC_LDS16_BYTES);
    hipLaunchKernelGGL((screen16_kernel<1, NQB, 2>), dim3(nqb * p.Sb), dim3(512), SC_LDS16_BYTES, s, a);
  } else
#endif
  hipLaunchKernelGGL((screen16_kernel<1, NQB>), dim3(nqb * p.Sb), dim3(512), SC_LDS16_BYTES, s, a);
  if (ev) hipEventRecord(ev[4], s);
  *n_slots_out = 0;
  *geom_out = g;
}

template <int WAVES, int PF, int COMPACT, int ACCEPT = 0>
void launch_pass_c_layout(int grid, hipStream_t s, const RsArgs& args) {
  static DynLds attr;
  attr.ensure(rescore_kernel<WAVES, PF, COMPACT, ACCEPT>, rs_lds_bytes(WAVES));
  hipLaunchKernelGGL((rescore_kernel<WAVES, PF, COMPACT, ACCEPT>), dim3(grid), dim3(64 * WAVES), rs_lds_bytes(WAVES), s, args);
}
// compact: the launch's records are counted lists (the 16x16x32 launches), else the lane-private slots + overflow list
template <int WAVES, int PF>
void launch_pass_c(int grid, hipStream_t s, const RsArgs& args, bool compact) {
  if (compact) launch_pass_c_layout<WAVES, PF, 1>(grid, s, args);
  else launch_pass_c_layout<WAVES, PF, 0>(grid, s, args);
}
// the same for a caller that named its ratio test (RsArgs::accept_ratio > 0): a wavefront per query, nothing prefetched
template <int WAVES>
void launch_pass_c_accept(int Q, hipStream_t s, const RsArgs& args, bool compact) {
  const int grid = (Q + WAVES - 1) / WAVES;
  if (compact) launch_pass_c_layout<WAVES, 0, 1, 1>(grid, s, args);
  else launch_pass_c_layout<WAVES, 0, 0, 1>(grid, s, args);
}

// which kernels a MATCH launch runs on (launch_match_screen): queries per workgroup / 256, and whether the 16x16x32 passes
struct ShapeChoice {
  int nqb_sel;
  bool passes16;
};
ShapeChoice choose_shape(int qe, int n_tiles) {
  static const int nqb_pin = exp_int("MH_SCREEN_NQB", 0);
  // queries per workgroup: 1024 (four 32-query blocks per wavefront: every row fragment read from LDS feeds four
  // MFMAs; 256 VGPRs, no prefetched copy of the next row block) when the launch is large enough for workgroups of
  // >= 16 tiles -- pass B alone 8-10% faster, config 2 +9.7% frames/s --, else 512 (two blocks, row fragments
  // prefetched), or 256 for small frames.  768 is selectable for experiments.
  int nqb_sel = qe > 640 ? 2 : 1;
  if (qe >= 2048 && (long)n_tiles * ((qe + 1023) / 1024) >= 16L * 256) nqb_sel = 4;
  if (nqb_pin >= 1 && nqb_pin <= 4) nqb_sel = nqb_pin;
  // the MFMA shape of the large launches: 16x16x32 (SC_SHAPE16_LARGE; MH_SCREEN_SHAPE = 1 / 2 pins 32x32x16 / 16x16x32 in experiment builds)
  static const int shape_pin = exp_int("MH_SCREEN_SHAPE", 0);
  const bool shape16 = shape_pin == 2 || (shape_pin == 0 && SC_SHAPE16_LARGE);
  // (16x16x32 from 12 query blocks of 1024: with fewer, 21 splits leave compute units without a workgroup)
  const bool p16 = shape16 && ((nqb_sel == 4 && (shape_pin == 2 || (qe + 1023) / 1024 >= 12)) || (nqb_sel == 2 && shape_pin == 2));
  return {nqb_sel, p16};
}

int screen_sample_every() {
  static const int sample = std::max(1, exp_int("MH_SCREEN_SAMPLE", 8));   // pass A looks at every `sample`-th tile
  return sample;
}

}  // namespace

void screen_launch_plan(int Q, int q_expected, int N, int out[8]) {
  const int qe = (q_expected > 0 && q_expected < Q) ? std::max(q_expected, std::min(Q, 256)) : Q;
  const int n_tiles = (N + SC_TILE - 1) / SC_TILE;
  for (int k = 0; k < 8; ++k) out[k] = 0;
  const ShapeChoice shape = choose_shape(qe, n_tiles);
  if (!shape.passes16) return;
  const int blocks_b = std::max(0, exp_int("MH_SCREEN_BLOCKS", 0)), blocks_a = std::max(1, exp_int("MH_SCREEN_BLOCKS_A", 256));
  const Plan16 p = shape.nqb_sel == 4 ? plan_passes16<4>(qe, n_tiles, screen_sample_every(), blocks_a, blocks_b)
                                      : plan_passes16<2>(qe, n_tiles, screen_sample_every(), blocks_a, blocks_b);
  const int v[8] = {p.onesweep ? 1 : 0, p.tile_first, p.stride, p.n_sel_a, p.Sa, p.pack_bits, p.Sb, p.n_sel_b};
  for (int k = 0; k < 8; ++k) out[k] = v[k];
}

void launch_match_screen(const float* qn, const float* qnorm, int Q, const float* db, const float* dnorm, int N,
                         const RowMap& rmap, const ScreenDb& sdb, const ScreenBufs& sb, int32_t* idx1, float* d1,
                         float* d2, hipStream_t s, const int32_t* q_count, int q_expected) {
  const int sample = screen_sample_every();
  static const int blocks_b = std::max(0, exp_int("MH_SCREEN_BLOCKS", 0));    // workgroups of pass B; 0 = by size (launch_passes)
  static const int blocks_a = std::max(1, exp_int("MH_SCREEN_BLOCKS_A", 256));
  const int q_pad = screen_q_pad(Q);
  const int qe = (q_expected > 0 && q_expected < Q) ? std::max(q_expected, std::min(Q, 256)) : Q;
  const int n_tiles = (N + SC_TILE - 1) / SC_TILE;

  if (sb.ev) hipEventRecord(sb.ev[0], s);
  hipLaunchKernelGGL(screen_prepare_kernel, dim3((q_pad * 16 + 255) / 256), dim3(256), 0, s, qn, qnorm, Q, q_count, q_pad,
                     sb.qh, sb.qbad);
  // the lane: everything from pass A to pass B on its stream, handed over by events
  hipStream_t sbig = s;
  if (sb.big && sb.ev_in && sb.ev_out) {
    hipEventRecord(sb.ev_in, s);
    hipStreamWaitEvent(sb.big, sb.ev_in, 0);
    sbig = sb.big;
  }
  if (sb.ev) hipEventRecord(sb.ev[1], sbig);
  ScreenArgs a;
  a.qh = sb.qh;
  a.dbh = sdb.dbh;
  a.dneg = sdb.dneg;
  a.qnorm = qnorm;
  a.qbad = sb.qbad;
  a.q_count = q_count;
  a.part = sb.part;
  a.part5 = reinterpret_cast<float*>(sb.part);
  a.pack_keep = ~0u;
  a.skip_first = a.skip_stride = 0;
  a.tau = sb.tau;
  a.recs = sb.recs;
  a.ovf_cnt = sb.ovf_cnt;
  a.ovf = sb.ovf;
  a.ovf_cap = sb.ovf_cap;
  a.sub_cap = 1;
  a.Q = Q;
  a.q_pad = q_pad;
  a.dmax = sdb.dmax;
#ifdef SC_PROF
  a.ablate = g_sc_ablate;
#else
  a.ablate = 0;
#endif
  const ShapeChoice shape = choose_shape(qe, n_tiles);
  const int nqb_sel = shape.nqb_sel;
  int n_slots = 0;
  SampleGeom geom = {0, 0, 0, 1, 0, 0, 0};
  // wavefronts per workgroup: four (two workgroups share a CU) for the large launches, see the top of the file
  static const int nw_pin = exp_int("MH_SCREEN_NW", 0);
  const int nw_sel = nw_pin == 4 || nw_pin == 8 ? nw_pin : (nqb_sel == 4 ? SC_NW_LARGE : 8);
  if (shape.passes16 && nqb_sel == 4) launch_passes16<4>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, &geom, sb.inc, sb.ev, sbig);
  else if (shape.passes16) launch_passes16<2>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, &geom, sb.inc, sb.ev, sbig);
  else if (nqb_sel == 4 && nw_sel == 4) launch_passes<4, 4>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  else if (nqb_sel == 4) launch_passes<4, 8>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  else if (nqb_sel == 3) launch_passes<3, 8>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  else if (nqb_sel == 2 && nw_sel == 4) launch_passes<2, 4>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  else if (nqb_sel == 2) launch_passes<2, 8>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  else launch_passes<1, 8>(a, Q, qe, n_tiles, sample, blocks_a, blocks_b, &n_slots, sb.ev, sbig, 256);
  if (sbig != s) {
    hipEventRecord(sb.ev_out, sbig);
    hipStreamWaitEvent(s, sb.ev_out, 0);
  }
  // pass C: a wavefront per query, four to a workgroup
  RsArgs ca;
  ca.qn = qn; ca.qnorm = qnorm; ca.qbad = sb.qbad; ca.Q = Q; ca.q_count = q_count; ca.db = db; ca.dnorm = dnorm; ca.N = N;
  ca.rmap = rmap; ca.recs = sb.recs; ca.n_slots = n_slots; ca.ovf_cnt = sb.ovf_cnt; ca.ovf = sb.ovf; ca.ovf_cap = sb.ovf_cap;
  ca.dmax = sdb.dmax; ca.tau = sb.tau; ca.spread = sdb.spread; ca.idx1 = idx1; ca.d1 = d1; ca.d2 = d2; ca.stats = sb.stats;
  ca.zero_idx = sdb.zero_idx; ca.zero_d1 = sdb.zero_d1; ca.zero_d2 = sdb.zero_d2; ca.g = geom;
  ca.inc = geom.sa_slots > 0 ? sb.inc : nullptr; ca.inc_count = sb.inc ? sb.inc + sb.q_pad : nullptr; ca.dbh = sdb.dbh; ca.dneg = sdb.dneg;
  ca.accept_ratio = sb.accept_ratio > 0.f ? sb.accept_ratio : 0.f;
  ca.prerej = sb.inc ? sb.inc + sb.q_pad + 1 : nullptr;   // (behind the incomplete words and their counter)
  if (ca.accept_ratio > 0.f) {
#ifdef MH_EXPERIMENTS
    // queries per workgroup of the accepting kernel (scripts/ab_env.sh; profiles/accept_reject_ab.txt): MH_PASSC_WAVES = 4 / 2
    static const int pa_waves = exp_int("MH_PASSC_WAVES", RS_WAVES_ACCEPT);
    if (pa_waves == 4) launch_pass_c_accept<4>(Q, s, ca, shape.passes16);
    else if (pa_waves == 2) launch_pass_c_accept<2>(Q, s, ca, shape.passes16);
    else
#endif
    launch_pass_c_accept<RS_WAVES_ACCEPT>(Q, s, ca, shape.passes16);
    if (sb.ev) hipEventRecord(sb.ev[5], s);
    return;
  }
#ifdef MH_EXPERIMENTS
  // the shapes that were measured against this one (rescore_kernel's comment; scripts/ab_env.sh): MH_PASSC_WAVES = 16 / 12
  // for the launches of more than two fat workgroups per compute unit (MH_PASSC_FAT_ALL = 1: for every launch), MH_PASSC_K
  // such workgroups per compute unit as the whole grid (0 = a wavefront per query), MH_PASSC_PREFETCH = 0 / 1 / 2
  static const int pc_waves = exp_int("MH_PASSC_WAVES", RS_WAVES), pc_k = exp_int("MH_PASSC_K", RS_FAT_K);
  static const int pc_pf = exp_int("MH_PASSC_PREFETCH", 0), pc_all = exp_int("MH_PASSC_FAT_ALL", 0);
  const int n_cus = sb.n_cus > 0 ? sb.n_cus : 256;
  const int fat_waves = pc_waves == 12 ? 12 : RS_WAVES_FAT;
  if (pc_waves != RS_WAVES && (pc_all || Q > RS_FAT_K * n_cus * RS_WAVES_FAT)) {
    const int cover = (Q + fat_waves - 1) / fat_waves, grid = pc_k > 0 ? std::min(cover, pc_k * n_cus) : cover;
    if (fat_waves == 12 && pc_pf == 0) launch_pass_c<12, 0>(grid, s, ca, shape.passes16);
    else if (fat_waves == 12 && pc_pf == 1) launch_pass_c<12, 1>(grid, s, ca, shape.passes16);
    else if (fat_waves == 12) launch_pass_c<12, 2>(grid, s, ca, shape.passes16);
    else if (pc_pf == 0) launch_pass_c<RS_WAVES_FAT, 0>(grid, s, ca, shape.passes16);
    else if (pc_pf == 1) launch_pass_c<RS_WAVES_FAT, 1>(grid, s, ca, shape.passes16);
    else launch_pass_c<RS_WAVES_FAT, 2>(grid, s, ca, shape.passes16);
  } else
#endif
  launch_pass_c<RS_WAVES, 0>((Q + RS_WAVES - 1) / RS_WAVES, s, ca, shape.passes16);
  if (sb.ev) hipEventRecord(sb.ev[5], s);
}

}  // namespace mh
