// Two-stage MATCH (match_screen.hip): passes A and B on v_mfma_f32_32x32x16_f16, a query's records in lane-private
// sub-lists (screen_int.h), with the SC_PROF build's ablation hooks and counters (scripts/screen_prof.py).
#include <hip/hip_fp16.h>

#include <algorithm>

#include "screen_int.h"

MH_TRACE_TU()

namespace mh {

namespace {

// hits a wavefront parks in LDS (80 bytes each: the block's 16 values go along) before they go to memory, written out at
// the workgroup's end
constexpr int SC_RECBUF = 112;
constexpr int SC_REC_BYTES = 80;                   // {slot, row0, thr, top, 16 dots}
constexpr int SC_LDS_BYTES = SC_LDS_TILES + SC_WAVES * SC_RECBUF * SC_REC_BYTES;   // the tiles + the wavefronts' hit buffers

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

template <int MODE, int NQB>
__global__ __launch_bounds__(64 * SC_WAVES, 2) void screen_kernel(const ScreenArgs A) {
  MH_TRACE_SCOPE(MODE == 0 ? mh::TK_PASS_A : mh::TK_PASS_B);
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
  // w, w + 8, w + 16, w + 24.  Chunk g = 64 piece + lane of the LDS
  // image is row g >> 4, position g & 15, and holds source chunk (g & 15) ^ (row & 15); row & 15 = (4 w + (lane >> 4)) & 15
  // for all pieces of a wavefront (they lie 32 rows apart: a multiple of 16), so one per-lane offset serves them and the
  // pieces differ by 8 KB in a scalar base.  The rows' -dd/2 terms (512 B per tile) and the row blocks' extrema (768 B
  // per tile) come the same way: wavefronts 0..2, 4 bytes per lane.
  const unsigned voff = (unsigned)(wave * 1024 + (lane >> 4) * 256 + (((lane & 15) ^ ((wave * 4 + (lane >> 4)) & 15)) << 4));
  const unsigned voff_dd = (unsigned)((wave * 64 + lane) * 4);
  auto stage = [&](int sel, int buf) {
    const int tile = A.tile_first + sel * A.tile_stride;
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(A.dbh) + (size_t)tile * SC_TILE_BYTES;
    const unsigned l = lds_base + buf * SC_TILE_BYTES + wave * 1024;
    constexpr int STEP = SC_WAVES * 1024;   // bytes between a wavefront's pieces (the same in the source tile and in LDS)
    dma16x4(voff, tb, tb + STEP, tb + 2 * STEP, tb + 3 * STEP, l, l + STEP, l + 2 * STEP, l + 3 * STEP);
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
    if (!SC_ABL(3)) {   // (experiment builds: 8 = no end-of-tile wait and barrier -- what the synchronisation costs)
    if (more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wavefront's pieces of the next group have landed
    __syncthreads();   // everybody's pieces have; nobody reads this group's buffers any more
    }
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

namespace {

template <int NQB>
void launch_passes32_nqb(ScreenArgs a, const ScreenPlan& p, hipEvent_t* ev, hipStream_t s) {
  constexpr int QB = 32 * NQB * SC_WAVES;
  static DynLds attr0, attr1;
  attr0.ensure(screen_kernel<0, NQB>, SC_LDS_BYTES);
  attr1.ensure(screen_kernel<1, NQB>, SC_LDS_BYTES);
  const int nqb = (a.Q + QB - 1) / QB;   // the grid covers the capacity (the splits are sized for the queries expected)
#ifdef SC_PROF
  a.ablate = g_sc_ablate;
#endif
  set_sweep(a, p.a_n_sel, p.a_tile_first, p.a_stride, p.a_splits);
  hipLaunchKernelGGL((screen_kernel<0, NQB>), dim3(nqb * p.a_splits), dim3(64 * SC_WAVES), SC_LDS_BYTES, s, a);
  if (ev) hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(screen_tau_kernel, dim3((a.q_pad + 255) / 256), dim3(256), 0, s, a.part, p.a_splits, a.q_pad, a.Q, a.q_count,
                     a.qnorm, a.qbad, a.dmax, const_cast<float*>(a.tau));
  if (ev) hipEventRecord(ev[3], s);
  // pass B: all tiles; a query's record slots are shared out over 2 x b_splits lane-private sub-lists
  set_sweep(a, p.b_n_sel, 0, 1, p.b_splits);
  hipLaunchKernelGGL((screen_kernel<1, NQB>), dim3(nqb * p.b_splits), dim3(64 * SC_WAVES), SC_LDS_BYTES, s, a);
  if (ev) hipEventRecord(ev[4], s);
}

}  // namespace

void launch_passes32(ScreenArgs a, const ScreenPlan& p, hipEvent_t* ev, hipStream_t s) {
  if (p.nqb == 4) launch_passes32_nqb<4>(a, p, ev, s);
  else if (p.nqb == 2) launch_passes32_nqb<2>(a, p, ev, s);
  else launch_passes32_nqb<1>(a, p, ev, s);
}

}  // namespace mh
