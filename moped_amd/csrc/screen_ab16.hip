// Two-stage MATCH (match_screen.hip): passes A and B on v_mfma_f32_16x16x32_f16, a query's records in one counted list
// (screen_int.h), and the hand-over kernel between them.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "screen_int.h"

MH_TRACE_TU()

namespace mh {

namespace {

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
constexpr int SC_REC16_BYTES = 48;                  // {slot, row0, thr, top, 8 dots}
// Parked hits per wavefront: what the 160 KB of a compute unit leave beside the tiles and the thresholds (the 256-register
// workgroup has the CU to itself whatever its LDS), 11.25 KB.  A hit that finds the buffer full appends from the hit path
// with an atomic add whose value it waits for, and seven wavefronts wait for it at the tile's barrier: with 170 places (8
// KB) 51 775 hits of a judged launch did; profiles/wave_sublists_ab.txt has what pass B costs without any.
constexpr int SC_RECBUF16 = 240;
constexpr int SC_LDS16_TAU = SC_LDS_TILES + 8 * SC_RECBUF16 * SC_REC16_BYTES;   // the wavefronts' thresholds: 8 x 128 floats
constexpr int SC_LDS16_BYTES = SC_LDS16_TAU + 8 * 128 * 4;
static_assert(SC_LDS16_BYTES <= 160 * 1024, "screen16_kernel's LDS fits a gfx950 compute unit");

template <int MODE, int NQB>
__global__ __launch_bounds__(512, 2) void screen16_kernel(const ScreenArgs A) {
  MH_TRACE_SCOPE(MODE == 0 ? mh::TK_PASS_A : mh::TK_PASS_B);
  constexpr int QW = 32 * NQB;            // queries per wavefront
  constexpr int QB = QW * SC_WAVES;            // queries per workgroup
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
      // buffer full.  (The list's address is worked out HERE: the lane's eight queries never change, and the compiler
      // would keep eight 64-bit addresses across the sweep for this branch alone -- 16 registers this kernel does not have.)
      const int at = atomicAdd(&A.ovf_cnt[q], 1);
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
      if (lane + 64 * i < n) at[i] = atomicAdd(&A.ovf_cnt[e[i].x], 1);
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

}  // namespace

int screen_park_places() { return SC_RECBUF16; }

namespace {

template <int NQB>
void launch_passes16_nqb(ScreenArgs a, const ScreenPlan& p, const SampleGeom& g, unsigned int* inc, hipEvent_t* ev, hipStream_t s) {
  constexpr int QB = 32 * NQB * SC_WAVES;
  static DynLds attr0, attr1;
  attr0.ensure(screen16_kernel<0, NQB>, SC_LDS16_BYTES);
  attr1.ensure(screen16_kernel<1, NQB>, SC_LDS16_BYTES);
  const int nqb = (a.Q + QB - 1) / QB;   // the grid covers the capacity (the splits are sized for the queries expected)
  set_sweep(a, p.a_n_sel, p.a_tile_first, p.a_stride, p.a_splits);
  hipLaunchKernelGGL((screen16_kernel<0, NQB>), dim3(nqb * p.a_splits), dim3(64 * SC_WAVES), SC_LDS16_BYTES, s, a);
  if (ev) hipEventRecord(ev[2], s);
  // 64 queries per workgroup, one wavefront per split of pass A (its four lane slots) -- or per two splits when pass A has
  // more than HO_PARTS_MAX
  static_assert(SC_SA_SPLITS_MAX <= 2 * HO_PARTS_MAX, "a thread of screen_handover_kernel holds at most 8 lane slots");
  if (p.a_splits <= HO_PARTS_MAX)
    hipLaunchKernelGGL(screen_handover_kernel<4>, dim3((a.q_pad + 63) / 64), dim3(64, p.a_splits), 0, s, (const float*)a.part5,
                       4 * p.a_splits, a.q_pad, a.Q, a.q_count, a.qnorm, a.qbad, a.dmax, g, const_cast<float*>(a.tau), a.recs, a.ovf_cnt, inc);
  else
    hipLaunchKernelGGL(screen_handover_kernel<8>, dim3((a.q_pad + 63) / 64), dim3(64, (p.a_splits + 1) / 2), 0, s, (const float*)a.part5,
                       4 * p.a_splits, a.q_pad, a.Q, a.q_count, a.qnorm, a.qbad, a.dmax, g, const_cast<float*>(a.tau), a.recs, a.ovf_cnt, inc);
#ifdef MH_EXPERIMENTS
  // what the records cost pass B: thresholds no value reaches (WRONG results: timing only)
  if (exp_int("MH_SCREEN_NO_HITS", 0)) hipMemsetAsync(const_cast<float*>(a.tau), 0x7f, (size_t)a.q_pad * sizeof(float), s);
#endif
  if (ev) hipEventRecord(ev[3], s);
  // pass B: the tiles pass A did not see (all tiles when there is no hand-over); a query's records go to its one counted
  // list, and pass C finds them by the count
  set_sweep(a, p.b_n_sel, 0, 1, p.b_splits);
  hipLaunchKernelGGL((screen16_kernel<1, NQB>), dim3(nqb * p.b_splits), dim3(64 * SC_WAVES), SC_LDS16_BYTES, s, a);
  if (ev) hipEventRecord(ev[4], s);
}

}  // namespace

void launch_passes16(ScreenArgs a, const ScreenPlan& p, const SampleGeom& g, unsigned int* inc, hipEvent_t* ev, hipStream_t s) {
#ifdef MH_EXPERIMENTS
  if (p.nqb == 2) return launch_passes16_nqb<2>(a, p, g, inc, ev, s);   // (only a pinned shape gets here: MH_SCREEN_SHAPE = 2 with two query blocks)
#endif
  launch_passes16_nqb<4>(a, p, g, inc, ev, s);
}

}  // namespace mh
