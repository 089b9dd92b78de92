// Two-stage MATCH (match_screen.hip): pass C, the canonical f32 arithmetic on the rows the screen could not rule out.
#include <type_traits>
#include <hip/hip_fp16.h>

#include <algorithm>

#include "screen_int.h"

MH_TRACE_TU()

namespace mh {

namespace {

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
// builds (launch_pass_c's MH_PASSC_* switches): workgroups of 16 wavefronts, two per compute unit (or of 12 at six
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

template <int WAVES, int PF, int COMPACT, int ACCEPT = 0>
void launch_pass_c_layout(int grid, hipStream_t s, const RsArgs& args) {
  static DynLds attr;
  attr.ensure(rescore_kernel<WAVES, PF, COMPACT, ACCEPT>, rs_lds_bytes(WAVES));
  hipLaunchKernelGGL((rescore_kernel<WAVES, PF, COMPACT, ACCEPT>), dim3(grid), dim3(64 * WAVES), rs_lds_bytes(WAVES), s, args);
}
// compact: the launch's records are counted lists (the 16x16x32 launches), else the lane-private slots + overflow list
template <int WAVES, int PF>
void launch_pass_c_shape(int grid, hipStream_t s, const RsArgs& args, bool compact) {
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

}  // namespace

int screen_prerej_words() { return RS_PREREJ_WORDS * RS_PREREJ_PITCH; }
int screen_prerej_pitch() { return RS_PREREJ_PITCH; }
void launch_screen_sample_values(const float* qn, int Q, const ScreenDb& sdb, const int32_t* row0, float* out, hipStream_t s) {
  if (Q <= 0) return;
  hipLaunchKernelGGL(screen_sample_values_kernel, dim3(Q), dim3(64), 0, s, qn, sdb.dbh, sdb.dneg, row0, out);
}

// pass C: a wavefront per query, four to a workgroup (one where the caller named its ratio test)
void launch_pass_c(const RsArgs& args, bool compact, int n_cus, hipStream_t s) {
  const int Q = args.Q;
  (void)n_cus;
  if (args.accept_ratio > 0.f) {
#ifdef MH_EXPERIMENTS
    // queries per workgroup of the accepting kernel (scripts/ab_env.sh; profiles/accept_reject_ab.txt): MH_PASSC_WAVES = 4 / 2
    static const int pa_waves = exp_int("MH_PASSC_WAVES", RS_WAVES_ACCEPT);
    if (pa_waves == 4) launch_pass_c_accept<4>(Q, s, args, compact);
    else if (pa_waves == 2) launch_pass_c_accept<2>(Q, s, args, compact);
    else
#endif
    launch_pass_c_accept<RS_WAVES_ACCEPT>(Q, s, args, compact);
    return;
  }
#ifdef MH_EXPERIMENTS
  // the shapes that were measured against this one (rescore_kernel's comment; scripts/ab_env.sh): MH_PASSC_WAVES = 16 / 12
  // for the launches of more than two fat workgroups per compute unit (MH_PASSC_FAT_ALL = 1: for every launch), MH_PASSC_K
  // such workgroups per compute unit as the whole grid (0 = a wavefront per query), MH_PASSC_PREFETCH = 0 / 1 / 2
  static const int pc_waves = exp_int("MH_PASSC_WAVES", RS_WAVES), pc_k = exp_int("MH_PASSC_K", RS_FAT_K);
  static const int pc_pf = exp_int("MH_PASSC_PREFETCH", 0), pc_all = exp_int("MH_PASSC_FAT_ALL", 0);
  if (n_cus <= 0) n_cus = 256;
  const int fat_waves = pc_waves == 12 ? 12 : RS_WAVES_FAT;
  if (pc_waves != RS_WAVES && (pc_all || Q > RS_FAT_K * n_cus * RS_WAVES_FAT)) {
    const int cover = (Q + fat_waves - 1) / fat_waves, grid = pc_k > 0 ? std::min(cover, pc_k * n_cus) : cover;
    if (fat_waves == 12 && pc_pf == 0) launch_pass_c_shape<12, 0>(grid, s, args, compact);
    else if (fat_waves == 12 && pc_pf == 1) launch_pass_c_shape<12, 1>(grid, s, args, compact);
    else if (fat_waves == 12) launch_pass_c_shape<12, 2>(grid, s, args, compact);
    else if (pc_pf == 0) launch_pass_c_shape<RS_WAVES_FAT, 0>(grid, s, args, compact);
    else if (pc_pf == 1) launch_pass_c_shape<RS_WAVES_FAT, 1>(grid, s, args, compact);
    else launch_pass_c_shape<RS_WAVES_FAT, 2>(grid, s, args, compact);
  } else
#endif
  launch_pass_c_shape<RS_WAVES, 0>((Q + RS_WAVES - 1) / RS_WAVES, s, args, compact);
}

}  // namespace mh
