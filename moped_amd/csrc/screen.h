// Two-stage MATCH (match_screen.hip and the screen_*.hip files): what the rest of the library needs to know about it.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mh {

// Per-database part of the screen, built at upload.
struct ScreenDb {
  const _Float16* dbh = nullptr;   // [rows padded to 128][128] f16 image of the (normalised) descriptors
  const float* dneg = nullptr;     // [tiles][192]: -dot(d,d)/2 of the tile's 128 rows (-inf on padding rows), then per 32-row block the largest and the smallest of them
  float dmax = 0.f;                // max_r |d_r| (sqrt of the largest norm term)
  float spread = __builtin_inff(); // largest (max - min) of -dd/2 inside a 32-row block of real rows
  bool usable = false;             // every norm term finite and non-negative, every coordinate inside f16's range
  // the answer for an all-zero query (its distance to row r is the row's norm term, exactly): a zero query ties with
  // every row of a normalised DB on the screen -- its candidate lists would overflow and it would go to brute force
  int32_t zero_idx = -1;
  float zero_d1 = __builtin_inff(), zero_d2 = __builtin_inff();
};

// Per-context scratch of the screen (frames of one context are stream ordered).
struct ScreenBufs {
  _Float16* qh = nullptr;          // [q_pad][128]
  uint8_t* qbad = nullptr;         // [q_pad] queries the screen does not vouch for (brute force in pass C)
  float2* part = nullptr;          // [screen_part_bytes(q_pad)] pass A's output: per-split top-2 values, or the lane slots' lists of the one-sweep launches
  float* tau = nullptr;            // [q_pad] the queries' thresholds for pass B
  // [q_pad][screen_rec_slots()] candidate records, all empty between frames.  Two layouts share the memory and that
  // invariant: lane-private sub-lists (+ the overflow list) in the 32x32x16 launches, ONE counted list per query from
  // slot 0 in the 16x16x32 launches (screen_int.h, SC_SLOT_PITCH)
  uint2* recs = nullptr;
  // [q_pad] zero between frames.  32x32x16 launches: records in the query's overflow list; 16x16x32 launches: records
  // in the query's list (more than screen_rec_slots() = some were dropped, brute force in pass C)
  int32_t* ovf_cnt = nullptr;
  uint2* ovf = nullptr;            // [q_pad][ovf_cap] (32x32x16 launches)
  int ovf_cap = 0, q_pad = 0;
  hipEvent_t* ev = nullptr;        // optional [6]: recorded around prepare / pass A / thresholds / pass B / pass C (mh_match_timing)
  // optional lane (mh_lane_create): passes A and B -- the kernels whose workgroups need whole compute units -- run on
  // `big` (a stream confined to a CU mask, or of lower priority) between two event hand-offs; the small kernels stay on
  // the context's stream
  hipStream_t big = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  unsigned int* stats = nullptr;   // optional [q_pad][3] per-query tallies: candidate rows, brute-force searches, searches
  // [q_pad] the queries' incomplete words of the one-sweep launches (which lane slots of pass A pass C has to sweep; 0 = none),
  // then one counter: queries that took that sweep since the last mh_match_incomplete(reset)
  // then screen_prerej_words() words: the counters of the queries pass C answered without a search (accept_ratio)
  unsigned int* inc = nullptr;
  // > 0: the caller applies the ratio test `d1 / d2 < accept_ratio` to every result and reads nothing else of a query that
  // fails it -- pass C then answers a query its records prove to fail with (-1, inf, inf) (screen_reject_proved); 0 = the
  // exact triple for every query
  float accept_ratio = 0.f;
  int n_cus = 0;                   // compute units of the device, 0 = not known (experiment builds: the grid of pass C's walking shapes)
};

// ---- the error model (the header of match_screen.hip) -----------------------------------------------------------------
// E(q), the bound of ONE screen value's distance from w = p - dd / 2; tau = T - screen_margin
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

// ---- what a candidate record says about its block (pass B writes it, pass C prunes by it) -------------------------
// Pass B works on the 16 dot products a lane holds of a 32-row block.  `top` = the largest of them, `thr` = tau(q) - the
// block's largest -dd/2: the record carries f16(top - thr) = the block's largest screen value above tau, seen through
// the block's largest norm term (an UPPER bound of the largest screen value of the record's rows).
__host__ __device__ inline unsigned short screen_record_value(float top, float thr) {
  const _Float16 h = (_Float16)(top - thr);
  unsigned short b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}
// Bounds of the largest screen value among the record's rows: hi >= it always; lo <= it when the block is 32 real
// rows (`spread` = the DB's largest in-block spread of -dd/2; a block with padding rows gives no lower bound).  Pass C
// drops a record whose `hi` lies below (second largest `lo` over the query's records) - screen_margin: two records hold
// different rows, so that second largest lower bound is a lower bound of the DB's second largest screen value, and a row
// of the exact top-2 lies at most 2E below THAT (the header of match_screen.hip).  tests/test_screen_bound_cpu.py checks
// both inequalities in host arithmetic (mh_screen_record_bounds).
__host__ __device__ inline void screen_record_bounds(unsigned short value_bits, unsigned row0, float tau_q, float spread, int N,
                                                     float dmax, float& lo, float& hi) {
  _Float16 h;
  __builtin_memcpy(&h, &value_bits, 2);
  const float dv = (float)h;
  // nearest f16: 2^-11 dv (2^-25 below the normals), doubled; + the f32 roundings on the way
  const float eps = fabsf(dv) * 0.001f + 1e-6f + 4e-7f * (fabsf(tau_q) + 0.5f * dmax * dmax);
  const bool fin = fabsf(dv) < 6.0e4f && fabsf(tau_q) < 1e30f;   // inf / nan: no information
  const bool whole = (int)(row0 | 31u) < N;                       // the block's 32 rows are all real rows
  hi = fin ? tau_q + dv + eps : __builtin_inff();
  lo = fin && whole && spread < 1e30f ? tau_q + dv - spread - eps : -__builtin_inff();
}

// ---- the one-sweep launches: pass A's block maxima carry their block's number ---------------------------------------
// screen16_kernel's pass A replaces the low `bits` mantissa bits of a block's largest screen value by the block's number
// inside its lane slot (screen_ab16.hip, "pass A of the one-sweep launches").
__host__ __device__ inline float screen_pack_value(float v, unsigned id, int bits) {
  const unsigned keep = ~((1u << bits) - 1u);
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  u = (u & keep) | (id & ~keep);
  __builtin_memcpy(&v, &u, 4);
  return v;
}
// How far a packed value can lie from the value it was made from, either way: the low `bits` bits of a normal float are
// worth less than 2^(bits - 23) |v|, those of a subnormal less than 2^(bits - 149); and every screen value of a query
// satisfies |v| <= W = |q_h| |d_h| + dd / 2 + the f32 accumulation <= 1.01 (|q| Dmax + Dmax^2 / 2) + 4e-7 (|q| + Dmax)
// (f16 rounding of the operands: a factor (1 + 2^-11)^2, and 2^-25 per element in the subnormal range, as in
// screen_margin).  tests/test_screen_pack_cpu.py checks it in float64.
__host__ __device__ inline float screen_pack_pert(float qq, float dmax, int bits) {
  const float nq = sqrtf(fmaxf(qq, 0.f));
  const float W = 1.01f * (nq * dmax + 0.5f * dmax * dmax) + 4e-7f * (nq + dmax) + 1e-30f;
  return W * ldexpf(1.f, bits - 23);
}
// Bounds of the largest screen value of a block of a SAMPLED tile from its record (screen_handover_kernel): the record
// carries f16(v' - tau) with v' the block's packed maximum -- pass A's accumulators start at the rows' own -dd/2, so the
// block's maximum is its largest screen value itself (no `spread`, and padding rows, at -inf, do not matter: a record's
// maximum is a real row's).  `pert` = screen_pack_pert of the query.
__host__ __device__ inline void screen_sample_bounds(unsigned short value_bits, float tau_q, float pert, float dmax, float& lo,
                                                     float& hi) {
  _Float16 h;
  __builtin_memcpy(&h, &value_bits, 2);
  const float dv = (float)h;
  const float eps = fabsf(dv) * 0.001f + 1e-6f + 4e-7f * (fabsf(tau_q) + 0.5f * dmax * dmax);   // as in screen_record_bounds
  const bool fin = fabsf(dv) < 6.0e4f && fabsf(tau_q) < 1e30f;
  hi = fin ? tau_q + dv + eps + pert : __builtin_inff();
  lo = fin ? tau_q + dv - eps - pert : -__builtin_inff();
}

constexpr int SCREEN_OVF_CAP = 64;   // records in a query's overflow list before the query falls back to brute force
size_t screen_rec_slots();           // record slots per query

int screen_prerej_words();   // words of ScreenBufs::inc behind the incomplete words and their counter
int screen_prerej_pitch();    // ... of which every screen_prerej_pitch()-th is a counter
// The screen values themselves, as the matrix pipe computes them (pass A's arithmetic: f16 operands, accumulator seeded
// with -dd/2, the block's MFMAs in ascending k -- eight v_mfma_f32_32x32x16_f16 or four k-steps of v_mfma_f32_16x16x32_f16):
// out[q][r] for q < Q, r < n_rows (both multiples of 32; qh =
// the queries' f16 image).  For tests of the error model against the HARDWARE's accumulation (mh_screen_values).
// shape: 0 = the instruction the large launches use, 1 = v_mfma_f32_32x32x16_f16, 2 = v_mfma_f32_16x16x32_f16
void launch_screen_values(const _Float16* qh, int Q, const ScreenDb& sdb, int n_rows, float* out, hipStream_t s, int shape);
// What pass C names the rows of a sampled tile's record by: for query q (device, [Q][128] f32, normalised) the screen values of
// the 8 + 8 rows of the blocks row0[2 q] and row0[2 q + 1] (a record's row0: tile x 128 + 32 row block + 4 quarter; bit b =
// row row0 + (b & 3) + 16 (b >> 2)), out[q][8 block + bit], by the code rescore_kernel runs (mh_screen_sample_values).
void launch_screen_sample_values(const float* qn, int Q, const ScreenDb& sdb, const int32_t* row0, float* out, hipStream_t s);
// the queries' f16 image and flags (q_count: optional device word, the frame's own number of queries)
void launch_screen_prepare(const float* qn, const float* qnorm, int Q, int q_pad, _Float16* qh, uint8_t* qbad, hipStream_t s,
                           const int32_t* q_count = nullptr);
size_t screen_db_half_elems(int N);
size_t screen_dneg_elems(int N);   // floats of the -dd/2 array: 192 per 128-row tile (rows, row blocks' extrema)
// f16 image + statistics {bits of max dd, bits of max |x|, non-finite flag, bits of the largest in-block spread,
// row / norm term / second norm term of an all-zero query's answer} (8 words, zeroed by the caller)
void launch_db_to_half(const float* db, const float* dnorm, int N, _Float16* dbh, float* dneg, unsigned int* stats,
                       hipStream_t s);
// the part of it that reads only the norm terms: the row blocks' extrema (entries 128..191 of every tile of dneg, stats[3])
// and the zero query's answer (stats[4..6]); launch_db_to_half ends with it, an edit of the DB (db_edit.hip) runs it
// behind its own pass over the rows
void launch_db_aggregates(const float* dnorm, int N, float* dneg, unsigned int* stats, hipStream_t s);
int screen_q_pad(int Q);
int screen_max_splits_a();
size_t screen_part_bytes(int q_pad);   // pass A's output buffer
// The launch plan of a MATCH call of Q queries (q_expected of them expected, 0 = Q) against N rows: host arithmetic,
// computed once by launch_match_screen and launched as stated; mh_screen_plan hands it out word by word, in this order.
struct ScreenPlan {
  int32_t family;        // 32 = screen_kernel (32x32x16, lane-private record lists), 16 = screen16_kernel (16x16x32, counted lists)
  int32_t nqb;           // 32-query blocks per wavefront: a workgroup takes 256 nqb queries
  // pass A sweeps the tiles a_tile_first + j * a_stride, j < a_n_sel, in a_splits splits
  int32_t a_tile_first, a_stride, a_n_sel, a_splits;
  int32_t pack_bits;     // (16) bits of a block maximum that carry the block's number; 0 = none
  int32_t onesweep;      // (16) pass A hands its tiles' records over, pass B skips them
  // pass B sweeps b_n_sel tiles in b_splits splits: all of them, or (one sweep) those that are not skip_first + i * skip_stride
  int32_t b_n_sel, b_splits;
  int32_t sub_cap;       // (32) slots of a lane's sub-list; 0 = counted lists
  int32_t skip_first, skip_stride;   // 0 = no tile is skipped
  int32_t n_slots;       // pass B's record slots per query that pass C scans: 2 b_splits sub_cap; 0 = by the list's count
};
ScreenPlan screen_plan(int Q, int q_expected, int N);
int screen_park_places();   // hits a wavefront of screen16_kernel's pass B parks before it appends from the hit path (SC_RECBUF16)
// mode: -1 = decide by size, 0 = never, 1 = whenever the DB has an f16 image (mh_match_set_mode)
bool screen_wanted(int q_expected, int N, int mode = -1);
// Same contract as launch_match (match.hip): exact (idx1, d1, d2) per query.
void launch_match_screen(const float* qn, const float* qnorm, int Q, const float* db, const float* dnorm, int N,
                         const RowMap& rmap, const ScreenDb& sdb, const ScreenBufs& sb, int32_t* idx1, float* d1,
                         float* d2, hipStream_t s, const int32_t* q_count, int q_expected);

}  // namespace mh
