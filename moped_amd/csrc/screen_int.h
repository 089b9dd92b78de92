// Two-stage MATCH, internal to the screen's own files (match_screen.hip has the argument and the launch plan; screen_db.hip
// the f16 images; screen_ab32.hip and screen_ab16.hip passes A and B on either MFMA shape; screen_rescore.hip pass C):
// the constants, argument structs and launch calls that more than one of them needs.
#pragma once
#include "common.h"
#include "screen.h"

namespace mh {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
#define MH_AS1 __attribute__((address_space(1)))
#define MH_AS3 __attribute__((address_space(3)))

constexpr int SC_QPAD = 3 * 1024;                  // the query image is padded to whole workgroups of every kernel width
constexpr int SC_TILE = 128;                       // DB rows per LDS tile (= the DB's row padding)
constexpr int SC_TILE_BYTES = SC_TILE * DIM * 2;   // 32 KB of f16
constexpr bool SC_SHAPE16_LARGE = true;   // the four-query-block launches run on v_mfma_f32_16x16x32_f16 (screen16_kernel)
constexpr int SC_WAVES = 8;                        // wavefronts per workgroup of passes A and B: one workgroup per CU, two of its wavefronts per SIMD
constexpr int SC_GROUP = 1;                       // tiles per barrier: the wavefronts of a workgroup drift apart within a group
constexpr int SC_NBUF = 2 * SC_GROUP;              // (a hit costs its wavefront ~300 cycles), every barrier makes seven wait for the slowest
constexpr int SC_DD = 192;                         // floats per tile of the -dd/2 array: 128 rows, the 4 row blocks' maxima, their minima, padding
constexpr int SC_LDS_TILES = SC_NBUF * SC_TILE_BYTES + SC_NBUF * SC_DD * 4;   // the tiles + their -dd/2 terms
static_assert(SC_TILE == 128 && DIM == 128, "tile image and chunk swizzle assume 128 x 128");

// ---- a query's candidate records (pass B writes them, pass C reads and re-empties them) ---------------------------
// screen_kernel (32x32x16):
// MODE 0 (pass A): top-2 VALUES of w~ per (split, query) over the sampled tiles -> part[split][q].
// MODE 1 (pass B): every row with w~ > tau(q) -> the query's candidate records {row0, bits}: rows
//                  row0 + (r & 3) + 8 (r >> 2) for the set bits r.  A lane owns the sub-list (query, split, half)
//                  -- `sub_cap` slots nobody else writes, no atomics; a sub-list that is full spills into the
//                  query's overflow list (atomic append, rare).  bits = 0 marks an empty slot.
constexpr int SC_SLOTS_MAX = 256;   // pass B's record slots per query: 2 halves x splits x sub_cap <= this
// ... and behind them the slots of the records pass A's sampled tiles leave (screen_handover_kernel; the one-sweep launches)
constexpr int SC_SA_SLOTS = 32;
constexpr int SC_SLOT_PITCH = SC_SLOTS_MAX + SC_SA_SLOTS;
// The 16x16x32 launches (screen16_kernel) use the same memory as ONE counted list per query instead: the records lie in
// recs[q * SC_SLOT_PITCH + 0 .. count), count = the query's word of `ovf_cnt` (those launches have no overflow list).
// screen_handover_kernel writes its records as the list's head and stores the count; pass B appends behind them with one
// atomic add per record, when a wavefront writes its parked hits out (screen16_kernel's flush_parked: outside the hit
// path).  A record that finds the list full is dropped and still counted: count > SC_SLOT_PITCH sends the query to pass
// C's brute-force search.  Pass C reads the count with its other scalars and 64 slots (one 512-byte line) in the same round
// trip, instead of every slot a sub-list might have used.  Between launches every slot is empty and every count zero, as
// the 32x32x16 launches -- which share a context's buffers with these -- need it: pass C re-empties what it consumed.

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
  int ablate;            // SC_PROF builds only (screen_ab32.hip sets it): 1 = no finish(), 2 = stage only the first tile, 4 = no MFMAs, 8 = no end-of-tile barrier
};

// pass A of the one-sweep launches (screen_ab16.hip has the argument)
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

// pass C's kernel argument (screen_rescore.hip)
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

// ---- the launches the plan states, per file ------------------------------------------------------------------------
// one sweep of a pass: the tiles tile_first + j * tile_stride, j < n_sel, shared out over n_splits splits
inline void set_sweep(ScreenArgs& a, int n_sel, int tile_first, int tile_stride, int n_splits) {
  a.n_sel = n_sel;
  a.tile_first = tile_first;
  a.tile_stride = tile_stride;
  a.n_splits = n_splits;
  a.tiles_base = n_sel / n_splits;
  a.tiles_rem = n_sel % n_splits;
}
// Pass A, the thresholds and pass B of a launch of `p.family` on stream s; `a` = everything but the sweeps' fields.
// ev (optional): [2], [3], [4] are recorded behind pass A, the thresholds and pass B.
void launch_passes32(ScreenArgs a, const ScreenPlan& p, hipEvent_t* ev, hipStream_t s);
// ... g = pass A's sweep as the hand-over kernel and pass C need it; inc = ScreenBufs::inc
void launch_passes16(ScreenArgs a, const ScreenPlan& p, const SampleGeom& g, unsigned int* inc, hipEvent_t* ev, hipStream_t s);
// pass C; compact = the launch's records are counted lists (family 16), else the lane-private slots + overflow list
void launch_pass_c(const RsArgs& args, bool compact, int n_cus, hipStream_t s);

}  // namespace mh
