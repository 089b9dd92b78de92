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
// its arithmetic (screen.h: screen_value_err, screen_margin) by tests/test_screen_bound_cpu.py.
//
// Shape (gfx950).  A workgroup of passes A and B = 8 wavefronts with a compute unit to itself, two wavefronts per SIMD.
// A wavefront keeps 32 NQB queries (NQB = 1, 2 or 4 by the size of the launch: screen_plan) in registers as the B
// operands of all k-steps; the f16 DB streams through LDS in 128-row tiles (32 KB, double buffered, filled by
// global_load_lds_dwordx4 with the 16-byte chunks of row r stored at chunk position c ^ (r & 15), so the A-operand
// ds_read_b128 of 16 lanes touch all 64 banks once).  Two kernel families share that shape and the exactness argument:
//   screen_ab32.hip   v_mfma_f32_32x32x16_f16.  Queries sit on the accumulator's lane axis, rows on its register axis: a
//                     lane's 16 values of a 32x32 block are 16 rows of ONE query, so the running maxima are lane-local
//                     v_max3_f32 (8 per block) and only a lane with a hit looks at individual values.  A query's records
//                     go to lane-private sub-lists.
//   screen_ab16.hip   v_mfma_f32_16x16x32_f16, the launches of 12 and more blocks of 1024 queries.  A query's records go
//                     to one counted list, and pass A hands the records of its own tiles over (one sweep of the DB).
// The f16 images are made by screen_db.hip, pass C is screen_rescore.hip; this file decides what is launched.
#include <algorithm>
#include <cstdlib>

#include "screen_int.h"

namespace mh {

size_t screen_rec_slots() { return SC_SLOT_PITCH; }

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

// The launch policy of a MATCH call, as host arithmetic: launch_match_screen launches what this says, mh_screen_plan
// shows it to the tests.
ScreenPlan screen_plan(int Q, int q_expected, int N) {
  // experiment builds (scripts/ab_env.sh); constants in the product
  static const int sample = std::max(1, exp_int("MH_SCREEN_SAMPLE", 8));   // pass A looks at every `sample`-th tile
  static const int blocks_a = std::max(1, exp_int("MH_SCREEN_BLOCKS_A", 256));   // workgroups of pass A
  static const int blocks_b_pin = std::max(0, exp_int("MH_SCREEN_BLOCKS", 0));   // ... of pass B; 0 = by size
  static const int sb_pin = exp_int("MH_SCREEN_SPLITS_B", 0);
  static const int nqb_pin = exp_int("MH_SCREEN_NQB", 0);
  static const int shape_pin = exp_int("MH_SCREEN_SHAPE", 0);
  static const int onesweep_on = exp_int("MH_SCREEN_ONESWEEP", 1);   // 0 = pass B sweeps every tile
  const int qe = (q_expected > 0 && q_expected < Q) ? std::max(q_expected, std::min(Q, 256)) : Q;
  const int n_tiles = (N + SC_TILE - 1) / SC_TILE;
  ScreenPlan p = {};

  // ---- which kernels.  Queries per workgroup: 1024 (four 32-query blocks per wavefront: every row fragment read from
  // LDS feeds four MFMAs; 256 VGPRs, no prefetched copy of the next row block) when the launch is large enough for
  // workgroups of >= 16 tiles -- pass B alone 8-10% faster, config 2 +9.7% frames/s --, else 512 (two blocks, row
  // fragments prefetched), or 256 for small frames.
  p.nqb = qe > 640 ? 2 : 1;
  if (qe >= 2048 && (long)n_tiles * ((qe + 1023) / 1024) >= 16L * 256) p.nqb = 4;
  if (nqb_pin == 1 || nqb_pin == 2 || nqb_pin == 4) p.nqb = nqb_pin;
  // the MFMA shape of the large launches: 16x16x32 (SC_SHAPE16_LARGE; MH_SCREEN_SHAPE = 1 / 2 pins 32x32x16 / 16x16x32 in
  // experiment builds), from 12 query blocks of 1024: with fewer, 21 splits leave compute units without a workgroup
  const bool shape16 = shape_pin == 2 || (shape_pin == 0 && SC_SHAPE16_LARGE);
  const bool p16 = shape16 && ((p.nqb == 4 && (shape_pin == 2 || (qe + 1023) / 1024 >= 12)) || (p.nqb == 2 && shape_pin == 2));
  p.family = p16 ? 16 : 32;

  const int QB = 32 * p.nqb * SC_WAVES;
  const int nqb_e = (qe + QB - 1) / QB;   // the splits are sized for the queries expected (the grid covers the capacity)
  auto splits_for = [&](int n_sel, int target, int s_max) {
    int S = std::max(1, target / nqb_e);
    S = std::min(std::min(S, n_sel), s_max);
    // whole splits per XCD (a split's rows stay in one L2) unless the rounding would leave CUs without a workgroup:
    // 24 query blocks x 8 splits fill 192 of 256 CUs, x 10 fill 240 (measured: 10% on the stage at Q = 12000)
    if (S >= 8 && (S / 8 * 8) * 33 >= S * 32) S = S / 8 * 8;
    return std::max(S, 1);
  };

  // ---- pass A: every `stride`-th tile, starting in the middle of the first stride
  // (a shard of a few models: the records a query leaves do not shrink with the shard, the MFMA work beside them does --
  // every 4th tile there: half the records for 1/8 more of pass A's rows.  15 000 rows x 96 000 queries: pass B 0.38 ->
  // 0.34 ms, pass A 0.055 -> 0.09, the rank's frames/s +2.5%)
  const int every = sample == 8 && n_tiles < 256 ? 4 : sample;
  p.a_stride = n_tiles >= 4 * every ? every : 1;
  p.a_n_sel = (n_tiles + p.a_stride - 1) / p.a_stride;
  // (16x16x32: the lists of 4 x a_splits lane slots per query, screen_part_bytes)
  p.a_splits = splits_for(p.a_n_sel, blocks_a, p16 ? SC_SA_SPLITS_MAX : screen_max_splits_a());
  p.a_tile_first = std::max(0, std::min(p.a_stride / 2, n_tiles - 1 - (p.a_n_sel - 1) * p.a_stride));

  if (!p16) {
    // ---- pass B, 32x32x16: all tiles; a query's record slots are shared out over 2 x b_splits lane-private sub-lists.
    // Twice as many workgroups as CUs when every one of them still sweeps >= 24 tiles: two rounds of half-length
    // workgroups finish more evenly than one round of ~240 (pass B alone 0.272 -> 0.261 ms at Q = 12000, N = 100k), and
    // under load a one-round grid stalls on every CU another frame's kernel holds (+5% frames/s at config 1, +3% at
    // config 2).  With fewer tiles per workgroup the query-operand prologue costs more than that (Q = 3000: 0.445 ->
    // 0.394 of peak), so small launches keep one workgroup per CU.
    const int blocks_b = blocks_b_pin > 0 ? blocks_b_pin : (long)n_tiles * nqb_e >= (p.nqb >= 4 ? 16L : 24L) * 512 ? 512 : 256;
    p.b_n_sel = n_tiles;
    p.b_splits = sb_pin > 0 ? std::min(std::min(sb_pin, n_tiles), SC_SLOTS_MAX / 2) : splits_for(n_tiles, blocks_b, SC_SLOTS_MAX / 2);
    // (few splits = long sub-streams: a lane sees many of its query's candidates, its sub-list must hold them)
    p.sub_cap = std::max(1, std::min(48, SC_SLOTS_MAX / (2 * p.b_splits)));
    p.n_slots = 2 * p.b_splits * p.sub_cap;
    return p;
  }

  // ---- 16x16x32.  One sweep: pass A keeps the identity of its best blocks (the block's number inside a lane slot in the
  // low mantissa bits of the block's maximum) and pass B leaves the sampled tiles out.  Not when pass A sees every tile
  // anyway, nor when a lane slot would have more blocks than SC_PACK_BITS_MAX bits count even with all the splits pass A
  // may have (7 M rows): pass B then sweeps all tiles as before, and the block maxima stay as they are (0 bits).
  if (onesweep_on && p.a_stride > 1)   // (a long sweep: more, shorter splits rather than wider block numbers)
    while (4 * ((p.a_n_sel + p.a_splits - 1) / p.a_splits) > (1 << SC_PACK_BITS_MAX) && p.a_splits < SC_SA_SPLITS_MAX) ++p.a_splits;
  const int blocks_slot = 4 * ((p.a_n_sel + p.a_splits - 1) / p.a_splits);
  int bits = 2;
  while ((1 << bits) < blocks_slot) ++bits;
  p.onesweep = onesweep_on && p.a_stride > 1 && bits <= SC_PACK_BITS_MAX;
  p.pack_bits = p.onesweep ? bits : 0;
  p.skip_first = p.onesweep ? p.a_tile_first : 0;
  p.skip_stride = p.onesweep ? p.a_stride : 0;
  // Pass B's splits.  b_splits <= 21 dates from the lane-private layout (a query's 256 slots shared out over 4 x Sb
  // sub-lists, each with room for three records: 12 000 queries x 250 000 rows ran 42 splits with ONE slot per sub-list for
  // a while, 42 brute-force queries per launch, pass C 10 ms instead of 0.03); the counted lists do not need it -- no
  // sub_cap, no n_slots: a query's records go to one list of SC_SLOT_PITCH places whatever the splits, and pass C reads by
  // the count -- and it stays because the launch geometry was not to change with them.  One workgroup per compute unit, so
  // the launch takes ceil(workgroups / 256) rounds of tiles / b_splits tiles each: the count with the least rounds x tiles,
  // the larger of equals.  (MH_SCREEN_BLOCKS: an experiment's request, capped the same way.)
  constexpr int SB16_MAX = SC_SLOTS_MAX / 12;
  p.b_n_sel = p.onesweep ? n_tiles - p.a_n_sel : n_tiles;
  p.b_splits = 1;
  if (blocks_b_pin > 0) {
    p.b_splits = std::min(splits_for(p.b_n_sel, blocks_b_pin, SC_SLOTS_MAX / 4), SB16_MAX);
  } else {
    double best = 1e30;
    for (int c = 1; c <= std::min(SB16_MAX, std::max(1, p.b_n_sel / 8)); ++c) {
      const double cost = (double)((nqb_e * c + 255) / 256) * (double)((p.b_n_sel + c - 1) / c);
      if (cost <= best) {
        best = cost;
        p.b_splits = c;
      }
    }
  }
  return p;
}

void launch_match_screen(const float* qn, const float* qnorm, int Q, const float* db, const float* dnorm, int N,
                         const RowMap& rmap, const ScreenDb& sdb, const ScreenBufs& sb, int32_t* idx1, float* d1,
                         float* d2, hipStream_t s, const int32_t* q_count, int q_expected) {
  const ScreenPlan p = screen_plan(Q, q_expected, N);
  const int q_pad = screen_q_pad(Q);

  if (sb.ev) hipEventRecord(sb.ev[0], s);
  launch_screen_prepare(qn, qnorm, Q, q_pad, sb.qh, sb.qbad, s, q_count);
  // the lane: everything from pass A to pass B on its stream, handed over by events
  hipStream_t sbig = s;
  if (sb.big && sb.ev_in && sb.ev_out) {
    hipEventRecord(sb.ev_in, s);
    hipStreamWaitEvent(sb.big, sb.ev_in, 0);
    sbig = sb.big;
  }
  if (sb.ev) hipEventRecord(sb.ev[1], sbig);
  ScreenArgs a = {};   // (the sweeps' fields: set_sweep, per launch)
  a.qh = sb.qh;
  a.dbh = sdb.dbh;
  a.dneg = sdb.dneg;
  a.qnorm = qnorm;
  a.qbad = sb.qbad;
  a.q_count = q_count;
  a.part = sb.part;
  a.part5 = reinterpret_cast<float*>(sb.part);
  a.tau = sb.tau;
  a.recs = sb.recs;
  a.ovf_cnt = sb.ovf_cnt;
  a.ovf = sb.ovf;
  a.ovf_cap = sb.ovf_cap;
  a.sub_cap = p.sub_cap;
  a.Q = Q;
  a.q_pad = q_pad;
  a.n_splits_a = p.a_splits;
  a.pack_keep = ~((1u << p.pack_bits) - 1u);
  a.skip_first = p.skip_first;
  a.skip_stride = p.skip_stride;
  a.dmax = sdb.dmax;
  // what pass C has to know about pass A's sweep (no hand-over: nothing)
  SampleGeom geom = {0, 0, 0, 1, 0, 0, 0};
  if (p.family == 16) {
    geom = {p.onesweep ? SC_SA_SLOTS : 0, p.pack_bits, p.a_tile_first, p.a_stride, p.a_n_sel / p.a_splits, p.a_n_sel % p.a_splits, p.a_n_sel};
    launch_passes16(a, p, geom, sb.inc, sb.ev, sbig);
  } else {
    launch_passes32(a, p, sb.ev, sbig);
  }
  if (sbig != s) {
    hipEventRecord(sb.ev_out, sbig);
    hipStreamWaitEvent(s, sb.ev_out, 0);
  }
  RsArgs ca;
  ca.qn = qn; ca.qnorm = qnorm; ca.qbad = sb.qbad; ca.Q = Q; ca.q_count = q_count; ca.db = db; ca.dnorm = dnorm; ca.N = N;
  ca.rmap = rmap; ca.recs = sb.recs; ca.n_slots = p.n_slots; ca.ovf_cnt = sb.ovf_cnt; ca.ovf = sb.ovf; ca.ovf_cap = sb.ovf_cap;
  ca.dmax = sdb.dmax; ca.tau = sb.tau; ca.spread = sdb.spread; ca.idx1 = idx1; ca.d1 = d1; ca.d2 = d2; ca.stats = sb.stats;
  ca.zero_idx = sdb.zero_idx; ca.zero_d1 = sdb.zero_d1; ca.zero_d2 = sdb.zero_d2; ca.g = geom;
  ca.inc = geom.sa_slots > 0 ? sb.inc : nullptr; ca.inc_count = sb.inc ? sb.inc + sb.q_pad : nullptr; ca.dbh = sdb.dbh; ca.dneg = sdb.dneg;
  ca.accept_ratio = sb.accept_ratio > 0.f ? sb.accept_ratio : 0.f;
  ca.prerej = sb.inc ? sb.inc + sb.q_pad + 1 : nullptr;   // (behind the incomplete words and their counter)
  launch_pass_c(ca, p.family == 16, sb.n_cus, s);
  if (sb.ev) hipEventRecord(sb.ev[5], s);
}

}  // namespace mh
