// C ABI of libmoped_hip.so: context, model database, MATCH entry points.
// (CLUSTER / POSE / FILTER / frame entry points live in api_frame.hip, api_stage.hip and api_step.hip.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "context.h"
#include "steps.h"

using namespace mh;

namespace mh {

int use_stream(mh_ctx* ctx) {
  if (!ctx->held.empty()) db_poll_held(ctx, false);
  if (ctx->stream) return MH_OK;
  if (!ctx->own_stream) MH_HIP(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
  ctx->stream = ctx->own_stream;
  return MH_OK;
}

int ensure_scratch(mh_ctx* ctx, size_t bytes) {
  if (bytes > ctx->scratch.cap) MH_HIP(ctx, ctx->scratch.ensure(bytes + bytes / 4 + 4096, ctx->stream));
  return MH_OK;
}

int ensure_pinned(mh_ctx* ctx, size_t bytes) {
  if (bytes > ctx->pinned.cap) MH_HIP(ctx, ctx->pinned.ensure(bytes + bytes / 4 + 4096, ctx->stream));
  return MH_OK;
}

int ensure_own_depth(mh_ctx* ctx, size_t px) {
  MH_HIP(ctx, ctx->own_depth.ensure(px * 4, ctx->stream));
  MH_HIP(ctx, ctx->own_fill.ensure(px, ctx->stream));
  return MH_OK;
}

// the context's view of its store
void bind_store(mh_ctx* ctx) {
  const DbStore* st = ctx->store.get();
  ctx->N = st ? st->N : 0;
  ctx->n_models = st ? st->n_models : 0;
  ctx->index_base = st ? st->index_base : 0;
  ctx->rmap = RowMap();
  if (st) {
    ctx->rmap.base = st->index_base;
    ctx->rmap.nb = st->n_blocks;
    ctx->rmap.glo = st->blk_glo;
    ctx->rmap.llo = st->blk_llo;
  }
  ctx->db_desc = st ? st->desc : nullptr;
  ctx->db_norm = st ? st->norm : nullptr;
  ctx->db_xyz = st ? st->xyz : nullptr;
  ctx->db_model = st ? st->model : nullptr;
  ctx->sdb = st ? st->screen : ScreenDb();
}

int ensure_match_scratch(mh_ctx* ctx, int Q) {
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, ctx->match_pack.ensure(match_pack_floats(Q), s));
  MH_HIP(ctx, ctx->match_scratch.ensure(match_scratch_elems(Q, ctx->N > 0 ? ctx->N : 1), s));
  // the screen's scratch (only for a DB the screen can serve)
  const int q_pad = screen_q_pad(Q);
  if (ctx->sdb.usable && q_pad > ctx->sbuf.q_pad) {
    ScreenBufs& b = ctx->sbuf;
    mh_ctx::ScreenOwn& o = ctx->screen_own;
    b = ScreenBufs();
    const size_t qp = (size_t)q_pad, slots = qp * screen_rec_slots();
    MH_HIP(ctx, o.qh.ensure(qp * DIM, s));
    MH_HIP(ctx, o.qbad.ensure(qp, s));
    MH_HIP(ctx, o.part.ensure(screen_part_bytes(q_pad), s));
    MH_HIP(ctx, o.tau.ensure(qp, s));
    MH_HIP(ctx, o.recs.ensure(slots, s));
    MH_HIP(ctx, o.ovf_cnt.ensure(qp, s));
    MH_HIP(ctx, o.ovf.ensure(qp * SCREEN_OVF_CAP, s));
    MH_HIP(ctx, o.stats.ensure(qp * 3, s));
    const size_t inc_words = qp + 1 + (size_t)screen_prerej_words();
    MH_HIP(ctx, o.inc.ensure(inc_words, s));
    MH_HIP(ctx, hipMemsetAsync(o.inc, 0, inc_words * sizeof(unsigned int), s));
    // (every slot empty, every count zero: the state both record layouts start from and pass C restores, screen.h)
    MH_HIP(ctx, hipMemsetAsync(o.recs, 0, slots * sizeof(uint2), s));
    MH_HIP(ctx, hipMemsetAsync(o.ovf_cnt, 0, qp * sizeof(int32_t), s));
    MH_HIP(ctx, hipMemsetAsync(o.stats, 0, qp * 3 * sizeof(unsigned int), s));
    b.qh = o.qh;
    b.qbad = o.qbad;
    b.part = reinterpret_cast<float2*>(o.part.p);
    b.tau = o.tau;
    b.recs = o.recs;
    b.ovf_cnt = o.ovf_cnt;
    b.ovf = o.ovf;
    b.stats = o.stats;
    b.inc = o.inc;
    b.ovf_cap = SCREEN_OVF_CAP;
    b.q_pad = q_pad;   // only now: a failed allocation above leaves q_pad = 0 and the next call starts over
  }
  return MH_OK;
}

int ctx_match(mh_ctx* ctx, const float* qn, const float* qnorm, int Q, int32_t* idx1, float* d1, float* d2,
              const int32_t* q_count, int q_expected, float accept_ratio) {
  if (Q <= 0) return MH_OK;
  int rc = ensure_match_scratch(ctx, Q);
  if (rc) return rc;
  const int qe = (q_expected > 0 && q_expected < Q) ? q_expected : Q;
  const int screen_mode = ctx->match_mode >= 2 ? 0 : ctx->match_mode;        // modes 2 / 3 pin one of the exact kernels
  const int kernel_pin = ctx->match_mode >= 2 ? ctx->match_mode - 2 : -1;
  if (ctx->sdb.usable && ctx->sbuf.q_pad >= screen_q_pad(Q) && screen_wanted(qe, ctx->N, screen_mode)) {
    ctx->sbuf.ev = nullptr;
    if (ctx->timing && ctx->ev_made) {   // one event set per launch sequence, a ring of them (mh_match_timing)
      ctx->sbuf.ev = ctx->mev[ctx->mev_next];
      ctx->mev_next = (ctx->mev_next + 1) % mh_ctx::MEV_SETS;
      ++ctx->mev_used;
    }
    ctx->sbuf.big = ctx->lane_stream;
    ctx->sbuf.n_cus = ctx->n_cus;
    ctx->sbuf.ev_in = ctx->lane_in;
    ctx->sbuf.ev_out = ctx->lane_out;
    ctx->sbuf.accept_ratio = accept_ratio > 0.f ? accept_ratio : 0.f;   // (the exact kernels below answer every query)
    launch_match_screen(qn, qnorm, Q, ctx->db_desc, ctx->db_norm, ctx->N, ctx->rmap, ctx->sdb, ctx->sbuf, idx1, d1,
                        d2, ctx->stream, q_count, q_expected);
    ++ctx->match_launches[2];
  } else {
    const int k = launch_match(qn, qnorm, Q, ctx->db_desc, ctx->db_norm, ctx->N, ctx->rmap, ctx->match_scratch,
                               ctx->match_pack, idx1, d1, d2, ctx->stream, q_count, q_expected, kernel_pin);
    if (k >= 0) ++ctx->match_launches[k];
  }
  return MH_OK;
}

int ensure_frame_buffers(mh_ctx* ctx, int Q) {
  if (Q <= ctx->max_q) return MH_OK;
  int cap = ctx->max_q > 0 ? ctx->max_q : 4096;
  while (cap < Q) cap *= 2;
  const size_t n = (size_t)cap;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, ctx->q_desc.ensure(n * DIM, s));
  MH_HIP(ctx, ctx->q_norm.ensure(n, s));
  MH_HIP(ctx, ctx->q_uv.ensure(n * 2, s));
  MH_HIP(ctx, ctx->nn_idx.ensure(n, s));
  MH_HIP(ctx, ctx->nn_d1.ensure(n, s));
  MH_HIP(ctx, ctx->nn_d2.ensure(n, s));
  ctx->max_q = cap;   // the group's guard, once every member has its size
  return MH_OK;
}

}  // namespace mh

extern "C" {

int mh_create(int device, mh_ctx** out) {
  if (!out) return MH_ERR_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return MH_ERR_NODEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MH_ERR_NODEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MH_ERR_NODEVICE;  // gfx950 code objects only
  if (hipSetDevice(device) != hipSuccess) return MH_ERR_HIP;
  mh_ctx* ctx = new (std::nothrow) mh_ctx;
  if (!ctx) return MH_ERR_HIP;
  ctx->device = device;
  ctx->n_cus = prop.multiProcessorCount;
  // The context's own stream is created on first use (mh_use_stream): a host that
  // installs its own stream with mh_set_stream never takes a hardware queue for it.
  ctx->stream = nullptr;
  *out = ctx;
  return MH_OK;
}

void mh_free_frame_state(mh_ctx* ctx);  // frame_rest.hip
void mh_free_sift_state(mh_ctx* ctx);   // api_sift.hip
void mh_free_undistort_state(mh_ctx* ctx);   // undistort.hip

// (the context's buffers free themselves with `delete ctx`, the store with its last user)
void mh_destroy(mh_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  mh_free_frame_state(ctx);
  mh_free_sift_state(ctx);
  mh_free_undistort_state(ctx);
  db_poll_held(ctx, true);
  for (hipEvent_t e : ctx->held_events) hipEventDestroy(e);
  for (hipEvent_t e : ctx->db_ev)
    if (e) hipEventDestroy(e);
  if (ctx->wb_ev) hipEventDestroy(ctx->wb_ev);
  if (ctx->wb_stream) hipStreamDestroy(ctx->wb_stream);
  if (ctx->ev_made)
    for (auto& e : ctx->ev) hipEventDestroy(e);
  for (auto& set : ctx->mev)
    for (auto& e : set)
      if (e) hipEventDestroy(e);
  if (ctx->dlv.done) hipEventDestroy(ctx->dlv.done);
  if (ctx->hulls.done) hipEventDestroy(ctx->hulls.done);
  if (ctx->lane_in) hipEventDestroy(ctx->lane_in);
  if (ctx->lane_out) hipEventDestroy(ctx->lane_out);
  if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

#ifdef MH_EXPERIMENTS
// ---- lanes (experiment builds only; tried in round 3 and NOT shipped) ------------------------------------------------
// A host that keeps several frames in flight mixes two kinds of kernels on the device: passes A and B of MATCH, whose
// workgroups each take the whole register file of a compute unit, and a dozen small, latency-bound launches per batch.
// scripts/cu_trace.py: a fifth of the chip's unit-time holds only small workgroups, a sixth nothing.  A lane = a few
// extra streams for the big passes, confined to a CU mask that leaves `reserve` units of each XCD to everything else
// (mask bit i = unit i / 8 of XCD i % 8: scripts/experiments/cu_mask_probe.hip); a context with a lane hands over to
// it before pass A and takes its stream back after pass B (two event waits per MATCH launch sequence, ~12 us each).
// Measured (config 1, one box, bench.py --lane streams,reserve): off 12 000 frames/s; 4,1 11 940; 4,2 11 690; 4,4 11 710;
// 2,2 10 710; 8,2 11 020 -- what the reserved units give the small kernels, the hand-offs and the lane's in-order
// streams take back.  Lowest-priority lane streams instead of a mask HUNG the run (events between streams of different
// priority on this runtime): that variant is refused.
extern "C" int mh_lane_create(int device, int n_streams, int reserve_cus_per_xcd, int low_priority, mh_lane** out) {
  if (low_priority) return MH_ERR_ARG;
  if (!out || n_streams < 1 || n_streams > 16 || reserve_cus_per_xcd < 0 || reserve_cus_per_xcd > 16) return MH_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return MH_ERR_NODEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MH_ERR_HIP;
  const int n_cu = prop.multiProcessorCount;
  mh_lane* lane = new mh_lane;
  lane->device = device;
  lane->reserve = reserve_cus_per_xcd;
  lane->low_priority = low_priority;
  // CU mask bit i = unit i / 8 of XCD i % 8 on this part (scripts/experiments/cu_mask_probe.hip): the last `reserve`
  // units of every XCD stay out of the lane
  std::vector<uint32_t> mask((n_cu + 31) / 32, 0u);
  const int per_xcd = n_cu / 8;
  for (int i = 0; i < n_cu; ++i)
    if (i / 8 < per_xcd - reserve_cus_per_xcd) mask[i / 32] |= 1u << (i % 32);
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = numerically largest = least urgent
  for (int k = 0; k < n_streams; ++k) {
    hipStream_t s = nullptr;
    hipError_t e;
    if (reserve_cus_per_xcd > 0) e = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
    else if (low_priority) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, lo);
    else e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) {
      for (hipStream_t t : lane->streams) hipStreamDestroy(t);
      delete lane;
      return MH_ERR_HIP;
    }
    lane->streams.push_back(s);
  }
  *out = lane;
  return MH_OK;
}

extern "C" int mh_lane_destroy(mh_lane* lane) {
  if (!lane) return MH_OK;
  hipSetDevice(lane->device);
  for (hipStream_t s : lane->streams) {
    hipStreamSynchronize(s);
    hipStreamDestroy(s);
  }
  delete lane;
  return MH_OK;
}

extern "C" int mh_set_lane(mh_ctx* ctx, mh_lane* lane) {
  if (!ctx) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->stream) MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->lane_stream) MH_HIP(ctx, hipStreamSynchronize(ctx->lane_stream));
  ctx->lane = nullptr;
  ctx->lane_stream = nullptr;
  if (!lane) return MH_OK;
  if (lane->device != ctx->device || lane->streams.empty()) {
    ctx->err = "mh_set_lane: the lane belongs to another device";
    return MH_ERR_ARG;
  }
  if (!ctx->lane_in) MH_HIP(ctx, hipEventCreateWithFlags(&ctx->lane_in, hipEventDisableTiming));
  if (!ctx->lane_out) MH_HIP(ctx, hipEventCreateWithFlags(&ctx->lane_out, hipEventDisableTiming));
  ctx->lane = lane;
  ctx->lane_stream = lane->streams[lane->next++ % lane->streams.size()];
  return MH_OK;
}
#endif   // MH_EXPERIMENTS

const char* mh_last_error(const mh_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mh_set_stream(mh_ctx* ctx, void* hip_stream) {
  if (!ctx) return MH_ERR_ARG;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : nullptr;
  return hip_stream ? MH_OK : mh::use_stream(ctx);
}

int mh_synchronize(mh_ctx* ctx) {
  if (!ctx) return MH_ERR_ARG;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_db_upload(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host,
                 const float* xyz_host, int N, int n_models, int32_t index_base) {
  return mh_db_upload_raw(ctx, desc_host, model_of_host, xyz_host, N, n_models, index_base, 0);
}

int mh_db_upload_raw(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host,
                     const float* xyz_host, int N, int n_models, int32_t index_base, int normalize) {
  if (!ctx || N < 0 || n_models < 0 || (N > 0 && (!desc_host || !model_of_host || !xyz_host))) {
    if (ctx) ctx->err = "mh_db_upload: bad argument";
    return MH_ERR_ARG;
  }
  // every later kernel indexes per-model tables with these values; an edit (db_edit.hip) needs the rows grouped by
  // model in ascending order, and then each model's row range
  bool grouped = true;
  std::vector<int32_t> model_begin((size_t)n_models + 1, 0);
  for (int i = 0; i < N; ++i) {
    if (model_of_host[i] < 0 || model_of_host[i] >= n_models) {
      ctx->err = "mh_db_upload: model_of value outside [0, n_models)";
      return MH_ERR_ARG;
    }
    if (i > 0 && model_of_host[i] < model_of_host[i - 1]) grouped = false;
    ++model_begin[model_of_host[i] + 1];
  }
  for (int m = 0; m < n_models; ++m) model_begin[m + 1] += model_begin[m];
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // rows are padded to whole 128-row tiles for the match kernels: zero descriptors,
  // +inf norm terms (a padding row can never enter a top-2)
  const size_t Npad = ((size_t)N + 127) / 128 * 128;
  if (!ctx->store || ctx->store.use_count() > 1) {   // other contexts read the old store: leave it alone
    ctx->store = make_store(ctx->device);
  }
  DbStore* st = ctx->store.get();
  st->N = 0;
  st->screen = ScreenDb();
  st->grouped = grouped;
  st->model_begin = grouped ? std::move(model_begin) : std::vector<int32_t>();
  st->generation = 0;
  bind_store(ctx);
  hipStream_t s = ctx->stream;
  if (Npad > st->cap) {
    st->cap = 0;   // until every array has its new size
    MH_HIP(ctx, st->desc.ensure(Npad * DIM, s));
    MH_HIP(ctx, st->norm.ensure(Npad, s));
    MH_HIP(ctx, st->xyz.ensure(Npad * 3, s));
    MH_HIP(ctx, st->model.ensure(Npad, s));
    st->cap = Npad;
  }
  st->n_models = n_models;
  st->index_base = index_base;
  st->n_blocks = 0;   // one run of global rows starting at index_base (mh_db_upload_blocks sets the tables afterwards)
  if (N > 0) {
    MH_HIP(ctx, hipMemcpyAsync(st->desc, desc_host, (size_t)N * DIM * sizeof(float),
                               hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(st->xyz, xyz_host, (size_t)N * 3 * sizeof(float),
                               hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(st->model, model_of_host, (size_t)N * sizeof(int32_t),
                               hipMemcpyHostToDevice, ctx->stream));
    if (Npad > (size_t)N) {
      MH_HIP(ctx, hipMemsetAsync(st->desc + (size_t)N * DIM, 0, (Npad - N) * DIM * sizeof(float), ctx->stream));
      MH_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)(st->norm + N), 0x7F800000, Npad - N, ctx->stream));
    }
    if (normalize)
      launch_normalize(st->desc, st->norm, N, ctx->stream);   // A1 on the device, like Update() (:94)
    else
      launch_row_norms(st->desc, st->norm, N, ctx->stream);
    MH_HIP(ctx, hipGetLastError());
    // the screen's f16 image + what it needs to know about the rows (match_screen.hip)
    if (screen_wanted(1 << 30, N)) {
      const size_t need_h = screen_db_half_elems(N);
      if (need_h > st->cap_h) {
        st->cap_h = 0;
        MH_HIP(ctx, st->desc_h.ensure(need_h, s));
        MH_HIP(ctx, st->neg_h.ensure(screen_dneg_elems(N), s));
        st->cap_h = need_h;
      }
      MH_HIP(ctx, st->stats.ensure(8, s));
      MH_HIP(ctx, hipMemsetAsync(st->stats, 0, 8 * sizeof(unsigned int), ctx->stream));
      launch_db_to_half(st->desc, st->norm, N, st->desc_h, st->neg_h, st->stats, ctx->stream);
      MH_HIP(ctx, hipGetLastError());
      unsigned int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      MH_HIP(ctx, hipMemcpyAsync(h, st->stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      screen_from_stats(st, h);
    }
  }
  if (st->grouped) {   // the per-model row ranges for the kernels that walk a model's rows (hull.hip)
    MH_HIP(ctx, st->model_begin_dev.ensure(st->model_begin.size(), s));
    MH_HIP(ctx, hipMemcpyAsync(st->model_begin_dev, st->model_begin.data(), st->model_begin.size() * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->N = N;
  bind_store(ctx);
  return MH_OK;
}

int mh_db_upload_blocks(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host, const float* xyz_host, int N,
                        int n_models, const int32_t* block_global_row, const int32_t* block_rows, int n_blocks,
                        int normalize) {
  if (!ctx || n_blocks < 0 || (n_blocks > 0 && (!block_global_row || !block_rows))) {
    if (ctx) ctx->err = "mh_db_upload_blocks: bad argument";
    return MH_ERR_ARG;
  }
  long long rows = 0;
  for (int b = 0; b < n_blocks; ++b) {
    if (block_rows[b] <= 0 || block_global_row[b] < 0 ||
        (b > 0 && (long long)block_global_row[b] < (long long)block_global_row[b - 1] + block_rows[b - 1])) {
      ctx->err = "mh_db_upload_blocks: blocks must be non-empty runs of global rows in ascending order";
      return MH_ERR_ARG;
    }
    rows += block_rows[b];
  }
  if (rows != N) {
    ctx->err = "mh_db_upload_blocks: the blocks' rows do not add up to N";
    return MH_ERR_ARG;
  }
  int rc = mh_db_upload_raw(ctx, desc_host, model_of_host, xyz_host, N, n_models, n_blocks > 0 ? block_global_row[0] : 0,
                            normalize);
  if (rc || n_blocks <= 1) return rc;
  DbStore* st = ctx->store.get();
  std::vector<int32_t> llo(n_blocks + 1);
  llo[0] = 0;
  for (int b = 0; b < n_blocks; ++b) llo[b + 1] = llo[b] + block_rows[b];
  MH_HIP(ctx, st->blk_glo.ensure(n_blocks, ctx->stream));
  MH_HIP(ctx, st->blk_llo.ensure((size_t)n_blocks + 1, ctx->stream));
  MH_HIP(ctx, hipMemcpy(st->blk_glo, block_global_row, sizeof(int32_t) * n_blocks, hipMemcpyHostToDevice));
  MH_HIP(ctx, hipMemcpy(st->blk_llo, llo.data(), sizeof(int32_t) * (n_blocks + 1), hipMemcpyHostToDevice));
  st->n_blocks = n_blocks;
  bind_store(ctx);
  return MH_OK;
}

int mh_db_share(mh_ctx* dst, mh_ctx* src) {
  if (!dst || !src || !src->store) {
    if (dst) dst->err = "mh_db_share: the source context holds no database";
    return MH_ERR_ARG;
  }
  if (dst == src) return MH_OK;
  if (dst->device != src->device) {
    dst->err = "mh_db_share: contexts on different devices";
    return MH_ERR_ARG;
  }
  MH_HIP(dst, hipSetDevice(dst->device));
  if (dst->stream) MH_HIP(dst, hipStreamSynchronize(dst->stream));   // frames of dst still reading its old DB
  if (src->stream) MH_HIP(src, hipStreamSynchronize(src->stream));   // the upload into src has completed (it is synchronous) -- cheap
  dst->store = src->store;
  dst->pool = src->pool;   // (the buffer sets of later edits, and what mh_db_reserve asked the per-model tables for)
  dst->db_models_reserved = src->db_models_reserved;
  bind_store(dst);
  return MH_OK;
}

int mh_db_size(const mh_ctx* ctx, int* N, int* n_models) {
  if (!ctx) return MH_ERR_ARG;
  if (N) *N = ctx->N;
  if (n_models) *n_models = ctx->n_models;
  return MH_OK;
}

int mh_normalize(mh_ctx* ctx, float* desc_host, int n) {
  if (!ctx || n < 0 || (n > 0 && !desc_host)) return MH_ERR_ARG;
  if (n == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ensure_frame_buffers(ctx, n);
  if (rc) return rc;
  const size_t bytes = (size_t)n * DIM * sizeof(float);
  MH_HIP(ctx, hipMemcpyAsync(ctx->q_desc, desc_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  launch_normalize(ctx->q_desc, ctx->q_norm, n, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  MH_HIP(ctx, hipMemcpyAsync(desc_host, ctx->q_desc, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_normalize_dev(mh_ctx* ctx, float* q_dev, float* qnorm_dev, int Q) {
  if (!ctx || Q < 0 || (Q > 0 && (!q_dev || !qnorm_dev))) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  launch_normalize(q_dev, qnorm_dev, Q, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_match_local_dev(mh_ctx* ctx, const float* qn_dev, const float* qnorm_dev, int Q,
                       int32_t* idx1_dev, float* d1_dev, float* d2_dev) {
  if (!ctx || Q < 0 || (Q > 0 && (!qn_dev || !qnorm_dev || !idx1_dev || !d1_dev || !d2_dev)))
    return MH_ERR_ARG;
  if (Q == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ctx_match(ctx, qn_dev, qnorm_dev, Q, idx1_dev, d1_dev, d2_dev);
  if (rc) return rc;
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_match_local_counted_dev(mh_ctx* ctx, const float* qn_dev, const float* qnorm_dev, int Q, const int32_t* q_count_dev,
                               int q_expected, int32_t* idx1_dev, float* d1_dev, float* d2_dev) {
  if (!ctx || Q < 0 || q_expected < 0 || !q_count_dev || (Q > 0 && (!qn_dev || !qnorm_dev || !idx1_dev || !d1_dev || !d2_dev)))
    return MH_ERR_ARG;
  if (Q == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ctx_match(ctx, qn_dev, qnorm_dev, Q, idx1_dev, d1_dev, d2_dev, q_count_dev, q_expected);
  if (rc) return rc;
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_match_merge_dev(mh_ctx* ctx, const int32_t* idx1_s_dev, const float* d1_s_dev,
                       const float* d2_s_dev, int n_shards, int Q, int32_t* idx1_dev,
                       float* d1_dev, float* d2_dev) {
  if (!ctx || Q < 0 || n_shards < 0) return MH_ERR_ARG;
  if (Q == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  launch_match_merge(idx1_s_dev, d1_s_dev, d2_s_dev, n_shards, Q, (size_t)Q, idx1_dev, d1_dev, d2_dev,
                     ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

// MATCH of host descriptors; `normalized_out` != nullptr: the rows are raw, are normalised on the device first and
// come back normalised (what MATCH_ANN_CPU::process does to frameData's descriptors in place, :157) -- one upload
// and one synchronisation for both.
static int match_host(mh_ctx* ctx, const float* q_host, float* normalized_out, int Q, float ratio, int32_t* nn_idx,
                      int32_t* nn_raw, float* d1, float* d2) {
  if (!ctx || Q < 0 || (Q > 0 && (!q_host || !nn_idx))) return MH_ERR_ARG;
  if (Q == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ensure_frame_buffers(ctx, Q);
  if (rc) return rc;
  if ((rc = ensure_match_scratch(ctx, Q))) return rc;
  if ((rc = ensure_pinned(ctx, (size_t)Q * 16))) return rc;
  if ((rc = ensure_scratch(ctx, (size_t)Q * 4))) return rc;
  const size_t bytes = (size_t)Q * DIM * sizeof(float);
  MH_HIP(ctx, hipMemcpyAsync(ctx->q_desc, q_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (normalized_out)
    launch_normalize(ctx->q_desc, ctx->q_norm, Q, ctx->stream);
  else
    launch_row_norms(ctx->q_desc, ctx->q_norm, Q, ctx->stream);
  // (mh_match_set_accept(r > 0): the raw triples are then exact only for the queries r accepts)
  if ((rc = ctx_match(ctx, ctx->q_desc, ctx->q_norm, Q, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, nullptr, 0,
                      ctx->match_accept > 0.f ? ctx->match_accept : 0.f)))
    return rc;
  // the reference's acceptance test on squared distances (MATCH_ANN_CPU.hpp:165)
  int32_t* d_acc = (int32_t*)ctx->scratch.p;
  launch_accept(ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, Q, ratio, d_acc, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  int32_t* h_acc = (int32_t*)ctx->pinned.p;
  int32_t* h_raw = h_acc + Q;
  float* h_d1 = (float*)(h_raw + Q);
  float* h_d2 = h_d1 + Q;
  MH_HIP(ctx, hipMemcpyAsync(h_acc, d_acc, (size_t)Q * 4, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(h_raw, ctx->nn_idx, (size_t)Q * 4, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(h_d1, ctx->nn_d1, (size_t)Q * 4, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(h_d2, ctx->nn_d2, (size_t)Q * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (normalized_out) MH_HIP(ctx, hipMemcpyAsync(normalized_out, ctx->q_desc, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(nn_idx, h_acc, (size_t)Q * 4);
  if (nn_raw) std::memcpy(nn_raw, h_raw, (size_t)Q * 4);
  if (d1) std::memcpy(d1, h_d1, (size_t)Q * 4);
  if (d2) std::memcpy(d2, h_d2, (size_t)Q * 4);
  return MH_OK;
}

int mh_match(mh_ctx* ctx, const float* q_host, int Q, float ratio, int32_t* nn_idx,
             int32_t* nn_raw, float* d1, float* d2) {
  return match_host(ctx, q_host, nullptr, Q, ratio, nn_idx, nn_raw, d1, d2);
}

int mh_normalize_match(mh_ctx* ctx, float* q_host, int Q, float ratio, int32_t* nn_idx, int32_t* nn_raw, float* d1,
                       float* d2) {
  return match_host(ctx, q_host, q_host, Q, ratio, nn_idx, nn_raw, d1, d2);
}

#ifdef MH_TRACE
// experiment builds: the workgroup residency trace (common.h).  on = 1 allocates the ring and points every translation
// unit's kernels at it; mh_trace_fetch copies up to cap records {kernel << 32 | HW_ID, block << 32 | XCC_ID, t0, t1}
// (100 MHz ticks) and rewinds the ring.
static unsigned long long* g_trace_dev = nullptr;
int mh_trace_enable(int on) {
  if (on && !g_trace_dev) {
    if (hipMalloc(&g_trace_dev, (8 + 4 * TRACE_CAP) * sizeof(unsigned long long)) != hipSuccess) return MH_ERR_HIP;
    hipMemset(g_trace_dev, 0, 64);
  }
  unsigned long long* p = on ? g_trace_dev : nullptr;
  const int n = std::min(trace_n_binds().load(), 32);
  for (int i = 0; i < n; ++i) trace_binds()[i](p);
  hipDeviceSynchronize();
  return MH_OK;
}
long long mh_trace_fetch(unsigned long long* out, long long cap) {
  if (!g_trace_dev) return -1;
  hipDeviceSynchronize();
  unsigned long long n = 0;
  hipMemcpy(&n, g_trace_dev, sizeof n, hipMemcpyDeviceToHost);
  const unsigned long long have = std::min<unsigned long long>(n, TRACE_CAP);
  const unsigned long long take = std::min<unsigned long long>(have, (unsigned long long)std::max(cap, 0ll));
  if (take && out) hipMemcpy(out, g_trace_dev + 8, take * 32, hipMemcpyDeviceToHost);
  hipMemset(g_trace_dev, 0, 8);
  return (long long)n;
}
#endif

float mh_screen_margin(float qq, float dmax) { return screen_margin(qq, dmax); }

int mh_screen_reject_proved(float qq, float dmax, float h1, float l2, float tau_q, float ratio) {
  return screen_reject_proved(qq, dmax, h1, l2, tau_q, ratio) ? 1 : 0;
}

uint16_t mh_screen_record_value(float top, float thr) { return screen_record_value(top, thr); }

void mh_screen_record_bounds(uint16_t value_bits, uint32_t row0, float tau, float spread, int N, float dmax, float* lo,
                             float* hi) {
  float l, h;
  screen_record_bounds(value_bits, row0, tau, spread, N, dmax, l, h);
  if (lo) *lo = l;
  if (hi) *hi = h;
}

float mh_screen_pack_value(float v, uint32_t id, int bits) { return screen_pack_value(v, id, bits); }

float mh_screen_pack_pert(float qq, float dmax, int bits) { return screen_pack_pert(qq, dmax, bits); }

void mh_screen_sample_bounds(uint16_t value_bits, float tau, float pert, float dmax, float* lo, float* hi) {
  float l, h;
  screen_sample_bounds(value_bits, tau, pert, dmax, l, h);
  if (lo) *lo = l;
  if (hi) *hi = h;
}

void mh_screen_plan(int Q, int q_expected, int N, int32_t out[MH_SCREEN_PLAN_WORDS]) {
  const ScreenPlan p = screen_plan(Q, q_expected, N);
  static_assert(sizeof p == MH_SCREEN_PLAN_WORDS * sizeof(int32_t), "ScreenPlan is the words mh_screen_plan documents, nothing else");
  memcpy(out, &p, sizeof p);
}

// the 16x16x32 launches' part of the plan (zeros for the others)
void mh_screen_launch_plan(int Q, int q_expected, int N, int32_t out[8]) {
  const ScreenPlan p = screen_plan(Q, q_expected, N);
  const int32_t v[8] = {p.onesweep, p.a_tile_first, p.a_stride, p.a_n_sel, p.a_splits, p.pack_bits, p.b_splits, p.b_n_sel};
  for (int k = 0; k < 8; ++k) out[k] = p.family == 16 ? v[k] : 0;
}

int mh_screen_park_places(void) { return screen_park_places(); }

int mh_match_incomplete(mh_ctx* ctx, uint32_t* count, int reset) {
  if (!ctx || !count) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *count = 0;
  if (ctx->sbuf.inc) {
    unsigned int* c = ctx->sbuf.inc + ctx->sbuf.q_pad;
    MH_HIP(ctx, hipMemcpy(count, c, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (reset) MH_HIP(ctx, hipMemset(c, 0, sizeof(unsigned int)));
  }
  return MH_OK;
}

int mh_screen_values(mh_ctx* ctx, const float* q_host, int Q, int n_rows, float* out_host, float* dmax, float* spread,
                     int shape) {
  if (!ctx || !q_host || !out_host || Q <= 0 || n_rows <= 0 || (Q & 31) || (n_rows & 31)) {
    if (ctx) ctx->err = "mh_screen_values: Q and n_rows must be positive multiples of 32";
    return MH_ERR_ARG;
  }
  if (!ctx->sdb.dbh || n_rows > (ctx->N + 127) / 128 * 128) {
    ctx->err = "mh_screen_values: the database has no f16 image (fewer than 4096 rows?) or fewer rows than asked for";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int q_pad = screen_q_pad(Q);
  hipStream_t s = ctx->stream;
  DevBuf<float> qd, qn, out;
  DevBuf<_Float16> qh;
  DevBuf<uint8_t> qbad;
  int rc = MH_OK;
  if (qd.ensure((size_t)Q * DIM, s) != hipSuccess || qn.ensure(Q, s) != hipSuccess ||
      out.ensure((size_t)Q * n_rows, s) != hipSuccess || qh.ensure((size_t)q_pad * DIM, s) != hipSuccess ||
      qbad.ensure(q_pad, s) != hipSuccess) {
    ctx->err = "mh_screen_values: out of device memory";
    return MH_ERR_HIP;
  }
  hipMemcpyAsync(qd, q_host, (size_t)Q * DIM * 4, hipMemcpyHostToDevice, ctx->stream);
  launch_row_norms(qd, qn, Q, ctx->stream);
  launch_screen_prepare(qd, qn, Q, q_pad, qh, qbad, ctx->stream);
  launch_screen_values(qh, Q, ctx->sdb, n_rows, out, ctx->stream, shape);
  if (hipMemcpyAsync(out_host, out, (size_t)Q * n_rows * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    ctx->err = "mh_screen_values: device error";
    rc = MH_ERR_HIP;
  }
  if (dmax) *dmax = ctx->sdb.dmax;
  if (spread) *spread = ctx->sdb.spread;
  return rc;
}

int mh_screen_sample_values(mh_ctx* ctx, const float* q_host, int Q, const int32_t* row0_host, float* out_host) {
  if (!ctx || !q_host || !row0_host || !out_host || Q <= 0) return MH_ERR_ARG;
  if (!ctx->sdb.dbh) {
    ctx->err = "mh_screen_sample_values: the database has no f16 image (fewer than 4096 rows?)";
    return MH_ERR_ARG;
  }
  const int n_pad = (ctx->N + 127) / 128 * 128;
  for (int i = 0; i < 2 * Q; ++i) {
    const int r = row0_host[i];
    if (r < 0 || (r & 3) || (r & 31) >= 16 || r + 19 >= n_pad) {
      ctx->err = "mh_screen_sample_values: row0 is not the first row of a lane's block (32 b + 4 quarter) inside the padded DB";
      return MH_ERR_ARG;
    }
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  hipStream_t s = ctx->stream;
  DevBuf<float> qd, out;
  DevBuf<int32_t> rd;
  int rc = MH_OK;
  if (qd.ensure((size_t)Q * DIM, s) != hipSuccess || out.ensure((size_t)Q * 16, s) != hipSuccess ||
      rd.ensure((size_t)Q * 2, s) != hipSuccess) {
    ctx->err = "mh_screen_sample_values: out of device memory";
    return MH_ERR_HIP;
  }
  hipMemcpyAsync(qd, q_host, (size_t)Q * DIM * 4, hipMemcpyHostToDevice, ctx->stream);
  hipMemcpyAsync(rd, row0_host, (size_t)Q * 2 * 4, hipMemcpyHostToDevice, ctx->stream);
  launch_screen_sample_values(qd, Q, ctx->sdb, rd, out, ctx->stream);
  if (hipMemcpyAsync(out_host, out, (size_t)Q * 16 * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
    ctx->err = "mh_screen_sample_values: device error";
    rc = MH_ERR_HIP;
  }
  return rc;
}

int mh_match_set_accept(mh_ctx* ctx, float ratio) {
  if (!ctx || !(ratio == ratio) || ratio > 1e30f) return MH_ERR_ARG;
  ctx->match_accept = ratio;
  return MH_OK;
}

int mh_match_prerejected(mh_ctx* ctx, uint32_t* count, int reset) {
  if (!ctx || !count) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *count = 0;
  if (ctx->sbuf.inc) {
    unsigned int* c = ctx->sbuf.inc + ctx->sbuf.q_pad + 1;
    std::vector<unsigned int> h((size_t)screen_prerej_words());
    MH_HIP(ctx, hipMemcpy(h.data(), c, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); k += (size_t)screen_prerej_pitch()) *count += h[k];
    if (reset) MH_HIP(ctx, hipMemset(c, 0, h.size() * sizeof(unsigned int)));
  }
  return MH_OK;
}

int mh_match_set_mode(mh_ctx* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 3) return MH_ERR_ARG;
  ctx->match_mode = mode;
  return MH_OK;
}

int mh_pose_set_split(mh_ctx* ctx, int on) {
  if (!ctx) return MH_ERR_ARG;
  ctx->pose_split = on ? 1 : 0;
  return MH_OK;
}

int mh_match_launches(mh_ctx* ctx, uint32_t out[3]) {
  if (!ctx || !out) return MH_ERR_ARG;
  for (int k = 0; k < 3; ++k) out[k] = ctx->match_launches[k];
  return MH_OK;
}

int mh_match_stats(mh_ctx* ctx, int Q, uint32_t stats[4], int reset) {
  if (!ctx || !stats) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (Q > 0) {
    int rc = ensure_match_scratch(ctx, Q);
    if (rc) return rc;
    stats[3] = (ctx->sdb.usable && ctx->sbuf.q_pad >= screen_q_pad(Q) && screen_wanted(Q, ctx->N, ctx->match_mode >= 2 ? 0 : ctx->match_mode)) ? 1u : 0u;
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->sbuf.stats) {
    std::vector<unsigned int> h((size_t)ctx->sbuf.q_pad * 3);
    MH_HIP(ctx, hipMemcpy(h.data(), ctx->sbuf.stats, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    unsigned long long sum[3] = {0, 0, 0};
    for (size_t i = 0; i < h.size(); ++i) sum[i % 3] += h[i];
    for (int k = 0; k < 3; ++k) stats[k] = (uint32_t)std::min<unsigned long long>(sum[k], 0xFFFFFFFFull);
    if (reset) MH_HIP(ctx, hipMemset(ctx->sbuf.stats, 0, h.size() * sizeof(unsigned int)));
  }
  return MH_OK;
}

int mh_match_query_candidates(mh_ctx* ctx, int Q, uint32_t* out) {
  if (!ctx || !out || Q <= 0) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!ctx->sbuf.stats || Q > ctx->sbuf.q_pad) {
    ctx->err = "mh_match_query_candidates: no two-stage scratch for that many queries";
    return MH_ERR_ARG;
  }
  std::vector<unsigned int> h((size_t)Q * 3);
  MH_HIP(ctx, hipMemcpy(h.data(), ctx->sbuf.stats, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
  for (int q = 0; q < Q; ++q) out[q] = h[3 * (size_t)q];
  return MH_OK;
}

int mh_enable_timing(mh_ctx* ctx, int on) {
  if (!ctx) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  if (on && !ctx->ev_made) {
    for (auto& e : ctx->ev) MH_HIP(ctx, hipEventCreate(&e));
    for (auto& set : ctx->mev)
      for (auto& e : set) MH_HIP(ctx, hipEventCreate(&e));
    ctx->ev_made = true;
  }
  ctx->timing = on != 0;
  ctx->mev_next = ctx->mev_used = 0;
  return MH_OK;
}

int mh_match_timing(mh_ctx* ctx, float ms[5]) {
  if (!ctx || !ms || !ctx->timing || !ctx->ev_made || ctx->mev_used == 0) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = std::min(ctx->mev_used, (int)mh_ctx::MEV_SETS);
  double sum[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < n; ++k) {
    const int set = ((ctx->mev_next - 1 - k) % mh_ctx::MEV_SETS + mh_ctx::MEV_SETS) % mh_ctx::MEV_SETS;
    for (int i = 0; i < 5; ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ctx->mev[set][i], ctx->mev[set][i + 1]) != hipSuccess) return MH_ERR_HIP;
      sum[i] += t;
    }
  }
  for (int i = 0; i < 5; ++i) ms[i] = (float)(sum[i] / n);
  ctx->mev_used = 0;
  return MH_OK;
}

}  // extern "C"
