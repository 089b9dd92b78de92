// The device-resident frame: its buffers (FrameState) and frame_rest, CLUSTER .. FILTER2 behind MATCH.
#include <cstring>
#include <type_traits>

#include "frame.h"
#include "depth_verify.h"
#include "hull.h"

namespace mh {

int ensure_fs(mh_ctx* ctx, int max_m, int max_clusters, int max_objects, int n_models, int n_arenas) {
  FrameState* fs = ctx->fs;
  if (fs && fs->max_m >= max_m && fs->max_clusters >= max_clusters &&
      fs->max_objects >= max_objects && fs->n_models_cap >= n_models && fs->n_arenas >= n_arenas)
    return MH_OK;
  int task_grid = 0, ms_grid = 0;
  DevBuf<unsigned char> kept_result;
  DevBuf<int32_t> kept_snap;
  if (fs) {
    n_arenas = std::max(n_arenas, fs->n_arenas);
    task_grid = fs->task_grid;
    ms_grid = fs->ms_grid;
    max_m = std::max(max_m, fs->max_m);
    max_clusters = std::max(max_clusters, fs->max_clusters);
    max_objects = std::max(max_objects, fs->max_objects);
    n_models = std::max(n_models, fs->n_models_cap);
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (max_objects == fs->max_objects) {   // the result blocks keep their size: frames not fetched yet stay fetchable
      kept_result = std::move(fs->result);
      kept_snap = std::move(fs->snap);
    }
    delete fs;
    ctx->fs = nullptr;
  }
  fs = new FrameState;
  ctx->fs = fs;
  fs->max_m = max_m;
  fs->max_clusters = max_clusters;
  fs->max_objects = max_objects;
  fs->n_models_cap = n_models;
  fs->n_arenas = n_arenas;
  if (task_grid) {   // (what the launches had learnt about the frames' task counts)
    fs->task_grid = task_grid;
    fs->ms_grid = ms_grid;
  }
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  auto also = [&e](hipError_t next) {   // the first failure is the one reported
    if (e == hipSuccess) e = next;
  };
  // two passes over the same list: sizes first (pointers are offsets into a null arena), then the real addresses
  for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
    size_t off = 0;
    unsigned char* const base = fs->arena;
    auto carve = [&](auto*& p, size_t n) {
      typedef typename std::remove_reference<decltype(*p)>::type T;
      p = reinterpret_cast<T*>(base + off);
      off += ((n > 0 ? n : 1) * sizeof(T) + 255) & ~(size_t)255;
    };
    carve(fs->counts, 1);
    carve(fs->n_slots, 1);
    carve(fs->n_clusters, 1);
    carve(fs->n_clusters2, 1);
    carve(fs->tickets, 8);
    carve(fs->acc_q, max_m);
    carve(fs->acc_model, max_m);
    carve(fs->m_q, max_m);
    carve(fs->m_model, max_m);
    carve(fs->m_rep, max_m);
    carve(fs->m_corr, max_m);
    carve(fs->m_depth, max_m);
    carve(fs->m_img, max_m);
    carve(fs->mi_img, max_m);
    carve(fs->mi_corr, max_m);
    carve(fs->off2, (size_t)n_models + 1);
    carve(fs->model_off, (size_t)n_models + 1);
    carve(fs->ms_members, max_m);
    carve(fs->ms_cl_start, (size_t)max_m + n_models + 1);
    carve(fs->ms_ncl, (size_t)n_models + 1);
    carve(fs->cl_model, max_clusters);
    carve(fs->cl_begin, max_clusters);
    carve(fs->cl_count, max_clusters);
    carve(fs->obj_model, max_objects);
    carve(fs->obj_ninl, max_objects);
    carve(fs->obj_cluster, max_objects);
    carve(fs->obj_valid, max_objects);
    carve(fs->obj_npts, max_objects);
    carve(fs->obj_clsize, (size_t)2 * max_objects);
    carve(fs->obj_pose, (size_t)7 * max_objects);
    carve(fs->obj_err, max_objects);
    carve(fs->obj_score, max_objects);
    carve(fs->obj_score_raw, max_objects);
    carve(fs->best, max_m);
    carve(fs->new_members, max_m);
    carve(fs->hyp, max_objects);
    carve(fs->rf_pts, (size_t)9 * max_m);
    carve(fs->rf_list, (size_t)4 * max_m);
    if (pass == 0) {
      fs->arena_bytes = off;
      also(fs->arena.ensure(off * n_arenas, s));
    }
  }
  fs->result_bytes = 16 + sizeof(mh_object) * (size_t)max_objects;
  if (kept_result) {
    fs->result = std::move(kept_result);
    fs->snap = std::move(kept_snap);
  } else {
    also(fs->result.ensure(fs->result_bytes * MH_MAX_BATCH, s));
    if (e == hipSuccess) also(hipMemsetAsync(fs->result, 0, fs->result_bytes * MH_MAX_BATCH, s));   // "0 objects" before the first frame
    also(fs->snap.ensure(4 * MH_MAX_BATCH, s));
    if (e == hipSuccess) also(hipMemsetAsync(fs->snap, 0, sizeof(int32_t) * 4 * MH_MAX_BATCH, s));   // (a slot fetched before it was written reads zeros)
  }
  also(fs->fuse_dev.ensure(2, s));
  also(fs->fb.ensure(3 * MH_MAX_BATCH, s));
  also(fs->fetch_pin.ensure(1, s));
  also(fs->host_block.ensure(1, s));
  if (e != hipSuccess) {   // a half-built state must not look valid to the next call
    delete fs;
    ctx->fs = nullptr;
    ctx->err = std::string("frame buffers: ") + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  std::memset(fs->fb, 0xFF, 3 * MH_MAX_BATCH * sizeof(int32_t));   // -1 = nothing known yet
  std::memset(fs->host_block, 0, sizeof(FrameHostBlock));
  // every frame's tickets, claim table (best), obj_valid / obj_score / obj_npts start at zero
  MH_HIP(ctx, hipMemsetAsync(fs->arena, 0, fs->arena_bytes * n_arenas, ctx->stream));
  fs->host_seq_expect = 0;   // (tickets[7], the device's count of host-block writes, is zero again)
  fs->host_armed = false;
  return MH_OK;
}

FilterBuffers make_fb(const FrameState* fs, int n_models) {
  FilterBuffers fb;
  fb.corr = fs->m_corr;
  fb.m_rep = fs->m_rep;
  fb.m_img = nullptr;
  fb.cams = nullptr;
  fb.n_images = 1;
  fb.model_off = fs->model_off;
  fb.n_models = n_models;
  fb.max_m = fs->max_m;
  fb.obj_model = fs->obj_model;
  fb.obj_pose = fs->obj_pose;
  fb.obj_score = fs->obj_score;
  fb.obj_score_raw = fs->obj_score_raw;
  fb.obj_valid = fs->obj_valid;
  fb.obj_npts = fs->obj_npts;
  fb.max_objects = fs->max_objects;
  fb.best = fs->best;
  fb.obj_clsize = fs->obj_clsize;
  fb.new_members = fs->new_members;
  fb.cl_model = fs->cl_model;
  fb.cl_begin = fs->cl_begin;
  fb.cl_count = fs->cl_count;
  fb.max_clusters = fs->max_clusters;
  return fb;
}

FilterDepthArgs make_filter_depth_args(const mh_ctx* ctx, const DepthImage& dimg, const mh_filter_depth_params& prm,
                                       const mh_cam& depth_cam) {
  FilterDepthArgs a;
  a.pts = ctx->fdepth.pts;
  a.pts_off = ctx->fdepth.off;
  a.img = dimg.img;
  a.fill = dimg.fill;
  a.w = dimg.w;
  a.h = dimg.h;
  a.dcam = make_devcam(depth_cam);
  a.plausible_sq_distance = prm.plausible_sq_distance;
  a.depth_fraction = prm.depth_fraction;
  a.min_keypoint_fraction = prm.min_keypoint_fraction;
  return a;
}

int filter_depth_points_ok(mh_ctx* ctx, const char* who, int n_models) {
  const mh_ctx::FilterDepthState& fd = ctx->fdepth;
  const char* why = nullptr;
  if (fd.n_models <= 0)
    why = "no test points: mh_filter_depth_set_points first";
  else if (fd.db_models != ctx->n_models || fd.db_generation != (ctx->store ? ctx->store->generation : 0))
    why = "the context's database is not the one the test points were set for: mh_filter_depth_set_points again after a DB "
          "edit or upload";
  else if (fd.n_models != n_models)
    why = "the test points are for another number of models: mh_filter_depth_set_points with one slice per model";
  if (!why) return MH_OK;
  ctx->err = std::string(who) + ": depth FILTER: " + why;
  return MH_ERR_ARG;
}

int hulls_frame_ok(mh_ctx* ctx, const char* who, int n_cameras, bool sharded) {
  const mh_ctx::HullState& hs = ctx->hulls;
  if (hs.max_vertices <= 0) return MH_OK;
  const int cams = std::max(n_cameras, ctx->q_img ? ctx->n_images : 1);
  const DbStore* st = ctx->store.get();
  const char* why = nullptr;
  if (sharded)
    why = "frames of a sharded database carry no hulls (model indices are shard-local): mh_frame_set_hulls(ctx, 0, 0) on the "
          "shards, mh_object_hulls on the gathered objects";
  else if (hs.image >= cams)
    why = "the camera whose hulls are wanted is not among the frame's";
  else if (!st || !st->grouped || st->n_blocks > 1)
    why = "the store's rows are not whole models in ascending order (mh_object_hulls has the same condition)";
  if (why) {
    ctx->err = std::string(who) + ": object hulls (mh_frame_set_hulls): " + why;
    return MH_ERR_ARG;
  }
  return MH_OK;
}

int depth_verify_frame_ok(mh_ctx* ctx, const char* who, const mh_frame_params* prm, int n_cameras, bool sharded) {
  if (!ctx->verify.on || !prm || !prm->run_stage2) return MH_OK;
  const DbStore* st = ctx->store.get();
  const char* why = nullptr;
  if (sharded)
    why = "frames of a sharded database cannot take it (model indices are shard-local): mh_frame_set_depth_verify(ctx, NULL, "
          "NULL) on the shards, mh_depth_verify on the gathered objects";
  else if (n_cameras > 1 || (ctx->q_img && ctx->n_images > 1))
    why = "one camera per frame";
  else if (!ctx->depth_img.img)
    why = "no depth map: mh_frame_set_depth_image[_batch | _host] first";
  else if (!st || !st->grouped || st->n_blocks > 1)
    why = "the store's rows are not whole models in ascending order (mh_depth_verify has the same condition)";
  if (why) {
    ctx->err = std::string(who) + ": DEPTH_VERIFY (mh_frame_set_depth_verify): " + why;
    return MH_ERR_ARG;
  }
  return MH_OK;
}

int filter_depth_frame_ok(mh_ctx* ctx, const char* who, const mh_frame_params* prm, int n_cameras, bool sharded) {
  if (int rc = hulls_frame_ok(ctx, who, n_cameras, sharded)) return rc;   // (every frame entry point asks here before it enqueues)
  if (int rc = depth_verify_frame_ok(ctx, who, prm, n_cameras, sharded)) return rc;
  const mh_ctx::FilterDepthState& fd = ctx->fdepth;
  if (!(fd.on[0] || fd.on[1]) || !prm || !prm->run_stage2) return MH_OK;
  const char* why = nullptr;
  if (sharded)
    why = "frames of a sharded database cannot take it (model indices are shard-local, the test points are not): "
          "mh_frame_set_filter_depth(ctx, NULL, NULL, NULL) on the shards, the check on the gathered objects";
  else if (n_cameras > 1 || (ctx->q_img && ctx->n_images > 1))
    why = "one camera per frame: mh_frame_set_images(ctx, NULL, NULL, 0) / one image per frame, or "
          "mh_frame_set_filter_depth(ctx, NULL, NULL, NULL)";
  else if (!ctx->depth_img.img)
    why = "no depth map: mh_frame_set_depth_image[_batch | _host] first";
  if (why) {
    ctx->err = std::string(who) + ": depth FILTER (mh_frame_set_filter_depth): " + why;
    return MH_ERR_ARG;
  }
  return filter_depth_points_ok(ctx, who, ctx->n_models);
}

namespace {

// Result block of a frame that stops after POSE (run_stage2 = 0): the valid objects in
// list order.  Frames with the FILTER stages get it from the last FILTER launch.
__global__ void pack_result_kernel(unsigned char* result, const int32_t* n_slots,
                                   const int32_t* obj_valid, const int32_t* obj_model,
                                   const float* obj_pose, const float* obj_score,
                                   const int32_t* obj_npts, int max_objects, const FrameCounts* counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  mh_object* out = reinterpret_cast<mh_object*>(result + 16);
  int k = 0;
  const int n = *n_slots;
  for (int o = 0; o < n && k < max_objects; ++o) {
    if (!obj_valid[o]) continue;
    mh_object ob;
    ob.model = obj_model[o];
    for (int j = 0; j < 7; ++j) ob.pose[j] = obj_pose[7 * o + j];
    ob.score = obj_score[o];
    ob.n_points = obj_npts[o];
    out[k++] = ob;
  }
  reinterpret_cast<int32_t*>(result)[0] = k;
  reinterpret_cast<int32_t*>(result)[1] = counts->error;   // capacity flags, as the last FILTER launch reports them
}

}  // namespace

int ensure_linkage_scratch(mh_ctx* ctx, size_t floats) {
  if (floats <= ctx->lk_scratch.cap) return MH_OK;
  // 3 n^2 floats per (model, frame) problem: 37 MB per frame at 3 000 matches, 0.6 GB for a batch of 16 -- and it grows
  // with the square of what a caller reserves.  Bounded per context (mh_set_linkage_scratch_limit, default 4 GiB)
  // with an error the caller can act on instead of an allocation that takes the device's memory from the other slots.
  if (floats * sizeof(float) > ctx->lk_scratch_limit) {
    ctx->err = "linkage clusterer: " + std::to_string(floats * sizeof(float) >> 20) + " MiB of similarity-matrix scratch asked for, the "
               "context's limit is " + std::to_string(ctx->lk_scratch_limit >> 20) + " MiB (fewer frames per batch, fewer queries "
               "reserved, or mh_set_linkage_scratch_limit)";
    return MH_ERR_CAPACITY;
  }
  MH_HIP(ctx, ctx->lk_scratch.ensure(floats, ctx->stream));
  return MH_OK;
}

// Device buffers of the depth rules: patch map, per-(model, patch) counts (kept zero), keep flags.
// (frames > 1: a merged batch -- every frame's patch map, counters and keep flags, frame after frame)
static int ensure_rule_buffers(mh_ctx* ctx, int patches, int Q, int frames) {
  mh_ctx::DepthRuleState& rs = ctx->rules;
  if (patches > 4096) {
    ctx->err = "depth rules: more than 4096 patches (raise PatchSize)";
    return MH_ERR_CAPACITY;
  }
  Q *= frames;
  MH_HIP(ctx, rs.inv_size.ensure((size_t)(patches * frames), ctx->stream));
  const size_t need = (size_t)std::max(ctx->n_models, 1) * patches * frames;
  if (need > rs.cnt.cap) {
    MH_HIP(ctx, rs.cnt.ensure(need, ctx->stream));
    MH_HIP(ctx, hipMemsetAsync(rs.cnt, 0, sizeof(int32_t) * need, ctx->stream));
  }
  MH_HIP(ctx, rs.keep1.ensure((size_t)std::max(Q, 0), ctx->stream));
  return MH_OK;
}

void stamp(mh_ctx* ctx, int i) {
  if (ctx->timing) hipEventRecord(ctx->ev[i], ctx->stream);
}

// The hull block and the sort scratch of a frame's hull launch (mh_frame_set_hulls): MH_MAX_BATCH slots of the frame
// state's max_objects records each, scratch for every workgroup of a full batch if a model needs any.  Grows only (the
// stream is waited for then), so frames in a steady state never stop here.
static int ensure_hull_block(mh_ctx* ctx) {
  mh_ctx::HullState& hs = ctx->hulls;
  const FrameState* fs = ctx->fs;
  const size_t slot_bytes = (size_t)fs->max_objects * hull_record_words(hs.max_vertices) * 4;
  if (slot_bytes != hs.slot_bytes || hs.block_vertices != hs.max_vertices) {
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (hulls of earlier frames may still be on their way out of the old layout)
    MH_HIP(ctx, hs.block.ensure(slot_bytes * MH_MAX_BATCH, ctx->stream));
    hs.slot_bytes = slot_bytes;
    hs.block_vertices = hs.max_vertices;
    for (int& v : hs.slot_vertices) v = 0;   // (records of another layout)
  }
  if (hs.scratch_store != ctx->store.get() || hs.scratch_generation != ctx->store->generation) {   // (a new or edited database)
    size_t stride = 0;
    const std::vector<int32_t>& mb = ctx->store->model_begin;
    for (size_t m = 0; m + 1 < mb.size(); ++m) stride = std::max(stride, hull_scratch_points(mb[m + 1] - mb[m]));
    if (stride) MH_HIP(ctx, hs.scratch.ensure(stride * HULL_FRAME_GRID * MH_MAX_BATCH, ctx->stream));
    hs.scratch_store = ctx->store.get();
    hs.scratch_generation = ctx->store->generation;
  }
  return MH_OK;
}

// CLUSTER .. FILTER2 of a device-resident frame in six launches, from the call's record (FrameCall, frame.h) and the
// context's longer-lived state alone.  c.gathered != nullptr: exchange-1 blocks ([n_shards][3][Q]) to merge first.
// c.batch_n > 1: the frames of a batch together, one launch per stage (FrameBatch, steps.h; the caller has checked
// merged_batch_ok) -- q_uv / the top-2 arrays name frame 0's, the slot is 0, c.seeds the frames' seeds.
// c.stage_lo .. c.stage_hi (mh_step_*: the six slots one call each on a frame that stays on the device): only the stages
// 0 MATCH's tail (ratio test + lists), 1 CLUSTER, 2 POSE, 3 FILTER, 4 POSE2, 5 FILTER2 in that range are launched, FILTER
// as launches of its own; everything else of the frame's state is left as the stage before wrote it.
int frame_rest(mh_ctx* ctx, const FrameCall& c) {
  FrameState* fs = ctx->fs;
  const float* const q_uv_dev = c.q_uv;
  const int Q = c.Q, batch_n = c.batch_n, stage_lo = c.stage_lo, stage_hi = c.stage_hi;
  const mh_frame_params* const prm = c.prm;
  const bool stepped = stage_lo != 0 || stage_hi != 5;
  auto runs = [&](int stage) { return stage >= stage_lo && stage <= stage_hi; };
  if (!stepped) ctx->step.done = -1;   // (a whole frame overwrites whatever a stepped frame left in the arrays)
  FrameBatch fb1, fb2;
  const FrameBatch *b1 = nullptr, *b2 = nullptr;
  if (batch_n > 1) {
    fb1.arena = fs->arena_bytes;
    fb1.q = Q;
    fb1.result_bytes = (int)fs->result_bytes;
    fb1.n = batch_n;
    fb2 = fb1;
    for (int f = 0; f < batch_n; ++f) {
      fb1.seed[f] = c.seeds[f];
      fb2.seed[f] = c.seeds[f] ^ 0x5DEECE66Dull;
    }
    b1 = &fb1;
    b2 = &fb2;
  }
  hipStream_t s = ctx->stream;
  const DevCam dc = make_devcam(*c.cam);
  const int nm = ctx->n_models;
  // group_kernel keeps one LDS histogram bin per model: every entry point (fused, sharded, batched)
  // comes through here, so the bound is checked here and not in the callers
  if (nm > MH_MAX_MODELS) {
    ctx->err = "more than 8192 models per context";
    return MH_ERR_CAPACITY;
  }
  unsigned char* const result = fs->result + (size_t)c.slot * fs->result_bytes;
  int32_t* const snap = fs->snap + 4 * c.slot;
  // (mh_frame_fetch_matches_slot: a merged batch leaves every frame's lists in its own arena, a frame on its own in arena 0)
  fs->list_first = c.slot;
  fs->list_n = batch_n > 1 ? batch_n : 1;
  // Every workgroup of the POSE / FILTER launches needs a free compute unit to start even if
  // it has no task, and MATCH kernels of other frames keep all of them busy: launch about as
  // many workgroups as the previous frame had tasks (experiment builds: MH_TASK_GRID pins the number, MH_MS_GRID the
  // CLUSTER launch's -- 0 = one workgroup per model, the old shape).
  static const int grid_env = exp_int("MH_TASK_GRID", 0);
  // POSE / POSE2: one row of workgroups for all frames of the launch, about as many as the launches before found tasks
  // (+ 25%); nothing known yet: the per-frame guess (the last fetched frame's task count) times the frames
  // (what the launches before found in the batch's frames, or `guess` where one of them is not known yet)
  auto found_or = [&](const int32_t* found, long guess) {
    long sum = 0;
    for (int f = 0; f < batch_n; ++f) {
      if (found[f] < 0) return guess;
      sum += found[f];
    }
    return sum;
  };
  auto pose_grid = [&](const int32_t* found) {
    if (grid_env > 0) return grid_env;
    const long sum = found_or(found, (long)fs->task_grid * batch_n / 2);
    return (int)std::min<long>(160, std::max<long>(8, sum + sum / 4 + 2));
  };
  const int grid = pose_grid(fs->fb), grid2 = pose_grid(fs->fb + MH_MAX_BATCH);
  static const int ms_grid_env = exp_int("MH_MS_GRID", -1);
  // CLUSTER: one row of workgroups for all frames of the launch, as many as the launches before found models to cluster
  // (+ 1 per 8); nothing known yet: the per-frame guess times the frames.  Every one of them takes a whole compute unit.
  int ms_grid = fs->ms_grid;
  {
    const long sum = found_or(fs->fb + 2 * MH_MAX_BATCH, (long)std::max(2, fs->ms_grid / 2) * batch_n);
    ms_grid = (int)std::min<long>(48, std::max<long>(batch_n > 1 ? 4 : 2, sum + sum / 8 + 1));
    if (batch_n == 1) ms_grid = std::max(ms_grid, std::min(fs->ms_grid, 8));
  }
  if (ms_grid_env >= 0) ms_grid = ms_grid_env;
  const bool multi = ctx->q_img && ctx->n_images > 1 && ctx->cams_view;
  DepthImage dimg = ctx->depth_img;   // as the setter left it, or with the frame's own map of a batch that has one per frame
  if (c.img) {
    dimg.img = c.img;
    dimg.fill = c.fill;
  }
  // moped3d's depth FILTER in a slot (mh_frame_set_filter_depth): whole frames only -- mh_step_filter stays the plain class
  const bool fdepth = (ctx->fdepth.on[0] || ctx->fdepth.on[1]) && prm->run_stage2 && !stepped;
  if (fdepth)
    if (int rc = filter_depth_frame_ok(ctx, "frame", prm, 1, c.gathered != nullptr)) return rc;
  // object hulls behind the frame's last stage (mh_frame_set_hulls): whole frames only
  const bool hulls = ctx->hulls.max_vertices > 0 && !stepped;
  if (hulls) {
    if (int rc = hulls_frame_ok(ctx, "frame", multi ? ctx->n_images : 1, c.gathered != nullptr)) return rc;
    if (int rc = ensure_hull_block(ctx)) return rc;
  }
  // moped3d's DEPTH_VERIFY behind FILTER2 (mh_frame_set_depth_verify): whole frames only
  const bool verify = ctx->verify.on && prm->run_stage2 && !stepped;
  if (verify) {
    if (int rc = depth_verify_frame_ok(ctx, "frame", prm, multi ? ctx->n_images : 1, c.gathered != nullptr)) return rc;
    mh_ctx::VerifyState& vs = ctx->verify;
    const size_t slot_bytes = 16 + (size_t)fs->max_objects * sizeof(mh_verify_record);
    if (slot_bytes != vs.slot_bytes || !vs.tickets) {
      MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (records of earlier frames may still be read out of the old layout)
      MH_HIP(ctx, vs.block.ensure(slot_bytes * MH_MAX_BATCH, ctx->stream));
      if (!vs.tickets) {
        MH_HIP(ctx, vs.tickets.ensure(MH_MAX_BATCH, ctx->stream));
        MH_HIP(ctx, hipMemsetAsync(vs.tickets, 0, MH_MAX_BATCH * sizeof(unsigned int), ctx->stream));
      }
      vs.slot_bytes = slot_bytes;
      for (bool& v : vs.slot_on) v = false;
    }
  }
  // moped3d's weighted mean shift (mh_frame_set_cluster_wms): whole single-camera frames of this context over a depth map
  if (ctx->wms_on) {
    const char* why = !dimg.img ? "no depth map (mh_frame_set_depth_image)" : multi ? "frames with several images" :
                      c.gathered ? "the sharded entry points" : stepped ? "stepped frames" : nullptr;
    if (why) {
      ctx->err = std::string("frame: the weighted mean-shift clusterer does not take ") + why;
      return MH_ERR_ARG;
    }
    if (int rc = ensure_wms_buffers(ctx)) return rc;
  }
  if (multi && (ctx->q_depth || dimg.img || ctx->linkage_on)) {
    ctx->err = "frames with several images: the moped3d depth steps are single-camera";
    return MH_ERR_ARG;
  }
  // a merged batch with a depth map per frame (mh_frame_set_depth_image_batch; merged_batch_ok has checked the count)
  DepthMaps dmaps;
  const DepthMaps* maps = nullptr;
  if (batch_n > 1 && dimg.img) {
    for (int f = 0; f < batch_n; ++f) {
      dmaps.img[f] = ctx->batch_img[f];
      dmaps.fill[f] = ctx->batch_fill[f];
    }
    maps = &dmaps;
  }
  // moped3d depth rules: patch maps of this frame's depth image, DEPTHFILTER on the features
  DepthRules rules;
  if (runs(0)) {
    ctx->rules.last = mh_ctx::DepthRuleState::Last();
    ctx->rules.last.depth = ctx->q_depth || dimg.img;   // group_kernel fills m_depth
  }
  if (ctx->rules.on && dimg.img && runs(0)) {
    mh_ctx::DepthRuleState& rs = ctx->rules;
    const int pw = (dimg.w + rs.patch - 1) / rs.patch, ph = (dimg.h + rs.patch - 1) / rs.patch;
    int rc = ensure_rule_buffers(ctx, pw * ph, Q, batch_n);
    if (rc) return rc;
    const bool filters = rs.feature_filter >= 0.f || rs.match_filter >= 0.f;
    rs.last.patches = pw * ph;
    rs.last.q = Q;
    rs.last.first = c.slot;
    rs.last.frames = std::max(1, batch_n);
    rs.last.inv = filters;
    rs.last.keep = rs.feature_filter >= 0.f;
    if (filters) launch_depth_patches(dimg, rs.K, rs.patch, rs.inv_size, s, maps, batch_n);
    if (rs.feature_filter >= 0.f) {
      launch_feature_density(q_uv_dev, Q, c.q_count, rs.patch, pw, ph, rs.inv_size, rs.feature_filter,
                             rs.keep1, s, batch_n);
      rules.keep1 = rs.keep1;
    }
    if (rs.match_filter >= 0.f) {
      rules.inv_size = rs.inv_size;
      rules.cnt = rs.cnt;
      rules.filter2 = rs.match_filter;
    }
    rules.patch = rs.patch;
    rules.pw = pw;
    rules.ph = ph;
    if (rs.ratio_table && rs.table_models >= nm) rules.ratio_table = reinterpret_cast<const float4*>(rs.ratio_table.p);
    rules.max_depth = rs.max_depth;
    rules.default_depth = rs.default_depth;
    rules.cauchy_scale = rs.cauchy_scale;
  }
  // MATCH tail: (shard merge,) ratio test + per-model lists; resets the frame's counters
  const int q0 = c.q0;   // frame of a batch matched in one launch: its slice of the top-2 arrays
  if (runs(0))
  launch_group(c.gathered, c.n_shards, ctx->nn_idx + q0, ctx->nn_d1 + q0, ctx->nn_d2 + q0, Q, prm->ratio, q_uv_dev,
               ctx->db_model, ctx->db_xyz, ctx->N, ctx->rmap, nm, fs->max_m, fs->acc_q,
               fs->acc_model, fs->m_q, fs->m_model, fs->m_corr, fs->m_rep, fs->model_off,
               ctx->q_depth ? ctx->q_depth + q0 : nullptr,   // (a batch's depth attributes lie frame after frame like its queries)
               fs->m_depth, dimg, fs->counts, fs->n_slots, fs->best, s, rules, c.shard_stride, c.plane_stride, b1,
               c.slot == 0 ? ctx->exchange_tags : nullptr, maps);
  stamp(ctx, 2);
  // CLUSTER (+ flat cluster table, snap[0..1])
  const bool have_depth = ctx->q_depth || dimg.img;
  if (runs(1)) fs->list_pairs = multi ? ctx->n_images : 1;   // (several images: MeanShift only, see above)
  if (runs(1)) fs->list_wms = ctx->wms_on;
  if (!runs(1)) {
  } else if (ctx->wms_on) {
    // (frame after frame: merged_batch_ok is false in this mode)
    launch_wms_models(fs->m_corr, reinterpret_cast<const float*>(fs->m_depth), fs->model_off, nm, fs->max_m, dimg, ctx->wms,
                      ctx->wms_state.p, ctx->wms_members.p, WMS_MEMBER_FACTOR, fs->ms_cl_start, fs->ms_ncl, fs->max_clusters,
                      fs->cl_model, fs->cl_begin, fs->cl_count, fs->n_clusters, snap, fs->counts, fs->tickets + 0, s);
  } else if (ctx->linkage_on && have_depth && dimg.img) {
    // moped3d: linkage over similarity matrices; 3 n^2 floats of scratch per model, n <= LK_CAP (MH_LINKAGE_ROWMAX: LK_MAX)
    // (a merged batch: every frame its own region)
    const bool rowmax = ctx->lk_mode == MH_LINKAGE_ROWMAX;
    const size_t need = 3 * (size_t)std::min(fs->max_m, rowmax ? LK_MAX : LK_CAP) * (size_t)fs->max_m;
    const size_t frames = (size_t)std::max(1, batch_n);
    // (ROWMAX: the plan, the headers and the per-point arrays of the matrix stage behind the frames' regions)
    const size_t aux_floats = rowmax ? (linkage_rowmax_aux_bytes((size_t)nm * frames, (size_t)fs->max_m * frames) + 3) / 4 + 16 : 0;
    int rc = ensure_linkage_scratch(ctx, need * frames + aux_floats);
    if (rc) return rc;
    if (rowmax) {
      if (!ctx->lk_stats) {
        MH_HIP(ctx, ctx->lk_stats.ensure(4, s));
        MH_HIP(ctx, hipMemsetAsync(ctx->lk_stats, 0, 4 * sizeof(unsigned long long), s));
      }
      // (the frames' regions first, `need` floats each; a frame alone has all that is left before the aux block)
      const size_t region = batch_n > 1 ? need : ctx->lk_scratch.cap - aux_floats;
      unsigned char* aux = reinterpret_cast<unsigned char*>(ctx->lk_scratch.p + ((ctx->lk_scratch.cap - aux_floats + 15) & ~(size_t)15));
      launch_linkage_rowmax_models(fs->m_corr, reinterpret_cast<const float*>(fs->m_depth), fs->model_off, nm, fs->max_m, dimg,
                                   ctx->linkage, ctx->lk_scratch, region, fs->ms_members, fs->ms_cl_start, fs->ms_ncl,
                                   fs->max_clusters, fs->cl_model, fs->cl_begin, fs->cl_count, fs->n_clusters, snap,
                                   fs->counts, fs->tickets + 0, s, ms_grid, b1, maps, fs->fb + 2 * MH_MAX_BATCH, aux,
                                   ctx->lk_stats);
    } else
    launch_linkage_models(fs->m_corr, reinterpret_cast<const float*>(fs->m_depth), fs->model_off, nm, dimg,
                          ctx->linkage, ctx->lk_scratch, batch_n > 1 ? need : ctx->lk_scratch.cap, fs->ms_members,
                          fs->ms_cl_start, fs->ms_ncl, fs->max_clusters, fs->cl_model, fs->cl_begin, fs->cl_count,
                          fs->n_clusters, snap, fs->counts, fs->tickets + 0, s, ms_grid, b1, maps,
                          fs->fb + 2 * MH_MAX_BATCH);
  } else if (multi) {
    // MeanShift per (model, image) in image order (CLUSTER_MEAN_SHIFT_CPU.hpp:189-195)
    launch_image_split(fs->m_corr, fs->m_q, fs->m_model, fs->model_off, nm, ctx->q_img + (size_t)c.frame * Q, ctx->n_images, fs->counts,
                       fs->m_img, fs->m_rep, fs->mi_corr, fs->mi_img, fs->off2, s);
    launch_meanshift_models(fs->mi_corr, fs->off2, nm * ctx->n_images, prm->ms_radius, prm->ms_merge,
                            prm->ms_min_pts, prm->ms_max_iter, fs->ms_members, fs->ms_cl_start,
                            fs->ms_ncl, fs->max_clusters, fs->cl_model, fs->cl_begin, fs->cl_count,
                            fs->n_clusters, snap, fs->counts, fs->tickets + 0, s, ctx->n_images, ms_grid);
  } else
  launch_meanshift_models(fs->m_corr, fs->model_off, nm, prm->ms_radius, prm->ms_merge,
                          prm->ms_min_pts, prm->ms_max_iter, fs->ms_members, fs->ms_cl_start,
                          fs->ms_ncl, fs->max_clusters, fs->cl_model, fs->cl_begin, fs->cl_count,
                          fs->n_clusters, snap, fs->counts, fs->tickets + 0, s, 1, ms_grid, b1, fs->fb + 2 * MH_MAX_BATCH);
  stamp(ctx, 3);
  PoseImages img1, img2;   // POSE works on the (model, image, query) copy, POSE2 on FILTER's clusters over the match lists
  if (multi) {
    img1.cams = img2.cams = ctx->cams_view;
    img1.n_images = img2.n_images = ctx->n_images;
    img1.img_of = fs->mi_img;
    img2.img_of = fs->m_img;
  }
  // POSE (+ slot count, snap[2] = objects after POSE).  With the FILTER stages on, each FILTER runs in the tail of
  // the POSE launch before it (its last workgroup: filter_dev.h) -- four launches per frame instead of six; a
  // dependent launch costs the pipeline ~5% of its throughput whatever is in it (MH_FUSE_FILTER=0: launches of
  // their own, the same objects).
  static const bool fuse_filter = exp_int("MH_FUSE_FILTER", 1) != 0;
  const float* depth4 = (ctx->q_depth || dimg.img) ? reinterpret_cast<const float*>(fs->m_depth) : nullptr;
  FilterBuffers fb = make_fb(fs, nm);
  if (multi) {
    fb.m_img = fs->m_img;
    fb.cams = ctx->cams_view;
    fb.n_images = ctx->n_images;
  }
  // (stage timing wants the steps apart; the depth class's fused F1 lives in the kernels of POSE's two launches only)
  const bool fdepth_fusable = !fdepth || (ctx->pose_split && pose_launch_splits(prm->pose1) && pose_launch_splits(prm->pose2));
  const bool fused = fuse_filter && prm->run_stage2 && !ctx->timing && !stepped && fdepth_fusable;
  // the depth class of a slot: a launch of its own (fda), or -- fused -- FilterFuseDepth behind the slot's fused
  // arguments, with the map of every frame of a merged batch
  FilterDepthArgs fda[2];
  FilterFuseDepth ffd[2];
  for (int k = 0; fdepth && k < 2; ++k) {
    if (!ctx->fdepth.on[k]) continue;
    fda[k] = make_filter_depth_args(ctx, dimg, ctx->fdepth.prm[k], ctx->fdepth.cam);
    ffd[k].on = 1;
    ffd[k].args = fda[k];
    ffd[k].args.img = nullptr;   // (the frames' maps are in the table)
    ffd[k].args.fill = nullptr;
    if (maps)
      ffd[k].maps = *maps;
    else {
      ffd[k].maps.img[0] = dimg.img;
      ffd[k].maps.fill[0] = dimg.fill;
    }
  }
  // (mh_frame_route)
  ctx->frame_route[0] = batch_n > 1 ? batch_n : 1;
  ctx->frame_route[1] = batch_n > 1;
  ctx->frame_route[2] = fused;
  ctx->frame_route[3] = fdepth ? (ctx->fdepth.on[0] ? 1 : 0) | (ctx->fdepth.on[1] ? 2 : 0) : 0;
  // (one frame alone in result slot 0: FILTER2's tail also writes the host's block, mh_frame_fetch reads it without a copy)
  // (not with DEPTH_VERIFY behind it: the erase rewrites the result slot, and the fetch copies from there)
  fs->host_armed = batch_n == 1 && c.slot == 0 && prm->run_stage2 && fs->host_block && !stepped && !verify;
  if (fs->host_armed) ++fs->host_seq_expect;
  const FilterTail ft1{fs->tickets + 2, snap + 3, nullptr, grid, nullptr, nullptr, nullptr},
      ft2{fs->tickets + 4, nullptr, result, grid, fs->host_armed ? fs->host_block : nullptr, fs->host_armed ? snap : nullptr,
          fs->host_armed ? fs->tickets + 7 : nullptr};
  FilterFuse ff1, ff2;
  ff1.fb = ff2.fb = &fb;
  ff1.tail = &ft1;
  ff2.tail = &ft2;
  ff1.n_clusters_dev = fs->n_clusters2;   // FILTER writes POSE2's cluster count, FILTER2 the frame's final one
  ff2.n_clusters_dev = fs->n_clusters;
  ff1.dev = fs->fuse_dev;
  ff1.shadow = &fs->fuse_shadow[0];
  ff1.shadow_valid = &fs->fuse_valid[0];
  ff2.dev = fs->fuse_dev + 1;
  ff2.shadow = &fs->fuse_shadow[1];
  ff2.shadow_valid = &fs->fuse_valid[1];
  ff1.min_points = prm->f1_min_points;
  ff1.feature_distance = prm->f1_feature_distance;
  ff1.min_score = prm->f1_min_score;
  ff2.min_points = prm->f2_min_points;
  ff2.feature_distance = prm->f2_feature_distance;
  ff2.min_score = prm->f2_min_score;
  if (fdepth && ctx->fdepth.on[0]) ff1.depth = &ffd[0];
  if (fdepth && ctx->fdepth.on[1]) ff2.depth = &ffd[1];
  PoseSplit split;
  split.hyp = (fused && ctx->pose_split) ? fs->hyp : nullptr;   // (the refine launch closes the frames through the fused FILTER tail)
  split.pts = fs->rf_pts;
  split.list = fs->rf_list;
  split.max_m = fs->max_m;
  if (runs(2))
  launch_pose(multi ? fs->mi_corr : fs->m_corr, depth4, ctx->depth_kind, ctx->depth_alpha,
              ctx->wms_on ? ctx->wms_members.p : fs->ms_members, fs->cl_model,
              fs->cl_begin, fs->cl_count, fs->n_clusters, fs->max_clusters, dc, prm->pose1, c.seed, fs->n_slots,
              fs->max_objects, fs->obj_model, fs->obj_pose, fs->obj_ninl, fs->obj_err, fs->obj_cluster,
              fs->obj_valid, fs->counts, PoseTail{fs->tickets + 1, fs->n_slots, snap + 2, grid, fs->fb}, s, img1,
              fused ? &ff1 : nullptr, b1, &split);
  stamp(ctx, 4);
  if (prm->run_stage2) {
    // FILTER (snap[3] = objects kept)
    if (!fused && runs(3) && fdepth && ctx->fdepth.on[0])
      launch_filter_depth(fb, dc, prm->f1_min_points, prm->f1_feature_distance, prm->f1_min_score, fda[0],
                          fs->n_slots, fs->n_clusters2, fs->counts, ft1, s);
    else if (!fused && runs(3))
      launch_filter(fb, dc, prm->f1_min_points, prm->f1_feature_distance, prm->f1_min_score,
                    fs->n_slots, fs->n_clusters2, fs->counts, ft1, s);
    stamp(ctx, 5);
    // POSE2 on the rewritten clusters, objects appended after the kept ones
    if (runs(4))
    launch_pose(fs->m_corr, depth4, ctx->depth_kind, ctx->depth_alpha, fs->new_members, fs->cl_model,
                fs->cl_begin, fs->cl_count, fs->n_clusters2, fs->max_clusters, dc, prm->pose2,
                c.seed ^ 0x5DEECE66Dull, fs->n_slots, fs->max_objects, fs->obj_model, fs->obj_pose,
                fs->obj_ninl, fs->obj_err, fs->obj_cluster, fs->obj_valid, fs->counts,
                PoseTail{fs->tickets + 3, fs->n_slots, nullptr, grid2, fs->fb + MH_MAX_BATCH}, s, img2, fused ? &ff2 : nullptr, b2,
                &split);
    stamp(ctx, 6);
    // FILTER2 (+ the frame's result block)
    if (!fused && runs(5) && fdepth && ctx->fdepth.on[1])
      launch_filter_depth(fb, dc, prm->f2_min_points, prm->f2_feature_distance, prm->f2_min_score, fda[1],
                          fs->n_slots, fs->n_clusters, fs->counts, ft2, s);
    else if (!fused && runs(5))
      launch_filter(fb, dc, prm->f2_min_points, prm->f2_feature_distance, prm->f2_min_score,
                    fs->n_slots, fs->n_clusters, fs->counts, ft2, s);
    stamp(ctx, 7);
  } else {
    for (int i = 5; i <= 7; ++i) stamp(ctx, i);
    hipLaunchKernelGGL(pack_result_kernel, dim3(1), dim3(1), 0, s, result, fs->n_slots,
                       fs->obj_valid, fs->obj_model, fs->obj_pose, fs->obj_score, fs->obj_npts,
                       fs->max_objects, fs->counts);
  }
  stamp(ctx, 8);
  // DEPTH_VERIFY of the objects the result slots now hold, in front of the hulls: one launch for all frames of the call,
  // the counts read on the device; the frames' last workgroups erase
  if (!stepped || runs(2))
    for (int f = 0; f < (batch_n > 1 ? batch_n : 1) && c.slot + f < MH_MAX_BATCH; ++f) ctx->verify.slot_on[c.slot + f] = false;
  if (verify) {
    mh_ctx::VerifyState& vs = ctx->verify;
    DepthVerifyFrameArgs va;
    va.core.xyz = ctx->db_xyz;
    va.core.model_begin = ctx->store->model_begin_dev;
    va.core.img = dimg.img;
    va.core.fill = dimg.fill;
    va.core.w = dimg.w;
    va.core.h = dimg.h;
    va.core.cam = dc;
    va.core.dcam = make_devcam(vs.cam);
    va.core.feature_distance = vs.prm.feature_distance;
    va.core.max_multiplier = vs.prm.max_multiplier;
    va.core.max_distance = vs.prm.max_distance;
    va.core.depth_fraction = vs.prm.depth_fraction;
    va.maps_on = maps != nullptr;
    if (maps) va.maps = *maps;
    va.corr = fs->m_corr;
    va.model_off = fs->model_off;
    va.arena_bytes = fs->arena_bytes;
    va.result = fs->result;
    va.result_bytes = fs->result_bytes;
    va.max_objects = fs->max_objects;
    va.first_slot = c.slot;
    va.block = vs.block;
    va.slot_bytes = vs.slot_bytes;
    va.tickets = vs.tickets;
    launch_frame_depth_verify(va, batch_n > 1 ? batch_n : 1, s);
    for (int f = 0; f < (batch_n > 1 ? batch_n : 1) && c.slot + f < MH_MAX_BATCH; ++f) vs.slot_on[c.slot + f] = true;
  }
  // the hulls of the objects the result slots now hold: one launch for all frames of the call, the counts read on the device
  if (!stepped || runs(2))
    for (int f = 0; f < (batch_n > 1 ? batch_n : 1) && c.slot + f < MH_MAX_BATCH; ++f) ctx->hulls.slot_vertices[c.slot + f] = 0;
  if (hulls) {
    mh_ctx::HullState& hs = ctx->hulls;
    HullFrameArgs ha;
    ha.core.xyz = ctx->db_xyz;
    ha.core.model_begin = ctx->store->model_begin_dev;
    ha.core.n_models = ctx->store->n_models;
    ha.core.cam = dc;
    ha.core.max_vertices = hs.max_vertices;
    ha.core.form = 0;   // (frames ignore mh_hull_debug_form)
    ha.core.scratch = hs.scratch;
    ha.core.scratch_stride = hs.scratch ? hs.scratch.cap / ((size_t)HULL_FRAME_GRID * MH_MAX_BATCH) : 0;
    ha.cams = multi ? ctx->cams_view : nullptr;
    ha.image = hs.image;
    ha.result = fs->result;
    ha.result_bytes = fs->result_bytes;
    ha.max_objects = fs->max_objects;
    ha.first_slot = c.slot;
    ha.block = hs.block;
    ha.slot_bytes = hs.slot_bytes;
    launch_frame_hulls(ha, batch_n > 1 ? batch_n : 1, s);
    for (int f = 0; f < (batch_n > 1 ? batch_n : 1) && c.slot + f < MH_MAX_BATCH; ++f) hs.slot_vertices[c.slot + f] = hs.max_vertices;
  }
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

// The frames of a batch can share their launches when nothing of the frame is per-context state: one image, no depth
// map / rules / linkage unless every frame brings its own map (below), the fused FILTER tails (the stand-alone FILTER and
// result-packing kernels are per frame), no stage timing, no graph replay.  MH_MERGE_BATCH=0: frame after frame.
// Per-query depth ATTRIBUTES (mh_frame_set_depth: B Q entries, frame after frame like the queries) travel with a merged
// batch where the caller says so (`attrs_ok`: mh_frame_enqueue_batch) -- group_kernel takes frame f's slice, the per-frame
// arenas hold every frame's m_depth, pose_kernel<1 | 2> shifts its pointers like pose_kernel<0>.
// A depth MAP per frame (mh_frame_set_depth_image_batch with as many maps as the batch has frames: `maps_for`), the depth
// rules and the linkage clusterer travel with it too (round 4): depth_patch / feature_density / group / linkage_models
// take frame f's map from a DepthMaps table and its rule buffers behind those of the frames before it.
// The depth FILTER (mh_frame_set_filter_depth) travels with the maps: the fused POSE tails score every object against its
// own frame's map (FilterFuseDepth, steps.h).
int ensure_wms_buffers(mh_ctx* ctx) {
  const FrameState* fs = ctx->fs;
  MH_HIP(ctx, ctx->wms_members.ensure((size_t)WMS_MEMBER_FACTOR * std::max(fs->max_m, 1), ctx->stream));
  MH_HIP(ctx, ctx->wms_state.ensure(wms_state_bytes((size_t)std::max(fs->n_models_cap, 1), (size_t)std::max(fs->max_m, 1)), ctx->stream));
  return MH_OK;
}

bool merged_batch_ok(const mh_ctx* ctx, const mh_frame_params* prm, bool attrs_ok, int maps_for) {
  if (ctx->wms_on) return false;   // the members' buffer is the context's: a batch runs frame by frame
  static const bool on = exp_int("MH_MERGE_BATCH", 1) != 0;
  static const bool fuse_filter = exp_int("MH_FUSE_FILTER", 1) != 0;
  static const bool merge_maps = exp_int("MH_MERGE_MAPS", 1) != 0;
  const bool maps_ok = merge_maps && attrs_ok && maps_for > 1 && ctx->batch_imgs == maps_for && ctx->depth_img.img;
  // the depth FILTER: a map per frame, and the fused route (frame_rest: POSE's two launches)
  if ((ctx->fdepth.on[0] || ctx->fdepth.on[1]) && prm->run_stage2 &&
      !(maps_ok && ctx->pose_split && pose_launch_splits(prm->pose1) && pose_launch_splits(prm->pose2)))
    return false;
  return on && fuse_filter && prm->run_stage2 && !ctx->timing && (attrs_ok || !ctx->q_depth) &&
         (maps_ok || (!ctx->depth_img.img && !ctx->rules.on && !ctx->linkage_on)) && !(ctx->q_img && ctx->n_images > 1);
}

int ensure_batch_arenas(mh_ctx* ctx, int B) {
  FrameState* fs = ctx->fs;
  if (fs->n_arenas >= B) return MH_OK;   // (the usual case; the first batch pays one reallocation)
  return ensure_fs(ctx, fs->max_m, fs->max_clusters, fs->max_objects, fs->n_models_cap, B);
}

// Buffers for a launch of Q queries = `frames` frames of q_frame queries each (0: one frame of Q): the MATCH side for
// all of them, the working arrays of the rest chain per frame (a frame has at most as many matches as queries) with
// `frames` copies, so that a merged batch never reallocates behind work that is already enqueued.
int prepare_frame(mh_ctx* ctx, int Q, int q_frame, int frames) {
  int rc = ensure_frame_buffers(ctx, Q);
  if (rc) return rc;
  if ((rc = ensure_match_scratch(ctx, Q))) return rc;
  const int want_m = ctx->fs ? ctx->fs->max_m : 0;
  const int mc = ctx->fs ? ctx->fs->max_clusters : 1024;
  const int mo = ctx->fs ? ctx->fs->max_objects : 4096;
  // (several images: CLUSTER's per-"model" tables hold one entry per (model, image) pair)
  return ensure_fs(ctx, std::max(want_m, q_frame > 0 ? q_frame : Q), mc, mo,
                   ctx->n_models * (ctx->n_images > 1 ? ctx->n_images : 1), frames);
}
}  // namespace mh

extern "C" void mh_free_frame_state(mh_ctx* ctx) {
  delete ctx->fs;
  ctx->fs = nullptr;
}
