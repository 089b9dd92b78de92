// C ABI: the device-resident frame's entry points -- reserve, the setters, enqueue (features, images, batches, the sharded
// rest chain), fetch and delivery.
#include <climits>
#include <cstring>

#include "frame.h"
#include "hull.h"

using namespace mh;

namespace {

// mh_ctx::ImagesFrame::words, [3][MH_MAX_BATCH]: FEAT's count per image first.  A batch keeps its frames' totals in the
// second row and its images' clamped counts in the third; a frame alone keeps its total at the head of the third row and
// its images' clamped counts right behind it, so that mh_frame_fetch reads them with one copy.
static_assert(1 + MH_MAX_IMAGES <= MH_MAX_BATCH, "a frame's total and counts fit one row of the words");
inline int32_t* images_single_total(const mh_ctx* ctx) { return ctx->imf.words ? ctx->imf.words + 2 * MH_MAX_BATCH : nullptr; }

// mh_frame_enqueue_image_batch: the B images' keypoints lie at a fixed stride of Q rows; rows past an image's count
// become zero rows with a norm term of -1 before MATCH -- "no such query" to the two-stage search (a plain zero query is
// its worst case: every row of a normalised DB ties, the candidate lists overflow and the query falls back to brute
// force), a finite dummy to the exact kernels ...
__global__ void image_batch_tail_kernel(float* __restrict__ desc, float* __restrict__ norm, const int32_t* __restrict__ counts,
                                        int Q, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // one 16-byte piece of a row
  if (i >= B * Q * (DIM / 4)) return;
  const int row = i / (DIM / 4), f = row / Q, q = row - f * Q;
  if (q < min(counts[f], Q)) return;
  reinterpret_cast<float4*>(desc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i % (DIM / 4) == 0) norm[row] = -1.f;
}
// ... and "no neighbour" after it, so that no step of the frame sees them
__global__ void image_batch_mask_kernel(int32_t* __restrict__ idx, float* __restrict__ d1, float* __restrict__ d2,
                                        const int32_t* __restrict__ counts, int Q, int B) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B * Q) return;
  const int f = row / Q, q = row - f * Q;
  if (q < min(counts[f], Q)) return;
  idx[row] = -1;
  d1[row] = __builtin_inff();
  d2[row] = __builtin_inff();
}

// mh_frame_fetch_batch_async: frame f's head {n, flags, counts[4], tag, f} + its first min(n, max_objects) objects out of
// result slot f into record f of the caller's block (dst: device-visible host memory, or the staging buffer).
__global__ void __launch_bounds__(128) deliver_kernel(const unsigned char* __restrict__ result, size_t result_bytes,
                                                      const int32_t* __restrict__ snap, unsigned char* __restrict__ dst,
                                                      int max_objects, int result_objects, uint32_t tag) {
  const int f = blockIdx.x;
  const int32_t* src = reinterpret_cast<const int32_t*>(result + (size_t)f * result_bytes);
  int32_t* out = reinterpret_cast<int32_t*>(dst + (size_t)f * (sizeof(mh_frame_head) + sizeof(mh_object) * (size_t)max_objects));
  const int n = src[0];
  const int take = max(0, min(n, min(max_objects, result_objects)));
  const int t = threadIdx.x;
  if (t < 8) {
    int32_t w;
    if (t == 0) w = n;
    else if (t == 1) w = src[1];
    else if (t < 6) w = snap[4 * f + t - 2];
    else if (t == 6) w = (int32_t)tag;
    else w = f;
    out[t] = w;
  }
  constexpr int OW = (int)(sizeof(mh_object) / 4);
  for (int w = t; w < take * OW; w += blockDim.x) out[8 + w] = src[4 + w];
  __threadfence_system();
}

// a fetched frame's error flags: into ctx->err and the return code
int frame_flags(mh_ctx* ctx, int32_t flags) {
  if (!flags) return MH_OK;
  ctx->err = (flags & ERR_EXCHANGE)
                 ? std::string("frame exchange: the ranks' blocks carry different sequence numbers / seeds -- the ranks issued "
                               "their collectives in different orders (every rank must enqueue its slots in the same order)")
                 : "frame: capacity exceeded (flags " + std::to_string(flags) + ")";
  return MH_ERR_CAPACITY;
}

// One frame's result as its caller sees it, from what a fetch brought to the host: head = {n, ..} and snap = the four
// counters, flags = the frame's error flags, first = the n_first objects that came with the head; a longer list's tail is
// copied from the result block on the device.  Also the feedback for the next launches' grids.
int read_out(mh_ctx* ctx, const int32_t* head, const int32_t* snap, int32_t flags, const mh_object* first, int n_first,
             const unsigned char* result_dev, mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts) {
  FrameState* fs = ctx->fs;
  const int n = head[0];
  *n_objects = n;
  if (counts) std::memcpy(counts, snap, 4 * sizeof(int32_t));
  // clusters x 4 replicas (POSE), kept objects x 4 (POSE2), + 50 % head room, in steps of 8
  const int tasks = 4 * std::max(snap[1], snap[3]);
  fs->task_grid = std::min(96, std::max(16, (tasks + tasks / 2 + 7) / 8 * 8));
  fs->ms_grid = std::min(32, std::max(4, snap[1] + 2));   // (a model with matches and no cluster still takes a turn: the workgroups loop)
  const int take = n < max_objects ? n : max_objects;
  if (take > 0 && objects_host) {
    const int have = std::min(take, n_first);
    std::memcpy(objects_host, first, sizeof(mh_object) * (size_t)have);
    if (take > have)
      MH_HIP(ctx, hipMemcpy(objects_host + have, result_dev + 16 + sizeof(mh_object) * (size_t)have,
                            sizeof(mh_object) * (size_t)(take - have), hipMemcpyDeviceToHost));
  }
  return frame_flags(ctx, flags);
}

// mh_frame_fetch_match*: the match count of result slot `slot` (-1: the last frame's) and where its lists lie --
// *arena: the byte offset of the slot's copy of the working arrays, *take: the entries the caller's `cap` leaves to copy.
int match_lists(mh_ctx* ctx, const char* who, int slot, int cap, int32_t* n_matches, size_t* arena, int* take) {
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  FrameState* fs = ctx->fs;
  if (slot < 0) slot = fs->list_first + fs->list_n - 1;
  if (slot < fs->list_first || slot >= fs->list_first + fs->list_n) {
    ctx->err = std::string(who) + ": the lists of that frame are gone (frames that went through the steps one "
               "after the other share one set of working arrays: only the last one's remain)";
    return MH_ERR_ARG;
  }
  *arena = (size_t)(slot - fs->list_first) * fs->arena_bytes;   // the frame's copy of the working arrays
  int32_t snap[4] = {0, 0, 0, 0};
  MH_HIP(ctx, hipMemcpyAsync(snap, fs->snap + 4 * slot, sizeof snap, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_matches = snap[0];
  *take = std::min(snap[0], cap);
  return MH_OK;
}

// mh_frame_result_copy*_dev: the bytes of one result block that hold max_objects objects (before the first frame: an
// empty block, "0 objects")
int result_copy_bytes(mh_ctx* ctx, int max_objects, size_t* bytes) {
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (!ctx->fs)
    if (int rc = prepare_frame(ctx, ctx->max_q > 0 ? ctx->max_q : 1)) return rc;
  *bytes = std::min(ctx->fs->result_bytes, 16 + sizeof(mh_object) * (size_t)max_objects);
  return MH_OK;
}

// The B frames of a batch through the rest chain, from frame 0's record (the frames' keypoints, top-2 entries and
// gathered blocks lie Q entries apart).  merge (the caller has asked merged_batch_ok and reserved B arenas' worth): ONE
// call for all of them.  Else frame f as a call of its own: result slot f, its slice of the top-2 arrays and of the image
// indices, and -- own_maps, a batch with a depth map per frame (mh_frame_set_depth_image_batch) -- its own map; c.q_count
// (an image batch): the frames' keypoint counts, one word per frame.
int rest_of_batch(mh_ctx* ctx, FrameCall c, int B, const uint64_t* seeds, bool merge, bool own_maps = false) {
  if (merge) {
    if (int rc = ensure_batch_arenas(ctx, B)) return rc;
    c.seed = seeds[0];
    c.seeds = seeds;
    c.batch_n = B;
    if (c.gathered) stamp(ctx, 1);   // (no MATCH of this rank before it: the chain's clock starts here)
    return frame_rest(ctx, c);
  }
  const float* const q_uv = c.q_uv;
  const int32_t* const gathered = c.gathered;
  const int32_t* const q_count = c.q_count;
  own_maps = own_maps && B > 1 && ctx->batch_imgs == B && ctx->depth_img.img;
  int rc = MH_OK;
  for (int f = 0; f < B && rc == MH_OK; ++f) {
    c.q_uv = q_uv + 2 * (size_t)f * c.Q;
    c.gathered = gathered ? gathered + (size_t)f * c.Q : nullptr;
    c.q0 = gathered ? 0 : f * c.Q;   // (gathered blocks are merged into the head of the top-2 arrays)
    c.slot = c.frame = f;
    c.seed = seeds[f];
    c.q_count = q_count ? q_count + f : nullptr;
    if (own_maps) {
      c.img = ctx->batch_img[f];
      c.fill = ctx->batch_fill[f];
    }
    if (gathered) stamp(ctx, 1);
    rc = frame_rest(ctx, c);
  }
  if (rc == MH_OK) ctx->frame_route[0] = B;   // (mh_frame_route: B frames, one after the other)
  return rc;
}

// mh_frame_enqueue_image[s] behind FEAT: launches for the capacity Q, the kernels read the frame's count from *n_dev
int image_frame_rest(mh_ctx* ctx, int Q, int32_t* n_dev, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  ctx->feat_count_dev = n_dev;
  stamp(ctx, 0);
  launch_normalize(ctx->q_desc, ctx->q_norm, Q, ctx->stream, n_dev);
  // (the frame's ratio goes along: group_kernel is the only reader of the top-2 arrays, frame_accept_ratio)
  if (int rc = ctx_match(ctx, ctx->q_desc, ctx->q_norm, Q, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, n_dev, ctx->feat_expected,
                         frame_accept_ratio(ctx, prm)))
    return rc;
  stamp(ctx, 1);
  FrameCall c{ctx->q_uv, Q, cam, prm, seed};
  c.q_count = n_dev;   // (DEPTHFILTER counts the frame's keypoints, not the capacity)
  return frame_rest(ctx, c);
}

// mh_frame_enqueue_image[s]_batch behind FEAT: B frames' keypoint lists lie Q rows apart in the context's query buffers,
// frame f's length in counts[f] (device) -- normalise, ONE MATCH launch sequence over all of them, the rest chain
// (own_maps: with the depth map mh_frame_set_depth_image_batch handed in for every frame)
int image_batch_rest(mh_ctx* ctx, int Q, int B, const int32_t* counts, const mh_cam* cam, const mh_frame_params* prm,
                     const uint64_t* seeds, bool merge, bool own_maps = false) {
  hipStream_t s = ctx->stream;
  launch_normalize_batch(ctx->q_desc, ctx->q_norm, Q, B, s, counts);   // (one launch: blockIdx.y = image)
  MH_HIP(ctx, hipGetLastError());
  ctx->feat_count_dev = nullptr;
  stamp(ctx, 0);
  hipLaunchKernelGGL(image_batch_tail_kernel, dim3((B * Q * (DIM / 4) + 255) / 256), dim3(256), 0, s, ctx->q_desc, ctx->q_norm,
                     counts, Q, B);
  if (int rc = ctx_match(ctx, ctx->q_desc, ctx->q_norm, B * Q, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, nullptr, 0, frame_accept_ratio(ctx, prm)))
    return rc;
  hipLaunchKernelGGL(image_batch_mask_kernel, dim3((B * Q + 255) / 256), dim3(256), 0, s, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2,
                     counts, Q, B);
  stamp(ctx, 1);
  FrameCall c{ctx->q_uv, Q, cam, prm, 0};
  c.q_count = counts;   // (rows past a frame's count hold what the slot's previous occupant left: DEPTHFILTER must not count them)
  return rest_of_batch(ctx, c, B, seeds, merge, own_maps);
}

// mh_frame_enqueue_rest*: one frame's rest chain behind the shards' gathered blocks -- shard k's block is [3][Q] words at
// gathered_dev + k * 3 Q (or the strides apart); the first launch merges them into the context's own top-2 arrays
int enqueue_rest(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards, int shard_stride,
                 int plane_stride, int slot, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  if (!ctx || Q <= 0 || !q_uv_dev || !gathered_dev || n_shards <= 0 || !cam || !prm) return MH_ERR_ARG;
  if (int rc = filter_depth_frame_ok(ctx, "mh_frame_enqueue_rest", prm, 1, true)) return rc;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (int rc = prepare_frame(ctx, Q)) return rc;
  stamp(ctx, 1);
  FrameCall c{q_uv_dev, Q, cam, prm, seed};
  c.gathered = gathered_dev;
  c.n_shards = n_shards;
  c.shard_stride = shard_stride;
  c.plane_stride = plane_stride;
  c.slot = slot;
  return frame_rest(ctx, c);
}

}  // namespace

namespace mh {

// the frame's cameras into the context's device table
int upload_cams(mh_ctx* ctx, const mh_cam* cams, int n_images) {
  MH_HIP(ctx, ctx->cams_dev.ensure(MH_MAX_IMAGES, ctx->stream));
  ctx->cams_view = ctx->cams_dev;
  DevCam h[MH_MAX_IMAGES];
  for (int i = 0; i < n_images; ++i) h[i] = make_devcam(cams[i]);
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // frames in flight still read the old table
  MH_HIP(ctx, hipMemcpy(ctx->cams_dev, h, sizeof(DevCam) * n_images, hipMemcpyHostToDevice));
  return MH_OK;
}

int enqueue_features(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q, const mh_cam* cam,
                     const mh_frame_params* prm, uint64_t seed, const FeatureOptions& opt) {
  if (opt.stage_lo == 0 && opt.stage_hi == 5)   // (a whole frame: mh_step_* keep the plain FILTER)
    if (int rc = filter_depth_frame_ok(ctx, "frame", prm)) return rc;
  if (int rc_enter = enter(ctx)) return rc_enter;
  if (int rc = prepare_frame(ctx, Q)) return rc;
  ctx->feat_count_dev = nullptr;
  stamp(ctx, 0);
  launch_normalize(q_desc_dev, ctx->q_norm, Q, ctx->stream);
  if (opt.write_back && ctx->wb_ev) hipEventRecord(ctx->wb_ev, ctx->stream);   // (mh_frame_run_host copies them back from here)
  // (a whole frame hands MATCH its ratio; a stepped one -- mh_step_*, whose later steps may come with other parameters --
  // keeps the exact triple of every query)
  const bool whole = opt.stage_lo == 0 && opt.stage_hi == 5;
  if (int rc_m = ctx_match(ctx, q_desc_dev, ctx->q_norm, Q, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, nullptr, 0,
                           whole ? frame_accept_ratio(ctx, prm) : 0.f))
    return rc_m;
  stamp(ctx, 1);
  ctx->step.done = -1;   // (whatever a stepped frame left on the device is overwritten from here on)
  FrameCall c{q_uv_dev, Q, cam, prm, seed};
  c.stage_lo = opt.stage_lo;
  c.stage_hi = opt.stage_hi;
  return frame_rest(ctx, c);
}

// The whole frame for a host that holds its features in HOST memory and wants the objects back before it goes on: the
// loop body of MopedPimpl::processImages (src/moped.cpp:183-191: MATCH .. FILTER2 one after the other on one FrameData)
// as ONE call -- two uploads, one stream-ordered chain of launches, one synchronisation -- instead of six steps with the
// frame's lists crossing PCIe between them (FRAME_RESIDENT_HIP, moped_amd/host).
int host_frame_begin(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                     const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, const FeatureOptions& opt) {
  if (!ctx || Q <= 0 || !q_desc_host || !q_uv_host || !cams || n_images < 1 || n_images > MH_MAX_IMAGES || !prm ||
      (n_images > 1 && !q_image_host)) {
    if (ctx) ctx->err = "mh_frame_run_host: bad argument";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // A write-back of the frame before may still be copying q_desc out on wb_stream (the caller skipped
  // mh_frame_wait_descriptors, or a call failed behind its copy): this frame's upload overwrites that buffer and
  // ensure_frame_buffers may free it -- wait for the stream whatever wb_pending says (nothing in flight: no cost).
  if (ctx->wb_stream) {
    MH_HIP(ctx, hipStreamSynchronize(ctx->wb_stream));
    ctx->wb_pending = false;
  }
  int rc = ensure_frame_buffers(ctx, Q);
  if (rc) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->q_desc, q_desc_host, (size_t)Q * DIM * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(ctx->q_uv, q_uv_host, (size_t)Q * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (n_images > 1) {
    if (ctx->hf_img.cap < (size_t)Q) MH_HIP(ctx, ctx->hf_img.ensure((size_t)ctx->max_q, ctx->stream));   // (as many rows as the frame buffers)
    MH_HIP(ctx, hipMemcpyAsync(ctx->hf_img, q_image_host, (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = mh_frame_set_images(ctx, ctx->hf_img, cams, n_images))) return rc;
  } else if (ctx->q_img) {
    if ((rc = mh_frame_set_images(ctx, nullptr, nullptr, 0))) return rc;
  }
  // the reference normalises the frame's descriptors in place (MATCH_ANN_CPU.hpp:157): the copy back starts as soon as
  // normalize_kernel is through -- on a stream of its own, beside the frame's other kernels; behind them on the frame's
  // stream it was another ~0.13 ms at the end of every frame
  if (opt.write_back && !ctx->wb_stream) {
    MH_HIP(ctx, hipStreamCreateWithFlags(&ctx->wb_stream, hipStreamNonBlocking));
    MH_HIP(ctx, hipEventCreateWithFlags(&ctx->wb_ev, hipEventDisableTiming));
  }
  if ((rc = enqueue_features(ctx, ctx->q_desc, ctx->q_uv, Q, &cams[0], prm, seed, opt))) return rc;
  if (opt.write_back) {
    MH_HIP(ctx, hipStreamWaitEvent(ctx->wb_stream, ctx->wb_ev, 0));
    ctx->wb_pending = true;   // (set before the copy: an error below must not hide a copy that did start)
    MH_HIP(ctx, hipMemcpyAsync(q_desc_host, ctx->q_desc, (size_t)Q * DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->wb_stream));
  }
  return MH_OK;
}

int delivery_begin(mh_ctx* ctx, void* host_block, size_t bytes, unsigned char** dst_dev) {
  auto& d = ctx->dlv;
  if (d.pending) {
    ctx->err = "delivery: the context's previous delivery has not been waited for (mh_frame_fetch_wait)";
    return MH_ERR_ARG;
  }
  if (!d.done) MH_HIP(ctx, hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, host_block, 0) == hipSuccess && dev) {
    *dst_dev = static_cast<unsigned char*>(dev);
    return MH_OK;
  }
  (void)hipGetLastError();   // not pinned / not mapped: through the staging buffer
  MH_HIP(ctx, d.stage.ensure(bytes, ctx->stream));
  *dst_dev = d.stage;
  return MH_OK;
}

int delivery_end(mh_ctx* ctx, void* host_block, size_t bytes, unsigned char* dst_dev, int B, int max_objects, uint32_t tag) {
  auto& d = ctx->dlv;
  MH_HIP(ctx, hipGetLastError());
  if (dst_dev == d.stage)
    MH_HIP(ctx, hipMemcpyAsync(host_block, d.stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipEventRecord(d.done, ctx->stream));
  d.pending = true;
  d.host_block = static_cast<unsigned char*>(host_block);
  d.B = B;
  d.max_objects = max_objects;
  d.tag = tag;
  return MH_OK;
}

}  // namespace mh

extern "C" {

size_t mh_frame_block_stride(int max_objects) {
  return sizeof(mh_frame_head) + sizeof(mh_object) * (size_t)(max_objects > 0 ? max_objects : 0);
}

int mh_frame_fetch_batch_async(mh_ctx* ctx, int B, int max_objects, void* host_block, uint32_t tag) {
  static_assert(sizeof(mh_frame_head) == 32 && sizeof(mh_object) == 40, "block layout");
  if (!ctx || !ctx->fs || !host_block || B < 1 || B > MH_MAX_BATCH || max_objects < 0) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  FrameState* fs = ctx->fs;
  const size_t bytes = mh_frame_block_stride(max_objects) * (size_t)B;
  unsigned char* dst = nullptr;
  if (int rc = delivery_begin(ctx, host_block, bytes, &dst)) return rc;
  hipLaunchKernelGGL(deliver_kernel, dim3(B), dim3(128), 0, ctx->stream, fs->result, fs->result_bytes, fs->snap, dst,
                     max_objects, fs->max_objects, tag);
  return delivery_end(ctx, host_block, bytes, dst, B, max_objects, tag);
}

/* ---- object hulls behind the frames (hull.hip) ---- */

int mh_frame_set_hulls(mh_ctx* ctx, int max_vertices, int image) {
  if (!ctx) return MH_ERR_ARG;
  if (max_vertices < 0 || max_vertices > (1 << 20) || image < 0 || image >= MH_MAX_IMAGES) {
    ctx->err = "mh_frame_set_hulls: max_vertices 0 (off) .. 2^20, image 0 .. MH_MAX_IMAGES - 1";
    return MH_ERR_ARG;
  }
  ctx->hulls.max_vertices = max_vertices;
  ctx->hulls.image = image;
  return MH_OK;
}

size_t mh_frame_hull_block_stride(int max_objects, int max_vertices) {
  if (max_objects < 0 || max_vertices < 0) return 0;
  return (size_t)max_objects * hull_record_words(max_vertices) * 4;
}

// the slot holds hulls (of the frame enqueued last into it), else MH_ERR_ARG with `who`
static int hull_slot_ok(mh_ctx* ctx, const char* who, int slot) {
  if (!ctx->fs || slot < 0 || slot >= MH_MAX_BATCH || ctx->hulls.slot_vertices[slot] <= 0 || !ctx->hulls.block) {
    ctx->err = std::string(who) + ": the frame in that result slot ran without hulls (mh_frame_set_hulls before it is enqueued)";
    return MH_ERR_ARG;
  }
  return MH_OK;
}

int mh_frame_fetch_hulls_slot(mh_ctx* ctx, int slot, int max_objects, int max_vertices, float* hull_xy_host,
                              int32_t* n_vertices, int32_t* n_behind, float* bbox_uv_host, int32_t* n_objects) {
  if (!ctx) return MH_ERR_ARG;
  if (!n_objects || max_objects < 0 || max_vertices < 1 || (max_objects > 0 && (!hull_xy_host || !n_vertices))) {
    ctx->err = "mh_frame_fetch_hulls: bad argument";
    return MH_ERR_ARG;
  }
  if (int rc = hull_slot_ok(ctx, "mh_frame_fetch_hulls", slot)) return rc;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  FrameState* fs = ctx->fs;
  mh_ctx::HullState& hs = ctx->hulls;
  hipStream_t s = ctx->stream;
  int32_t head[4] = {0, 0, 0, 0};
  MH_HIP(ctx, hipMemcpyAsync(head, fs->result + (size_t)slot * fs->result_bytes, sizeof head, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  const int n = std::min(std::max(head[0], 0), fs->max_objects);   // the objects mh_frame_fetch_slot reports, in its order
  *n_objects = n;
  const int take = std::min(n, max_objects);
  if (take == 0) return MH_OK;
  const size_t rec = hull_record_words(hs.block_vertices);
  if (int rc = ensure_pinned(ctx, (size_t)take * rec * 4)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->pinned.p, hs.block + (size_t)slot * hs.slot_bytes, (size_t)take * rec * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  const int32_t* const w = reinterpret_cast<const int32_t*>(ctx->pinned.p);
  for (int o = 0; o < take; ++o) {
    const int32_t* const r = w + (size_t)o * rec;
    n_vertices[o] = r[0];
    if (n_behind) n_behind[o] = r[1];
    if (bbox_uv_host) std::memcpy(bbox_uv_host + 16 * (size_t)o, r + 2, 64);
    const int kept = std::min(std::min(r[0], hs.block_vertices), max_vertices);
    if (kept > 0) std::memcpy(hull_xy_host + 2 * (size_t)o * max_vertices, r + 18, (size_t)kept * 8);
  }
  return MH_OK;
}

int mh_frame_fetch_hulls(mh_ctx* ctx, int max_objects, int max_vertices, float* hull_xy_host, int32_t* n_vertices,
                         int32_t* n_behind, float* bbox_uv_host, int32_t* n_objects) {
  return mh_frame_fetch_hulls_slot(ctx, 0, max_objects, max_vertices, hull_xy_host, n_vertices, n_behind, bbox_uv_host, n_objects);
}

/* ---- DEPTH_VERIFY behind the frames (depth_verify.hip) ---- */

int mh_frame_set_depth_verify(mh_ctx* ctx, const mh_depth_verify_params* prm, const mh_cam* depth_cam) {
  if (!ctx) return MH_ERR_ARG;
  if (prm && !depth_cam) {
    ctx->err = "mh_frame_set_depth_verify: the depth map's camera is missing";
    return MH_ERR_ARG;
  }
  ctx->verify.on = prm != nullptr;
  if (prm) {
    ctx->verify.prm = *prm;
    ctx->verify.cam = *depth_cam;
  }
  return MH_OK;
}

// mh_frame_fetch_verify[_slot] (`who`: the entry point, for its messages)
static int fetch_verify(mh_ctx* ctx, const char* who, int slot, int max_records, mh_verify_record* records, int32_t* n_records) {
  if (!ctx) return MH_ERR_ARG;
  if (!n_records || max_records < 0 || (max_records > 0 && !records)) {
    ctx->err = std::string(who) + ": bad argument";
    return MH_ERR_ARG;
  }
  mh_ctx::VerifyState& vs = ctx->verify;
  if (!ctx->fs || slot < 0 || slot >= MH_MAX_BATCH || !vs.slot_on[slot] || !vs.block) {
    ctx->err = std::string(who) + ": the frame in that result slot ran without DEPTH_VERIFY (mh_frame_set_depth_verify before "
               "it is enqueued)";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (int rc = ensure_pinned(ctx, vs.slot_bytes)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->pinned.p, vs.block.p + (size_t)slot * vs.slot_bytes, vs.slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t* const head = reinterpret_cast<const int32_t*>(ctx->pinned.p);
  *n_records = head[0];
  const int take = std::min(std::min(head[0], max_records), ctx->fs->max_objects);
  if (take > 0) std::memcpy(records, head + 4, (size_t)take * sizeof(mh_verify_record));
  return MH_OK;
}

int mh_frame_fetch_verify_slot(mh_ctx* ctx, int slot, int max_records, mh_verify_record* records, int32_t* n_records) {
  return fetch_verify(ctx, "mh_frame_fetch_verify_slot", slot, max_records, records, n_records);
}

int mh_frame_fetch_verify(mh_ctx* ctx, int max_records, mh_verify_record* records, int32_t* n_records) {
  return fetch_verify(ctx, "mh_frame_fetch_verify", 0, max_records, records, n_records);
}

int mh_frame_fetch_batch_hulls_async(mh_ctx* ctx, int B, int max_objects, void* host_block) {
  if (!ctx) return MH_ERR_ARG;
  if (!host_block || B < 1 || B > MH_MAX_BATCH || max_objects < 1) {
    ctx->err = "mh_frame_fetch_batch_hulls_async: bad argument";
    return MH_ERR_ARG;
  }
  for (int f = 0; f < B; ++f)
    if (int rc = hull_slot_ok(ctx, "mh_frame_fetch_batch_hulls_async", f)) return rc;
  mh_ctx::HullState& hs = ctx->hulls;
  if (hs.pending) {
    ctx->err = "mh_frame_fetch_batch_hulls_async: the previous delivery has not been waited for (mh_frame_fetch_wait)";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (!hs.done) MH_HIP(ctx, hipEventCreateWithFlags(&hs.done, hipEventDisableTiming));
  const size_t stride = mh_frame_hull_block_stride(std::min(max_objects, ctx->fs->max_objects), hs.block_vertices);
  const size_t pitch = mh_frame_hull_block_stride(max_objects, hs.block_vertices);
  MH_HIP(ctx, hipMemcpy2DAsync(host_block, pitch, hs.block, hs.slot_bytes, stride, (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipEventRecord(hs.done, ctx->stream));
  hs.pending = true;
  return MH_OK;
}

int mh_frame_fetch_query(mh_ctx* ctx) {
  if (!ctx) return MH_ERR_ARG;
  if (ctx->hulls.pending) {   // (mh_frame_fetch_batch_hulls_async: enqueued behind the objects' delivery, so it ends last)
    MH_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t eh = hipEventQuery(ctx->hulls.done);
    if (eh == hipErrorNotReady) {
      (void)hipGetLastError();
      return 1;
    }
    MH_HIP(ctx, eh);
  }
  if (!ctx->dlv.pending) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  const hipError_t e = hipEventQuery(ctx->dlv.done);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    return 1;
  }
  MH_HIP(ctx, e);
  return MH_OK;
}

int mh_frame_fetch_wait(mh_ctx* ctx, int32_t* flags_or) {
  if (!ctx) return MH_ERR_ARG;
  if (flags_or) *flags_or = 0;
  if (ctx->hulls.pending) {   // (mh_frame_fetch_batch_hulls_async)
    MH_HIP(ctx, hipSetDevice(ctx->device));
    MH_HIP(ctx, hipEventSynchronize(ctx->hulls.done));
    ctx->hulls.pending = false;
  }
  auto& d = ctx->dlv;
  if (!d.pending) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  MH_HIP(ctx, hipEventSynchronize(d.done));
  d.pending = false;
  int32_t flags = 0;
  const size_t stride = mh_frame_block_stride(d.max_objects);
  for (int f = 0; f < d.B; ++f) {
    const mh_frame_head* h = reinterpret_cast<const mh_frame_head*>(d.host_block + (size_t)f * stride);
    flags |= h->flags;
    if (h->tag != d.tag || h->frame != f) {   // the block was written by something else in the meantime
      ctx->err = "mh_frame_fetch_wait: the host block does not hold the delivery that was enqueued into it";
      return MH_ERR_ARG;
    }
  }
  if (flags_or) *flags_or = flags;
  return frame_flags(ctx, flags);
}

int mh_reserve(mh_ctx* ctx, int max_queries, int max_clusters, int max_objects) {
  if (!ctx || max_queries <= 0 || max_clusters <= 0 || max_objects <= 0) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  int rc = ensure_frame_buffers(ctx, max_queries);
  if (rc) return rc;
  // (after mh_db_reserve: per-model tables for as many models as the edits may bring, so that no frame reallocates them)
  return ensure_fs(ctx, ctx->max_q, max_clusters, max_objects, std::max(ctx->n_models, ctx->db_models_reserved));
}

int mh_reserve_batch(mh_ctx* ctx, int queries_per_frame, int frames, int max_clusters, int max_objects) {
  if (!ctx || queries_per_frame <= 0 || frames < 1 || frames > MH_MAX_BATCH || max_clusters <= 0 || max_objects <= 0)
    return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  int rc = ensure_frame_buffers(ctx, queries_per_frame * frames);
  if (rc) return rc;
  if ((rc = ensure_match_scratch(ctx, queries_per_frame * frames))) return rc;
  return ensure_fs(ctx, queries_per_frame, max_clusters, max_objects, std::max(ctx->n_models, ctx->db_models_reserved), frames);
}

void mh_frame_default_params(mh_frame_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->ratio = 0.8f;            // config.hpp:83
  p->ms_radius = 200.f;       // config.hpp:101
  p->ms_merge = 20.f;
  p->ms_min_pts = 7;
  p->ms_max_iter = 100;
  // (LM caps: 2 iterations on plain residuals -- a warm start; the squared-residual phase, Newton-scaled since round 4,
  //  converges from there as fast as from a converged plain phase: single frame 0.70 -> 0.675 ms, frame_stress unchanged)
  p->pose1 = {1024, 4, 5, 6, 10.f, 2, 10};   // config.hpp:110 (…, 4, 5, 6, 10)
  p->f1_min_points = 5;       // config.hpp:115
  p->f1_feature_distance = 4096.f;
  p->f1_min_score = 2.f;
  p->pose2 = {1024, 4, 6, 8, 5.f, 2, 10};    // config.hpp:118 (…, 4, 6, 8, 5)
  p->f2_min_points = 7;       // config.hpp:120
  p->f2_feature_distance = 4096.f;
  p->f2_min_score = 3.f;
  p->run_stage2 = 1;
}


int mh_frame_set_images(mh_ctx* ctx, const int32_t* q_image_dev, const mh_cam* cams, int n_images) {
  if (!ctx) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (!q_image_dev || !cams || n_images <= 1) {   // back to one image: the camera of mh_frame_enqueue*
    ctx->q_img = nullptr;
    ctx->n_images = 1;
    return MH_OK;
  }
  if (n_images > MH_MAX_IMAGES) {
    ctx->err = "mh_frame_set_images: more than MH_MAX_IMAGES images";
    return MH_ERR_CAPACITY;
  }
  if (int rc = upload_cams(ctx, cams, n_images)) return rc;
  ctx->q_img = q_image_dev;
  ctx->n_images = n_images;
  return MH_OK;
}

int mh_frame_set_depth(mh_ctx* ctx, const mh_depth* q_depth_dev, int kind, float alpha) {
  if (!ctx) return MH_ERR_ARG;
  if (q_depth_dev && kind != MH_DEPTH_BACKPROJECTION && kind != MH_DEPTH_REPROJECTION) return MH_ERR_ARG;
  ctx->q_depth = q_depth_dev;
  ctx->depth_img = DepthImage{};
  ctx->depth_kind = q_depth_dev ? kind : MH_DEPTH_NONE;
  ctx->depth_alpha = alpha;
  return MH_OK;
}

int mh_frame_set_depth_image(mh_ctx* ctx, const float* depth_xyzn_dev, const float* fill_distance_dev, int width,
                             int height, int kind, float alpha, float cauchy_scale) {
  if (!ctx) return MH_ERR_ARG;
  if (depth_xyzn_dev && ((kind != MH_DEPTH_BACKPROJECTION && kind != MH_DEPTH_REPROJECTION) || width <= 0 ||
                         height <= 0 || !(cauchy_scale > 0.f)))
    return MH_ERR_ARG;
  ctx->q_depth = nullptr;
  ctx->depth_img = DepthImage{};
  ctx->batch_imgs = 0;
  if (depth_xyzn_dev) {
    ctx->depth_img.img = reinterpret_cast<const float4*>(depth_xyzn_dev);
    ctx->depth_img.fill = fill_distance_dev;
    ctx->depth_img.w = width;
    ctx->depth_img.h = height;
    ctx->depth_img.cauchy_scale = cauchy_scale;
  }
  ctx->depth_kind = depth_xyzn_dev ? kind : MH_DEPTH_NONE;
  ctx->depth_alpha = alpha;
  return MH_OK;
}

int mh_frame_set_depth_image_batch(mh_ctx* ctx, const float* const* depth_xyzn_dev, const float* const* fill_distance_dev,
                                   int n_frames, int width, int height, int kind, float alpha, float cauchy_scale) {
  if (!ctx || !depth_xyzn_dev || n_frames < 1 || n_frames > MH_MAX_BATCH) return MH_ERR_ARG;
  for (int f = 0; f < n_frames; ++f)
    if (!depth_xyzn_dev[f]) return MH_ERR_ARG;
  const int rc = mh_frame_set_depth_image(ctx, depth_xyzn_dev[0], fill_distance_dev ? fill_distance_dev[0] : nullptr, width,
                                          height, kind, alpha, cauchy_scale);
  if (rc) return rc;
  for (int f = 0; f < n_frames; ++f) {
    ctx->batch_img[f] = reinterpret_cast<const float4*>(depth_xyzn_dev[f]);
    ctx->batch_fill[f] = fill_distance_dev ? fill_distance_dev[f] : nullptr;
  }
  ctx->batch_imgs = n_frames;
  return MH_OK;
}

int mh_frame_set_depth_image_host(mh_ctx* ctx, const float* depth_xyzn_host, const float* fill_distance_host,
                                  int width, int height, int kind, float alpha, float cauchy_scale) {
  if (!ctx) return MH_ERR_ARG;
  if (!depth_xyzn_host) return mh_frame_set_depth_image(ctx, nullptr, nullptr, 0, 0, 0, alpha, cauchy_scale);
  if (width <= 0 || height <= 0) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const size_t px = (size_t)width * height;
  if (int rc = ensure_own_depth(ctx, px)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_depth, depth_xyzn_host, px * 4 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (fill_distance_host)
    MH_HIP(ctx, hipMemcpyAsync(ctx->own_fill, fill_distance_host, px * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host maps may change after the call
  return mh_frame_set_depth_image(ctx, ctx->own_depth, fill_distance_host ? ctx->own_fill : nullptr, width, height, kind,
                                  alpha, cauchy_scale);
}

// FILTER / FILTER2 of the frames as FILTER_PROJECTION_DEPTH_CPU (moped3d .../filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329)
int mh_frame_set_filter_depth(mh_ctx* ctx, const mh_filter_depth_params* f1, const mh_filter_depth_params* f2,
                              const mh_cam* depth_cam) {
  if (!ctx) return MH_ERR_ARG;
  if ((f1 || f2) && !depth_cam) {
    ctx->err = "mh_frame_set_filter_depth: the depth map's camera is missing";
    return MH_ERR_ARG;
  }
  mh_ctx::FilterDepthState& fd = ctx->fdepth;
  fd.on[0] = f1 != nullptr;
  fd.on[1] = f2 != nullptr;
  if (f1) fd.prm[0] = *f1;
  if (f2) fd.prm[1] = *f2;
  if (depth_cam) fd.cam = *depth_cam;
  return MH_OK;
}

// how the last frame or batch enqueued went through CLUSTER .. FILTER2 (frame_rest's record; no device work)
int mh_frame_route(mh_ctx* ctx, int32_t out[4]) {
  if (!ctx || !out) return MH_ERR_ARG;
  for (int k = 0; k < 4; ++k) out[k] = ctx->frame_route[k];
  return MH_OK;
}

int mh_set_linkage_scratch_limit(mh_ctx* ctx, size_t bytes) {
  if (!ctx) return MH_ERR_ARG;
  ctx->lk_scratch_limit = bytes ? bytes : (size_t)4 << 30;
  return MH_OK;
}

int mh_frame_set_cluster_linkage(mh_ctx* ctx, const mh_linkage_params* prm) {
  if (!ctx) return MH_ERR_ARG;
  if (prm && (prm->linkage_type < 0 || prm->linkage_type > 2)) {   // (before anything of the context changes)
    ctx->err = "mh_frame_set_cluster_linkage: linkage_type must be 0 (minimum), 1 (average) or 2 (maximum)";
    return MH_ERR_ARG;
  }
  ctx->linkage_on = prm != nullptr;
  if (prm) {
    ctx->wms_on = false;   // (the two clusterers exclude each other: the one set last is on)
    ctx->linkage.cutoff = prm->cutoff;
    ctx->linkage.min_pts = prm->min_pts;
    ctx->linkage.use3d_filter = prm->use3d_filter;
    ctx->linkage.sigma2d = prm->sigma2d;
    ctx->linkage.sigma3d = prm->sigma3d;
    ctx->linkage.linkage_type = prm->linkage_type;
  }
  return MH_OK;
}

int mh_frame_set_cluster_wms(mh_ctx* ctx, const mh_wms_params* prm) {
  if (!ctx) return MH_ERR_ARG;
  if (prm) {   // (before anything of the context changes)
    const char* bad = !(prm->radius >= 0.f) ? "radius must be a number >= 0" : !(prm->merge >= 0.f) ? "merge must be a number >= 0"
                      : !(prm->half_weight_distance >= 0.f) ? "half_weight_distance must be a number >= 0"
                      : prm->max_iter < 0 ? "max_iter < 0" : nullptr;
    if (bad) {
      ctx->err = std::string("mh_frame_set_cluster_wms: ") + bad;
      return MH_ERR_ARG;
    }
  }
  ctx->wms_on = prm != nullptr;
  if (prm) {
    ctx->linkage_on = false;   // (the one set last is on)
    ctx->wms.radius = prm->radius;
    ctx->wms.merge = prm->merge;
    ctx->wms.min_pts = prm->min_pts;
    ctx->wms.max_iter = prm->max_iter;
    ctx->wms.half_weight_distance = prm->half_weight_distance;
    // the members' buffer, for the matches the context has reserved (a frame that reserves more regrows it)
    if (ctx->fs) {
      if (int rc_enter = mh::enter(ctx)) return rc_enter;
      if (int rc = ensure_wms_buffers(ctx)) return rc;
    }
  }
  return MH_OK;
}

int mh_frame_set_depth_rules(mh_ctx* ctx, const mh_depth_rules* r, const float K[4]) {
  if (!ctx) return MH_ERR_ARG;
  mh_ctx::DepthRuleState& rs = ctx->rules;
  if (!r) {
    rs.on = false;
    return MH_OK;
  }
  const bool filters = r->feature_density >= 0.f || r->match_density >= 0.f;
  if ((filters && (r->patch_size <= 0 || !K)) || (r->ratio_table && (r->n_models <= 0 || !(r->cauchy_scale > 0.f)))) {
    ctx->err = "mh_frame_set_depth_rules: bad argument";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  rs.patch = r->patch_size > 0 ? r->patch_size : 64;
  // `Float filter = Density*100*100` (DEPTHFILTER_CPU.hpp:132)
  rs.feature_filter = r->feature_density >= 0.f ? r->feature_density * 100 * 100 : -1.f;
  rs.match_filter = r->match_density >= 0.f ? r->match_density * 100 * 100 : -1.f;
  for (int i = 0; i < 4; ++i) rs.K[i] = K ? K[i] : 0.f;
  rs.max_depth = r->maximum_depth;
  rs.default_depth = r->default_depth;
  rs.cauchy_scale = r->cauchy_scale;
  if (r->ratio_table) {
    rs.table_models = 0;
    MH_HIP(ctx, rs.ratio_table.ensure((size_t)4 * r->n_models, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(rs.ratio_table, r->ratio_table, sizeof(float) * 4 * r->n_models, hipMemcpyHostToDevice,
                               ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host table may go away after the call
    rs.table_models = r->n_models;
  } else if (rs.ratio_table) {
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rs.ratio_table.reset();   // (null = no table to the kernels)
    rs.table_models = 0;
  }
  rs.on = true;
  return MH_OK;
}

int mh_frame_enqueue(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q,
                     const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  if (!ctx || Q <= 0 || !q_desc_dev || !q_uv_dev || !cam || !prm) return MH_ERR_ARG;
  return enqueue_features(ctx, q_desc_dev, q_uv_dev, Q, cam, prm, seed, FeatureOptions());
}

int mh_host_alloc(mh_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return MH_ERR_ARG;
  *out = nullptr;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  MH_HIP(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return MH_OK;
}

int mh_host_free(mh_ctx* ctx, void* p) {
  if (!ctx) return MH_ERR_ARG;
  if (p) MH_HIP(ctx, hipHostFree(p));
  return MH_OK;
}

int mh_frame_run_host_begin(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                            const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, int write_back) {
  return host_frame_begin(ctx, q_desc_host, q_uv_host, q_image_host, Q, cams, n_images, prm, seed,
                          FeatureOptions{0, 5, write_back != 0});
}

int mh_frame_wait_descriptors(mh_ctx* ctx) {
  if (!ctx) return MH_ERR_ARG;
  if (ctx->wb_pending) {
    MH_HIP(ctx, hipSetDevice(ctx->device));
    MH_HIP(ctx, hipStreamSynchronize(ctx->wb_stream));   // (the next frame's upload overwrites q_desc)
    ctx->wb_pending = false;
  }
  return MH_OK;
}

int mh_frame_run_host(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                      const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, int write_back,
                      mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts) {
  if (!n_objects) {
    if (ctx) ctx->err = "mh_frame_run_host: bad argument";
    return MH_ERR_ARG;
  }
  int rc = mh_frame_run_host_begin(ctx, q_desc_host, q_uv_host, q_image_host, Q, cams, n_images, prm, seed, write_back);
  if (rc) return rc;
  rc = mh_frame_fetch(ctx, objects_host, max_objects, n_objects, counts);
  const int rc_wb = mh_frame_wait_descriptors(ctx);
  return rc ? rc : rc_wb;
}

int mh_frame_enqueue_image(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size,
                           int max_keypoints, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  if (!ctx || !gray_dev || width <= 0 || height <= 0 || max_keypoints <= 0 || !cam || !prm) return MH_ERR_ARG;
  if (int rc_fd = filter_depth_frame_ok(ctx, "mh_frame_enqueue_image", prm)) return rc_fd;
  if (int rc_if = image_format_frame_ok(ctx, "mh_frame_enqueue_image", width, height)) return rc_if;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const int Q = max_keypoints;
  int rc = prepare_frame(ctx, Q);
  if (rc) return rc;
  // the camera's image (mh_frame_set_image_format): its gray copy in a staging buffer of its own
  if ((rc = image_format_stage(ctx, &gray_dev, 1, &gray_dev))) return rc;
  // UNDISTORTED_IMAGE (mh_frame_set_undistort): FEAT reads the remapped copy in the context's staging buffer
  if (ctx->und_on && (rc = undistort_frame(ctx, &gray_dev, 1, width, height, cam->K, &gray_dev))) return rc;
  // FEAT: keypoints straight into the frame's query buffers; their number stays on the device
  int32_t* n_dev = nullptr;
  if ((rc = sift_into(ctx, gray_dev, width, height, double_size, Q, ctx->q_desc, ctx->q_uv, &n_dev))) return rc;
  return image_frame_rest(ctx, Q, n_dev, cam, prm, seed);
}

int mh_frame_enqueue_image_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int B, int width, int height, int double_size,
                                 int max_keypoints, const mh_cam* cam, const mh_frame_params* prm, const uint64_t* seeds) {
  if (!ctx || !gray_dev || B < 1 || B > MH_MAX_BATCH || width <= 0 || height <= 0 || max_keypoints <= 0 || !cam || !prm || !seeds)
    return MH_ERR_ARG;
  for (int f = 0; f < B; ++f)
    if (!gray_dev[f]) return MH_ERR_ARG;
  // moped3d's front end (a depth map per image, the rules, the linkage clusterer, either depth residual) travels with the
  // batch; what belongs to host-made queries does not.  Nothing of the context has changed when a refusal returns.
  auto refuse = [&](const char* why) {
    ctx->err = std::string("mh_frame_enqueue_image_batch: ") + why;
    return MH_ERR_ARG;
  };
  if (ctx->q_depth)
    return refuse("per-query depth attributes (mh_frame_set_depth) cannot belong to keypoints the device makes: hand in the "
                  "depth maps (mh_frame_set_depth_image_batch), or clear them with mh_frame_set_depth(ctx, NULL, ..)");
  if (ctx->q_img && ctx->n_images > 1)
    return refuse("a per-query image index (mh_frame_set_images) cannot belong to keypoints the device makes: "
                  "mh_frame_enqueue_images_batch takes frames of several cameras");
  const bool maps = ctx->depth_img.img != nullptr;
  const int n_maps = !maps ? 0 : (ctx->batch_imgs > 0 ? ctx->batch_imgs : 1);   // (mh_frame_set_depth_image: one map)
  if (maps && n_maps != B)
    return refuse("the context holds another number of depth maps than the batch has images: mh_frame_set_depth_image_batch "
                  "with one map per image (one image: mh_frame_set_depth_image), or mh_frame_set_depth_image(ctx, NULL, ..) "
                  "for a batch without depth");
  if (!maps && ctx->rules.on)
    return refuse("the depth rules (mh_frame_set_depth_rules) need a depth map per image: mh_frame_set_depth_image_batch, or "
                  "mh_frame_set_depth_rules(ctx, NULL, NULL) for a batch without them");
  if (int rc_fd = filter_depth_frame_ok(ctx, "mh_frame_enqueue_image_batch", prm)) return rc_fd;
  if (int rc_if = image_format_frame_ok(ctx, "mh_frame_enqueue_image_batch", width, height)) return rc_if;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const int Q = max_keypoints;
  const bool merge = B > 1 && merged_batch_ok(ctx, prm, true, B);
  int rc = prepare_frame(ctx, B * Q, Q, merge ? B : 1);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  if (!ctx->img_counts) {
    MH_HIP(ctx, ctx->img_counts.ensure(MH_MAX_BATCH, s));
    MH_HIP(ctx, hipMemsetAsync(ctx->img_counts, 0, MH_MAX_BATCH * sizeof(int32_t), s));
  }
  // the cameras' images (mh_frame_set_image_format): one launch for the B gray copies, a staging buffer of their own
  const uint8_t* converted[MH_MAX_BATCH];
  if (ctx->img_fmt_on) {
    if ((rc = image_format_stage(ctx, gray_dev, B, converted))) return rc;
    gray_dev = converted;
  }
  // UNDISTORTED_IMAGE (mh_frame_set_undistort): one remap launch for the B images into the context's staging buffer
  const uint8_t* staged[MH_MAX_BATCH];
  if (ctx->und_on) {
    if ((rc = undistort_frame(ctx, gray_dev, B, width, height, cam->K, staged))) return rc;
    gray_dev = staged;
  }
  // FEAT image by image into the batch's query rows (image f: rows f Q ..), every image's count in a word of its own
  // (round 4: ONE launch per FEAT stage for all B images -- a frame's 26 dependent launches were what bounded this path)
  if ((rc = sift_into_batch(ctx, gray_dev, B, width, height, double_size, Q, ctx->q_desc, ctx->q_uv, ctx->img_counts)))
    return rc;
  return image_batch_rest(ctx, Q, B, ctx->img_counts, cam, prm, seeds, merge, true);
}

// Storage of the image hand-over: FEAT's staging for `images` images of `cap` rows, the count words, the rig's table,
// the image index of `list_rows` packed rows.
static int ensure_images_frame(mh_ctx* ctx, int images, int cap, size_t list_rows) {
  mh_ctx::ImagesFrame& m = ctx->imf;
  hipStream_t s = ctx->stream;
  const size_t rows = (size_t)images * cap;
  MH_HIP(ctx, m.desc.ensure(rows * DIM, s));   // (a frame in flight may still read the old staging: ensure waits for it)
  MH_HIP(ctx, m.xy.ensure(rows * 2, s));
  if (!m.words) {
    MH_HIP(ctx, m.words.ensure(3 * MH_MAX_BATCH, s));
    MH_HIP(ctx, hipMemsetAsync(m.words, 0, 3 * MH_MAX_BATCH * sizeof(int32_t), s));
  }
  MH_HIP(ctx, m.cams.ensure(MH_MAX_IMAGES, s));
  if (list_rows > m.q_img.cap) {
    MH_HIP(ctx, m.q_img.ensure(list_rows, s));
    MH_HIP(ctx, hipMemsetAsync(m.q_img, 0, list_rows * sizeof(int32_t), s));   // (rows past a frame's total are never written)
  }
  return MH_OK;
}

// F frames of n cameras each from F n device images: FEAT of all of them with one launch per stage into the staging
// area, ONE launch that packs every frame's list (images_pack.hip), then the frame(s) as mh_frame_enqueue_image
// (batched = false: F = 1) or mh_frame_enqueue_image_batch run theirs, every keypoint in its own image.
static int enqueue_images(mh_ctx* ctx, const char* who, const uint8_t* const* gray_dev, int F, int n, int width, int height,
                          int double_size, int cap, const mh_cam* cams, const mh_frame_params* prm, const uint64_t* seeds,
                          bool batched) {
  if (!ctx) return MH_ERR_ARG;
  auto refuse = [&](int rc, const char* why) {
    ctx->err = std::string(who) + ": " + why;
    return rc;
  };
  if (!gray_dev || F < 1 || n < 1 || width <= 0 || height <= 0 || cap <= 0 || !cams || !prm || !seeds)
    return refuse(MH_ERR_ARG, "bad argument");
  if (n > MH_MAX_IMAGES) return refuse(MH_ERR_CAPACITY, "more than MH_MAX_IMAGES cameras");
  if (F > MH_MAX_BATCH || F * n > MH_MAX_BATCH) return refuse(MH_ERR_CAPACITY, "more than MH_MAX_BATCH images in one call");
  if ((long long)F * n * cap > INT_MAX) return refuse(MH_ERR_CAPACITY, "too many rows");
  for (int j = 0; j < F * n; ++j)
    if (!gray_dev[j]) return refuse(MH_ERR_ARG, "null image");
  if (int rc_fd = filter_depth_frame_ok(ctx, who, prm, n)) return rc_fd;
  if (ctx->depth_img.img || ctx->rules.on || ctx->q_depth || (n > 1 && (ctx->linkage_on || ctx->wms_on)))
    return refuse(MH_ERR_ARG, "depth maps / rules / attributes and the linkage / weighted mean-shift clusterers are single-camera");
  if (ctx->imf.und_n && ctx->imf.und_n != n)
    return refuse(MH_ERR_ARG, "mh_frame_set_undistort_images gave coefficients for another number of cameras");
  if (int rc_if = image_format_frame_ok(ctx, who, width, height)) return rc_if;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // the call points the context's views of the image indices and cameras at its own for its own duration: whatever
  // mh_frame_set_images left is the caller's again afterwards, and a later one-camera frame finds no image index of this one
  struct Restore {
    mh_ctx* ctx;
    const int32_t* q_img;
    const DevCam* cams_view;
    int n_images;
    ~Restore() {
      ctx->q_img = q_img;
      ctx->cams_view = cams_view;
      ctx->n_images = n_images;
    }
  } restore{ctx, ctx->q_img, ctx->cams_view, ctx->n_images};
  ctx->q_img = nullptr;
  ctx->n_images = n;   // (sizes CLUSTER's per-(model, image) tables in prepare_frame)
  const int Q = n * cap;   // rows of one frame
  const bool merge = batched && F > 1 && n == 1 && merged_batch_ok(ctx, prm);
  int rc = prepare_frame(ctx, F * Q, Q, merge ? F : 1);
  if (rc) return rc;
  if ((rc = ensure_images_frame(ctx, F * n, cap, (size_t)F * Q))) return rc;
  mh_ctx::ImagesFrame& m = ctx->imf;
  if (n > 1) {
    ctx->q_img = m.q_img;
    ctx->cams_view = m.cams;
  }
  hipStream_t s = ctx->stream;
  // the cameras' images (mh_frame_set_image_format): one launch for the F n gray copies, a staging buffer of their own
  const uint8_t* converted[MH_MAX_BATCH];
  if (ctx->img_fmt_on) {
    if ((rc = image_format_stage(ctx, gray_dev, F * n, converted))) return rc;
    gray_dev = converted;
  }
  // UNDISTORTED_IMAGE per camera: one remap launch, every image with the map of its camera (one set of coefficients
  // from mh_frame_set_undistort goes with every camera's K)
  const uint8_t* staged[MH_MAX_BATCH];
  if (m.und_n || ctx->und_on) {
    float one[MH_MAX_IMAGES][4];
    for (int i = 0; i < n; ++i) std::memcpy(one[i], ctx->und_dist, sizeof one[i]);
    if ((rc = undistort_frame_images(ctx, gray_dev, F * n, n, width, height, cams, m.und_n ? m.und_dist : one, staged))) return rc;
    gray_dev = staged;
  }
  // FEAT: one launch per stage for the F n images, image j's list at rows j cap .. of the staging area
  if ((rc = sift_into_batch(ctx, gray_dev, F * n, width, height, double_size, cap, m.desc, m.xy, m.words))) return rc;
  ImagesPackArgs pa;
  pa.sdesc = m.desc;
  pa.sxy = m.xy;
  pa.scount = m.words;
  pa.desc = ctx->q_desc;
  pa.uv = ctx->q_uv;
  pa.q_img = m.q_img;
  pa.totals = batched ? m.words + MH_MAX_BATCH : images_single_total(ctx);
  pa.counts = batched ? m.words + 2 * MH_MAX_BATCH : images_single_total(ctx) + 1;
  pa.cams_dev = m.cams;
  pa.cap = cap;
  pa.n_images = n;
  for (int i = 0; i < MH_MAX_IMAGES; ++i) pa.cams[i] = make_devcam(cams[i < n ? i : 0]);
  launch_images_pack(pa, F, s);
  MH_HIP(ctx, hipGetLastError());
  if (!batched) {   // the frame alone, as mh_frame_enqueue_image: launches for the capacity, the kernels read the total
    m.n_live = n;
    return image_frame_rest(ctx, Q, pa.totals, &cams[0], prm, seeds[0]);
  }
  // the batch, as mh_frame_enqueue_image_batch with a frame's packed list in an image's place
  m.n_live = 0;
  return image_batch_rest(ctx, Q, F, pa.totals, &cams[0], prm, seeds, merge);
}

int mh_frame_enqueue_images(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_images, int width, int height, int double_size,
                            int max_keypoints_per_image, const mh_cam* cams, const mh_frame_params* prm, uint64_t seed) {
  return enqueue_images(ctx, "mh_frame_enqueue_images", gray_dev, 1, n_images, width, height, double_size,
                        max_keypoints_per_image, cams, prm, &seed, false);
}

int mh_frame_enqueue_images_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_frames, int n_images, int width,
                                  int height, int double_size, int max_keypoints_per_image, const mh_cam* cams,
                                  const mh_frame_params* prm, const uint64_t* seeds) {
  return enqueue_images(ctx, "mh_frame_enqueue_images_batch", gray_dev, n_frames, n_images, width, height, double_size,
                        max_keypoints_per_image, cams, prm, seeds, true);
}

int mh_frame_image_counts(mh_ctx* ctx, int32_t* counts, int cap, int32_t* n_images) {
  if (!ctx || !n_images || cap < 0 || (cap > 0 && !counts) || ctx->imf.last_n <= 0) return MH_ERR_ARG;
  *n_images = ctx->imf.last_n;
  for (int i = 0; i < ctx->imf.last_n && i < cap; ++i) counts[i] = ctx->imf.last[i];
  return MH_OK;
}

int mh_frame_features_image_dev(mh_ctx* ctx, int32_t** q_image_dev) {
  if (!ctx || !q_image_dev || !ctx->feat_count_dev || ctx->feat_count_dev != images_single_total(ctx) || !ctx->imf.n_live)
    return MH_ERR_ARG;
  *q_image_dev = ctx->imf.q_img;
  return MH_OK;
}

int mh_frame_features_dev(mh_ctx* ctx, float** desc_dev, float** uv_dev, int32_t** n_dev) {
  if (!ctx || !ctx->feat_count_dev) return MH_ERR_ARG;
  if (desc_dev) *desc_dev = ctx->q_desc;
  if (uv_dev) *uv_dev = ctx->q_uv;
  if (n_dev) *n_dev = ctx->feat_count_dev;
  return MH_OK;
}

int mh_frame_keypoints(mh_ctx* ctx, int32_t* n_keypoints) {
  if (!ctx || !n_keypoints || ctx->feat_last < 0) return MH_ERR_ARG;
  *n_keypoints = ctx->feat_last;
  return MH_OK;
}

int mh_frame_enqueue_batch(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q, int B, const mh_cam* cam,
                           const mh_frame_params* prm, const uint64_t* seeds) {
  if (!ctx || Q <= 0 || B < 1 || B > MH_MAX_BATCH || !q_desc_dev || !q_uv_dev || !cam || !prm || !seeds)
    return MH_ERR_ARG;
  if (B > 1 && (ctx->depth_img.img || ctx->rules.on) && ctx->batch_imgs != B) {
    ctx->err = "mh_frame_enqueue_batch: a depth map belongs to ONE frame (mh_frame_set_depth_image_batch hands in one per "
               "frame of the batch)";
    return MH_ERR_ARG;
  }
  if (int rc_fd = filter_depth_frame_ok(ctx, "mh_frame_enqueue_batch", prm)) return rc_fd;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const bool merge = B > 1 && merged_batch_ok(ctx, prm, true, B);
  int rc = prepare_frame(ctx, B * Q, Q, merge ? B : 1);   // (the arenas before any work is enqueued)
  if (rc) return rc;
  ctx->feat_count_dev = nullptr;
  stamp(ctx, 0);
  launch_normalize(q_desc_dev, ctx->q_norm, B * Q, ctx->stream);
  if ((rc = ctx_match(ctx, q_desc_dev, ctx->q_norm, B * Q, ctx->nn_idx, ctx->nn_d1, ctx->nn_d2, nullptr, 0, frame_accept_ratio(ctx, prm))))
    return rc;
  stamp(ctx, 1);
  // merged: the B frames through group / CLUSTER / POSE / POSE2 in one launch each
  return rest_of_batch(ctx, FrameCall{q_uv_dev, Q, cam, prm, 0}, B, seeds, merge, true);
}

int mh_frame_enqueue_match_local(mh_ctx* ctx, float* q_desc_dev, int Q, int32_t* top2_dev) {
  if (!ctx || Q <= 0 || !q_desc_dev || !top2_dev) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // (the working arrays of the rest chain are sized by the calls that run it: a batch's MATCH covers B frames' queries)
  int rc = ensure_frame_buffers(ctx, Q);
  if (rc) return rc;
  if ((rc = ensure_match_scratch(ctx, Q))) return rc;
  if (!ctx->fs && (rc = prepare_frame(ctx, Q))) return rc;
  float* d1 = reinterpret_cast<float*>(top2_dev + Q);
  ctx->feat_count_dev = nullptr;
  stamp(ctx, 0);
  launch_normalize(q_desc_dev, ctx->q_norm, Q, ctx->stream);
  if (int rc_m = ctx_match(ctx, q_desc_dev, ctx->q_norm, Q, top2_dev, d1, d1 + Q)) return rc_m;
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_frame_enqueue_rest(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev,
                          int n_shards, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  return enqueue_rest(ctx, q_uv_dev, Q, gathered_dev, n_shards, 0, 0, 0, cam, prm, seed);
}

int mh_frame_fetch(mh_ctx* ctx, mh_object* objects_host, int max_objects, int32_t* n_objects,
                   int32_t* counts) {
  if (!ctx || !n_objects || !ctx->fs) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  FrameState* fs = ctx->fs;
  FrameState::FetchPin& pin = *fs->fetch_pin;
  if (fs->host_armed && !ctx->feat_count_dev) {
    // the frame's FILTER2 wrote the host's block itself: wait for the stream, read
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const FrameHostBlock& h = *fs->host_block;
    const uint32_t seq = h.seq;
    if (seq != fs->host_seq_expect) fs->host_seq_expect = seq;   // (stale block: the stream is idle, the device's count is final -- resynchronise)
    else
      return read_out(ctx, h.head, h.snap, h.error, h.objects, FRAME_HOST_OBJECTS, fs->result, objects_host, max_objects,
                      n_objects, counts);
    // (the tail did not run -- a launch failed: the copies below report what there is)
  }
  const size_t first = std::min(fs->result_bytes, sizeof pin.head + sizeof pin.objects);   // head + the first objects: one copy
  MH_HIP(ctx, hipMemcpyAsync(pin.head, fs->result, first, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(pin.snap, fs->snap, sizeof pin.snap, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(&pin.fc, fs->counts, sizeof pin.fc, hipMemcpyDeviceToHost, ctx->stream));
  pin.n_feat = -1;
  // (a frame of several cameras: its images' counts come with its total)
  const int rig = ctx->feat_count_dev && ctx->feat_count_dev == images_single_total(ctx) ? ctx->imf.n_live : 0;
  if (ctx->feat_count_dev)
    MH_HIP(ctx, hipMemcpyAsync(&pin.n_feat, ctx->feat_count_dev, sizeof(int32_t) * (1 + rig), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t n_feat = pin.n_feat;
  if (n_feat >= 0) {
    ctx->feat_expected = ctx->feat_last = n_feat;
    ctx->imf.last_n = rig ? rig : 1;
    ctx->imf.last[0] = n_feat;
    for (int i = 0; i < rig; ++i) ctx->imf.last[i] = pin.img_n[i];
  }
  return read_out(ctx, pin.head, pin.snap, pin.fc.error, pin.objects, FETCH_PIN_OBJECTS, fs->result, objects_host, max_objects,
                  n_objects, counts);
}

int mh_frame_enqueue_rest_strided(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards,
                                  int shard_stride_words, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed) {
  if (!ctx || shard_stride_words < 3 * Q) return MH_ERR_ARG;
  return enqueue_rest(ctx, q_uv_dev, Q, gathered_dev, n_shards, shard_stride_words, 0, 0, cam, prm, seed);
}

int mh_frame_enqueue_rest_batch(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards,
                                int shard_stride_words, int plane_stride_words, int slot, const mh_cam* cam,
                                const mh_frame_params* prm, uint64_t seed) {
  if (!ctx || slot < 0 || slot >= MH_MAX_BATCH || plane_stride_words < Q || shard_stride_words < 3 * plane_stride_words)
    return MH_ERR_ARG;
  return enqueue_rest(ctx, q_uv_dev, Q, gathered_dev, n_shards, shard_stride_words, plane_stride_words, slot, cam, prm, seed);
}

int mh_frame_enqueue_rest_frames(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards,
                                 int shard_stride_words, int plane_stride_words, int B, const mh_cam* cam,
                                 const mh_frame_params* prm, const uint64_t* seeds) {
  if (!ctx || Q <= 0 || !q_uv_dev || !gathered_dev || n_shards <= 0 || !cam || !prm || !seeds || B < 1 || B > MH_MAX_BATCH ||
      plane_stride_words < Q || shard_stride_words < 3 * plane_stride_words)
    return MH_ERR_ARG;
  if (int rc_fd = filter_depth_frame_ok(ctx, "mh_frame_enqueue_rest_frames", prm, 1, true)) return rc_fd;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const bool merge = B > 1 && merged_batch_ok(ctx, prm);
  if (int rc = prepare_frame(ctx, merge ? B * Q : Q, Q, merge ? B : 1)) return rc;
  // merged: frame f merges the shards' blocks into [f Q, (f + 1) Q) of the context's top-2 arrays
  FrameCall c{q_uv_dev, Q, cam, prm, 0};
  c.gathered = gathered_dev;
  c.n_shards = n_shards;
  c.shard_stride = shard_stride_words;
  c.plane_stride = plane_stride_words;
  return rest_of_batch(ctx, c, B, seeds, merge);
}

int mh_frame_fetch_slot(mh_ctx* ctx, int slot, mh_object* objects_host, int max_objects, int32_t* n_objects,
                        int32_t* counts) {
  if (!ctx || !n_objects || !ctx->fs || slot < 0 || slot >= MH_MAX_BATCH) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  FrameState* fs = ctx->fs;
  const unsigned char* result = fs->result + (size_t)slot * fs->result_bytes;
  FrameState::FetchPin& pin = *fs->fetch_pin;
  const size_t first = std::min(fs->result_bytes, sizeof pin.head + sizeof pin.objects);
  MH_HIP(ctx, hipMemcpyAsync(pin.head, result, first, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(pin.snap, fs->snap + 4 * slot, sizeof pin.snap, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return read_out(ctx, pin.head, pin.snap, pin.head[1], pin.objects, FETCH_PIN_OBJECTS, result, objects_host, max_objects,
                  n_objects, counts);
}

int mh_frame_result_copy_slots_dev(mh_ctx* ctx, void* dst_dev, int n_slots, int max_objects) {
  if (!ctx || !dst_dev || max_objects < 0 || n_slots <= 0 || n_slots > MH_MAX_BATCH) return MH_ERR_ARG;
  size_t bytes = 0;
  if (int rc = result_copy_bytes(ctx, max_objects, &bytes)) return rc;
  MH_HIP(ctx, hipMemcpy2DAsync(dst_dev, bytes, ctx->fs->result, ctx->fs->result_bytes, bytes, (size_t)n_slots,
                               hipMemcpyDeviceToDevice, ctx->stream));
  return MH_OK;
}

int mh_frame_result_copy_dev(mh_ctx* ctx, void* dst_dev, int max_objects) {
  if (!ctx || !dst_dev || max_objects < 0) return MH_ERR_ARG;
  size_t bytes = 0;
  if (int rc = result_copy_bytes(ctx, max_objects, &bytes)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(dst_dev, ctx->fs->result, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return MH_OK;
}

int mh_frame_fetch_matches_slot(mh_ctx* ctx, int slot, int32_t* query_host, int32_t* model_host, int cap,
                                int32_t* n_matches) {
  if (!ctx || !ctx->fs || !n_matches || cap < 0 || slot < 0 || slot >= MH_MAX_BATCH) return MH_ERR_ARG;
  size_t a = 0;
  int take = 0;
  if (int rc = match_lists(ctx, "mh_frame_fetch_matches_slot", slot, cap, n_matches, &a, &take)) return rc;
  const FrameState* fs = ctx->fs;
  if (take > 0 && query_host)
    MH_HIP(ctx, hipMemcpy(query_host, reinterpret_cast<const unsigned char*>(fs->m_q) + a, sizeof(int32_t) * (size_t)take,
                          hipMemcpyDeviceToHost));
  if (take > 0 && model_host)
    MH_HIP(ctx, hipMemcpy(model_host, reinterpret_cast<const unsigned char*>(fs->m_model) + a, sizeof(int32_t) * (size_t)take,
                          hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_frame_fetch_match_reps_slot(mh_ctx* ctx, int slot, int32_t* rep_host, int cap, int32_t* n_matches) {
  if (!ctx || !ctx->fs || !n_matches || cap < 0 || (cap > 0 && !rep_host) || slot < -1 || slot >= MH_MAX_BATCH)
    return MH_ERR_ARG;
  size_t a = 0;
  int take = 0;   // (slot -1: the last frame, mh_frame_fetch_matches' lists)
  if (int rc = match_lists(ctx, "mh_frame_fetch_match_reps_slot", slot, cap, n_matches, &a, &take)) return rc;
  if (take > 0)
    MH_HIP(ctx, hipMemcpy(rep_host, reinterpret_cast<const unsigned char*>(ctx->fs->m_rep) + a, sizeof(int32_t) * (size_t)take,
                          hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_frame_fetch_match_points(mh_ctx* ctx, mh_corr* corr_host, int cap, int32_t* n_matches) {
  if (!ctx || !ctx->fs || !n_matches || cap < 0 || (cap > 0 && !corr_host)) return MH_ERR_ARG;
  size_t a = 0;
  int take = 0;
  if (int rc = match_lists(ctx, "mh_frame_fetch_match_points", -1, cap, n_matches, &a, &take)) return rc;
  if (take > 0)
    MH_HIP(ctx, hipMemcpy(corr_host, reinterpret_cast<const unsigned char*>(ctx->fs->m_corr) + a, sizeof(mh_corr) * (size_t)take,
                          hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_depth_rules_debug_fetch(mh_ctx* ctx, int which, int slot, void* out_host, size_t bytes) {
  static const char* const who = "mh_depth_rules_debug_fetch";
  if (!ctx || which < 0 || which > 2 || slot < 0 || slot >= MH_MAX_BATCH || (bytes > 0 && !out_host)) return MH_ERR_ARG;
  auto refuse = [&](const char* why) {
    ctx->err = std::string(who) + ": " + why;
    return MH_ERR_ARG;
  };
  const mh_ctx::DepthRuleState& rs = ctx->rules;
  if (which == 2) {
    if (!ctx->fs || !rs.last.depth) return refuse("the last frame carried no depth attributes");
    size_t a = 0;
    int take = 0;
    int32_t n = 0;
    if (int rc = match_lists(ctx, who, slot, INT_MAX, &n, &a, &take)) return rc;
    if (bytes != sizeof(mh_depth) * (size_t)n) return refuse("bytes is not the frame's match count times sizeof(mh_depth)");
    if (n > 0)
      MH_HIP(ctx, hipMemcpy(out_host, reinterpret_cast<const unsigned char*>(ctx->fs->m_depth) + a, bytes, hipMemcpyDeviceToHost));
    return MH_OK;
  }
  const int f = slot - rs.last.first;
  if (f < 0 || f >= rs.last.frames) return refuse("no depth rules ran on that frame (or its maps have been overwritten)");
  if (which == 0 ? !rs.last.inv : !rs.last.keep) return refuse("the last frame's rules did not write that array");
  const size_t extent = which == 0 ? sizeof(double) * (size_t)rs.last.patches : (size_t)rs.last.q;
  if (bytes != extent) return refuse("bytes is not the array's size (0: 8 pw ph, 1: Q)");
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const void* src = which == 0 ? static_cast<const void*>(rs.inv_size + (size_t)f * rs.last.patches)
                               : static_cast<const void*>(rs.keep1 + (size_t)f * rs.last.q);
  if (bytes > 0) MH_HIP(ctx, hipMemcpy(out_host, src, bytes, hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_frame_debug_fetch_clusters_slot(mh_ctx* ctx, int slot, int32_t* cl_model_host, int32_t* cl_off_host,
                                       int32_t* members_host, int cap_clusters, int cap_members, int32_t* n_clusters) {
  static const char* const who = "mh_frame_debug_fetch_clusters_slot";
  if (!ctx || !ctx->fs || !n_clusters || cap_clusters < 0 || cap_members < 0 || slot < 0 || slot >= MH_MAX_BATCH)
    return MH_ERR_ARG;
  *n_clusters = 0;
  size_t a = 0;
  int take = 0;
  int32_t M = 0;
  if (int rc = match_lists(ctx, who, slot, INT_MAX, &M, &a, &take)) return rc;
  const FrameState* fs = ctx->fs;
  // a frame with several images: the clusterer's "models" were the (model, image) pairs, their lists off2 over mi_corr
  const int pairs = fs->list_pairs > 1 ? fs->list_pairs : 1;
  const int nm = ctx->n_models * pairs;
  if (M < 0 || M > fs->max_m || nm > fs->n_models_cap) {
    ctx->err = std::string(who) + ": inconsistent match count";
    return MH_ERR_HIP;
  }
  // the per-model lists as the clusterers write them (steps.h: members / cl_start / ncl of launch_meanshift_models)
  std::vector<int32_t> off(nm + 1), ncl(nm + 1), start((size_t)M + nm + 1), mem(std::max(M, 1));
  auto get = [&](std::vector<int32_t>& to, const int32_t* from, size_t n) {
    return hipMemcpy(to.data(), reinterpret_cast<const unsigned char*>(from) + a, n * sizeof(int32_t), hipMemcpyDeviceToHost);
  };
  MH_HIP(ctx, get(off, pairs > 1 ? fs->off2 : fs->model_off, (size_t)nm + 1));
  MH_HIP(ctx, get(ncl, fs->ms_ncl, (size_t)nm));
  MH_HIP(ctx, get(start, fs->ms_cl_start, (size_t)M + nm + 1));
  // (the weighted mean shift: model m's members at factor x off[m] of the context's buffer, up to factor x its matches)
  const int fct = fs->list_wms ? WMS_MEMBER_FACTOR : 1;
  if (fs->list_wms) {
    if (pairs > 1 || !ctx->wms_members || ctx->wms_members.cap < (size_t)fct * M) {
      ctx->err = std::string(who) + ": inconsistent member buffer";
      return MH_ERR_HIP;
    }
    mem.resize((size_t)fct * std::max(M, 1));
    if (M > 0) MH_HIP(ctx, hipMemcpy(mem.data(), ctx->wms_members.p, (size_t)fct * M * sizeof(int32_t), hipMemcpyDeviceToHost));
  } else if (M > 0) MH_HIP(ctx, get(mem, fs->ms_members, (size_t)M));
  int n = 0, w = 0;
  for (int m = 0; m < nm; ++m) {
    const int b = off[m], k = off[m + 1] - b;
    if (b < 0 || k < 0 || b + k > M || ncl[m] < 0 || ncl[m] > k) {
      ctx->err = std::string(who) + ": inconsistent cluster lists";
      return MH_ERR_HIP;
    }
    const int32_t* st = start.data() + b + m;
    for (int c = 0; c < ncl[m]; ++c, ++n) {
      if (st[c] < 0 || st[c + 1] < st[c] || st[c + 1] > fct * k) {
        ctx->err = std::string(who) + ": inconsistent cluster lists";
        return MH_ERR_HIP;
      }
      if (n < cap_clusters) {
        if (cl_model_host) cl_model_host[n] = m / pairs;
        if (cl_off_host) cl_off_host[n] = w;
      }
      for (int j = st[c]; j < st[c + 1]; ++j, ++w)
        if (members_host && w < cap_members) members_host[w] = mem[(size_t)fct * b + j] - b;   // index inside the model's match list
    }
  }
  if (cl_off_host && n <= cap_clusters) cl_off_host[n] = w;
  *n_clusters = n;
  if (n > cap_clusters || w > cap_members) {
    ctx->err = std::string(who) + ": more clusters or members than the caller's buffers hold";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_frame_debug_fetch_cluster_table_slot(mh_ctx* ctx, int slot, int32_t* cl_model_host, int32_t* cl_begin_host,
                                            int32_t* cl_count_host, int cap_clusters, int32_t* n_clusters,
                                            int32_t* n_clusters_now) {
  static const char* const who = "mh_frame_debug_fetch_cluster_table_slot";
  if (!ctx || !ctx->fs || !n_clusters || cap_clusters < 0 || slot < 0 || slot >= MH_MAX_BATCH) return MH_ERR_ARG;
  *n_clusters = 0;
  if (n_clusters_now) *n_clusters_now = 0;
  size_t a = 0;
  int take = 0;
  int32_t M = 0;
  if (int rc = match_lists(ctx, who, slot, INT_MAX, &M, &a, &take)) return rc;   // (the stream is through with the frame)
  const FrameState* fs = ctx->fs;
  auto at = [a](const void* p) { return reinterpret_cast<const unsigned char*>(p) + a; };
  FrameCounts fc;
  int32_t now = 0;
  MH_HIP(ctx, hipMemcpy(&fc, at(fs->counts), sizeof fc, hipMemcpyDeviceToHost));
  MH_HIP(ctx, hipMemcpy(&now, at(fs->n_clusters), sizeof now, hipMemcpyDeviceToHost));
  const int n = fc.n_clusters;
  if (n < 0 || n > fs->max_clusters) {
    ctx->err = std::string(who) + ": inconsistent cluster count";
    return MH_ERR_HIP;
  }
  *n_clusters = n;
  if (n_clusters_now) *n_clusters_now = now;
  const size_t bytes = sizeof(int32_t) * (size_t)std::min(n, cap_clusters);
  if (bytes > 0 && cl_model_host) MH_HIP(ctx, hipMemcpy(cl_model_host, at(fs->cl_model), bytes, hipMemcpyDeviceToHost));
  if (bytes > 0 && cl_begin_host) MH_HIP(ctx, hipMemcpy(cl_begin_host, at(fs->cl_begin), bytes, hipMemcpyDeviceToHost));
  if (bytes > 0 && cl_count_host) MH_HIP(ctx, hipMemcpy(cl_count_host, at(fs->cl_count), bytes, hipMemcpyDeviceToHost));
  if (n > cap_clusters) {
    ctx->err = std::string(who) + ": more clusters than the caller's buffers hold";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_frame_fetch_matches(mh_ctx* ctx, int32_t* query_host, int32_t* model_host, int cap, int32_t* n_matches) {
  if (!ctx || !ctx->fs) return MH_ERR_ARG;
  return mh_frame_fetch_matches_slot(ctx, ctx->fs->list_first + ctx->fs->list_n - 1, query_host, model_host, cap, n_matches);
}

int mh_frame_result_dev(mh_ctx* ctx, void** block_dev, int64_t* bytes) {
  if (!ctx || !ctx->fs || !block_dev || !bytes) return MH_ERR_ARG;
  *block_dev = ctx->fs->result;
  *bytes = (int64_t)ctx->fs->result_bytes;
  return MH_OK;
}

int mh_frame_counters(mh_ctx* ctx, int32_t out[8]) {
  if (!ctx || !out || !ctx->fs) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  static_assert(sizeof(FrameCounts) == 8 * sizeof(int32_t), "mh_frame_counters hands the block out as 8 words");
  MH_HIP(ctx, hipMemcpyAsync(out, ctx->fs->counts, sizeof(FrameCounts), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_pose_kernel_info(mh_ctx* ctx, int kind, int32_t out[8]) {
  if (!ctx || !out || kind < 0 || kind > 3) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  return pose_kernel_info(kind, out);
}

int mh_timing(mh_ctx* ctx, mh_times* out) {
  if (!ctx || !out || !ctx->timing || !ctx->ev_made) return MH_ERR_ARG;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  MH_HIP(ctx, hipEventSynchronize(ctx->ev[8]));
  float* dst[8] = {&out->match_ms, &out->group_ms, &out->cluster_ms, &out->pose1_ms,
                   &out->filter1_ms, &out->pose2_ms, &out->filter2_ms, nullptr};
  for (int i = 0; i < 7; ++i) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]);
    *dst[i] = ms;
  }
  float tot = 0.f;
  hipEventElapsedTime(&tot, ctx->ev[0], ctx->ev[8]);
  out->total_ms = tot;
  return MH_OK;
}

}  // extern "C"
