// C ABI: mh_step_*, the per-step plugins' hand-over.
#include <cstring>

#include "frame.h"

using namespace mh;

// ---- the frame's six slots ONE CALL EACH on a frame that stays on the device between them -----------------------------
// The per-step plugins' hand-over (moped_amd/host/hip_session.hpp, HipHandover): MATCH leaves the frame's lists in the
// context's working arrays, CLUSTER clusters them where they lie, POSE poses those clusters, FILTER filters those
// objects ... -- every call launches its slot's kernels behind the previous call's (frame_rest with a stage range),
// copies what the slot's contract says the host's FrameData must hold into page-locked memory, and waits once.  What
// the steps uploaded again and again before (the match list three times, the objects twice, ~25 small copies per
// FILTER) stays where it is.  ctx->step says where the resident frame stands; a call out of order, or after anything
// else has used the context's working arrays, is refused (MH_ERR_ARG) and the plugin takes its upload path.
namespace {

int step_refuse(mh_ctx* ctx, const char* who) {
  ctx->err = std::string(who) + ": the resident frame is not at the stage before this one (the steps must run in pipeline "
             "order on one frame; any other call that uses the frame's working arrays ends the hand-over)";
  return MH_ERR_ARG;
}

int step_flags(mh_ctx* ctx, const FrameCounts& fc, const char* who) {
  if (!fc.error) return MH_OK;
  ctx->step.done = -1;
  ctx->err = std::string(who) + ": capacity exceeded (flags " + std::to_string(fc.error) + ")";
  return MH_ERR_CAPACITY;
}

// An error behind a stage's launch: the frame may no longer be where `done` said, the hand-over ends.
int step_fail(mh_ctx* ctx, int rc) {
  if (rc) ctx->step.done = -1;
  return rc;
}

// one stage of the resident frame
int step_stage(mh_ctx* ctx, const mh_frame_params* prm, uint64_t seed, int stage) {
  FrameCall c{ctx->q_uv, ctx->step.Q, &ctx->step.cam, prm, seed};
  c.stage_lo = c.stage_hi = stage;
  return step_fail(ctx, frame_rest(ctx, c));
}

// A stage's results -- a handful of short arrays -- go to the host by ONE kernel that writes them into the context's
// page-locked block, one after the other, and one stream synchronisation: six stream-ordered copies of a few hundred
// bytes each were 40-60 us of every stepped slot (each a transfer of its own behind the stage's kernel).
constexpr int GATHER_SEGS = 8;
struct GatherArgs {
  const uint32_t* src[GATHER_SEGS];
  uint32_t words[GATHER_SEGS], dst_word[GATHER_SEGS];
  int n;
};
__global__ void __launch_bounds__(256) step_gather_kernel(GatherArgs a, uint32_t* __restrict__ dst) {
  for (int k = 0; k < a.n; ++k) {
    const uint32_t* __restrict__ src = a.src[k];
    uint32_t* out = dst + a.dst_word[k];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.words[k]; i += gridDim.x * blockDim.x) out[i] = src[i];
  }
}
struct PinCursor {
  unsigned char* base;
  size_t off = 0;
  GatherArgs g = {};
  bool overflow = false;   // more arrays asked for than GatherArgs holds: run() reports it
  // n elements of T that the gather kernel fills from device array `src` (4-byte aligned, like every array of the frame)
  template <typename T> T* take(size_t n, const void* src) {
    T* p = reinterpret_cast<T*>(base + off);
    if (src && n > 0 && g.n == GATHER_SEGS) overflow = true;
    else if (src && n > 0) {
      g.src[g.n] = static_cast<const uint32_t*>(src);
      g.words[g.n] = (uint32_t)((n * sizeof(T) + 3) / 4);
      g.dst_word[g.n] = (uint32_t)(off / 4);
      ++g.n;
    }
    off += (n * sizeof(T) + 15) & ~(size_t)15;
    return p;
  }
  int run(mh_ctx* ctx) {   // behind the stage's kernels on the context's stream; returns when the block is filled
    if (overflow) {
      ctx->err = "step hand-over: more arrays in one gather than GATHER_SEGS";
      return MH_ERR_CAPACITY;
    }
    size_t total = 0;
    for (int k = 0; k < g.n; ++k) total += g.words[k];
    const unsigned blocks = (unsigned)std::min<size_t>(64, std::max<size_t>(1, total / 1024));
    hipLaunchKernelGGL(step_gather_kernel, dim3(blocks), dim3(256), 0, ctx->stream, g, reinterpret_cast<uint32_t*>(base));
    MH_HIP(ctx, hipGetLastError());
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MH_OK;
  }
};

// The depth map a stand-alone depth step reads: the caller's host map through the context's own buffers, or (NULL) the
// map the context holds.  The own buffers may be the frame's map (mh_frame_set_depth_image_host): overwritten, it is off.
int step_depth_map(mh_ctx* ctx, const char* who, const float* depth_host, const float* fill_host, int width, int height,
                   DepthImage* out) {
  if (!depth_host) {
    if (!ctx->depth_img.img) {
      ctx->err = std::string(who) + ": no depth map (hand one in, or mh_frame_set_depth_image[_host] first)";
      return MH_ERR_ARG;
    }
    *out = ctx->depth_img;
    return MH_OK;
  }
  if (width <= 0 || height <= 0) {
    ctx->err = std::string(who) + ": bad argument";
    return MH_ERR_ARG;
  }
  if (ctx->depth_img.img && ctx->own_depth && reinterpret_cast<const float*>(ctx->depth_img.img) == ctx->own_depth.p)
    mh_frame_set_depth_image(ctx, nullptr, nullptr, 0, 0, 0, ctx->depth_alpha, 0.f);
  const size_t px = (size_t)width * height;
  if (int rc = ensure_own_depth(ctx, px)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_depth, depth_host, px * 4 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (fill_host)
    MH_HIP(ctx, hipMemcpyAsync(ctx->own_fill, fill_host, px * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  *out = DepthImage{};
  out->img = reinterpret_cast<const float4*>(ctx->own_depth.p);
  out->fill = fill_host ? ctx->own_fill.p : nullptr;
  out->w = width;
  out->h = height;
  return MH_OK;
}

// What a Kinect frame does once its gray image is in own_gray and its map in own_depth (mh_frame_run_kinect_host,
// mh_frame_run_kinect_raw_host): DEPTHFILL (fill_scale != 0) or the host's distance map (fill_in_host, or none), the maps
// set, the image enqueued, the maps as the frame used them copied back where asked (depth_out_host; fill_out_host, which
// a caller passes only with a fill), the objects fetched.
int kinect_frame_tail(mh_ctx* ctx, const char* who, const float* fill_in_host, float* depth_out_host, float* fill_out_host,
                      int width, int height, int double_size, int max_keypoints, const mh_cam* cam,
                      const mh_frame_params* prm, int fill_scale, int bilinear, int kind, float alpha, float cauchy_scale,
                      uint64_t seed, mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts) {
  hipStream_t s = ctx->stream;
  const size_t px = (size_t)width * height;
  const bool fill = fill_scale != 0;
  const bool have_fill = fill || fill_in_host;
  if (fill) {
    if (int rc = mh_depth_fill(ctx, ctx->own_depth, width, height, fill_scale, bilinear, cam->K, ctx->own_fill, nullptr)) return rc;
  } else if (fill_in_host) {
    MH_HIP(ctx, hipMemcpyAsync(ctx->own_fill, fill_in_host, px * sizeof(float), hipMemcpyHostToDevice, s));
  }
  if (int rc = mh_frame_set_depth_image(ctx, ctx->own_depth, have_fill ? ctx->own_fill.p : nullptr, width, height, kind,
                                        alpha, cauchy_scale)) {
    ctx->err = std::string(who) + ": kind must be MH_DEPTH_BACKPROJECTION or MH_DEPTH_REPROJECTION, cauchy_scale > 0";
    return rc;
  }
  if (int rc = mh_frame_enqueue_image(ctx, ctx->own_gray, width, height, double_size, max_keypoints, cam, prm, seed)) return rc;
  // the frame's images as DEPTH_FILL_EXACT_CPU::process leaves them, behind the frame's launches
  if (depth_out_host)
    MH_HIP(ctx, hipMemcpyAsync(depth_out_host, ctx->own_depth, px * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
  if (fill_out_host)
    MH_HIP(ctx, hipMemcpyAsync(fill_out_host, ctx->own_fill, px * sizeof(float), hipMemcpyDeviceToHost, s));
  const int rc = mh_frame_fetch(ctx, objects_host, max_objects, n_objects, counts);
  const int rc_fill = fill ? mh_depth_fill_status(ctx) : MH_OK;
  return rc ? rc : rc_fill;
}

}  // namespace
extern "C" {

// ---- moped3d's DEPTHFILTER / DEPTHFILTER2 / DEPTHPROP slots as steps of their own (kernels: depth.hip) ------------------
int mh_depth_filter(mh_ctx* ctx, const float* depth_xyzn_host, int width, int height, const float K[4], int patch_size,
                    float density, const float* uv_host, const int32_t* group_off_host, int n_groups, uint8_t* keep_host) {
  if (!ctx) return MH_ERR_ARG;
  if (!K || patch_size <= 0 || n_groups < 0 || (n_groups > 0 && !group_off_host)) {
    ctx->err = "mh_depth_filter: bad argument";
    return MH_ERR_ARG;
  }
  if (n_groups == 0) return MH_OK;
  for (int g = 0; g < n_groups; ++g)
    if (group_off_host[0] != 0 || group_off_host[g + 1] < group_off_host[g]) {
      ctx->err = "mh_depth_filter: offsets must start at 0 and not decrease";
      return MH_ERR_ARG;
    }
  const int n = group_off_host[n_groups];
  if (n == 0) return MH_OK;
  if (!uv_host || !keep_host) {
    ctx->err = "mh_depth_filter: bad argument";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  DepthImage dimg;
  if (int rc = step_depth_map(ctx, "mh_depth_filter", depth_xyzn_host, nullptr, width, height, &dimg)) return rc;
  const int pw = (dimg.w + patch_size - 1) / patch_size, ph = (dimg.h + patch_size - 1) / patch_size;
  const size_t P = (size_t)pw * ph;
  if (P > (size_t)depth_filter_max_patches()) {
    ctx->err = "mh_depth_filter: more than 4096 patches (raise PatchSize)";
    return MH_ERR_CAPACITY;
  }
  // device layout: inv_size (double) | uv | group_off | keep
  const size_t b_inv = P * sizeof(double), b_uv = (size_t)n * 2 * sizeof(float);
  const size_t b_off = (((size_t)n_groups + 1) * sizeof(int32_t) + 15) & ~(size_t)15;
  if (int rc = ensure_scratch(ctx, b_inv + b_uv + b_off + (size_t)n + 64)) return rc;
  if (int rc = ensure_pinned(ctx, (size_t)n)) return rc;
  unsigned char* base = ctx->scratch;
  double* d_inv = reinterpret_cast<double*>(base);
  float* d_uv = reinterpret_cast<float*>(base + b_inv);
  int32_t* d_off = reinterpret_cast<int32_t*>(base + b_inv + b_uv);
  uint8_t* d_keep = base + b_inv + b_uv + b_off;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(d_uv, uv_host, b_uv, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_off, group_off_host, ((size_t)n_groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  launch_depth_patches(dimg, K, patch_size, d_inv, s);
  // `Float filter = Density*100*100` (DEPTHFILTER_CPU.hpp:130)
  launch_group_density(d_uv, d_off, n_groups, patch_size, pw, ph, d_inv, density * 100 * 100, d_keep, s);
  MH_HIP(ctx, hipGetLastError());
  MH_HIP(ctx, hipMemcpyAsync(ctx->pinned.p, d_keep, (size_t)n, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  std::memcpy(keep_host, ctx->pinned.p, (size_t)n);
  return MH_OK;
}

int mh_depth_prop(mh_ctx* ctx, const float* depth_xyzn_host, const float* fill_distance_host, int width, int height,
                  const float* uv_host, int n, mh_depth_info* out_host) {
  if (!ctx) return MH_ERR_ARG;
  if (n < 0 || (n > 0 && (!uv_host || !out_host))) {
    ctx->err = "mh_depth_prop: bad argument";
    return MH_ERR_ARG;
  }
  if (n == 0) return MH_OK;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  DepthImage dimg;
  if (int rc = step_depth_map(ctx, "mh_depth_prop", depth_xyzn_host, fill_distance_host, width, height, &dimg)) return rc;
  const size_t b_uv = ((size_t)n * 2 * sizeof(float) + 15) & ~(size_t)15, b_out = (size_t)n * sizeof(mh_depth_info);
  if (int rc = ensure_scratch(ctx, b_uv + b_out + 64)) return rc;
  if (int rc = ensure_pinned(ctx, b_out)) return rc;
  float* d_uv = reinterpret_cast<float*>(ctx->scratch.p);
  mh_depth_info* d_out = reinterpret_cast<mh_depth_info*>(ctx->scratch.p + b_uv);
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(d_uv, uv_host, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, s));
  launch_depth_prop(dimg, d_uv, n, d_out, s);
  MH_HIP(ctx, hipGetLastError());
  MH_HIP(ctx, hipMemcpyAsync(ctx->pinned.p, d_out, b_out, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  std::memcpy(out_host, ctx->pinned.p, b_out);
  return MH_OK;
}

// ---- moped3d's Kinect frame in one call: the composition of mh_depth_fill, mh_frame_set_depth_image, --------------------
// mh_frame_enqueue_image and mh_frame_fetch over context-owned copies of the host's image and maps (no kernel of its own)
int mh_frame_run_kinect_host(mh_ctx* ctx, const uint8_t* gray_host, float* depth_xyzn_host, float* fill_distance_host,
                             int width, int height, int double_size, int max_keypoints, const mh_cam* cam,
                             const mh_frame_params* prm, int fill_scale, int bilinear, int kind, float alpha,
                             float cauchy_scale, uint64_t seed, mh_object* objects_host, int max_objects,
                             int32_t* n_objects, int32_t* counts) {
  if (!ctx) return MH_ERR_ARG;
  const bool fill = fill_scale != 0;
  if (!gray_host || !depth_xyzn_host || (fill && !fill_distance_host) || width <= 0 || height <= 0 || max_keypoints <= 0 ||
      !cam || !prm || !n_objects || (fill_scale < 1 && fill_scale != 0 && fill_scale != -1)) {
    ctx->err = "mh_frame_run_kinect_host: bad argument";
    return MH_ERR_ARG;
  }
  *n_objects = 0;
  if (int rc_if = image_format_frame_ok(ctx, "mh_frame_run_kinect_host", width, height)) return rc_if;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  hipStream_t s = ctx->stream;
  const size_t px = (size_t)width * height;
  const size_t image_bytes = image_format_bytes(ctx, width, height);   // (mh_frame_set_image_format: the raw extent)
  mh_frame_set_depth_image(ctx, nullptr, nullptr, 0, 0, 0, alpha, 0.f);   // (the own buffers may move)
  if (int rc = ensure_own_depth(ctx, px)) return rc;
  MH_HIP(ctx, ctx->own_gray.ensure(image_bytes, s));
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_gray, gray_host, image_bytes, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_depth, depth_xyzn_host, px * 4 * sizeof(float), hipMemcpyHostToDevice, s));
  return kinect_frame_tail(ctx, "mh_frame_run_kinect_host", fill ? nullptr : fill_distance_host, fill ? depth_xyzn_host : nullptr,
                           fill ? fill_distance_host : nullptr, width, height, double_size, max_keypoints, cam, prm,
                           fill_scale, bilinear, kind, alpha, cauchy_scale, seed, objects_host, max_objects, n_objects, counts);
}

// ... and from what the sensor delivers: the raw depth goes up instead of the map, depthmap.hip builds the map into
// own_depth (moped3d/moped3d.cpp:279-333), the tail is the same
int mh_frame_run_kinect_raw_host(mh_ctx* ctx, const uint8_t* gray_host, const void* raw_host, const mh_raw_depth* raw,
                                 float* depth_xyzn_host, float* fill_distance_host, int width, int height,
                                 int double_size, int max_keypoints, const mh_cam* cam, const mh_frame_params* prm,
                                 int fill_scale, int bilinear, int kind, float alpha, float cauchy_scale, uint64_t seed,
                                 mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts) {
  if (!ctx) return MH_ERR_ARG;
  const bool fill = fill_scale != 0;
  if (!gray_host || !raw_host || !raw || width <= 0 || height <= 0 || max_keypoints <= 0 || !cam || !prm || !n_objects ||
      (fill_scale < 1 && fill_scale != 0 && fill_scale != -1)) {
    ctx->err = "mh_frame_run_kinect_raw_host: bad argument";
    return MH_ERR_ARG;
  }
  *n_objects = 0;
  if (int rc_if = image_format_frame_ok(ctx, "mh_frame_run_kinect_raw_host", width, height)) return rc_if;
  mh_frame_set_depth_image(ctx, nullptr, nullptr, 0, 0, 0, alpha, 0.f);   // (the own buffers may move)
  if (int rc = depth_map_from_raw_own(ctx, "mh_frame_run_kinect_raw_host", raw_host, raw, cam->K, width, height)) return rc;
  hipStream_t s = ctx->stream;
  const size_t image_bytes = image_format_bytes(ctx, width, height);   // (mh_frame_set_image_format: the raw extent)
  MH_HIP(ctx, ctx->own_gray.ensure(image_bytes, s));
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_gray, gray_host, image_bytes, hipMemcpyHostToDevice, s));
  return kinect_frame_tail(ctx, "mh_frame_run_kinect_raw_host", nullptr, depth_xyzn_host, fill ? fill_distance_host : nullptr,
                           width, height, double_size, max_keypoints, cam, prm, fill_scale, bilinear, kind, alpha,
                           cauchy_scale, seed, objects_host, max_objects, n_objects, counts);
}

int mh_step_match(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, int Q, const mh_cam* cam, float ratio,
                  int write_back) {
  if (!ctx || Q <= 0 || !q_desc_host || !q_uv_host || !cam) {
    if (ctx) ctx->err = "mh_step_match: bad argument";
    return MH_ERR_ARG;
  }
  mh_frame_params p;
  mh_frame_default_params(&p);
  p.ratio = ratio;
  // the whole frame's upload and MATCH, of the rest chain only MATCH's tail
  if (int rc = host_frame_begin(ctx, q_desc_host, q_uv_host, nullptr, Q, cam, 1, &p, 0, FeatureOptions{0, 0, write_back != 0}))
    return rc;
  mh_ctx::StepState& st = ctx->step;
  st.done = 0;
  st.Q = Q;
  st.M = -1;   // (known once mh_step_match_fetch has run)
  st.n_clusters = st.n_slots = 0;
  st.cam = *cam;
  st.valid.clear();
  st.valid_model.clear();
  return MH_OK;
}

int mh_step_match_fetch(mh_ctx* ctx, int32_t* model_off_host, int32_t* match_query, mh_corr* match_pts, int cap,
                        int32_t* n_matches) {
  if (!ctx || !n_matches || cap < 0 || (cap > 0 && (!match_query || !match_pts))) return MH_ERR_ARG;
  *n_matches = 0;
  if (!ctx->fs || ctx->step.done != 0) return step_refuse(ctx, "mh_step_match_fetch");
  MH_HIP(ctx, hipSetDevice(ctx->device));
  mh_ctx::StepState& st = ctx->step;
  FrameState* fs = ctx->fs;
  const int nm = ctx->n_models, take = std::min(st.Q, fs->max_m);   // (a frame accepts at most one match per query)
  if (int rc = ensure_pinned(ctx, 64 + (size_t)(nm + 1 + take) * 4 + (size_t)take * sizeof(mh_corr) + 64)) return rc;
  PinCursor pc{ctx->pinned};
  FrameCounts* fc = pc.take<FrameCounts>(1, fs->counts);
  int32_t* off = pc.take<int32_t>(nm + 1, fs->model_off);
  int32_t* mq = pc.take<int32_t>(take, fs->m_q);
  mh_corr* mc = pc.take<mh_corr>(take, fs->m_corr);
  if (int rc = pc.run(ctx)) return rc;
  if (int rc = step_flags(ctx, *fc, "mh_step_match_fetch")) return rc;
  const int M = off[nm];
  if (M < 0 || M > take) {
    st.done = -1;
    ctx->err = "mh_step_match_fetch: inconsistent match count";
    return MH_ERR_HIP;
  }
  st.M = M;
  st.model_off.assign(off, off + nm + 1);
  *n_matches = M;
  if (model_off_host) std::memcpy(model_off_host, off, (size_t)(nm + 1) * 4);
  const int give = std::min(M, cap);
  if (give > 0) {
    std::memcpy(match_query, mq, (size_t)give * 4);
    std::memcpy(match_pts, mc, (size_t)give * sizeof(mh_corr));
  }
  if (M > cap) {   // (the first `cap` are written, the resident frame stays valid: a larger buffer can fetch again)
    ctx->err = "mh_step_match_fetch: more matches than the caller's buffers hold (cap >= Q always suffices)";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_step_cluster(mh_ctx* ctx, float radius, float merge, int min_pts, int max_iter, int32_t* cl_model_host,
                    int32_t* cl_off_host, int32_t* members_host, int cap_clusters, int cap_members, int32_t* n_clusters) {
  if (!ctx || !n_clusters || cap_clusters < 0 || cap_members < 0) return MH_ERR_ARG;
  *n_clusters = 0;
  mh_ctx::StepState& st = ctx->step;
  if (!ctx->fs || st.done != 0 || st.M < 0) return step_refuse(ctx, "mh_step_cluster");
  MH_HIP(ctx, hipSetDevice(ctx->device));
  FrameState* fs = ctx->fs;
  mh_frame_params p;
  mh_frame_default_params(&p);
  p.ms_radius = radius;
  p.ms_merge = merge;
  p.ms_min_pts = min_pts;
  p.ms_max_iter = max_iter;
  // (the page-locked block before the launch: nothing that can fail without a launch comes after it)
  const int M = st.M, tab = std::min(fs->max_clusters, std::max(M, 1));
  if (int rc = ensure_pinned(ctx, 256 + (size_t)(3 * tab + std::max(M, 1)) * 4)) return rc;
  if (int rc = step_stage(ctx, &p, 0, 1)) return rc;
  PinCursor pc{ctx->pinned};
  FrameCounts* fc = pc.take<FrameCounts>(1, fs->counts);
  int32_t* ncl = pc.take<int32_t>(1, fs->n_clusters);
  int32_t* cm = pc.take<int32_t>(tab, fs->cl_model);
  int32_t* cb = pc.take<int32_t>(tab, fs->cl_begin);
  int32_t* cc = pc.take<int32_t>(tab, fs->cl_count);
  int32_t* mem = pc.take<int32_t>(std::max(M, 1), M > 0 ? fs->ms_members : nullptr);
  if (int rc = pc.run(ctx)) return step_fail(ctx, rc);
  if (int rc = step_flags(ctx, *fc, "mh_step_cluster")) return rc;
  const int n = *ncl;
  if (n < 0 || n > tab) {
    st.done = -1;
    ctx->err = "mh_step_cluster: inconsistent cluster count";
    return MH_ERR_HIP;
  }
  *n_clusters = n;
  int w = 0;
  for (int c = 0; c < n; ++c) {
    const int model = cm[c], b = st.model_off[model];
    if (c < cap_clusters) {
      if (cl_model_host) cl_model_host[c] = model;
      if (cl_off_host) cl_off_host[c] = w;
    }
    for (int j = 0; j < cc[c]; ++j, ++w)
      if (members_host && w < cap_members) members_host[w] = mem[cb[c] + j] - b;   // index inside the model's match list
  }
  if (cl_off_host && n <= cap_clusters) cl_off_host[n] = w;
  st.n_clusters = n;
  st.done = 1;
  return (n > cap_clusters || w > cap_members) ? MH_ERR_CAPACITY : MH_OK;
}

int mh_step_pose(mh_ctx* ctx, int which, const mh_pose_params* prm, uint64_t seed, mh_step_object* out, int cap,
                 int32_t* n_out) {
  if (!ctx || !prm || !n_out || cap < 0 || (cap > 0 && !out) || (which != 1 && which != 2) ||
      prm->max_objects_per_cluster < 1)
    return MH_ERR_ARG;
  *n_out = 0;
  mh_ctx::StepState& st = ctx->step;
  if (!ctx->fs || st.done != (which == 1 ? 1 : 3)) return step_refuse(ctx, "mh_step_pose");
  MH_HIP(ctx, hipSetDevice(ctx->device));
  FrameState* fs = ctx->fs;
  const int stage = which == 1 ? 2 : 4;
  const int base = which == 1 ? 0 : st.n_slots, n_new = st.n_clusters * prm->max_objects_per_cluster;
  if (base + n_new > fs->max_objects) {
    ctx->err = "mh_step_pose: more (cluster, replica) tasks than object slots reserved";
    return MH_ERR_CAPACITY;
  }
  mh_frame_params p;
  mh_frame_default_params(&p);
  (which == 1 ? p.pose1 : p.pose2) = *prm;
  // (frame_rest keys POSE2's random streams with seed ^ 0x5DEECE66D: undone here, the caller's seed is the stage's)
  if (int rc = ensure_pinned(ctx, 256 + (size_t)std::max(n_new, 1) * (4 + 4 + 28))) return rc;
  if (int rc = step_stage(ctx, &p, which == 1 ? seed : seed ^ 0x5DEECE66Dull, stage)) return rc;
  PinCursor pc{ctx->pinned};
  FrameCounts* fc = pc.take<FrameCounts>(1, fs->counts);
  int32_t* valid = pc.take<int32_t>(n_new, fs->obj_valid + base);
  int32_t* model = pc.take<int32_t>(n_new, fs->obj_model + base);
  float* pose = pc.take<float>((size_t)7 * n_new, fs->obj_pose + (size_t)7 * base);
  if (int rc = pc.run(ctx)) return step_fail(ctx, rc);
  if (int rc = step_flags(ctx, *fc, "mh_step_pose")) return rc;
  if (which == 1) {
    st.valid.clear();
    st.valid_model.clear();
  }
  int k = 0;
  for (int o = 0; o < n_new; ++o) {
    if (!valid[o]) continue;
    st.valid.push_back(base + o);
    st.valid_model.push_back(model[o]);
    if (k < cap) {
      out[k].model = model[o];
      std::memcpy(out[k].pose, pose + (size_t)7 * o, 28);
    }
    ++k;
  }
  *n_out = k;
  st.n_slots = base + n_new;
  st.done = stage;
  return k > cap ? MH_ERR_CAPACITY : MH_OK;
}

int mh_step_filter(mh_ctx* ctx, int which, int min_points, float feature_distance, float min_score, int n_objects,
                   float* score, uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off, int cap_members,
                   int32_t* n_kept) {
  if (!ctx || !n_kept || n_objects < 0 || cap_members < 0 || (which != 1 && which != 2)) return MH_ERR_ARG;
  *n_kept = 0;
  if (cl_off) cl_off[0] = 0;
  mh_ctx::StepState& st = ctx->step;
  if (!ctx->fs || st.done != (which == 1 ? 2 : 4)) return step_refuse(ctx, "mh_step_filter");
  if (n_objects != (int)st.valid.size()) {
    st.done = -1;
    ctx->err = "mh_step_filter: the host's object list is not the one the device holds";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  FrameState* fs = ctx->fs;
  const int stage = which == 1 ? 3 : 5;
  mh_frame_params p;
  mh_frame_default_params(&p);
  if (which == 1) {
    p.f1_min_points = min_points;
    p.f1_feature_distance = feature_distance;
    p.f1_min_score = min_score;
  } else {
    p.f2_min_points = min_points;
    p.f2_feature_distance = feature_distance;
    p.f2_min_score = min_score;
  }
  const int nb = std::max(st.n_slots, 1), tab = std::min(nb, fs->max_clusters), M = std::max(st.M, 1);
  if (int rc = ensure_pinned(ctx, 512 + (size_t)(2 * nb + 2 * tab + M) * 4)) return rc;
  if (int rc = step_stage(ctx, &p, 0, stage)) return rc;
  PinCursor pc{ctx->pinned};
  FrameCounts* fc = pc.take<FrameCounts>(1, fs->counts);
  int32_t* kept_p = pc.take<int32_t>(1, fs->n_slots);
  float* sc = pc.take<float>(nb, fs->obj_score_raw);
  int32_t* old_of = pc.take<int32_t>(nb, fs->obj_clsize + fs->max_objects);
  int32_t* cb = pc.take<int32_t>(tab, fs->cl_begin);
  int32_t* cc = pc.take<int32_t>(tab, fs->cl_count);
  int32_t* mem = pc.take<int32_t>(M, st.M > 0 ? fs->new_members : nullptr);
  if (int rc = pc.run(ctx)) return step_fail(ctx, rc);
  if (int rc = step_flags(ctx, *fc, "mh_step_filter")) return rc;
  const int kept = *kept_p;
  if (kept < 0 || kept > n_objects || kept > tab) {
    st.done = -1;
    ctx->err = "mh_step_filter: inconsistent object count";
    return MH_ERR_HIP;
  }
  for (int i = 0; i < n_objects; ++i) {
    if (score) score[i] = sc[st.valid[i]];
    if (keep) keep[i] = 0;
  }
  std::vector<int32_t> new_model(kept);
  int w = 0;
  bool over = false;
  for (int k = 0; k < kept; ++k) {
    // kept object k sat in slot old_of[k]: the slots that held an object are in ascending order = the host's list order
    const int i = (int)(std::lower_bound(st.valid.begin(), st.valid.end(), old_of[k]) - st.valid.begin());
    if (i >= n_objects || st.valid[i] != old_of[k]) {
      st.done = -1;
      ctx->err = "mh_step_filter: a kept object does not come from a slot that held one";
      return MH_ERR_HIP;
    }
    const int model = st.valid_model[i], b = st.model_off[model];
    new_model[k] = model;
    if (keep) keep[i] = 1;
    if (out_order) out_order[k] = i;
    if (cl_off) cl_off[k] = w;
    for (int j = 0; j < cc[k]; ++j, ++w) {
      if (w >= cap_members) over = true;
      else if (cl_members) cl_members[w] = mem[cb[k] + j] - b;
    }
  }
  if (cl_off) cl_off[kept] = w;
  *n_kept = kept;
  st.valid.resize(kept);
  for (int k = 0; k < kept; ++k) st.valid[k] = k;   // FILTER compacts the kept objects to slots 0 .. kept - 1, in order
  st.valid_model.swap(new_model);
  st.n_slots = kept;
  st.n_clusters = kept;
  st.done = stage;
  return over ? MH_ERR_CAPACITY : MH_OK;
}

}  // extern "C"
