// C ABI: the stand-alone stage calls on host pointers (CLUSTER / POSE / FILTER one step at a time: upload, launch, read
// back).  They borrow the frame's working arrays (FrameState, frame.h), so each of them ends a stepped frame.
#include <cmath>
#include <cstring>

#include "depth_verify.h"
#include "frame.h"
#include "hull.h"

using namespace mh;

namespace {
__global__ void set_scalar_kernel(int32_t* p, int32_t v) { *p = v; }

// mh_meanshift_batch / mh_cluster_linkage: the clusterers' results as they come back in one block -- members | label |
// cl_start (total + n_problems + 1) | ncl -- into the caller's per-problem arrays
void unpack_clusters(const int32_t* h, const int32_t* off, int n_problems, int32_t* label, int32_t* order, int32_t* n_clusters) {
  const int total = off[n_problems];
  const int32_t* h_members = h;
  const int32_t* h_label = h + total;
  const int32_t* h_start = h_label + total;
  const int32_t* h_ncl = h_start + (size_t)total + n_problems + 1;
  for (int p = 0; p < n_problems; ++p) {
    const int b = off[p], n = off[p + 1] - b;
    n_clusters[p] = n > 0 ? h_ncl[p] : 0;
    for (int i = 0; i < n; ++i) label[b + i] = h_label[b + i];
    if (order) {
      for (int i = 0; i < n; ++i) order[b + i] = -1;
      if (n > 0) {
        const int kept = h_start[b + p + h_ncl[p]];
        for (int i = 0; i < kept; ++i) order[b + i] = h_members[b + i];
      }
    }
  }
}

// points per problem in the context's mode (mh_linkage_set_mode)
int linkage_cap(const mh_ctx* ctx) { return ctx->lk_mode == MH_LINKAGE_ROWMAX ? LK_MAX : LK_CAP; }

// mh_cluster_linkage and the debug entries behind it, once the arguments are checked: upload, ONE launch of
// linkage_batch_kernel, the clusters back.  `need`: floats of matrix scratch (3 n^2 per problem).  K_given (with
// lp.given_matrix, one problem): its similarity matrix, in place of the matches.
int linkage_problems(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, const int32_t* off, int n_problems,
                     size_t need, const LinkageParams& lp, const float* K_given, int32_t* label, int32_t* order,
                     int32_t* n_clusters) {
  const int total = off[n_problems];
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  int rc = ensure_linkage_scratch(ctx, need);
  if (rc) return rc;
  // device layout: corr | depth | off | members | label | cl_start (total + n_problems + 1) | ncl
  const size_t b_corr = ((size_t)total * sizeof(mh_corr) + 15) & ~(size_t)15;
  const size_t b_depth = (size_t)total * sizeof(mh_depth);
  const size_t n_off = (size_t)n_problems + 1, n_start = (size_t)total + n_problems + 1;
  const size_t ints = n_off + 2 * (size_t)total + n_start + n_problems;
  // (MH_LINKAGE_ROWMAX: the plan, the headers and the per-point arrays of the matrix stage behind them)
  const bool rowmax = ctx->lk_mode == MH_LINKAGE_ROWMAX;
  const size_t b_ints = (ints * sizeof(int32_t) + 63) & ~(size_t)63;
  const size_t b_aux = rowmax ? linkage_rowmax_aux_bytes(n_problems, total) : 0;
  if (rowmax && !ctx->lk_stats) {
    MH_HIP(ctx, ctx->lk_stats.ensure(4, ctx->stream));
    MH_HIP(ctx, hipMemsetAsync(ctx->lk_stats, 0, 4 * sizeof(unsigned long long), ctx->stream));
  }
  if ((rc = ensure_scratch(ctx, b_corr + b_depth + b_ints + b_aux + 64))) return rc;
  if ((rc = ensure_pinned(ctx, (2 * (size_t)total + n_start + n_problems) * sizeof(int32_t)))) return rc;
  unsigned char* base = ctx->scratch;
  mh_corr* d_corr = (mh_corr*)base;
  float* d_depth = (float*)(base + b_corr);
  int32_t* d_off = (int32_t*)(base + b_corr + b_depth);
  int32_t* d_members = d_off + n_off;
  int32_t* d_label = d_members + total;
  int32_t* d_start = d_label + total;
  int32_t* d_ncl = d_start + n_start;
  hipStream_t s = ctx->stream;
  if (!K_given) {
    MH_HIP(ctx, hipMemcpyAsync(d_corr, corr_host, (size_t)total * sizeof(mh_corr), hipMemcpyHostToDevice, s));
    MH_HIP(ctx, hipMemcpyAsync(d_depth, depth_host, b_depth, hipMemcpyHostToDevice, s));
  }
  MH_HIP(ctx, hipMemcpyAsync(d_off, off, n_off * sizeof(int32_t), hipMemcpyHostToDevice, s));
  // (the debug entries: one problem, whose matrix region starts the scratch -- A | Dm | member lists, linkage.hip)
  if (K_given)
    MH_HIP(ctx, hipMemcpyAsync(ctx->lk_scratch.p + (size_t)total * total, K_given, (size_t)total * total * sizeof(float),
                               hipMemcpyHostToDevice, s));
  if (rowmax) {
    int n_tiles = 0, n_rowblocks = 0;
    for (int p = 0; p < n_problems; ++p) linkage_rowmax_units(off[p + 1] - off[p], n_tiles, n_rowblocks);
    launch_linkage_rowmax_batch(d_corr, d_depth, d_off, n_problems, total, n_tiles, n_rowblocks, ctx->depth_img, lp,
                                ctx->lk_scratch, ctx->lk_scratch.cap, d_members, d_start, d_ncl, d_label,
                                base + b_corr + b_depth + b_ints, ctx->lk_stats, s);
  } else {
    launch_linkage_batch(d_corr, d_depth, d_off, n_problems, ctx->depth_img, lp, ctx->lk_scratch, ctx->lk_scratch.cap,
                         d_members, d_start, d_ncl, d_label, s);
  }
  MH_HIP(ctx, hipGetLastError());
  int32_t* hbuf = (int32_t*)ctx->pinned.p;
  MH_HIP(ctx, hipMemcpyAsync(hbuf, d_members, (2 * (size_t)total + n_start + n_problems) * sizeof(int32_t),
                             hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  unpack_clusters(hbuf, off, n_problems, label, order, n_clusters);
  return MH_OK;
}

}  // namespace

extern "C" {

int mh_meanshift(mh_ctx* ctx, const float* pts_host, int n, int dim, float radius, float merge,
                 int min_pts, int max_iter, int32_t* label, int32_t* order, int32_t* n_clusters) {
  if (!ctx || n < 0 || (dim != 2 && dim != 3) || !n_clusters || (n > 0 && (!pts_host || !label))) {
    if (ctx) ctx->err = "mh_meanshift: bad argument";
    return MH_ERR_ARG;
  }
  *n_clusters = 0;
  if (n == 0) return MH_OK;
  if (n > MS_CAP) {
    ctx->err = "mh_meanshift: more than 2048 points";
    return MH_ERR_CAPACITY;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const size_t b_pts = (size_t)n * dim * sizeof(float);
  const size_t b_i = (size_t)(n + 2) * sizeof(int32_t);
  int rc = ensure_scratch(ctx, b_pts + 4 * b_i + 64);
  if (rc) return rc;
  unsigned char* base = ctx->scratch;
  float* d_pts = (float*)base;
  int32_t* d_members = (int32_t*)(base + ((b_pts + 15) & ~(size_t)15));
  int32_t* d_start = d_members + (n + 2);
  int32_t* d_label = d_start + (n + 2);
  int32_t* d_misc = d_label + (n + 2);  // [0] ncl, [1] iterations
  MH_HIP(ctx, hipMemcpyAsync(d_pts, pts_host, b_pts, hipMemcpyHostToDevice, ctx->stream));
  launch_meanshift_single(d_pts, n, dim, radius, merge, min_pts, max_iter, d_members, d_start,
                          d_misc, d_label, d_misc + 1, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  int32_t misc[2];
  MH_HIP(ctx, hipMemcpyAsync(misc, d_misc, sizeof misc, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(label, d_label, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_clusters = misc[0];
  if (order) {
    std::vector<int32_t> st(misc[0] + 1);
    MH_HIP(ctx, hipMemcpy(st.data(), d_start, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int total = st[misc[0]];
    for (int i = 0; i < n; ++i) order[i] = -1;
    if (total > 0)
      MH_HIP(ctx, hipMemcpy(order, d_members, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return MH_OK;
}

int mh_meanshift_batch(mh_ctx* ctx, const float* pts_host, const int32_t* off, int n_problems, int dim,
                       float radius, float merge, int min_pts, int max_iter, int32_t* label,
                       int32_t* order, int32_t* n_clusters) {
  if (!ctx || n_problems < 0 || (dim != 2 && dim != 3) || (n_problems > 0 && (!off || !n_clusters))) {
    if (ctx) ctx->err = "mh_meanshift_batch: bad argument";
    return MH_ERR_ARG;
  }
  if (n_problems == 0) return MH_OK;
  const int total = off[n_problems];
  for (int p = 0; p < n_problems; ++p) {
    n_clusters[p] = 0;
    const int n = off[p + 1] - off[p];
    if (n < 0 || off[0] != 0) {
      ctx->err = "mh_meanshift_batch: offsets must start at 0 and not decrease";
      return MH_ERR_ARG;
    }
    if (n > MS_CAP) {
      ctx->err = "mh_meanshift_batch: more than 2048 points in one problem";
      return MH_ERR_CAPACITY;
    }
  }
  if (total == 0) return MH_OK;
  if (!pts_host || !label) {
    ctx->err = "mh_meanshift_batch: bad argument";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // device layout: pts | off | members | label | cl_start (total + n_problems + 1) | ncl
  const size_t b_pts = ((size_t)total * dim * sizeof(float) + 15) & ~(size_t)15;
  const size_t n_off = (size_t)n_problems + 1;
  const size_t n_start = (size_t)total + n_problems + 1;
  const size_t ints = n_off + 2 * (size_t)total + n_start + n_problems;
  int rc = ensure_scratch(ctx, b_pts + ints * sizeof(int32_t) + 64);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, (2 * (size_t)total + n_start + n_problems) * sizeof(int32_t)))) return rc;
  unsigned char* base = ctx->scratch;
  float* d_pts = (float*)base;
  int32_t* d_off = (int32_t*)(base + b_pts);
  int32_t* d_members = d_off + n_off;
  int32_t* d_label = d_members + total;
  int32_t* d_start = d_label + total;
  int32_t* d_ncl = d_start + n_start;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(d_pts, pts_host, (size_t)total * dim * sizeof(float), hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_off, off, n_off * sizeof(int32_t), hipMemcpyHostToDevice, s));
  launch_meanshift_batch(d_pts, d_off, n_problems, dim, radius, merge, min_pts, max_iter, d_members, d_start,
                         d_ncl, d_label, s);
  MH_HIP(ctx, hipGetLastError());
  // members, label, cl_start, ncl are contiguous on the device: one copy back
  int32_t* h = (int32_t*)ctx->pinned.p;
  MH_HIP(ctx, hipMemcpyAsync(h, d_members, (2 * (size_t)total + n_start + n_problems) * sizeof(int32_t),
                             hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  unpack_clusters(h, off, n_problems, label, order, n_clusters);
  return MH_OK;
}

static int pose_ransac_impl(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, int kind,
                            float alpha, const int32_t* cluster_off, int n_clusters, const mh_cam* cam,
                            const mh_pose_params* prm, uint64_t seed, mh_pose_out* out_host,
                            int32_t* n_out, const int32_t* image_of_host = nullptr, int n_images = 1) {
  if (!ctx || n_clusters < 0 || !cam || !prm || !n_out || (n_clusters > 0 && (!corr_host || !cluster_off || !out_host)) ||
      n_images < 1 || n_images > MH_MAX_IMAGES) {
    if (ctx) ctx->err = "mh_pose_ransac: bad argument";
    return MH_ERR_ARG;
  }
  *n_out = 0;
  if (n_clusters == 0) return MH_OK;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const int R_ = prm->max_objects_per_cluster > 0 ? prm->max_objects_per_cluster : 1;
  const int total = cluster_off[n_clusters];
  const int n_obj = n_clusters * R_;
  ctx->step.done = -1;   // (the frame's working arrays are this call's now)
  int rc = ensure_fs(ctx, std::max(total, 1), n_clusters, n_obj, std::max(ctx->n_models, 1));
  if (rc) return rc;
  FrameState* fs = ctx->fs;
  hipStream_t s = ctx->stream;
  std::vector<int32_t> h_members(std::max(total, 1)), h_model(n_clusters, 0), h_begin(n_clusters), h_count(n_clusters);
  for (int i = 0; i < total; ++i) h_members[i] = i;
  for (int c = 0; c < n_clusters; ++c) {
    h_model[c] = c;   // the step-level call has no models: every cluster its own (keys the task's random stream)
    h_begin[c] = cluster_off[c];
    h_count[c] = cluster_off[c + 1] - cluster_off[c];
  }
  PoseImages images;
  if (image_of_host && n_images > 1) {   // every correspondence in its own image: cam[0..n_images)
    for (int i = 0; i < total; ++i)
      if (image_of_host[i] < 0 || image_of_host[i] >= n_images) {
        ctx->err = "mh_pose_ransac_images: image index outside [0, n_images)";
        return MH_ERR_ARG;
      }
    if ((rc = upload_cams(ctx, cam, n_images))) return rc;
    MH_HIP(ctx, hipMemcpyAsync(fs->m_img, image_of_host, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, s));
    images.cams = ctx->cams_view;
    images.img_of = fs->m_img;
    images.n_images = n_images;
  }
  MH_HIP(ctx, hipMemcpyAsync(fs->m_corr, corr_host, (size_t)total * sizeof(mh_corr), hipMemcpyHostToDevice, s));
  if (depth_host)
    MH_HIP(ctx, hipMemcpyAsync(fs->m_depth, depth_host, (size_t)total * sizeof(mh_depth), hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->ms_members, h_members.data(), (size_t)total * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->cl_model, h_model.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->cl_begin, h_begin.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->cl_count, h_count.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemsetAsync(fs->counts, 0, sizeof(FrameCounts), s));
  hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, fs->n_clusters, n_clusters);
  hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, fs->n_slots, 0);
  const DevCam dc = make_devcam(*cam);
  launch_pose(fs->m_corr, depth_host ? reinterpret_cast<const float*>(fs->m_depth) : nullptr, kind, alpha,
              fs->ms_members, fs->cl_model, fs->cl_begin, fs->cl_count, fs->n_clusters, n_clusters, dc, *prm, seed, fs->n_slots, fs->max_objects, fs->obj_model, fs->obj_pose,
              fs->obj_ninl, fs->obj_err, fs->obj_cluster, fs->obj_valid, fs->counts, PoseTail{nullptr, nullptr, nullptr, 0, nullptr}, s,
              images);
  MH_HIP(ctx, hipGetLastError());
  // the five result arrays into one pinned block (pageable destinations make every one of these copies a blocking one)
  if (int rc_pin = ensure_pinned(ctx, (size_t)n_obj * 11 * 4)) return rc_pin;
  int32_t* const valid = reinterpret_cast<int32_t*>(ctx->pinned.p);
  int32_t* const ninl = valid + n_obj;
  int32_t* const ocl = ninl + n_obj;
  float* const err = reinterpret_cast<float*>(ocl + n_obj);
  float* const pose = err + n_obj;
  MH_HIP(ctx, hipMemcpyAsync(valid, fs->obj_valid, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(ninl, fs->obj_ninl, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(ocl, fs->obj_cluster, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(pose, fs->obj_pose, (size_t)n_obj * 28, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(err, fs->obj_err, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  int k = 0;
  for (int o = 0; o < n_obj; ++o) {
    if (!valid[o]) continue;
    mh_pose_out& po = out_host[k++];
    std::memcpy(po.pose, &pose[(size_t)7 * o], 28);
    po.cluster = ocl[o];
    po.n_inliers = ninl[o];
    po.err = err[o];
  }
  *n_out = k;
  return MH_OK;
}

int mh_pose_ransac(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* cluster_off,
                   int n_clusters, const mh_cam* cam, const mh_pose_params* prm, uint64_t seed,
                   mh_pose_out* out_host, int32_t* n_out) {
  return pose_ransac_impl(ctx, corr_host, nullptr, MH_DEPTH_NONE, 0.f, cluster_off, n_clusters, cam, prm, seed,
                          out_host, n_out);
}

int mh_pose_ransac_images(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* image_of_host,
                          const int32_t* cluster_off, int n_clusters, const mh_cam* cams, int n_images,
                          const mh_pose_params* prm, uint64_t seed, mh_pose_out* out_host, int32_t* n_out) {
  if (n_clusters > 0 && n_images > 1 && !image_of_host) return MH_ERR_ARG;
  return pose_ransac_impl(ctx, corr_host, nullptr, MH_DEPTH_NONE, 0.f, cluster_off, n_clusters, cams, prm, seed,
                          out_host, n_out, image_of_host, n_images);
}

int mh_pose_ransac_depth(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host,
                         const int32_t* cluster_off, int n_clusters, const mh_cam* cam,
                         const mh_pose_params* prm, int kind, float alpha, uint64_t seed,
                         mh_pose_out* out_host, int32_t* n_out) {
  if (kind != MH_DEPTH_BACKPROJECTION && kind != MH_DEPTH_REPROJECTION) return MH_ERR_ARG;
  if (n_clusters > 0 && !depth_host) return MH_ERR_ARG;
  return pose_ransac_impl(ctx, corr_host, depth_host, kind, alpha, cluster_off, n_clusters, cam, prm, seed,
                          out_host, n_out);
}

int mh_cluster_linkage(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, const int32_t* off,
                       int n_problems, const mh_linkage_params* prm, int32_t* label, int32_t* order,
                       int32_t* n_clusters) {
  if (!ctx || n_problems < 0 || !prm || (n_problems > 0 && (!off || !n_clusters))) {
    if (ctx) ctx->err = "mh_cluster_linkage: bad argument";
    return MH_ERR_ARG;
  }
  if (prm->linkage_type < 0 || prm->linkage_type > 2) {   // (before any upload is enqueued)
    ctx->err = "mh_cluster_linkage: linkage_type must be 0 (minimum), 1 (average) or 2 (maximum)";
    return MH_ERR_ARG;
  }
  if (n_problems == 0) return MH_OK;
  if (!ctx->depth_img.img) {
    ctx->err = "mh_cluster_linkage: no depth map (mh_frame_set_depth_image)";
    return MH_ERR_ARG;
  }
  const int total = off[n_problems];
  size_t need = 0;
  for (int p = 0; p < n_problems; ++p) {
    n_clusters[p] = 0;
    const int n = off[p + 1] - off[p];
    if (n < 0 || off[0] != 0) {
      ctx->err = "mh_cluster_linkage: offsets must start at 0 and not decrease";
      return MH_ERR_ARG;
    }
    if (n > linkage_cap(ctx)) {
      ctx->err = ctx->lk_mode == MH_LINKAGE_ROWMAX ? "mh_cluster_linkage: more than 4096 points in one problem"
                                                   : "mh_cluster_linkage: more than 1024 points in one problem";
      return MH_ERR_CAPACITY;
    }
    need += 3 * (size_t)n * n;
  }
  if (total == 0) return MH_OK;
  if (!corr_host || !depth_host || !label) {
    ctx->err = "mh_cluster_linkage: bad argument";
    return MH_ERR_ARG;
  }
  LinkageParams lp;
  lp.cutoff = prm->cutoff;
  lp.min_pts = prm->min_pts;
  lp.use3d_filter = prm->use3d_filter;
  lp.sigma2d = prm->sigma2d;
  lp.sigma3d = prm->sigma3d;
  lp.linkage_type = prm->linkage_type;
  return linkage_problems(ctx, corr_host, depth_host, off, n_problems, need, lp, nullptr, label, order, n_clusters);
}

int mh_linkage_set_mode(mh_ctx* ctx, int mode) {
  if (!ctx) return MH_ERR_ARG;
  if (mode != MH_LINKAGE_SCAN && mode != MH_LINKAGE_ROWMAX) {
    ctx->err = "mh_linkage_set_mode: MH_LINKAGE_SCAN or MH_LINKAGE_ROWMAX";
    return MH_ERR_ARG;
  }
  ctx->lk_mode = mode;
  return MH_OK;
}

int mh_linkage_get_mode(mh_ctx* ctx, int* mode) {
  if (!ctx || !mode) return MH_ERR_ARG;
  *mode = ctx->lk_mode;
  return MH_OK;
}

int mh_linkage_stats(mh_ctx* ctx, int64_t out[4], int reset) {
  if (!ctx || !out) return MH_ERR_ARG;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!ctx->lk_stats) return MH_OK;   // (no MH_LINKAGE_ROWMAX call on this context yet)
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters are 64-bit words");
  MH_HIP(ctx, hipMemcpyAsync(out, ctx->lk_stats, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (reset) MH_HIP(ctx, hipMemsetAsync(ctx->lk_stats, 0, 4 * sizeof(int64_t), ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_linkage_debug_matrix(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, int n,
                            const mh_linkage_params* prm, float* A_host, float* K_host) {
  if (!ctx) return MH_ERR_ARG;
  if (!corr_host || !depth_host || !prm || !A_host || !K_host) {
    ctx->err = "mh_linkage_debug_matrix: bad argument";
    return MH_ERR_ARG;
  }
  if (n < 1 || n > linkage_cap(ctx)) {
    ctx->err = ctx->lk_mode == MH_LINKAGE_ROWMAX ? "mh_linkage_debug_matrix: one problem of 1 .. 4096 points"
                                                 : "mh_linkage_debug_matrix: one problem of 1 .. 1024 points";
    return n >= 1 ? MH_ERR_CAPACITY : MH_ERR_ARG;
  }
  if (!ctx->depth_img.img) {
    ctx->err = "mh_linkage_debug_matrix: no depth map (mh_frame_set_depth_image)";
    return MH_ERR_ARG;
  }
  // the shipped kernel with a cutoff no similarity reaches: hierarchicalCluster's loop leaves in its first scan
  // (CLUSTER_LINKAGE_CPU.hpp:468) with the matrices of passes 2 and 3 still in the problem's scratch region
  LinkageParams lp;
  lp.cutoff = __builtin_inff();
  lp.min_pts = prm->min_pts;
  lp.use3d_filter = prm->use3d_filter;
  lp.sigma2d = prm->sigma2d;
  lp.sigma3d = prm->sigma3d;
  const int32_t off[2] = {0, n};
  const size_t nn = (size_t)n * n;
  std::vector<int32_t> label(n);
  int32_t ncl = 0;
  if (int rc = linkage_problems(ctx, corr_host, depth_host, off, 1, 3 * nn, lp, nullptr, label.data(), nullptr, &ncl)) return rc;
  MH_HIP(ctx, hipMemcpy(A_host, ctx->lk_scratch.p, nn * sizeof(float), hipMemcpyDeviceToHost));
  MH_HIP(ctx, hipMemcpy(K_host, ctx->lk_scratch.p + nn, nn * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)   // (the kernel fills A for j >= i only)
    for (int j = 0; j < i; ++j) A_host[(size_t)i * n + j] = A_host[(size_t)j * n + i];
  return MH_OK;
}

int mh_linkage_debug_agglomerate(mh_ctx* ctx, const float* K_host, int n, float cutoff, int min_pts, int linkage_type,
                                 int32_t* label, int32_t* order, int32_t* n_clusters) {
  if (!ctx) return MH_ERR_ARG;
  if (!K_host || !label || !n_clusters) {
    ctx->err = "mh_linkage_debug_agglomerate: bad argument";
    return MH_ERR_ARG;
  }
  if (linkage_type < 0 || linkage_type > 2) {
    ctx->err = "mh_linkage_debug_agglomerate: linkage_type must be 0 (minimum), 1 (average) or 2 (maximum)";
    return MH_ERR_ARG;
  }
  if (n < 1 || n > linkage_cap(ctx)) {
    ctx->err = ctx->lk_mode == MH_LINKAGE_ROWMAX ? "mh_linkage_debug_agglomerate: a matrix of 1 .. 4096 rows"
                                                 : "mh_linkage_debug_agglomerate: a matrix of 1 .. 1024 rows";
    return n >= 1 ? MH_ERR_CAPACITY : MH_ERR_ARG;
  }
  LinkageParams lp;
  lp.cutoff = cutoff;
  lp.min_pts = min_pts;
  lp.linkage_type = linkage_type;
  lp.given_matrix = 1;
  const int32_t off[2] = {0, n};
  return linkage_problems(ctx, nullptr, nullptr, off, 1, 3 * (size_t)n * n, lp, K_host, label, order, n_clusters);
}

int mh_project_test(mh_ctx* ctx, const float pose[7], const mh_corr* corr_host, int n,
                    const mh_cam* cam, float thr, uint8_t* inlier_host, float* err2_host,
                    int32_t* n_inliers) {
  if (!ctx || !pose || !cam || n < 0 || (n > 0 && !corr_host)) return MH_ERR_ARG;
  if (n_inliers) *n_inliers = 0;
  if (n == 0) return MH_OK;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const size_t b_c = (size_t)n * sizeof(mh_corr);
  int rc = ensure_scratch(ctx, b_c + (size_t)n * 5 + 256);
  if (rc) return rc;
  unsigned char* base = ctx->scratch;
  mh_corr* d_c = (mh_corr*)base;
  float* d_e = (float*)(base + ((b_c + 15) & ~(size_t)15));
  float* d_pose = d_e + n;
  int32_t* d_cnt = (int32_t*)(d_pose + 8);
  uint8_t* d_in = (uint8_t*)(d_cnt + 4);
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(d_c, corr_host, b_c, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_pose, pose, 28, hipMemcpyHostToDevice, s));
  launch_project_test(d_pose, d_c, n, make_devcam(*cam), thr, d_in, d_e, d_cnt, s);
  MH_HIP(ctx, hipGetLastError());
  int32_t cnt = 0;
  MH_HIP(ctx, hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, s));
  if (inlier_host) MH_HIP(ctx, hipMemcpyAsync(inlier_host, d_in, n, hipMemcpyDeviceToHost, s));
  if (err2_host) MH_HIP(ctx, hipMemcpyAsync(err2_host, d_e, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  if (n_inliers) *n_inliers = cnt;
  return MH_OK;
}

int mh_filter(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
              const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
              int min_points, float feature_distance, float min_score, float* score,
              uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off,
              int32_t* n_kept) {
  return mh_filter_images(ctx, corr_host, nullptr, model_off, n_models, obj_model, obj_pose, n_obj, cam, 1, min_points,
                          feature_distance, min_score, score, keep, out_order, cl_members, cl_off, n_kept);
}

// mh_filter_depth's additions to a FILTER call (depth == nullptr: the plain class)
struct FilterDepthCall {
  const mh_cam* depth_cam;
  const mh_filter_depth_params* prm;
  float* incorrect_score;
  int32_t* used;
  int32_t* plausible;
};

static int filter_impl(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* image_of_host, const int32_t* model_off,
                       int n_models, const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                       int n_images, int min_points, float feature_distance, float min_score, float* score,
                       uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off, int32_t* n_kept,
                       const FilterDepthCall* depth) {
  if (!ctx || !model_off || n_models <= 0 || n_obj < 0 || !cam || !n_kept || n_images < 1 || n_images > MH_MAX_IMAGES ||
      (n_images > 1 && !image_of_host))
    return MH_ERR_ARG;
  *n_kept = 0;
  if (cl_off) cl_off[0] = 0;
  if (n_obj == 0) return MH_OK;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const int M = model_off[n_models];
  ctx->step.done = -1;   // (the frame's working arrays are this call's now)
  int rc = ensure_fs(ctx, std::max(M, 1), std::max(n_obj, 1), std::max(n_obj, 1), n_models);
  if (rc) return rc;
  FrameState* fs = ctx->fs;
  hipStream_t s = ctx->stream;
  std::vector<int32_t> ones(n_obj, 1);
  const bool multi = image_of_host && n_images > 1;
  if (multi) {
    for (int i = 0; i < M; ++i)
      if (image_of_host[i] < 0 || image_of_host[i] >= n_images) {
        ctx->err = "mh_filter_images: image index outside [0, n_images)";
        return MH_ERR_ARG;
      }
    if ((rc = upload_cams(ctx, cam, n_images))) return rc;
    MH_HIP(ctx, hipMemcpyAsync(fs->m_img, image_of_host, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  MH_HIP(ctx, hipMemcpyAsync(fs->m_corr, corr_host, (size_t)M * sizeof(mh_corr), hipMemcpyHostToDevice, s));
  launch_rep(fs->m_corr, M, fs->m_rep, s, multi ? fs->m_img : nullptr);
  MH_HIP(ctx, hipMemcpyAsync(fs->model_off, model_off, (size_t)(n_models + 1) * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->obj_model, obj_model, (size_t)n_obj * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->obj_pose, obj_pose, (size_t)n_obj * 28, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(fs->obj_valid, ones.data(), (size_t)n_obj * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemsetAsync(fs->counts, 0, sizeof(FrameCounts), s));
  MH_HIP(ctx, hipMemsetAsync(fs->best, 0, sizeof(unsigned long long) * (size_t)std::max(M, 1), s));
  hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, fs->n_slots, n_obj);
  FilterBuffers fb = make_fb(fs, n_models);
  fb.max_objects = n_obj;  // grid size; arrays are at least this large
  if (multi) {
    fb.m_img = fs->m_img;
    fb.cams = ctx->cams_view;
    fb.n_images = n_images;
  }
  const FilterTail tail{fs->tickets + 5, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
  float* d_is = nullptr;   // the depth class's per-object outputs: IS | used | plausible in the context's byte scratch
  if (depth) {
    if ((rc = ensure_scratch(ctx, 3 * (size_t)n_obj * 4))) return rc;
    d_is = reinterpret_cast<float*>(ctx->scratch.p);
    FilterDepthArgs da = make_filter_depth_args(ctx, ctx->depth_img, *depth->prm, *depth->depth_cam);
    da.out_is = d_is;
    da.out_used = reinterpret_cast<int32_t*>(d_is) + n_obj;
    da.out_plausible = reinterpret_cast<int32_t*>(d_is) + 2 * (size_t)n_obj;
    (ctx->fdepth.debug_form == 1 ? launch_filter_depth_wave : launch_filter_depth)(
        fb, make_devcam(*cam), min_points, feature_distance, min_score, da, fs->n_slots, fs->n_clusters, fs->counts, tail, s);
  } else
    launch_filter(fb, make_devcam(*cam), min_points, feature_distance, min_score, fs->n_slots, fs->n_clusters, fs->counts,
                  tail, s);
  MH_HIP(ctx, hipGetLastError());
  // results: everything the host needs in ONE pinned block, copied behind the kernel, one synchronisation (five
  // blocking copies after it cost the step 0.1 ms: profiles/r02_host_step_timing.txt)
  const size_t words = 1 + 4 * (size_t)n_obj + (size_t)std::max(M, 1) + (depth ? 3 * (size_t)n_obj : 0);
  if ((rc = ensure_pinned(ctx, words * 4))) return rc;
  int32_t* const hp = reinterpret_cast<int32_t*>(ctx->pinned.p);
  int32_t* const h_kept = hp;
  float* const sc = reinterpret_cast<float*>(hp + 1);
  int32_t* const old_of = hp + 1 + n_obj;
  int32_t* const begin = old_of + n_obj;
  int32_t* const count = begin + n_obj;
  int32_t* const mem = count + n_obj;
  MH_HIP(ctx, hipMemcpyAsync(h_kept, fs->n_slots, 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(sc, fs->obj_score_raw, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(old_of, fs->obj_clsize + n_obj, (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(begin, fs->cl_begin, (size_t)std::min(n_obj, fs->max_clusters) * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(count, fs->cl_count, (size_t)std::min(n_obj, fs->max_clusters) * 4, hipMemcpyDeviceToHost, s));
  if (M > 0) MH_HIP(ctx, hipMemcpyAsync(mem, fs->new_members, (size_t)M * 4, hipMemcpyDeviceToHost, s));
  int32_t* const extra = mem + std::max(M, 1);   // (the depth class: IS | used | plausible)
  if (depth) MH_HIP(ctx, hipMemcpyAsync(extra, d_is, 3 * (size_t)n_obj * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  if (depth) {
    if (depth->incorrect_score) std::memcpy(depth->incorrect_score, extra, (size_t)n_obj * 4);
    if (depth->used) std::memcpy(depth->used, extra + n_obj, (size_t)n_obj * 4);
    if (depth->plausible) std::memcpy(depth->plausible, extra + 2 * (size_t)n_obj, (size_t)n_obj * 4);
  }
  const int32_t kept = std::min(*h_kept, n_obj);
  if (keep) std::memset(keep, 0, n_obj);
  if (score)
    for (int o = 0; o < n_obj; ++o) score[o] = sc[o];
  int w = 0;
  for (int k = 0; k < kept; ++k) {
    const int o = old_of[k];
    if (keep) keep[o] = 1;
    if (out_order) out_order[k] = o;
    if (cl_off) cl_off[k] = w;
    const int b = model_off[obj_model[o]];
    for (int j = 0; j < count[k]; ++j, ++w)
      if (cl_members) cl_members[w] = mem[begin[k] + j] - b;  // index inside the model
  }
  if (cl_off) cl_off[kept] = w;
  *n_kept = kept;
  return MH_OK;
}

int mh_filter_images(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* image_of_host, const int32_t* model_off,
                     int n_models, const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                     int n_images, int min_points, float feature_distance, float min_score, float* score,
                     uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off, int32_t* n_kept) {
  return filter_impl(ctx, corr_host, image_of_host, model_off, n_models, obj_model, obj_pose, n_obj, cam, n_images,
                     min_points, feature_distance, min_score, score, keep, out_order, cl_members, cl_off, n_kept, nullptr);
}

// TestPoints of FILTER_PROJECTION_DEPTH_CPU (moped3d .../filter/FILTER_PROJECTION_DEPTH_CPU.hpp:94-116)
int mh_filter_depth_set_points(mh_ctx* ctx, const float* xyz_host, const int32_t* off_host, int n_models) {
  if (!ctx || n_models < 0) return MH_ERR_ARG;
  mh_ctx::FilterDepthState& fd = ctx->fdepth;
  if (n_models == 0) {
    fd.n_models = 0;
    return MH_OK;
  }
  auto refuse = [&](const char* why) {
    ctx->err = std::string("mh_filter_depth_set_points: ") + why;
    return MH_ERR_ARG;
  };
  if (!off_host || off_host[0] != 0) return refuse("offsets must start at 0");
  for (int m = 0; m < n_models; ++m)
    if (off_host[m + 1] < off_host[m]) return refuse("offsets must not decrease");
  const int total = off_host[n_models];
  if (total > 0 && !xyz_host) return refuse("no points");
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  hipStream_t s = ctx->stream;
  fd.n_models = 0;   // (a failure below leaves "no points")
  MH_HIP(ctx, fd.pts.ensure(3 * (size_t)std::max(total, 1), s));
  MH_HIP(ctx, fd.off.ensure((size_t)n_models + 1, s));
  MH_HIP(ctx, hipStreamSynchronize(s));   // frames in flight still read the old points
  if (total > 0) MH_HIP(ctx, hipMemcpy(fd.pts, xyz_host, 3 * (size_t)total * sizeof(float), hipMemcpyHostToDevice));
  MH_HIP(ctx, hipMemcpy(fd.off, off_host, ((size_t)n_models + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  fd.n_models = n_models;
  fd.db_models = ctx->n_models;                                    // mh_db_size
  fd.db_generation = ctx->store ? ctx->store->generation : 0;      // mh_db_generation
  return MH_OK;
}

// FILTER_PROJECTION_DEPTH_CPU::process (moped3d .../filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329)
int mh_filter_depth(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
                    const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam, int min_points,
                    float feature_distance, float min_score, const mh_cam* depth_cam, const mh_filter_depth_params* prm,
                    float* score, uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off,
                    int32_t* n_kept, float* incorrect_score, int32_t* used, int32_t* plausible) {
  if (!ctx) return MH_ERR_ARG;
  if (!depth_cam || !prm || !model_off || n_models <= 0 || n_obj < 0 || !cam || !n_kept || (n_obj > 0 && (!obj_model || !obj_pose))) {
    ctx->err = "mh_filter_depth: bad argument";
    return MH_ERR_ARG;
  }
  if (!ctx->depth_img.img) {
    ctx->err = "mh_filter_depth: no depth map (mh_frame_set_depth_image / mh_frame_set_depth_image_host)";
    return MH_ERR_ARG;
  }
  if (int rc = filter_depth_points_ok(ctx, "mh_filter_depth", n_models)) return rc;
  for (int o = 0; o < n_obj; ++o)   // (the kernel reads the model's slice of the test points)
    if (obj_model[o] < 0 || obj_model[o] >= n_models) {
      ctx->err = "mh_filter_depth: object model outside [0, n_models)";
      return MH_ERR_ARG;
    }
  const FilterDepthCall dc{depth_cam, prm, incorrect_score, used, plausible};
  return filter_impl(ctx, corr_host, nullptr, model_off, n_models, obj_model, obj_pose, n_obj, cam, 1, min_points,
                     feature_distance, min_score, score, keep, out_order, cl_members, cl_off, n_kept, &dc);
}

// which device form of F1 mh_filter_depth scores with (a debug entry; frames ignore it)
int mh_filter_depth_debug_form(mh_ctx* ctx, int form) {
  if (!ctx) return MH_ERR_ARG;
  if (form != 0 && form != 1) {
    ctx->err = "mh_filter_depth_debug_form: 0 (the workgroup form) or 1 (filter_depth_score_wave)";
    return MH_ERR_ARG;
  }
  ctx->fdepth.debug_form = form;
  return MH_OK;
}

// Object::getObjectHull (moped2/libmoped/include/moped.hpp:266-327) for n_obj objects + the projected corners of their
// models' bounding boxes (src/GLOBAL_DISPLAY.hpp:197-207): hull.hip
int mh_object_hulls(mh_ctx* ctx, const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                    int max_vertices, float* hull_xy_host, int32_t* n_vertices, int32_t* n_behind, float* bbox_uv_host) {
  if (!ctx) return MH_ERR_ARG;
  auto refuse = [&](const char* why) {
    ctx->err = std::string("mh_object_hulls: ") + why;
    return MH_ERR_ARG;
  };
  if (n_obj < 0 || !cam || max_vertices < 1) return refuse("bad argument");
  if (n_obj == 0) return MH_OK;
  if (!obj_model || !obj_pose || !hull_xy_host || !n_vertices) return refuse("null pointer");
  const DbStore* st = ctx->store.get();
  if (!st) return refuse("no model database");
  if (!st->grouped) return refuse("the rows of the store are not grouped by model in ascending order");
  if (st->n_blocks > 1) return refuse("the store was uploaded in blocks (a sharded store has no whole models)");
  if ((size_t)n_obj * (size_t)max_vertices > ((size_t)1 << 28)) return refuse("n_obj * max_vertices above 2^28");
  size_t stride = 0;   // global scratch per object: what the largest model among them may need
  for (int o = 0; o < n_obj; ++o) {
    const int m = obj_model[o];
    if (m < 0 || m >= st->n_models) return refuse("object model outside [0, n_models)");
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(obj_pose[7 * (size_t)o + k])) return refuse("non-finite pose element");
    stride = std::max(stride, hull_scratch_points(st->model_begin[m + 1] - st->model_begin[m]));
  }
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(cam->K[k])) return refuse("non-finite camera");
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(cam->cam[k])) return refuse("non-finite camera");
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // one device block: models | poses | n_vertices | n_behind | corners | vertices | sort scratch
  const size_t n = (size_t)n_obj;
  const size_t w_out = 2 * n + 16 * n + 2 * n * (size_t)max_vertices;   // words the host reads back
  const size_t w_in = n + 7 * n;
  const size_t bytes = (w_in + w_out) * 4 + 16 + n * stride * sizeof(float2);
  int rc = ensure_scratch(ctx, bytes);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, w_out * 4))) return rc;
  hipStream_t s = ctx->stream;
  int32_t* const d_model = reinterpret_cast<int32_t*>(ctx->scratch.p);
  float* const d_pose = reinterpret_cast<float*>(d_model + n);
  int32_t* const d_nv = reinterpret_cast<int32_t*>(d_pose + 7 * n);
  int32_t* const d_nb = d_nv + n;
  float* const d_bb = reinterpret_cast<float*>(d_nb + n);
  float* const d_xy = d_bb + 16 * n;
  const size_t scratch_at = ((w_in + w_out) * 4 + 15) & ~(size_t)15;
  MH_HIP(ctx, hipMemcpyAsync(d_model, obj_model, n * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_pose, obj_pose, n * 28, hipMemcpyHostToDevice, s));
  HullArgs a;
  a.core.xyz = ctx->db_xyz;
  a.core.model_begin = st->model_begin_dev;
  a.core.n_models = st->n_models;
  a.core.cam = make_devcam(*cam);
  a.core.max_vertices = max_vertices;
  a.core.form = ctx->hull_debug_form;
  a.core.scratch = stride ? reinterpret_cast<float2*>(ctx->scratch.p + scratch_at) : nullptr;
  a.core.scratch_stride = stride;
  a.obj_model = d_model;
  a.obj_pose = d_pose;
  a.n_obj_dev = nullptr;
  a.n_obj = n_obj;
  a.hull_xy = d_xy;
  a.n_vertices = d_nv;
  a.n_behind = d_nb;
  a.bbox_uv = d_bb;
  launch_object_hulls(a, s);
  MH_HIP(ctx, hipGetLastError());
  // the counts and corners in one copy, then only the vertices that exist (a host array's rows beyond them stay untouched)
  int32_t* const hp = reinterpret_cast<int32_t*>(ctx->pinned.p);
  MH_HIP(ctx, hipMemcpyAsync(hp, d_nv, w_out * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  const float* const h_bb = reinterpret_cast<const float*>(hp + 2 * n);
  const float* const h_xy = h_bb + 16 * n;
  for (int o = 0; o < n_obj; ++o)
    if (hp[o] < 0) {
      ctx->err = "mh_object_hulls: the sort scratch was too small for an object";
      return MH_ERR_HIP;
    }
  for (int o = 0; o < n_obj; ++o) {
    n_vertices[o] = hp[o];
    if (n_behind) n_behind[o] = hp[n + o];
    const size_t kept = (size_t)std::min(hp[o], max_vertices);
    std::memcpy(hull_xy_host + 2 * (size_t)o * max_vertices, h_xy + 2 * (size_t)o * max_vertices, kept * 8);
  }
  if (bbox_uv_host) std::memcpy(bbox_uv_host, h_bb, 16 * n * 4);
  return MH_OK;
}

// which device form mh_object_hulls runs (a debug entry; frames ignore it)
int mh_hull_debug_form(mh_ctx* ctx, int form) {
  if (!ctx) return MH_ERR_ARG;
  if (form != 0 && form != 1) {
    ctx->err = "mh_hull_debug_form: 0 (the octagon prefilter) or 1 (sort and chain every point)";
    return MH_ERR_ARG;
  }
  ctx->hull_debug_form = form;
  return MH_OK;
}

// DEPTH_VERIFY_CPU::process (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp:86-208) for n_obj objects:
// depth_verify.hip
int mh_depth_verify(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
                    const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                    const mh_cam* depth_cam, const mh_depth_verify_params* prm, mh_verify_record* records) {
  if (!ctx) return MH_ERR_ARG;
  auto refuse = [&](const char* why) {
    ctx->err = std::string("mh_depth_verify: ") + why;
    return MH_ERR_ARG;
  };
  if (n_obj < 0 || n_models < 0) return refuse("bad argument");
  if (!model_off || !cam || !depth_cam || !prm) return refuse("null pointer");
  if (n_obj > 0 && (!obj_model || !obj_pose || !records)) return refuse("null pointer");
  if (!ctx->depth_img.img) return refuse("no depth map (mh_frame_set_depth_image / mh_frame_set_depth_image_host)");
  const DbStore* st = ctx->store.get();
  if (!st) return refuse("no model database");
  if (!st->grouped) return refuse("the rows of the store are not grouped by model in ascending order");
  if (st->n_blocks > 1) return refuse("the store was uploaded in blocks (a sharded store has no whole models)");
  if (n_models != st->n_models) return refuse("n_models is not the number of models of the database");
  if (model_off[0] != 0) return refuse("offsets must start at 0");
  for (int m = 0; m < n_models; ++m)
    if (model_off[m + 1] < model_off[m]) return refuse("offsets must not decrease");
  const int M = model_off[n_models];
  if (M > 0 && !corr_host) return refuse("null pointer");
  for (int o = 0; o < n_obj; ++o)
    if (obj_model[o] < 0 || obj_model[o] >= n_models) return refuse("object model outside [0, n_models)");
  if (n_obj == 0) return MH_OK;
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  // one device block: records | poses | models | offsets | matches
  const size_t n = (size_t)n_obj;
  const size_t w_rec = n * (sizeof(mh_verify_record) / 4);
  const size_t words = w_rec + 7 * n + n + ((size_t)n_models + 1) + 5 * (size_t)std::max(M, 1);
  int rc = ensure_scratch(ctx, words * 4);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, w_rec * 4))) return rc;
  hipStream_t s = ctx->stream;
  mh_verify_record* const d_rec = reinterpret_cast<mh_verify_record*>(ctx->scratch.p);
  float* const d_pose = reinterpret_cast<float*>(ctx->scratch.p) + w_rec;
  int32_t* const d_model = reinterpret_cast<int32_t*>(d_pose + 7 * n);
  int32_t* const d_off = d_model + n;
  mh_corr* const d_corr = reinterpret_cast<mh_corr*>(d_off + n_models + 1);
  MH_HIP(ctx, hipMemcpyAsync(d_pose, obj_pose, n * 28, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_model, obj_model, n * 4, hipMemcpyHostToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(d_off, model_off, ((size_t)n_models + 1) * 4, hipMemcpyHostToDevice, s));
  if (M > 0) MH_HIP(ctx, hipMemcpyAsync(d_corr, corr_host, (size_t)M * sizeof(mh_corr), hipMemcpyHostToDevice, s));
  DepthVerifyListArgs a;
  a.core.xyz = ctx->db_xyz;
  a.core.model_begin = st->model_begin_dev;
  a.core.img = ctx->depth_img.img;
  a.core.fill = ctx->depth_img.fill;
  a.core.w = ctx->depth_img.w;
  a.core.h = ctx->depth_img.h;
  a.core.cam = make_devcam(*cam);
  a.core.dcam = make_devcam(*depth_cam);
  a.core.feature_distance = prm->feature_distance;
  a.core.max_multiplier = prm->max_multiplier;
  a.core.max_distance = prm->max_distance;
  a.core.depth_fraction = prm->depth_fraction;
  a.corr = d_corr;
  a.model_off = d_off;
  a.obj_model = d_model;
  a.obj_pose = d_pose;
  a.n_obj = n_obj;
  a.rec = d_rec;
  launch_depth_verify(a, ctx->depth_verify_debug_form, s);
  MH_HIP(ctx, hipGetLastError());
  MH_HIP(ctx, hipMemcpyAsync(ctx->pinned.p, d_rec, w_rec * 4, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  std::memcpy(records, ctx->pinned.p, w_rec * 4);
  return MH_OK;
}

// which device form mh_depth_verify runs (a debug entry)
int mh_depth_verify_debug_form(mh_ctx* ctx, int form) {
  if (!ctx) return MH_ERR_ARG;
  if (form != 0 && form != 1) {
    ctx->err = "mh_depth_verify_debug_form: 0 (a workgroup per object) or 1 (a wavefront per object)";
    return MH_ERR_ARG;
  }
  ctx->depth_verify_debug_form = form;
  return MH_OK;
}

}  // extern "C"
