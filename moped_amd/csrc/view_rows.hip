// 3-D models from Kinect views: FEAT's list of a view + the view's depth map + the object's pose in that view -> model
// rows at the measured points.  The map is the [h][w][4] (x, y, z, valid) image every depth entry point takes
// (DEPTHMAP_PROP_CPU.hpp:103-131), the depth camera at the origin (moped3d.cpp:259-260,275-276); a keypoint's point is
// the one of its truncated pixel, its model coordinates X_model = inverseTransform(pose, point) (moped.hpp:189-194)
// through tm_from_pose / tm_apply_inv (geom.h: one rounding per operation, the reference's order).  The rules, their
// order and the statistics are the block above mh_view_spec in moped_hip.h.
//
// The launch is planar_rows_kernel's (planar.hip): one workgroup of 1024 threads per view, the list walked in chunks of
// 1024 keypoints, ballot + popcount inside a wavefront, the 16 wavefront counts through LDS, the chunk's base carried
// from chunk to chunk -- a stable compaction, which mh_db_splice's byte-equality with an upload depends on.  Unlike the
// planar kernel it walks the whole list even when the output is full: every keypoint lands in a counter.
#include <cmath>

#include "context.h"
#include "view_check.h"
#include "view_rows_dev.h"

using namespace mh;

namespace {

constexpr int VR_THREADS = 1024;
constexpr int VR_WAVES = VR_THREADS / 64;

__global__ __launch_bounds__(VR_THREADS) void view_rows_kernel(const ViewArgs a) {
  __shared__ int wcnt[VR_WAVES];
  __shared__ int src_s[VR_THREADS];
  __shared__ float red[VR_WAVES][6];
  __shared__ int drop_s[8];
  const int view = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* desc = a.desc + (size_t)view * a.cap * DIM;
  float* desc_out = a.desc_out + (size_t)view * a.out_pitch * DIM;
  float* desc_copy = a.desc_copy ? a.desc_copy + (size_t)view * a.out_pitch * DIM : nullptr;
  float* xyz_out = a.xyz_out + (size_t)view * a.out_pitch * 3;
  ViewJudge J;
  view_judge_init(J, a, view);
  const int n = min(max(a.n[view], 0), a.cap);
  const int limit = a.spec.max_rows > 0 ? min(a.out_cap, a.spec.max_rows) : a.out_cap;
  Box6 bb = box6_empty();
  if (t < 8) drop_s[t] = 0;
  // the rows the model has already: the box is the whole model's after the edit
  if (a.dup.xyz_dev)
    for (int r = a.dup.row_begin + t; r < a.dup.row_end; r += VR_THREADS)
      bb.add(a.dup.xyz_dev[(size_t)r * 3], a.dup.xyz_dev[(size_t)r * 3 + 1], a.dup.xyz_dev[(size_t)r * 3 + 2]);
  __syncthreads();
  int base = 0;        // rows written so far (uniform)
  int over = 0;        // kept keypoints behind the limit (uniform)
  for (int c0 = 0; c0 < n; c0 += VR_THREADS) {
    const int i = c0 + t;
    int why = VR_NONE;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < n) why = view_verdict(a, J, i, x, y, z);
    const bool keep = why == VR_KEEP;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(bal);
#pragma unroll
    for (int k = VR_PIXEL; k <= VR_DUP; ++k) {
      const unsigned long long b = __ballot(why == k);
      if (lane == 0 && b) atomicAdd(&drop_s[k], __popcll(b));
    }
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < VR_WAVES; ++w) {
      const int c = wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int at = before + __popcll(bal & ((1ull << lane) - 1ull));   // place among the chunk's kept rows
    if (keep && base + at < limit) {
      float* o = xyz_out + (size_t)(base + at) * 3;
      o[0] = x;
      o[1] = y;
      o[2] = z;
      bb.add(x, y, z);
      src_s[at] = i;
    }
    __syncthreads();
    const int rows = min(total, limit - base);   // (limit - base >= 0)
    for (int k = t; k < rows * (DIM / 4); k += VR_THREADS) {
      const int r = k >> 5, c = k & 31;
      const float4 d = reinterpret_cast<const float4*>(desc + (size_t)src_s[r] * DIM)[c];
      reinterpret_cast<float4*>(desc_out + (size_t)(base + r) * DIM)[c] = d;
      if (desc_copy) reinterpret_cast<float4*>(desc_copy + (size_t)(base + r) * DIM)[c] = d;
    }
    base += rows;
    over += total - rows;
    __syncthreads();   // wcnt and src_s are the next chunk's
  }
  // the box: wavefront, then workgroup (the accumulators hold no NaN)
  bb.wave_reduce();
  if (lane == 0) {
    red[wave][0] = bb.mn0;
    red[wave][1] = bb.mn1;
    red[wave][2] = bb.mn2;
    red[wave][3] = bb.mx0;
    red[wave][4] = bb.mx1;
    red[wave][5] = bb.mx2;
  }
  __syncthreads();
  if (t < 6) {
    float m = red[0][t];
    for (int w = 1; w < VR_WAVES; ++w) m = t < 3 ? fminf(m, red[w][t]) : fmaxf(m, red[w][t]);
    a.bbox[(size_t)view * 6 + t] = m;
  }
  if (t < 8) a.stats[(size_t)view * 8 + t] = t == 0 ? n : t == VR_LIMIT ? over : drop_s[t];
  if (t == 0) a.n_out[view] = base;
}

}  // namespace

namespace mh {

void launch_view_rows(const ViewArgs& a, int n_views, hipStream_t s) {
  if (n_views <= 0) return;
  hipLaunchKernelGGL(view_rows_kernel, dim3(n_views), dim3(VR_THREADS), 0, s, a);
}

int view_args_check(mh_ctx* ctx, const char* who, const mh_view* views, int n_views, int width, int height,
                    const mh_view_spec* spec, ViewArgs* a) {
  const char* why = view_call_why(views, n_views, width, height, spec);
  if (why) {
    ctx->err = std::string(who) + ": " + why;
    return MH_ERR_ARG;
  }
  a->w = width;
  a->h = height;
  a->spec = *spec;
  a->roi_all = view_all_zero(spec->roi, 4);
  a->box_all = view_all_zero(spec->box, 6);
  for (int i = 0; i < n_views; ++i) {
    a->v[i].map = static_cast<const float4*>(views[i].depth_xyzn_dev);
    a->v[i].fill = views[i].fill_distance_dev;
    std::memcpy(a->v[i].pose, views[i].pose, sizeof views[i].pose);
  }
  return MH_OK;
}

}  // namespace mh

// both entry points below; `who` names the one called in the error text
static int view_rows_call(mh_ctx* ctx, const char* who, const float* desc_dev, const float* xy_dev, const int32_t* n_dev,
                          int n_views, int cap, const mh_view* views, int width, int height, const mh_view_spec* spec,
                          const mh_view_dup* dup, float* desc_out_dev, float* xyz_out_dev, int out_cap, int32_t* n_out_dev,
                          float* bbox_dev, int32_t* stats_dev) {
  if (!ctx) return MH_ERR_ARG;
  if (!desc_dev || !xy_dev || !n_dev || cap <= 0 || !desc_out_dev || !xyz_out_dev || out_cap <= 0 || !n_out_dev || !bbox_dev ||
      !stats_dev || ((uintptr_t)desc_dev & 15) || ((uintptr_t)desc_out_dev & 15) || ((uintptr_t)xy_dev & 7)) {
    ctx->err = std::string(who) + ": bad argument (descriptor arrays are 16-byte aligned, xy 8-byte)";
    return MH_ERR_ARG;
  }
  if (const char* why = view_dup_why(dup)) {
    ctx->err = std::string(who) + ": " + why;
    return MH_ERR_ARG;
  }
  ViewArgs a = {};
  if (int rc = view_args_check(ctx, who, views, n_views, width, height, spec, &a)) return rc;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  a.desc = desc_dev;
  a.xy = xy_dev;
  a.n = n_dev;
  a.cap = cap;
  if (dup) a.dup = *dup;
  a.dup_on = dup && spec->merge_ratio > 0.f && spec->merge_dist >= 0.f;
  a.desc_out = desc_out_dev;
  a.desc_copy = nullptr;
  a.xyz_out = xyz_out_dev;
  a.out_pitch = (size_t)out_cap;
  a.out_cap = out_cap;
  a.n_out = n_out_dev;
  a.bbox = bbox_dev;
  a.stats = stats_dev;
  launch_view_rows(a, n_views, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

extern "C" {

int mh_view_rows_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int cap,
                     const mh_view* view, int width, int height, const mh_view_spec* spec, const mh_view_dup* dup,
                     float* desc_out_dev, float* xyz_out_dev, int out_cap, int32_t* n_out_dev, float* bbox_dev,
                     int32_t* stats_dev) {
  return view_rows_call(ctx, "mh_view_rows_dev", desc_dev, xy_dev, n_dev, 1, cap, view, width, height, spec, dup, desc_out_dev,
                        xyz_out_dev, out_cap, n_out_dev, bbox_dev, stats_dev);
}

int mh_view_rows_batch_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int n_views,
                           int cap, const mh_view* views, int width, int height, const mh_view_spec* spec,
                           const mh_view_dup* dup, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                           int32_t* n_out_dev, float* bbox_dev, int32_t* stats_dev) {
  return view_rows_call(ctx, "mh_view_rows_batch_dev", desc_dev, xy_dev, n_dev, n_views, cap, views, width, height, spec, dup,
                        desc_out_dev, xyz_out_dev, out_cap, n_out_dev, bbox_dev, stats_dev);
}

}  // extern "C"
