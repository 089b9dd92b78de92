// The Kinect depth map from what the sensor delivers, on the device: the block of moped3d's ROS node that stands in
// front of the pipeline (moped3d/moped3d.cpp:279-333).  Raw depth in -- an organised point cloud's z field read in place,
// float metres with NaN for "no reading", or OpenNI's 16-bit millimetres with 0 for it -- the [height][width][4] map of
// camera-frame x, y, z, norm (all -1 where invalid) out, the layout every other depth entry point takes.
//
//   raw value   NaN / 0 -> -1e30 (:288-292); mm -> __fmul_rn((float)mm, 0.001f)
//   same size   data = the raw value (:298-300)
//   any other   data = the raw map resized to exactly (2 rw, 2 rh) (:303); pixels beyond it are invalid (:313-316), a
//               smaller target crops it
//   data < 0    -1, -1, -1, -1 (:318-319); else x = data (u - K2) / K0, y = data (v - K3) / K1, z = data,
//               norm = sqrt(x x + y y + z z) (:325-330), one correctly rounded float operation at a time.  (DEPTHFILL
//               recomputes ((u - K2) / K0) z, depthfill.hip: another reference line, another order; no shared helper.)
//
// The resize is cv::resize's generic bilinear path for float as OpenCV 2.x computes it, restated WITHOUT OpenCV at hand:
// UNPINNED, like every other OpenCV call the project restates.  Horizontal pass first, then vertical, every
// product and every sum rounded on its own:
//   column dx   fx = (float)((dx + 0.5) 0.5 - 0.5), sx = floor(fx), fx -= sx; sx < 0: sx = 0, fx = 0;
//               sx >= rw - 1: S[rw - 1] alone; else S[sx] (1 - fx) + S[sx + 1] fx
//   row dy      fy, sy the same way without a reset at the borders, b0 = 1 - fy, b1 = fy, the two rows clamped to
//               [0, rh - 1]: r0 b0 + r1 b1
// The -1e30 stand-ins go through it like any value: one missing reading at (x, y) makes the output pixels
// [2x - 1, 2x + 2] x [2y - 1, 2y + 2] negative, hence invalid.
//
// One thread per output pixel, one 16-byte store per pixel, no LDS, no atomics; blockIdx.y = the frame of a batch.
// tests/depthmap_ref.py restates this in numpy float32; tests/test_gpu_depthmap.py compares the bytes.
#include <climits>

#include "frame.h"

namespace mh {

namespace {

constexpr int DM_THREADS = 256;

struct DmRaw {
  int format, rw, rh, elem_stride, row_stride, offset;
};
struct DmFrames {
  const unsigned char* raw[MH_MAX_BATCH] = {};
  float4* out[MH_MAX_BATCH] = {};
};

// the raw value at (x, y), 0 <= x < rw, 0 <= y < rh
__device__ __forceinline__ float dm_raw_at(const unsigned char* __restrict__ raw, const DmRaw& r, int x, int y) {
  const unsigned char* p = raw + (size_t)r.offset + (size_t)y * (size_t)r.row_stride + (size_t)x * (size_t)r.elem_stride;
  if (r.format == MH_RAW_DEPTH_F32_M) {
    const float v = *reinterpret_cast<const float*>(p);
    return v != v ? -1e30f : v;   // isnan (:288-289)
  }
  const unsigned short mm = *reinterpret_cast<const unsigned short*>(p);
  return mm == 0 ? -1e30f : __fmul_rn((float)mm, 0.001f);
}

// row y of the horizontally resized map at destination column dx
__device__ __forceinline__ float dm_hresize(const unsigned char* __restrict__ raw, const DmRaw& r, int y, int sx, float fx) {
  if (sx >= r.rw - 1) return dm_raw_at(raw, r, r.rw - 1, y);
  const float a = __fmul_rn(dm_raw_at(raw, r, sx, y), __fsub_rn(1.f, fx));
  const float b = __fmul_rn(dm_raw_at(raw, r, sx + 1, y), fx);
  return __fadd_rn(a, b);
}

__global__ void __launch_bounds__(DM_THREADS) depth_map_from_raw_kernel(DmFrames fr, DmRaw r, int w, int h, float k0,
                                                                        float k1, float k2, float k3) {
  const unsigned i = blockIdx.x * DM_THREADS + threadIdx.x;   // (w * h <= INT_MAX: checked on the host)
  if (i >= (unsigned)w * (unsigned)h) return;
  const int v = (int)(i / (unsigned)w), u = (int)(i - (unsigned)v * (unsigned)w);
  const unsigned char* __restrict__ raw = fr.raw[blockIdx.y];
  float data;
  if (w == r.rw && h == r.rh) {
    data = dm_raw_at(raw, r, u, v);
  } else if (u >= 2 * r.rw || v >= 2 * r.rh) {
    data = -1.f;   // beyond the resized map (:313-316)
  } else {
    float fx = (float)(((double)u + 0.5) * 0.5 - 0.5);
    int sx = (int)floorf(fx);
    fx = __fsub_rn(fx, (float)sx);
    if (sx < 0) {
      sx = 0;
      fx = 0.f;
    }
    float fy = (float)(((double)v + 0.5) * 0.5 - 0.5);
    const int sy = (int)floorf(fy);
    fy = __fsub_rn(fy, (float)sy);
    const int y0 = min(max(sy, 0), r.rh - 1), y1 = min(max(sy + 1, 0), r.rh - 1);
    const float r0 = dm_hresize(raw, r, y0, sx, fx), r1 = dm_hresize(raw, r, y1, sx, fx);
    data = __fadd_rn(__fmul_rn(r0, __fsub_rn(1.f, fy)), __fmul_rn(r1, fy));
  }
  float4 px;
  if (data < 0.f) {
    px = make_float4(-1.f, -1.f, -1.f, -1.f);
  } else {
    const float x = __fdiv_rn(__fmul_rn(data, __fsub_rn((float)u, k2)), k0);
    const float y = __fdiv_rn(__fmul_rn(data, __fsub_rn((float)v, k3)), k1);
    px.x = x;
    px.y = y;
    px.z = data;
    // (sqrtf is the correctly rounded square root here, as in depthfill.hip; __fsqrt_rn is the native approximation)
    px.w = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(data, data)));
  }
  fr.out[blockIdx.y][i] = px;
}

int dm_elem_size(int format) { return format == MH_RAW_DEPTH_F32_M ? 4 : format == MH_RAW_DEPTH_U16_MM ? 2 : 0; }

// MH_ERR_ARG (and ctx->err) for a description or a target size no launch may see
int raw_depth_check(mh_ctx* ctx, const char* who, const mh_raw_depth* raw, const float K[4], int width, int height) {
  const char* what = nullptr;
  const int es = raw ? dm_elem_size(raw->format) : 0;
  if (!raw || !K) what = "a null pointer";
  else if (!es) what = "an unknown format";
  else if (raw->width <= 0 || raw->height <= 0 || width <= 0 || height <= 0) what = "a size that is not positive";
  else if ((long long)width * height > INT_MAX || raw->width > INT_MAX / 2 || raw->height > INT_MAX / 2)
    what = "more than 2^31 - 1 pixels";
  else if (raw->elem_stride < es || raw->row_stride < es || raw->offset < 0)
    what = "a stride smaller than the element, or a negative offset";
  else if (raw->elem_stride % es || raw->row_stride % es || raw->offset % es)
    what = "a stride or an offset that is no multiple of the element size";
  if (!what) return MH_OK;
  ctx->err = std::string(who) + ": " + what;
  return MH_ERR_ARG;
}

size_t raw_depth_bytes(const mh_raw_depth* raw) {
  return (size_t)raw->offset + (size_t)(raw->height - 1) * (size_t)raw->row_stride +
         (size_t)(raw->width - 1) * (size_t)raw->elem_stride + (size_t)dm_elem_size(raw->format);
}

// n_frames maps in one launch on the context's stream; the arguments are checked (raw_depth_check, the pointers)
int launch_depth_map_from_raw(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_depth* raw, const float K[4],
                              float* const* out_dev, int n_frames, int width, int height) {
  DmFrames fr;
  for (int f = 0; f < n_frames; ++f) {
    fr.raw[f] = static_cast<const unsigned char*>(raw_dev[f]);
    fr.out[f] = reinterpret_cast<float4*>(out_dev[f]);
  }
  const DmRaw r{raw->format, raw->width, raw->height, raw->elem_stride, raw->row_stride, raw->offset};
  const unsigned blocks = (unsigned)(((size_t)width * height + DM_THREADS - 1) / DM_THREADS);
  hipLaunchKernelGGL(depth_map_from_raw_kernel, dim3(blocks, (unsigned)n_frames), dim3(DM_THREADS), 0, ctx->stream, fr, r,
                     width, height, K[0], K[1], K[2], K[3]);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

}  // namespace

}  // namespace mh

using namespace mh;

extern "C" int mh_depth_map_from_raw_batch_dev(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_depth* raw,
                                               const float K[4], float* const* depth_xyzn_dev, int n_frames, int width,
                                               int height) {
  if (!ctx) return MH_ERR_ARG;
  if (!raw_dev || !depth_xyzn_dev || n_frames < 1 || n_frames > MH_MAX_BATCH) {
    ctx->err = "mh_depth_map_from_raw_batch_dev: a null pointer, or n_frames outside 1 .. MH_MAX_BATCH";
    return MH_ERR_ARG;
  }
  if (int rc = raw_depth_check(ctx, "mh_depth_map_from_raw_batch_dev", raw, K, width, height)) return rc;
  const size_t es = raw->format == MH_RAW_DEPTH_F32_M ? 4 : 2;
  for (int f = 0; f < n_frames; ++f) {
    if (!raw_dev[f] || !depth_xyzn_dev[f] || reinterpret_cast<uintptr_t>(raw_dev[f]) % es ||
        reinterpret_cast<uintptr_t>(depth_xyzn_dev[f]) % 16) {
      ctx->err = "mh_depth_map_from_raw_batch_dev: a null or misaligned pointer (raw: the element size, the map: 16 bytes)";
      return MH_ERR_ARG;
    }
    for (int g = 0; g < f; ++g)
      if (depth_xyzn_dev[f] == depth_xyzn_dev[g]) {
        ctx->err = "mh_depth_map_from_raw_batch_dev: the same map for two frames (every frame writes a map of its own)";
        return MH_ERR_ARG;
      }
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  return launch_depth_map_from_raw(ctx, raw_dev, raw, K, depth_xyzn_dev, n_frames, width, height);
}

extern "C" int mh_depth_map_from_raw_dev(mh_ctx* ctx, const void* raw_dev, const mh_raw_depth* raw, const float K[4],
                                         float* depth_xyzn_dev, int width, int height) {
  return mh_depth_map_from_raw_batch_dev(ctx, &raw_dev, raw, K, &depth_xyzn_dev, 1, width, height);
}

namespace mh {

// The raw buffer of a host into own_raw, its map into own_depth, behind each other on the context's stream.  The own
// buffers may be the frame's map (mh_frame_set_depth_image_host): overwritten, it is off (as in step_depth_map).
int depth_map_from_raw_own(mh_ctx* ctx, const char* who, const void* raw_host, const mh_raw_depth* raw, const float K[4],
                           int width, int height) {
  if (int rc = raw_depth_check(ctx, who, raw, K, width, height)) return rc;
  if (!raw_host) {
    ctx->err = std::string(who) + ": a null pointer";
    return MH_ERR_ARG;
  }
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  if (ctx->depth_img.img && ctx->own_depth && reinterpret_cast<const float*>(ctx->depth_img.img) == ctx->own_depth.p)
    mh_frame_set_depth_image(ctx, nullptr, nullptr, 0, 0, 0, ctx->depth_alpha, 0.f);
  const size_t bytes = raw_depth_bytes(raw);
  if (int rc = ensure_own_depth(ctx, (size_t)width * height)) return rc;
  MH_HIP(ctx, ctx->own_raw.ensure(bytes, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(ctx->own_raw, raw_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  const void* raw_dev = ctx->own_raw.p;
  float* out_dev = ctx->own_depth.p;
  return launch_depth_map_from_raw(ctx, &raw_dev, raw, K, &out_dev, 1, width, height);
}

}  // namespace mh

extern "C" int mh_depth_map_from_raw_host(mh_ctx* ctx, const void* raw_host, const mh_raw_depth* raw, const float K[4],
                                          float* depth_xyzn_host, int width, int height) {
  if (!ctx) return MH_ERR_ARG;
  if (int rc = depth_map_from_raw_own(ctx, "mh_depth_map_from_raw_host", raw_host, raw, K, width, height)) return rc;
  if (depth_xyzn_host)
    MH_HIP(ctx, hipMemcpyAsync(depth_xyzn_host, ctx->own_depth, (size_t)width * height * 4 * sizeof(float),
                               hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host's raw buffer may change after the call
  return MH_OK;
}
