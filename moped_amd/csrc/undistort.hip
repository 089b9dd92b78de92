// UNDISTORTED_IMAGE: UTIL_UNDISTORT (src/util/UTIL_UNDISTORT.hpp) on the device.
//
// The reference builds one pair of float maps per camera with cvInitUndistortMap (:68-98, OpenCV 2.x
// initUndistortRectifyMap with R = I and the new camera = K) and resamples every image in place with
// cvRemap(CV_INTER_LINEAR + CV_WARP_FILL_OUTLIERS) (:121-131): bilinear in 5-bit fixed point, border = 0.
// map_build_kernel restates the map arithmetic in f64 (one thread per row: the reference's running sum along
// the row), remap_kernel the fixed-point resampling in integers.  The checker is tests/undistort_ref.py.
#include <climits>
#include <cmath>
#include <cstring>

#include "context.h"

using namespace mh;

namespace {

constexpr int UND_ENTRIES = MH_MAX_IMAGES;   // cameras kept (the reference keeps every one it meets)
constexpr int UND_MAX_SIDE = 32767;          // the remap's int16 source coordinates

// remap's position of one output pixel: source tap (sx, sy) and its 5-bit fractions, a = ay 32 + ax
struct FixPos {
  int16_t sx, sy;
  uint16_t a, pad;
};

struct UndMap {
  int width = 0, height = 0;
  float K[4] = {}, dist[4] = {};
  DevBuf<float> mapx;      // [height][width]
  DevBuf<float> mapy;
  DevBuf<FixPos> fix;
  size_t cap = 0;          // pixels every one of the three holds
  uint64_t used = 0;       // LRU stamp; 0 = empty
};

struct RemapImages {
  const uint8_t* src[MH_MAX_BATCH];
  uint8_t* dst[MH_MAX_BATCH];
  const FixPos* fix[MH_MAX_BATCH];   // every image its camera's map (one camera: the same pointer throughout)
};

// cvRound of mapx * INTER_TAB_SIZE (round half to even); NaN and values beyond int32 give INT_MIN, as the
// conversion the reference's remap uses does, and land outside the image
__device__ __forceinline__ int fixed5(float m) {
  const float v = m * 32.f;   // exact
  if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
  return (int)rintf(v);
}

__device__ __forceinline__ int16_t sat16(int v) { return (int16_t)min(max(v, -32768), 32767); }

// initUndistortRectifyMap (OpenCV 2.x, undistort.cpp) for R = I, newCameraMatrix = K, k3 = 0: row i, columns in order
__global__ void map_build_kernel(int w, int h, double fx, double fy, double cx, double cy, double k1, double k2,
                                 double p1, double p2, float* __restrict__ mapx, float* __restrict__ mapy,
                                 FixPos* __restrict__ fix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h) return;
  const double k3 = 0.0;
  // iR = inverse of K through its determinant
  const double d = 1.0 / (fx * fy);
  const double ir0 = fy * d, ir2 = -(cx * fy) * d, ir4 = fx * d, ir5 = -(fx * cy) * d, ir8 = (fx * fy) * d;
  double _x = i * 0.0 + ir2;
  const double _y = i * ir4 + ir5, _w = i * 0.0 + ir8;
  const size_t row = (size_t)i * w;
  for (int j = 0; j < w; ++j, _x += ir0) {
    const double iw = 1.0 / _w, x = _x * iw, y = _y * iw;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + cx;
    const double v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + cy;
    const float mx = (float)u, my = (float)v;
    mapx[row + j] = mx;
    mapy[row + j] = my;
    // remap's fixed-point form: sx = X >> 5 saturated to int16 (a side is at most 32767 pixels, so an outside tap
    // stays outside), the fraction X & 31
    const int X = fixed5(mx), Y = fixed5(my);
    FixPos f;
    f.sx = sat16(X >> 5);
    f.sy = sat16(Y >> 5);
    f.a = (uint16_t)((Y & 31) * 32 + (X & 31));
    f.pad = 0;
    fix[row + j] = f;
  }
}

// remapBilinear (OpenCV 2.x, imgwarp.cpp) on 8-bit pixels, BORDER_CONSTANT 0: one thread per output pixel,
// blockIdx.z = image of a batch (all of one size, every one with the map of its camera)
__global__ void remap_kernel(RemapImages imgs, int w, int h) {
  const size_t n = (size_t)w * h;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint8_t* __restrict__ src = imgs.src[blockIdx.z];
  const FixPos* __restrict__ fix = imgs.fix[blockIdx.z];
  const FixPos f = fix[p];
  const int sx = f.sx, sy = f.sy, ax = f.a & 31, ay = f.a >> 5;
  const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
  const bool y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
  const size_t r0 = (size_t)sy * w, r1 = r0 + w;
  const int v00 = x0 && y0 ? src[r0 + sx] : 0;
  const int v10 = x1 && y0 ? src[r0 + sx + 1] : 0;
  const int v01 = x0 && y1 ? src[r1 + sx] : 0;
  const int v11 = x1 && y1 ? src[r1 + sx + 1] : 0;
  // weights of INTER_REMAP_COEF_SCALE = 2^15; the sum is at most 255 2^15, so the result fits 8 bits
  const int s = v00 * ((32 - ax) * (32 - ay) * 32) + v10 * (ax * (32 - ay) * 32) + v01 * ((32 - ax) * ay * 32) +
                v11 * (ax * ay * 32);
  imgs.dst[blockIdx.z][p] = (uint8_t)((s + (1 << 14)) >> 15);
}

bool finite4(const float* v) {
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

int bad(mh_ctx* ctx, const char* what, const char* why) {
  if (ctx) ctx->err = std::string(what) + ": " + why;
  return MH_ERR_ARG;
}

int check_camera(mh_ctx* ctx, const char* what, int width, int height, const float* K, const float* dist) {
  if (!K || !dist) return bad(ctx, what, "null calibration");
  if (width <= 0 || height <= 0 || width > UND_MAX_SIDE || height > UND_MAX_SIDE)
    return bad(ctx, what, "width and height must lie in 1 .. 32767");
  if (!finite4(K) || !finite4(dist)) return bad(ctx, what, "non-finite calibration");
  if (K[0] == 0.f || K[1] == 0.f) return bad(ctx, what, "fx and fy must not be 0");
  return MH_OK;
}

}  // namespace

// The context's maps (UTIL_UNDISTORT.hpp:52-66 keys them by size and calibration) and staging buffers.
struct UndistortState {
  UndMap maps[UND_ENTRIES];
  uint64_t tick = 0;
  DevBuf<uint8_t> in;    // mh_undistort: the host image
  DevBuf<uint8_t> out;   // mh_undistort's result; the resident path's undistorted image(s)
};

namespace {

// the map of (width, height, K, dist), built on the context's stream on a miss (no host synchronisation unless an
// entry has to grow)
int get_map(mh_ctx* ctx, int width, int height, const float* K, const float* dist, UndMap** out) {
  if (!ctx->und) ctx->und = new UndistortState;
  UndistortState* st = ctx->und;
  UndMap* slot = nullptr;
  for (UndMap& m : st->maps) {
    if (m.used && m.width == width && m.height == height && m.K[0] == K[0] && m.K[1] == K[1] && m.K[2] == K[2] &&
        m.K[3] == K[3] && m.dist[0] == dist[0] && m.dist[1] == dist[1] && m.dist[2] == dist[2] && m.dist[3] == dist[3]) {
      m.used = ++st->tick;
      *out = &m;
      return MH_OK;
    }
    if (!slot || m.used < slot->used) slot = &m;   // an empty entry, else the least recently used
  }
  const size_t n = (size_t)width * height;
  if (n > slot->cap) {
    slot->cap = 0;
    slot->used = 0;
    MH_HIP(ctx, slot->mapx.ensure(n, ctx->stream));
    MH_HIP(ctx, slot->mapy.ensure(n, ctx->stream));
    MH_HIP(ctx, slot->fix.ensure(n, ctx->stream));
    slot->cap = n;
  }
  slot->width = width;
  slot->height = height;
  std::memcpy(slot->K, K, sizeof slot->K);
  std::memcpy(slot->dist, dist, sizeof slot->dist);
  // float calibration widened to double as the reference's CV_32F matrices are (:77-87)
  hipLaunchKernelGGL(map_build_kernel, dim3((height + 63) / 64), dim3(64), 0, ctx->stream, width, height, (double)K[0],
                     (double)K[1], (double)K[2], (double)K[3], (double)dist[0], (double)dist[1], (double)dist[2],
                     (double)dist[3], slot->mapx, slot->mapy, slot->fix);
  MH_HIP(ctx, hipGetLastError());
  slot->used = ++st->tick;
  *out = slot;
  return MH_OK;
}

// maps[f % n_maps] = the map of image f (a rig's images lie camera after camera, frame after frame)
int launch_remap(mh_ctx* ctx, UndMap* const* maps, int n_maps, const uint8_t* const* src, uint8_t* const* dst, int n_images) {
  RemapImages imgs = {};
  for (int f = 0; f < n_images; ++f) {
    imgs.src[f] = src[f];
    imgs.dst[f] = dst[f];
    imgs.fix[f] = maps[f % n_maps]->fix;
  }
  const UndMap* m = maps[0];
  const size_t n = (size_t)m->width * m->height;
  hipLaunchKernelGGL(remap_kernel, dim3((unsigned)((n + 255) / 256), 1, n_images), dim3(256), 0, ctx->stream, imgs,
                     m->width, m->height);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}
int launch_remap(mh_ctx* ctx, UndMap* m, const uint8_t* const* src, uint8_t* const* dst, int n_images) {
  return launch_remap(ctx, &m, 1, src, dst, n_images);
}

int enter(mh_ctx* ctx) {
  MH_HIP(ctx, hipSetDevice(ctx->device));
  return mh::use_stream(ctx);
}

}  // namespace

namespace mh {

// The resident image path (mh_frame_set_undistort): the n images remapped into the context's staging buffer with
// the map of (width, height, K, ctx->und_dist), one launch; staged[f] = image f's undistorted copy.
int undistort_frame(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int width, int height, const float K[4],
                    const uint8_t** staged) {
  if (int rc = check_camera(ctx, "mh_frame_enqueue_image (undistortion)", width, height, K, ctx->und_dist)) return rc;
  UndMap* m = nullptr;
  if (int rc = get_map(ctx, width, height, K, ctx->und_dist, &m)) return rc;
  const size_t px = (size_t)width * height;
  UndistortState* st = ctx->und;
  MH_HIP(ctx, st->out.ensure(px * n, ctx->stream));
  uint8_t* dst[MH_MAX_BATCH];
  for (int f = 0; f < n; ++f) dst[f] = st->out + f * px;
  if (int rc = launch_remap(ctx, m, gray_dev, dst, n)) return rc;
  for (int f = 0; f < n; ++f) staged[f] = dst[f];   // (after the launch: staged may be gray_dev itself)
  return MH_OK;
}

// Frames with several cameras (mh_frame_enqueue_images*): image f belongs to camera f % n_cams and is remapped with the
// map of (width, height, cams[f % n_cams].K, dist[f % n_cams]) -- the entries of the same cache, still one launch.
int undistort_frame_images(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int n_cams, int width, int height,
                           const mh_cam* cams, const float (*dist)[4], const uint8_t** staged) {
  static_assert(UND_ENTRIES >= MH_MAX_IMAGES, "a rig's maps must fit the cache together");
  if (n_cams < 1 || n_cams > MH_MAX_IMAGES) return bad(ctx, "mh_frame_enqueue_images (undistortion)", "camera count");
  for (int i = 0; i < n_cams; ++i)
    if (int rc = check_camera(ctx, "mh_frame_enqueue_images (undistortion)", width, height, cams[i].K, dist[i])) return rc;
  UndMap* maps[MH_MAX_IMAGES];
  for (int i = 0; i < n_cams; ++i)   // (a miss evicts the least recently used entry: never one this loop has just touched)
    if (int rc = get_map(ctx, width, height, cams[i].K, dist[i], &maps[i])) return rc;
  const size_t px = (size_t)width * height;
  UndistortState* st = ctx->und;
  MH_HIP(ctx, st->out.ensure(px * n, ctx->stream));
  uint8_t* dst[MH_MAX_BATCH];
  for (int f = 0; f < n; ++f) dst[f] = st->out + f * px;
  if (int rc = launch_remap(ctx, maps, n_cams, gray_dev, dst, n)) return rc;
  for (int f = 0; f < n; ++f) staged[f] = dst[f];
  return MH_OK;
}

}  // namespace mh

extern "C" {

void mh_free_undistort_state(mh_ctx* ctx) {
  delete ctx->und;
  ctx->und = nullptr;
}

int mh_undistort_map(mh_ctx* ctx, int width, int height, const float K[4], const float dist[4], float* mapx_host,
                     float* mapy_host) {
  if (!ctx) return MH_ERR_ARG;
  if (!mapx_host || !mapy_host) return bad(ctx, "mh_undistort_map", "null pointer");
  if (int rc = check_camera(ctx, "mh_undistort_map", width, height, K, dist)) return rc;
  if (int rc = enter(ctx)) return rc;
  UndMap* m = nullptr;
  if (int rc = get_map(ctx, width, height, K, dist, &m)) return rc;
  const size_t bytes = (size_t)width * height * sizeof(float);
  MH_HIP(ctx, hipMemcpyAsync(mapx_host, m->mapx, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(mapy_host, m->mapy, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_undistort(mh_ctx* ctx, const uint8_t* gray_host, uint8_t* out_host, int width, int height, const float K[4],
                 const float dist[4]) {
  if (!ctx) return MH_ERR_ARG;
  if (!gray_host || !out_host) return bad(ctx, "mh_undistort", "null pointer");
  if (int rc = check_camera(ctx, "mh_undistort", width, height, K, dist)) return rc;
  if (int rc = enter(ctx)) return rc;
  UndMap* m = nullptr;
  if (int rc = get_map(ctx, width, height, K, dist, &m)) return rc;
  UndistortState* st = ctx->und;
  const size_t px = (size_t)width * height;
  MH_HIP(ctx, st->in.ensure(px, ctx->stream));
  MH_HIP(ctx, st->out.ensure(px, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(st->in, gray_host, px, hipMemcpyHostToDevice, ctx->stream));
  const uint8_t* src = st->in;
  uint8_t* dst = st->out;
  if (int rc = launch_remap(ctx, m, &src, &dst, 1)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(out_host, st->out, px, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}

int mh_undistort_dev(mh_ctx* ctx, const uint8_t* gray_dev, uint8_t* out_dev, int width, int height, const float K[4],
                     const float dist[4]) {
  if (!ctx) return MH_ERR_ARG;
  if (!gray_dev || !out_dev) return bad(ctx, "mh_undistort_dev", "null pointer");
  if ((const void*)gray_dev == (const void*)out_dev) return bad(ctx, "mh_undistort_dev", "out must differ from in");
  if (int rc = check_camera(ctx, "mh_undistort_dev", width, height, K, dist)) return rc;
  if (int rc = enter(ctx)) return rc;
  UndMap* m = nullptr;
  if (int rc = get_map(ctx, width, height, K, dist, &m)) return rc;
  return launch_remap(ctx, m, &gray_dev, &out_dev, 1);
}

int mh_frame_set_undistort(mh_ctx* ctx, const float dist[4]) {
  if (!ctx) return MH_ERR_ARG;
  if (!dist) {
    ctx->und_on = false;
    return MH_OK;
  }
  if (!finite4(dist)) return bad(ctx, "mh_frame_set_undistort", "non-finite coefficients");
  std::memcpy(ctx->und_dist, dist, sizeof ctx->und_dist);
  ctx->und_on = true;
  return MH_OK;
}

int mh_frame_set_undistort_images(mh_ctx* ctx, const float (*dist)[4], int n_images) {
  if (!ctx) return MH_ERR_ARG;
  if (!dist || n_images <= 0) {
    ctx->imf.und_n = 0;
    return MH_OK;
  }
  if (n_images > MH_MAX_IMAGES) {
    ctx->err = "mh_frame_set_undistort_images: more than MH_MAX_IMAGES cameras";
    return MH_ERR_CAPACITY;
  }
  for (int i = 0; i < n_images; ++i)
    if (!finite4(dist[i])) return bad(ctx, "mh_frame_set_undistort_images", "non-finite coefficients");
  std::memcpy(ctx->imf.und_dist, dist, sizeof(float) * 4 * n_images);
  ctx->imf.und_n = n_images;
  return MH_OK;
}

}  // extern "C"
