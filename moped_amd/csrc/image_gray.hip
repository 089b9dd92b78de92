// The 8-bit gray image from what a camera delivers, on the device: the first line of moped3d's image callback,
// cv_bridge::toCvCopy(iMsg, "mono8") (moped3d/moped3d.cpp:249).  A raw buffer -- 8-bit gray with strides, interleaved
// bgr8 / rgb8 / bgra8 / rgba8, or a Bayer mosaic -- in, the packed [height][width] gray image every image entry point
// takes out.
//
// The arithmetic restates what OpenCV 2.x cvtColor does for 8-bit data, WITHOUT OpenCV at hand: UNPINNED, like every
// other OpenCV call the project restates.  Integers only, unsigned 32-bit, the largest sum below 2^25:
//   R2Y = 4899, G2Y = 9617, B2Y = 1868 (sum 2^14)
//   gray8          the byte
//   interleaved    (R2Y R + G2Y G + B2Y B + 8192) >> 14, alpha ignored
//   Bayer          interior site (x, y) with byte p, ca = the coefficient of the row's colour (R or B), cb = the other's:
//                    R or B site   (cb (4 diagonal) + G2Y (4 edge) + 4 ca p + 32768) >> 16
//                    G site        (ca (left + right) + cb (up + down) + 2 G2Y p + 16384) >> 15
//                  (the own colour of an R / B site and the horizontal neighbours of a G site are the row's colour, the
//                  opposite colour and the vertical neighbours the other one; the sums are taken column by column, up +
//                  down first -- integers, so the same bits in any order); columns 0 and w - 1 copy 1 and w - 2, then
//                  rows 0 and h - 1 copy 1 and h - 2: pixel (x, y) = the interior value at (clamp(x, 1, w - 2),
//                  clamp(y, 1, h - 2)).
//
// A pure stream, no LDS, no atomics.  Neither pointer is aligned to anything and 3-byte pixels never line up with
// dwords, so every output row is cut at the 8-byte boundaries of ITS OWN output address: run 0 is the row's head (0 .. 7
// pixels), run k >= 1 the eight pixels behind it, the last one the tail.  One thread owns one run.  A whole run whose
// input lies inside the extent moves words: the aligned dwords that cover its input bytes (2, 6 or 8 of them and one
// more when the input address is odd; Bayer: 3 + 1 for each of the three rows, ten bytes each, shared by the run's eight
// pixels), a funnel shift to the byte address, one 8-byte store.  Heads, tails, Bayer's border columns and a run whose
// dwords would reach over either end of the extent go byte by byte (Bayer: a sliding 3 x 3 window, three loads per
// step).  Hence no load outside [raw, raw + offset + (h - 1) row_stride + w bpp), no store outside [out, out + w h).
// blockIdx.y = the image of a batch; one launch for any image of fewer than 2^32 - 256 runs (else one per range of rows).  At 640 x 480 bgr8 the call moves 0.92 MB in and 0.31 MB out: its time is the
// launch's, which is why a batch is one launch (profiles/image_gray.txt).
// tests/image_gray_ref.py restates the arithmetic in numpy; tests/test_gpu_image_gray.py compares the bytes.
#include <climits>

#include "frame.h"
#include "image_fmt_check.h"

namespace mh {

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_RUN = 8;   // output pixels of a run = bytes of its store
constexpr unsigned IG_R2Y = 4899u, IG_G2Y = 9617u, IG_B2Y = 1868u;

enum { IG_COPY = 0, IG_PIX3 = 3, IG_PIX4 = 4, IG_BAYER = 9 };

struct IgImages {
  const unsigned char* raw[MH_MAX_BATCH] = {};
  unsigned char* out[MH_MAX_BATCH] = {};
};
struct IgDesc {
  int w, h, row_stride, offset;
  unsigned extent;   // bytes of the raw buffer the description speaks of
  unsigned c0, c2;   // interleaved: the coefficients of a pixel's bytes 0 and 2 (byte 1 is G)
  int g_par, r_row;  // Bayer: site (x, y) is G where ((x + y) & 1) == g_par; rows with (y & 1) == r_row hold R
  int y0, rows;      // the launch converts rows [y0, y0 + rows) of every image
};

// The NW dwords that begin at byte address p: the aligned dwords covering them, shifted.  The caller has asked
// ig_words_inside for the same p and NW.
template <int NW>
__device__ __forceinline__ void ig_load_words(const unsigned char* __restrict__ p, unsigned (&v)[NW]) {
  const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
  const unsigned* __restrict__ al = reinterpret_cast<const unsigned*>(p - sh);
  unsigned t[NW + 1];
#pragma unroll
  for (int i = 0; i < NW; ++i) t[i] = al[i];
  t[NW] = sh ? al[NW] : 0u;
#pragma unroll
  for (int i = 0; i < NW; ++i) v[i] = (unsigned)((((unsigned long long)t[i + 1] << 32) | t[i]) >> (8u * sh));
}
// ... all of which lie inside [raw, raw + extent): at = p - raw
template <int NW>
__device__ __forceinline__ bool ig_words_inside(const unsigned char* raw, size_t at, unsigned extent) {
  const long long sh = (long long)(reinterpret_cast<uintptr_t>(raw + at) & 3u);
  const long long lo = (long long)at - sh, hi = lo + 4 * (NW + (sh ? 1 : 0));
  return lo >= 0 && hi <= (long long)extent;
}
__device__ __forceinline__ unsigned ig_byte(const unsigned* v, int j) { return (v[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// an interior Bayer site from its centre p, h = left + right, v1 = up + down and the two vertical sums beside it
// (v0 = up-left + down-left, v2 = up-right + down-right)
__device__ __forceinline__ unsigned ig_bayer_g(unsigned p, unsigned h, unsigned v1, unsigned ca, unsigned cb) {
  return (ca * h + cb * v1 + 2u * IG_G2Y * p + 16384u) >> 15;
}
__device__ __forceinline__ unsigned ig_bayer_c(unsigned p, unsigned h, unsigned v0, unsigned v1, unsigned v2, unsigned ca, unsigned cb) {
  return (cb * (v0 + v2) + IG_G2Y * (v1 + h) + 4u * ca * p + 32768u) >> 16;
}
// eight sites in a row from the ten columns under them: G_EVEN = the run's pixels 0, 2, 4, 6 are the G sites
template <bool G_EVEN>
__device__ __forceinline__ void ig_bayer_run(const unsigned (&up)[3], const unsigned (&mid)[3], const unsigned (&dn)[3], unsigned ca,
                                             unsigned cb, unsigned (&g)[IG_RUN]) {
  unsigned v[IG_RUN + 2], m[IG_RUN + 2];
#pragma unroll
  for (int j = 0; j < IG_RUN + 2; ++j) {
    v[j] = ig_byte(up, j) + ig_byte(dn, j);
    m[j] = ig_byte(mid, j);
  }
#pragma unroll
  for (int j = 0; j < IG_RUN; ++j) {
    const unsigned h = m[j] + m[j + 2];
    g[j] = ((j & 1) == 0) == G_EVEN ? ig_bayer_g(m[j + 1], h, v[j + 1], ca, cb) : ig_bayer_c(m[j + 1], h, v[j], v[j + 1], v[j + 2], ca, cb);
  }
}

__device__ __forceinline__ void ig_store_run(unsigned char* __restrict__ dst, const unsigned (&g)[IG_RUN]) {
  uint2 o;
  o.x = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
  o.y = g[4] | (g[5] << 8) | (g[6] << 16) | (g[7] << 24);
  *reinterpret_cast<uint2*>(dst) = o;   // (8-byte aligned: that is where the runs are cut)
}

template <int KIND>
__global__ void __launch_bounds__(IG_THREADS) image_gray_kernel(IgImages im, IgDesc d, unsigned runs_per_row) {
  const unsigned i = blockIdx.x * IG_THREADS + threadIdx.x;   // (rows runs_per_row + 255 < 2^32: launch_image_gray)
  const unsigned row = i / runs_per_row;
  if (row >= (unsigned)d.rows) return;
  const unsigned k = i - row * runs_per_row;   // the thread's run inside its row
  const int y = d.y0 + (int)row;
  const unsigned char* __restrict__ raw = im.raw[blockIdx.y];
  unsigned char* __restrict__ out = im.out[blockIdx.y] + (size_t)y * (size_t)d.w;
  const unsigned w = (unsigned)d.w;
  const unsigned head = min(w, (unsigned)((0 - reinterpret_cast<uintptr_t>(out)) & (uintptr_t)(IG_RUN - 1)));
  const unsigned x0 = k == 0 ? 0u : head + (k - 1) * IG_RUN;   // (<= w + 15 < 2^32)
  if (x0 >= w) return;
  const unsigned x1 = k == 0 ? head : min(w, x0 + IG_RUN);
  if (x0 >= x1) return;
  const bool whole = x1 - x0 == IG_RUN && k > 0;

  if constexpr (KIND == IG_BAYER) {
    const int ys = min(max(y, 1), d.h - 2);
    const size_t at = (size_t)d.offset + (size_t)ys * (size_t)d.row_stride;   // row ys, column 0
    const size_t stride = (size_t)d.row_stride;
    const bool r_row = (ys & 1) == d.r_row;
    const unsigned ca = r_row ? IG_R2Y : IG_B2Y, cb = r_row ? IG_B2Y : IG_R2Y;
    // columns x0 - 1 .. x0 + 8 of the three rows: ten bytes in three dwords each
    if (whole && x0 >= 1 && x1 + 1 <= w) {
      const size_t a0 = at + x0 - 1;
      if (ig_words_inside<3>(raw, a0 - stride, d.extent) && ig_words_inside<3>(raw, a0, d.extent) &&
          ig_words_inside<3>(raw, a0 + stride, d.extent)) {
        unsigned up[3], mid[3], dn[3], g[IG_RUN];
        ig_load_words<3>(raw + a0 - stride, up);
        ig_load_words<3>(raw + a0, mid);
        ig_load_words<3>(raw + a0 + stride, dn);
        if ((((int)x0 + ys) & 1) == d.g_par)   // (the same for every run of a row: x0 = head + 8 (k - 1))
          ig_bayer_run<true>(up, mid, dn, ca, cb, g);
        else
          ig_bayer_run<false>(up, mid, dn, ca, cb, g);
        ig_store_run(out + x0, g);
        return;
      }
    }
    // by bytes: the 3 x 3 window slides with the clamped column (c[row][column])
    unsigned c[3][3];
    int cur = -2;
    for (unsigned x = x0; x < x1; ++x) {
      const int xs = min(max((int)x, 1), d.w - 2);
      if (xs != cur) {
        const unsigned char* __restrict__ p = raw + (at - stride) + (size_t)(xs - 1);   // row ys - 1, column xs - 1
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (xs == cur + 1) {   // one step to the right: only the new right column is loaded
            c[r][0] = c[r][1];
            c[r][1] = c[r][2];
          } else {
            c[r][0] = p[(size_t)r * stride];
            c[r][1] = p[(size_t)r * stride + 1];
          }
          c[r][2] = p[(size_t)r * stride + 2];
        }
        cur = xs;
      }
      const unsigned h = c[1][0] + c[1][2], v0 = c[0][0] + c[2][0], v1 = c[0][1] + c[2][1], v2 = c[0][2] + c[2][2];
      out[x] = (unsigned char)(((xs + ys) & 1) == d.g_par ? ig_bayer_g(c[1][1], h, v1, ca, cb) : ig_bayer_c(c[1][1], h, v0, v1, v2, ca, cb));
    }
  } else {
    constexpr int BPP = KIND == IG_COPY ? 1 : KIND;
    constexpr int NW = IG_RUN * BPP / 4;
    const size_t at = (size_t)d.offset + (size_t)y * (size_t)d.row_stride + (size_t)x0 * BPP;
    if (whole && ig_words_inside<NW>(raw, at, d.extent)) {
      unsigned v[NW], g[IG_RUN];
      ig_load_words<NW>(raw + at, v);
#pragma unroll
      for (int j = 0; j < IG_RUN; ++j) {
        if constexpr (KIND == IG_COPY)
          g[j] = ig_byte(v, j);
        else
          g[j] = (d.c0 * ig_byte(v, j * BPP) + IG_G2Y * ig_byte(v, j * BPP + 1) + d.c2 * ig_byte(v, j * BPP + 2) + 8192u) >> 14;
      }
      ig_store_run(out + x0, g);
      return;
    }
    const unsigned char* __restrict__ p = raw + at;
    for (unsigned x = x0; x < x1; ++x, p += BPP) {
      if constexpr (KIND == IG_COPY)
        out[x] = p[0];
      else
        out[x] = (unsigned char)((d.c0 * p[0] + IG_G2Y * p[1] + d.c2 * p[2] + 8192u) >> 14);
    }
  }
}

// n images in one launch on the context's stream; the arguments are checked (image_call_why)
int launch_image_gray(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_image* f, uint8_t* const* out_dev, int n) {
  IgImages im;
  for (int i = 0; i < n; ++i) {
    im.raw[i] = static_cast<const unsigned char*>(raw_dev[i]);
    im.out[i] = out_dev[i];
  }
  IgDesc d = {};
  d.w = f->width;
  d.h = f->height;
  d.row_stride = f->row_stride;
  d.offset = f->offset;
  d.extent = (unsigned)image_extent(f);
  const bool r_first = f->format == MH_IMAGE_RGB8 || f->format == MH_IMAGE_RGBA8;
  d.c0 = r_first ? IG_R2Y : IG_B2Y;
  d.c2 = r_first ? IG_B2Y : IG_R2Y;
  d.g_par = f->format == MH_IMAGE_BAYER_RGGB8 || f->format == MH_IMAGE_BAYER_BGGR8 ? 1 : 0;
  d.r_row = f->format == MH_IMAGE_BAYER_BGGR8 || f->format == MH_IMAGE_BAYER_GBRG8 ? 1 : 0;
  const unsigned runs_per_row = (unsigned)((f->width + IG_RUN - 1) / IG_RUN) + 1u;   // the head, the whole runs, the tail
  // A grid holds fewer than 2^32 threads: an image of more rows than that allows (more than 26 million rows of 1280 pixels;
  // no camera's) goes in several launches, each a range of rows.
  const int rows_max = (int)std::min<unsigned long long>((unsigned long long)f->height, ((1ull << 32) - IG_THREADS) / runs_per_row);
  const int bpp = image_bpp(f->format);
  for (d.y0 = 0; d.y0 < f->height; d.y0 += d.rows) {
    d.rows = std::min(rows_max, f->height - d.y0);
    const unsigned long long threads = (unsigned long long)d.rows * runs_per_row;
    const dim3 grid((unsigned)((threads + IG_THREADS - 1) / IG_THREADS), (unsigned)n), block(IG_THREADS);
    if (image_is_bayer(f->format))
      hipLaunchKernelGGL(image_gray_kernel<IG_BAYER>, grid, block, 0, ctx->stream, im, d, runs_per_row);
    else if (bpp == 1)
      hipLaunchKernelGGL(image_gray_kernel<IG_COPY>, grid, block, 0, ctx->stream, im, d, runs_per_row);
    else if (bpp == 3)
      hipLaunchKernelGGL(image_gray_kernel<IG_PIX3>, grid, block, 0, ctx->stream, im, d, runs_per_row);
    else
      hipLaunchKernelGGL(image_gray_kernel<IG_PIX4>, grid, block, 0, ctx->stream, im, d, runs_per_row);
  }
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int refuse(mh_ctx* ctx, const char* who, const char* why) {
  ctx->err = std::string(who) + ": " + why;
  return MH_ERR_ARG;
}

}  // namespace

int image_format_frame_ok(mh_ctx* ctx, const char* who, int width, int height) {
  if (!ctx->img_fmt_on || (width == ctx->img_fmt.width && height == ctx->img_fmt.height)) return MH_OK;
  return refuse(ctx, who, "width and height are not those of the image format (mh_frame_set_image_format)");
}

size_t image_format_bytes(const mh_ctx* ctx, int width, int height) {
  return ctx->img_fmt_on ? image_extent(&ctx->img_fmt) : (size_t)width * (size_t)height;
}

int image_format_stage(mh_ctx* ctx, const uint8_t* const* raw_dev, int n, const uint8_t** staged) {
  if (!ctx->img_fmt_on) return MH_OK;
  const size_t px = (size_t)ctx->img_fmt.width * (size_t)ctx->img_fmt.height;
  MH_HIP(ctx, ctx->img_stage.ensure(px * (size_t)n, ctx->stream));
  const void* src[MH_MAX_BATCH];
  uint8_t* dst[MH_MAX_BATCH];
  for (int f = 0; f < n; ++f) {
    src[f] = raw_dev[f];
    dst[f] = ctx->img_stage + (size_t)f * px;
  }
  if (int rc = launch_image_gray(ctx, src, &ctx->img_fmt, dst, n)) return rc;
  for (int f = 0; f < n; ++f) staged[f] = dst[f];   // (after the launch: staged may be raw_dev itself)
  return MH_OK;
}

}  // namespace mh

using namespace mh;

extern "C" int mh_image_gray_batch_dev(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_image* fmt,
                                       uint8_t* const* gray_dev, int n) {
  if (!ctx) return MH_ERR_ARG;
  if (const char* why = image_call_why(raw_dev, fmt, gray_dev, n)) return refuse(ctx, "mh_image_gray_batch_dev", why);
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  return launch_image_gray(ctx, raw_dev, fmt, gray_dev, n);
}

extern "C" int mh_image_gray_dev(mh_ctx* ctx, const void* raw_dev, const mh_raw_image* fmt, uint8_t* gray_dev) {
  return mh_image_gray_batch_dev(ctx, &raw_dev, fmt, &gray_dev, 1);
}

extern "C" int mh_image_gray_host(mh_ctx* ctx, const void* raw_host, const mh_raw_image* fmt, uint8_t* gray_host) {
  if (!ctx) return MH_ERR_ARG;
  if (const char* why = image_call_why(&raw_host, fmt, &gray_host, 1)) return refuse(ctx, "mh_image_gray_host", why);
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const size_t extent = image_extent(fmt), px = (size_t)fmt->width * (size_t)fmt->height;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, ctx->img_raw.ensure(extent, s));
  MH_HIP(ctx, ctx->img_stage.ensure(px, s));
  MH_HIP(ctx, hipMemcpyAsync(ctx->img_raw, raw_host, extent, hipMemcpyHostToDevice, s));
  const void* src = ctx->img_raw.p;
  uint8_t* dst = ctx->img_stage.p;
  if (int rc = launch_image_gray(ctx, &src, fmt, &dst, 1)) return rc;
  MH_HIP(ctx, hipMemcpyAsync(gray_host, dst, px, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));   // the host's buffers are the caller's again after the call
  return MH_OK;
}

extern "C" int mh_frame_set_image_format(mh_ctx* ctx, const mh_raw_image* fmt) {
  if (!ctx) return MH_ERR_ARG;
  if (!fmt) {
    ctx->img_fmt_on = false;
    return MH_OK;
  }
  if (const char* why = image_fmt_why(fmt)) return refuse(ctx, "mh_frame_set_image_format", why);
  ctx->img_fmt = *fmt;
  ctx->img_fmt_on = true;
  return MH_OK;
}
