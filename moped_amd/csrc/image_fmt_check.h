// Host-only parts of the sensor image conversion (image_gray.hip): what a description is, how many bytes it spans, and
// what the entry points refuse before anything is launched.  No HIP in here, so that a plain C++ program can run them
// under the sanitizers (host/image_fmt_check_test.cpp).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/moped_hip.h"

namespace mh {

// bytes per pixel; 0 = no such format
inline int image_bpp(int format) {
  switch (format) {
    case MH_IMAGE_GRAY8:
    case MH_IMAGE_BAYER_RGGB8:
    case MH_IMAGE_BAYER_BGGR8:
    case MH_IMAGE_BAYER_GBRG8:
    case MH_IMAGE_BAYER_GRBG8: return 1;
    case MH_IMAGE_BGR8:
    case MH_IMAGE_RGB8: return 3;
    case MH_IMAGE_BGRA8:
    case MH_IMAGE_RGBA8: return 4;
    default: return 0;
  }
}
inline bool image_is_bayer(int format) { return format >= MH_IMAGE_BAYER_RGGB8 && format <= MH_IMAGE_BAYER_GRBG8; }

// why a description is refused (nullptr: it is not); every product in 64 bits
inline const char* image_fmt_why(const mh_raw_image* f) {
  if (!f) return "no mh_raw_image";
  const int bpp = image_bpp(f->format);
  if (!bpp) return "an unknown format";
  if (f->width <= 0 || f->height <= 0) return "a width or height that is not positive";
  if (image_is_bayer(f->format) && (f->width < 3 || f->height < 3)) return "a Bayer image below 3 x 3";
  if (f->offset < 0) return "a negative offset";
  if ((long long)f->row_stride < (long long)f->width * bpp) return "a row_stride below width times the bytes of a pixel";
  if ((long long)f->width * f->height > INT_MAX) return "width times height beyond INT_MAX";
  const long long extent = (long long)f->offset + (long long)(f->height - 1) * f->row_stride + (long long)f->width * bpp;
  if (extent > INT_MAX) return "an extent (offset + (height - 1) row_stride + width bytes-per-pixel) beyond INT_MAX";
  return nullptr;
}

// the bytes [raw, raw + extent) a checked description speaks of
inline size_t image_extent(const mh_raw_image* f) {
  return (size_t)f->offset + (size_t)(f->height - 1) * (size_t)f->row_stride + (size_t)f->width * (size_t)image_bpp(f->format);
}

inline bool image_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// why a call over n raw buffers and n outputs of one description is refused (nullptr: it is not).  One launch converts
// them all, so no output may touch another output or any raw buffer of the call, its own first of all.
inline const char* image_call_why(const void* const* raw, const mh_raw_image* f, uint8_t* const* out, int n) {
  if (!raw || !out) return "a null pointer array";
  if (n < 1 || n > MH_MAX_BATCH) return "n outside 1 .. MH_MAX_BATCH";
  if (const char* why = image_fmt_why(f)) return why;
  for (int i = 0; i < n; ++i)
    if (!raw[i] || !out[i]) return "a null image pointer";
  const size_t extent = image_extent(f), px = (size_t)f->width * (size_t)f->height;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < i; ++j)
      if (image_ranges_overlap(out[i], px, out[j], px)) return "two images writing the same output";
    for (int j = 0; j < n; ++j)
      if (image_ranges_overlap(out[i], px, raw[j], extent))
        return j == i ? "an output that overlaps its own raw buffer" : "an output that overlaps a raw buffer of the batch";
  }
  return nullptr;
}

}  // namespace mh
