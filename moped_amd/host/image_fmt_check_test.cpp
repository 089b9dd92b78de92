// image_fmt_check_test -- the host-only parts of the sensor image conversion (csrc/image_fmt_check.h) under ASan + UBSan:
// every refusal of mh_image_gray_* / mh_frame_set_image_format on its own, the extent arithmetic at the edges of int, and
// the overlap rule at its four boundaries.  No GPU, no HIP runtime.  `make image_fmt_check_check`.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/image_fmt_check.h"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static bool says(const char* why, const char* part) { return why && std::strstr(why, part); }

static mh_raw_image make(int format, int w, int h, int row_stride, int offset) {
  mh_raw_image f;
  f.format = format;
  f.width = w;
  f.height = h;
  f.row_stride = row_stride;
  f.offset = offset;
  return f;
}

int main() {
  // ---- a description ----
  for (int format = MH_IMAGE_GRAY8; format <= MH_IMAGE_BAYER_GRBG8; ++format) {
    const int bpp = mh::image_bpp(format);
    CHECK(bpp == (format == MH_IMAGE_BGR8 || format == MH_IMAGE_RGB8 ? 3 : format == MH_IMAGE_BGRA8 || format == MH_IMAGE_RGBA8 ? 4 : 1));
    CHECK(mh::image_is_bayer(format) == (format >= MH_IMAGE_BAYER_RGGB8));
    mh_raw_image f = make(format, 640, 480, 640 * bpp, 0);
    CHECK(mh::image_fmt_why(&f) == nullptr);
    CHECK(mh::image_extent(&f) == (size_t)640 * 480 * bpp);
    f = make(format, 641, 479, 641 * bpp + 13, 3);
    CHECK(mh::image_fmt_why(&f) == nullptr);
    CHECK(mh::image_extent(&f) == 3 + (size_t)478 * (641 * bpp + 13) + (size_t)641 * bpp);
    f = make(format, 641, 479, 641 * bpp - 1, 0);
    CHECK(says(mh::image_fmt_why(&f), "row_stride"));
    f = make(format, 3, 3, 3 * bpp, -1);
    CHECK(says(mh::image_fmt_why(&f), "negative offset"));
    f = make(format, 0, 3, 12, 0);
    CHECK(says(mh::image_fmt_why(&f), "not positive"));
    f = make(format, 3, INT_MIN, 12, 0);
    CHECK(says(mh::image_fmt_why(&f), "not positive"));
    f = make(format, 2, 3, 8, 0);
    CHECK(mh::image_is_bayer(format) ? says(mh::image_fmt_why(&f), "Bayer") : mh::image_fmt_why(&f) == nullptr);
    f = make(format, 3, 2, 12, 0);
    CHECK(mh::image_is_bayer(format) ? says(mh::image_fmt_why(&f), "Bayer") : mh::image_fmt_why(&f) == nullptr);
  }
  CHECK(mh::image_bpp(-1) == 0 && mh::image_bpp(9) == 0 && mh::image_bpp(INT_MAX) == 0);
  {
    mh_raw_image f = make(9, 4, 4, 16, 0);
    CHECK(says(mh::image_fmt_why(&f), "unknown format"));
    f.format = -1;
    CHECK(says(mh::image_fmt_why(&f), "unknown format"));
    CHECK(says(mh::image_fmt_why(nullptr), "no mh_raw_image"));
  }
  // ---- the edges of int: every product is taken in 64 bits ----
  {
    mh_raw_image f = make(MH_IMAGE_GRAY8, 46341, 46341, 46341, 0);   // w h = 2^31 + 4 880
    CHECK(says(mh::image_fmt_why(&f), "width times height"));
    f = make(MH_IMAGE_GRAY8, 46340, 46340, 46340, 0);                 // w h = 2 147 395 600: the largest square
    CHECK(mh::image_fmt_why(&f) == nullptr && mh::image_extent(&f) == (size_t)2147395600u);
    f = make(MH_IMAGE_GRAY8, INT_MAX, 1, INT_MAX, 0);
    CHECK(mh::image_fmt_why(&f) == nullptr && mh::image_extent(&f) == (size_t)INT_MAX);
    f = make(MH_IMAGE_GRAY8, INT_MAX, 1, INT_MAX, 1);
    CHECK(says(mh::image_fmt_why(&f), "extent"));
    f = make(MH_IMAGE_GRAY8, 1, INT_MAX, 1, 0);
    CHECK(mh::image_fmt_why(&f) == nullptr && mh::image_extent(&f) == (size_t)INT_MAX);
    f = make(MH_IMAGE_GRAY8, 1, 3, INT_MAX, 0);                        // (h - 1) row_stride alone is beyond int
    CHECK(says(mh::image_fmt_why(&f), "extent"));
    f = make(MH_IMAGE_BGRA8, INT_MAX / 2, 1, INT_MAX, 0);              // width times 4 is beyond int
    CHECK(says(mh::image_fmt_why(&f), "row_stride"));
    f = make(MH_IMAGE_BGR8, 715827882, 1, INT_MAX, 0);                 // 3 w = 2^31 - 2: fits
    CHECK(mh::image_fmt_why(&f) == nullptr && mh::image_extent(&f) == (size_t)2147483646u);
    f = make(MH_IMAGE_BGR8, 715827882, 1, INT_MAX, 2);
    CHECK(says(mh::image_fmt_why(&f), "extent"));
    f = make(MH_IMAGE_BGR8, 640, 480, 640 * 3, INT_MAX);
    CHECK(says(mh::image_fmt_why(&f), "extent"));
  }
  // ---- a call ----
  {
    const mh_raw_image f = make(MH_IMAGE_BGR8, 8, 4, 30, 2);
    const size_t extent = mh::image_extent(&f), px = 32;
    CHECK(extent == 2 + 3 * 30 + 24);
    std::vector<unsigned char> mem(4096);
    unsigned char* base = &mem[1024];
    const void* raw[MH_MAX_BATCH + 1];
    uint8_t* out[MH_MAX_BATCH + 1];
    for (int i = 0; i <= MH_MAX_BATCH; ++i) {
      raw[i] = base;
      out[i] = &mem[2048] + i * px;
    }
    CHECK(mh::image_call_why(raw, &f, out, 1) == nullptr);
    CHECK(mh::image_call_why(raw, &f, out, MH_MAX_BATCH) == nullptr);   // (one raw buffer may serve many outputs)
    CHECK(says(mh::image_call_why(raw, &f, out, 0), "MH_MAX_BATCH"));
    CHECK(says(mh::image_call_why(raw, &f, out, -3), "MH_MAX_BATCH"));
    CHECK(says(mh::image_call_why(raw, &f, out, MH_MAX_BATCH + 1), "MH_MAX_BATCH"));
    CHECK(says(mh::image_call_why(nullptr, &f, out, 1), "null"));
    CHECK(says(mh::image_call_why(raw, &f, nullptr, 1), "null"));
    CHECK(says(mh::image_call_why(raw, nullptr, out, 1), "no mh_raw_image"));
    raw[1] = nullptr;
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "null image pointer"));
    CHECK(mh::image_call_why(raw, &f, out, 1) == nullptr);               // (only the call's n entries are read)
    raw[1] = base;
    out[1] = nullptr;
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "null image pointer"));
    // two outputs: the same, and one byte into each other from either side
    out[1] = out[0];
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "same output"));
    out[1] = out[0] + px - 1;
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "same output"));
    out[1] = out[0] - px + 1;
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "same output"));
    out[1] = out[0] + px;
    CHECK(mh::image_call_why(raw, &f, out, 2) == nullptr);
    out[1] = out[0] - px;
    CHECK(mh::image_call_why(raw, &f, out, 2) == nullptr);
    // an output against its raw extent: touching is fine, one byte inside is not
    out[0] = base + extent;
    CHECK(mh::image_call_why(raw, &f, out, 1) == nullptr);
    out[0] = base + extent - 1;
    CHECK(says(mh::image_call_why(raw, &f, out, 1), "its own raw"));
    out[0] = base - px;
    CHECK(mh::image_call_why(raw, &f, out, 1) == nullptr);
    out[0] = base - px + 1;
    CHECK(says(mh::image_call_why(raw, &f, out, 1), "its own raw"));
    out[0] = base;
    CHECK(says(mh::image_call_why(raw, &f, out, 1), "its own raw"));
    out[0] = base + 40;   // (inside a row's padding is inside the extent all the same)
    CHECK(says(mh::image_call_why(raw, &f, out, 1), "its own raw"));
    // ... and against another image's
    out[0] = &mem[2048];
    out[1] = &mem[3000];
    raw[1] = &mem[2048] + 8;
    CHECK(says(mh::image_call_why(raw, &f, out, 2), "a raw buffer of the batch"));
  }
  CHECK(mh::image_ranges_overlap((void*)16, 0, (void*)16, 8) == false);   // an empty range overlaps nothing
  if (failures) {
    std::fprintf(stderr, "image_fmt_check_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("image_fmt_check_test: ok\n");
  return 0;
}
