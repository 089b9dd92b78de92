// sensor_image_test -- the gray image of a camera's buffer, made twice: by a plain C++ loop on the host, pixel by pixel
// the way a node without the device would do it, and by hipSensorGray (SENSOR_IMAGE_HIP.hpp) on the device.  The bytes
// must agree: both are the same integer sums.
//
//   sensor_image_test [--encoding mono8|bgr8|rgb8|bgra8|rgba8|bayer_rggb8|bayer_bggr8|bayer_gbrg8|bayer_grbg8]
//                     [--size W H] [--pad BYTES] [--loop N | --dump file]
//
// --pad: bytes behind every row (the message's step = W bytes-per-pixel + BYTES).  --dump file runs the host loop alone (no
// device): int32 {format, width, height, row_stride, offset, raw bytes, 0, 0}, the raw buffer, the host loop's gray image
// (tests/test_image_gray_cpu.py compares it with the numpy restatement).  The raw buffer is made here: a hashed pattern
// with black, white and saturated patches.  Prints
//   DIFF <differing bytes> OF <bytes>
// and with --loop N the mean time per image over N images of each:  HOST_MS <ms>  /  HIP_MS <ms>.
// Exit status: 0 = no differing byte, 1 = the images differ, 2 = usage, 3 = no device.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <string>
#include <vector>

#include "moped_types.hpp"

#include "SENSOR_IMAGE_HIP.hpp"

using namespace MopedNS;

// ---- the host way ---------------------------------------------------------------------------------------------------------
static const unsigned R2Y = 4899, G2Y = 9617, B2Y = 1868;

// the colour of Bayer site (x, y): 0 R, 1 G, 2 B -- the four letters of the encoding are the top-left 2 x 2 row by row
static int siteColour(int format, int x, int y) {
  static const int table[4][4] = {{0, 1, 1, 2}, {2, 1, 1, 0}, {1, 2, 0, 1}, {1, 0, 2, 1}};   // rggb, bggr, gbrg, grbg
  return table[format - MH_IMAGE_BAYER_RGGB8][2 * (y & 1) + (x & 1)];
}
static unsigned coef(int colour) { return colour == 0 ? R2Y : colour == 1 ? G2Y : B2Y; }

static void hostGray(const unsigned char* raw, const mh_raw_image& f, std::vector<unsigned char>& out) {
  const int w = f.width, h = f.height;
  out.assign((size_t)w * h, 0);
  const bool bayer = f.format >= MH_IMAGE_BAYER_RGGB8;
  const int bpp = f.format == MH_IMAGE_BGR8 || f.format == MH_IMAGE_RGB8 ? 3 : f.format == MH_IMAGE_BGRA8 || f.format == MH_IMAGE_RGBA8 ? 4 : 1;
#define AT(x, y, k) ((unsigned)raw[(size_t)f.offset + (size_t)(y) * f.row_stride + (size_t)(x) * bpp + (k)])
  if (!bayer) {
    const int rAt = f.format == MH_IMAGE_RGB8 || f.format == MH_IMAGE_RGBA8 ? 0 : 2;
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++)
        out[(size_t)y * w + x] = bpp == 1 ? (unsigned char)AT(x, y, 0)
                                          : (unsigned char)((R2Y * AT(x, y, rAt) + G2Y * AT(x, y, 1) + B2Y * AT(x, y, 2 - rAt) + 8192u) >> 14);
    return;
  }
  for (int y = 1; y < h - 1; y++)
    for (int x = 1; x < w - 1; x++) {
      const int o = siteColour(f.format, x, y);
      const unsigned p = AT(x, y, 0);
      unsigned v;
      if (o == 1) {
        const unsigned ch = coef(siteColour(f.format, x + 1, y)), cv = coef(siteColour(f.format, x, y + 1));
        v = (ch * (AT(x - 1, y, 0) + AT(x + 1, y, 0)) + cv * (AT(x, y - 1, 0) + AT(x, y + 1, 0)) + 2 * G2Y * p + 16384u) >> 15;
      } else {
        const unsigned diag = AT(x - 1, y - 1, 0) + AT(x + 1, y - 1, 0) + AT(x - 1, y + 1, 0) + AT(x + 1, y + 1, 0);
        const unsigned edge = AT(x, y - 1, 0) + AT(x, y + 1, 0) + AT(x - 1, y, 0) + AT(x + 1, y, 0);
        v = (coef(2 - o) * diag + G2Y * edge + 4 * coef(o) * p + 32768u) >> 16;
      }
      out[(size_t)y * w + x] = (unsigned char)v;
    }
#undef AT
  for (int y = 1; y < h - 1; y++) {
    out[(size_t)y * w] = out[(size_t)y * w + 1];
    out[(size_t)y * w + w - 1] = out[(size_t)y * w + w - 2];
  }
  std::memcpy(&out[0], &out[w], w);
  std::memcpy(&out[(size_t)(h - 1) * w], &out[(size_t)(h - 2) * w], w);
}

// ---- the raw buffer -------------------------------------------------------------------------------------------------------
static void makeRaw(const mh_raw_image& f, int bpp, std::vector<unsigned char>& buf) {
  buf.assign((size_t)f.offset + (size_t)(f.height - 1) * f.row_stride + (size_t)f.width * bpp, 0x5a);
  for (int y = 0; y < f.height; y++)
    for (int x = 0; x < f.width * bpp; x++) {
      uint32_t v = (uint32_t)x * 2654435761u ^ (uint32_t)y * 2246822519u;
      v ^= v >> 15;
      v *= 2246822519u;
      v ^= v >> 13;
      unsigned char b = (unsigned char)(v >> 8);
      const int px = x / bpp, third = f.width / 3 + 1;
      if (y < f.height / 4) b = px < third ? 0 : px < 2 * third ? 255 : (unsigned char)(x % bpp == 0 ? 255 : 0);   // black, white, one channel
      buf[(size_t)f.offset + (size_t)y * f.row_stride + x] = b;
    }
}

int main(int argc, char** argv) {
  std::string encoding = "bgr8", dump;
  int w = 640, h = 480, pad = 0, loop = 0;
  for (int a = 1; a < argc; a++) {
    const std::string o = argv[a];
    if (o == "--encoding" && a + 1 < argc) encoding = argv[++a];
    else if (o == "--size" && a + 2 < argc) { w = std::atoi(argv[a + 1]); h = std::atoi(argv[a + 2]); a += 2; }
    else if (o == "--pad" && a + 1 < argc) pad = std::atoi(argv[++a]);
    else if (o == "--loop" && a + 1 < argc) loop = std::atoi(argv[++a]);
    else if (o == "--dump" && a + 1 < argc) dump = argv[++a];
    else {
      std::fprintf(stderr, "usage: %s [--encoding mono8|bgr8|rgb8|bgra8|rgba8|bayer_*8] [--size W H] [--pad BYTES] [--loop N | --dump file]\n", argv[0]);
      return 2;
    }
  }
  mh_raw_image f;
  if (w <= 0 || h <= 0 || w > 16384 || h > 16384 || pad < 0 || pad > 4096 || !hipImageFormat(encoding, w, h, 0, &f)) return 2;
  if (f.format >= MH_IMAGE_BAYER_RGGB8 && (w < 3 || h < 3)) return 2;
  const int bpp = f.row_stride / w;
  if (!hipImageFormat(encoding, w, h, w * bpp + pad, &f)) return 2;   // the message's step
  std::vector<unsigned char> buf, host, dev;
  makeRaw(f, bpp, buf);
  hostGray(&buf[0], f, host);
  if (!dump.empty()) {   // no device needed: the description, the raw buffer and the host loop's image
    FILE* out = std::fopen(dump.c_str(), "wb");
    if (!out) { std::perror(dump.c_str()); return 2; }
    const int32_t head[8] = {f.format, f.width, f.height, f.row_stride, f.offset, (int32_t)buf.size(), 0, 0};
    const bool ok = std::fwrite(head, 4, 8, out) == 8 && std::fwrite(&buf[0], 1, buf.size(), out) == buf.size() &&
                    std::fwrite(&host[0], 1, host.size(), out) == host.size();
    std::fclose(out);
    return ok ? 0 : 2;
  }
  if (!HipSession::get()) {
    std::fprintf(stderr, "no gfx950 device / HIP library\n");
    return 3;
  }
  if (!hipSensorGray(0, &buf[0], f, dev)) return 3;
  if (dev.size() != host.size()) return 1;
  size_t diff = 0;
  for (size_t i = 0; i < host.size(); i++) diff += host[i] != dev[i];
  std::printf("DIFF %zu OF %zu\n", diff, host.size());

  if (loop > 0) {
    typedef std::chrono::steady_clock clk;
    clk::time_point t0 = clk::now();
    for (int i = 0; i < loop; i++) hostGray(&buf[0], f, host);
    clk::time_point t1 = clk::now();
    for (int i = 0; i < loop; i++)
      if (!hipSensorGray(0, &buf[0], f, dev)) return 3;
    clk::time_point t2 = clk::now();
    std::printf("HOST_MS %.4f\n", std::chrono::duration<double, std::milli>(t1 - t0).count() / loop);
    std::printf("HIP_MS %.4f\n", std::chrono::duration<double, std::milli>(t2 - t1).count() / loop);
  }
  return diff ? 1 : 0;
}
