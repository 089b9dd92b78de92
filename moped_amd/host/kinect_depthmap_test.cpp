// kinect_depthmap_test -- the Kinect depth map from raw sensor depth, built twice from one raw buffer: by a plain C++
// loop on the host, the way a node without the device would do it (raw values out of the buffer, NaN / 0 -> -1e30, a
// bilinear resize to twice the size when the sizes differ, back-projection through K), and by hipKinectDepthmap
// (KINECT_DEPTHMAP_HIP.hpp) on the device.  The bytes must agree: both are sequences of single float operations.
//
//   kinect_depthmap_test [--format f32|u16|cloud] [--raw W H] [--map W H] [--loop N | --dump file]
//
// --dump file runs the host loop alone (no device): int32 {format, raw width, raw height, elem_stride, row_stride, offset,
// raw bytes, 0}, float K[4], the raw buffer, the host loop's map [H][W][4] (tests/test_depthmap_cpu.py compares it with
// the numpy restatement).
// The raw buffer is made here: a slanted plane with missing readings in the corners, on the borders, as rows and as
// blocks ("cloud": points of 32 bytes, z at byte 8, rows padded by 64 bytes).  Prints
//   DIFF <differing bytes> OF <bytes> INVALID <pixels>
// and with --loop N the mean time per map over N maps of each:  HOST_MS <ms>  /  HIP_MS <ms>.
// Exit status: 0 = no differing byte, 1 = the maps differ, 2 = usage, 3 = no device.
#define MOPED_AMD_WITH_DEPTH
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <string>
#include <vector>

#include "moped_types.hpp"

#include "KINECT_DEPTHMAP_HIP.hpp"

using namespace MopedNS;

// ---- the host way -------------------------------------------------------------------------------------------------------
static float rawValue(const unsigned char* raw, const mh_raw_depth& d, int x, int y) {
  const unsigned char* p = raw + d.offset + (size_t)y * d.row_stride + (size_t)x * d.elem_stride;
  if (d.format == MH_RAW_DEPTH_F32_M) {
    float v;
    std::memcpy(&v, p, 4);
    return v != v ? -1e30f : v;
  }
  uint16_t mm;
  std::memcpy(&mm, p, 2);
  return mm == 0 ? -1e30f : (float)mm * 0.001f;
}

// source index and weight of destination index i of a resize to twice the size
static void tap(int i, int* s, float* f) {
  float v = (float)((i + 0.5) * 0.5 - 0.5);
  const int k = (int)std::floor(v);
  *s = k;
  *f = v - (float)k;
}

static void hostDepthmap(const unsigned char* raw, const mh_raw_depth& d, const float K[4], int w, int h,
                         std::vector<float>& out) {
  const int rw = d.width, rh = d.height;
  std::vector<float> z((size_t)rw * rh);
  for (int y = 0; y < rh; y++)
    for (int x = 0; x < rw; x++) z[(size_t)y * rw + x] = rawValue(raw, d, x, y);
  const std::vector<float>* data = &z;
  int dw = rw, dh = rh;
  std::vector<float> rows, up;
  if (w != rw || h != rh) {
    dw = 2 * rw;
    dh = 2 * rh;
    rows.resize((size_t)rh * dw);   // the horizontal pass
    for (int x = 0; x < dw; x++) {
      int sx;
      float fx;
      tap(x, &sx, &fx);
      if (sx < 0) {
        sx = 0;
        fx = 0.f;
      }
      for (int y = 0; y < rh; y++) {
        const float* S = &z[(size_t)y * rw];
        float v;
        if (sx >= rw - 1) {
          v = S[rw - 1];
        } else {
          const float a = S[sx] * (1.f - fx), b = S[sx + 1] * fx;
          v = a + b;
        }
        rows[(size_t)y * dw + x] = v;
      }
    }
    up.resize((size_t)dh * dw);     // the vertical pass
    for (int y = 0; y < dh; y++) {
      int sy;
      float fy;
      tap(y, &sy, &fy);
      const int y0 = sy < 0 ? 0 : sy > rh - 1 ? rh - 1 : sy, y1 = sy + 1 < 0 ? 0 : sy + 1 > rh - 1 ? rh - 1 : sy + 1;
      const float b0 = 1.f - fy, b1 = fy;
      for (int x = 0; x < dw; x++) {
        const float a = rows[(size_t)y0 * dw + x] * b0, b = rows[(size_t)y1 * dw + x] * b1;
        up[(size_t)y * dw + x] = a + b;
      }
    }
    data = &up;
  }
  out.resize((size_t)w * h * 4);
  for (int v = 0; v < h; v++)
    for (int u = 0; u < w; u++) {
      float* px = &out[((size_t)v * w + u) * 4];
      const float depth = (u < dw && v < dh) ? (*data)[(size_t)v * dw + u] : -1.f;
      if (depth < 0) {
        px[0] = px[1] = px[2] = px[3] = -1.f;
        continue;
      }
      const float du = (float)u - K[2], dv = (float)v - K[3];
      const float pu = depth * du, pv = depth * dv;
      const float x = pu / K[0], y = pv / K[1];
      const float xx = x * x, yy = y * y, zz = depth * depth;
      const float s = xx + yy;
      px[0] = x;
      px[1] = y;
      px[2] = depth;
      px[3] = std::sqrt(s + zz);
    }
}

// ---- the raw buffer ---------------------------------------------------------------------------------------------------------
static bool missing(int x, int y, int rw, int rh) {
  if ((x == 0 || x == rw - 1) && (y == 0 || y == rh - 1)) return true;             // the corners
  if ((y == 0 && x == rw / 2) || (x == 0 && y == rh / 2) || (x == rw - 1 && y == rh / 3)) return true;
  if (rh > 40 && y >= rh / 8 && y < rh / 8 + rh / 16) return true;                  // rows without a reading
  if (rw > 40 && x > rw / 2 && x < rw / 2 + rw / 10 && y > rh / 2 && y < rh / 2 + rh / 10) return true;   // a block
  return (x * 7 + y * 13) % 97 == 0;                                                // speckle
}

static mh_raw_depth makeRaw(const std::string& format, int rw, int rh, std::vector<unsigned char>& buf) {
  mh_raw_depth d = format == "u16" ? hipRawDepthOfImage16(rw, rh) : format == "cloud" ? hipRawDepthOfCloud(rw, rh, 32, rw * 32 + 64, 8)
                                                                                       : hipRawDepthOfImage32(rw, rh);
  buf.assign((size_t)d.offset + (size_t)(rh - 1) * d.row_stride + (size_t)(rw - 1) * d.elem_stride + (format == "u16" ? 2 : 4), 0x5a);
  for (int y = 0; y < rh; y++)
    for (int x = 0; x < rw; x++) {
      unsigned char* p = &buf[d.offset + (size_t)y * d.row_stride + (size_t)x * d.elem_stride];
      const bool gone = missing(x, y, rw, rh);
      if (format == "u16") {
        const uint16_t mm = gone ? 0 : (uint16_t)(600 + (x * 3 + y * 5) % 3000);
        std::memcpy(p, &mm, 2);
      } else {
        const float m = gone ? std::nanf("") : 0.6f + 0.001f * (float)((x * 3 + y * 5) % 3000);
        std::memcpy(p, &m, 4);
      }
    }
  return d;
}

int main(int argc, char** argv) {
  std::string format = "f32", dump;
  int rw = 640, rh = 480, w = 0, h = 0, loop = 0;
  for (int a = 1; a < argc; a++) {
    const std::string o = argv[a];
    if (o == "--format" && a + 1 < argc) format = argv[++a];
    else if (o == "--raw" && a + 2 < argc) { rw = std::atoi(argv[a + 1]); rh = std::atoi(argv[a + 2]); a += 2; }
    else if (o == "--map" && a + 2 < argc) { w = std::atoi(argv[a + 1]); h = std::atoi(argv[a + 2]); a += 2; }
    else if (o == "--loop" && a + 1 < argc) loop = std::atoi(argv[++a]);
    else if (o == "--dump" && a + 1 < argc) dump = argv[++a];
    else {
      std::fprintf(stderr, "usage: %s [--format f32|u16|cloud] [--raw W H] [--map W H] [--loop N | --dump file]\n", argv[0]);
      return 2;
    }
  }
  if (!w) w = rw;
  if (!h) h = rh;
  if ((format != "f32" && format != "u16" && format != "cloud") || rw <= 0 || rh <= 0 || w <= 0 || h <= 0 || rw > 8192 || rh > 8192 ||
      w > 16384 || h > 16384)
    return 2;
  std::vector<unsigned char> buf;
  const mh_raw_depth d = makeRaw(format, rw, rh, buf);
  Pt<4> K, nonlinear;
  K.init(525.0 * w / 640, 525.0 * w / 640, 0.5 * w - 0.5, 0.5 * h - 0.5);
  nonlinear.init(0.0, 0.0, 0.0, 0.0);
  const float Kf[4] = {K[0], K[1], K[2], K[3]};

  std::vector<float> host;
  hostDepthmap(&buf[0], d, Kf, w, h, host);
  if (!dump.empty()) {   // no device needed: the description, K, the raw buffer and the host loop's map
    FILE* f = std::fopen(dump.c_str(), "wb");
    if (!f) { std::perror(dump.c_str()); return 2; }
    const int32_t head[8] = {d.format, d.width, d.height, d.elem_stride, d.row_stride, d.offset, (int32_t)buf.size(), 0};
    const bool ok = std::fwrite(head, 4, 8, f) == 8 && std::fwrite(Kf, 4, 4, f) == 4 &&
                    std::fwrite(&buf[0], 1, buf.size(), f) == buf.size() && std::fwrite(&host[0], 4, host.size(), f) == host.size();
    std::fclose(f);
    return ok ? 0 : 2;
  }
  if (!HipSession::get()) {
    std::fprintf(stderr, "no gfx950 device / HIP library\n");
    return 3;
  }
  Image depthmap;
  if (!hipKinectDepthmap(depthmap, &buf[0], d, K, nonlinear, w, h)) return 3;
  if (depthmap.imageType != IMAGE_TYPE_DEPTH_MAP || depthmap.width != w || depthmap.height != h ||
      depthmap.data.size() != host.size() * sizeof(float))
    return 1;
  const unsigned char* hb = (const unsigned char*)&host[0];
  size_t diff = 0, invalid = 0;
  for (size_t i = 0; i < depthmap.data.size(); i++) diff += hb[i] != depthmap.data[i];
  for (size_t i = 0; i < host.size(); i += 4) invalid += host[i + 2] < 0;
  std::printf("DIFF %zu OF %zu INVALID %zu\n", diff, depthmap.data.size(), invalid);

  if (loop > 0) {
    typedef std::chrono::steady_clock clk;
    clk::time_point t0 = clk::now();
    for (int i = 0; i < loop; i++) hostDepthmap(&buf[0], d, Kf, w, h, host);
    clk::time_point t1 = clk::now();
    for (int i = 0; i < loop; i++)
      if (!hipKinectDepthmap(depthmap, &buf[0], d, K, nonlinear, w, h)) return 3;
    clk::time_point t2 = clk::now();
    std::printf("HOST_MS %.4f\n", std::chrono::duration<double, std::milli>(t1 - t0).count() / loop);
    std::printf("HIP_MS %.4f\n", std::chrono::duration<double, std::milli>(t2 - t1).count() / loop);
  }
  return diff ? 1 : 0;
}
