// oracle/sift_oracle.cpp -- TEST INFRASTRUCTURE ONLY (part of liboracle.so).
//
// CPU restatement of the SIFT extractor behind FEAT_SIFT_CPU
// (moped2/libmoped/src/feat/FEAT_SIFT_CPU.hpp:78-112): libsiftfast 1.1
// (moped2/libmoped/libs/libs.tgz -> libsiftfast-1.1-src/libsiftfast.cpp) in the arithmetic
// MOPED actually builds: its copy of the library `#undef`s __SSE__/__SSE2__/__SSE3__
// (:39-41), so the plain-C branches run (ConvHorizontal / ConvVertical / GradOriImages with
// libm's atan2f, two-pass descriptor normalisation).
//
// PINNED: bit-identical -- keypoint count, order, position, scale, orientation and all 128
// descriptor values -- to the reference's own build of that library (oracle/_ref: ref_sift2,
// run with one OpenMP thread) on the five frames of moped2/test_data/timing.bag
// (tests/golden/sift_ref_frames.npz, tests/test_sift_cpu.py).  With more threads the
// reference's list ORDER depends on thread timing (rows are spliced into the list under
// `omp critical`, :944-952); the order here is the single-thread one.
//
// Line numbers below refer to libsiftfast.cpp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "oracle.h"

namespace {

constexpr float kPi = 3.141592654f;   // :65
constexpr float kSqrt2 = 1.4142136f;  // :66
constexpr int kScales = 3;            // :108
constexpr float kInitSigma = 1.6f;    // :109

struct Img {
  int rows = 0, cols = 0;
  std::vector<float> px;
  Img() {}
  Img(int r, int c) : rows(r), cols(c), px((size_t)r * c, 0.f) {}
  float& at(int r, int c) { return px[(size_t)r * cols + c]; }
  float at(int r, int c) const { return px[(size_t)r * cols + c]; }
};

// GaussianBlur's kernel (:470-506): ksize odd, >= 3; weights expf(-(i-w)^2 / (2 s^2)) for
// i = 0..ksize INCLUSIVE summed in double, only the first ksize of them divided by the sum.
std::vector<float> gauss_kernel(float fblur) {
  const float trunc = 4.0f;
  int ksize = (int)(2.0f * trunc * fblur + 1.0f);
  if (ksize < 3) ksize = 3;
  ksize += !(ksize & 1);
  const int width = ksize >> 1;
  std::vector<float> k(ksize + 1);
  double acc = 0;
  for (int i = 0; i <= ksize; ++i) {
    const float w = expf(-(float)(i - width) * (i - width) / (2.0f * fblur * fblur));
    acc += (double)w;
    k[i] = w;
  }
  for (int i = 0; i < ksize; ++i) k[i] /= (float)acc;
  k.resize(ksize);
  return k;
}

// ConvHorizontal + ConvVertical (:523-584): edge pixels replicated, float accumulator,
// taps added in ascending order; rows first, then columns of the row-blurred image.
void blur(Img& dst, const Img& src, float fblur) {
  const std::vector<float> k = gauss_kernel(fblur);
  const int ks = (int)k.size(), w = ks >> 1, rows = src.rows, cols = src.cols;
  Img tmp(rows, cols);
  std::vector<float> buf((size_t)std::max(rows, cols) + ks);
  for (int r = 0; r < rows; ++r) {
    for (int j = 0; j < w; ++j) buf[j] = src.at(r, 0);
    for (int j = 0; j < cols; ++j) buf[w + j] = src.at(r, j);
    for (int j = 0; j < w; ++j) buf[cols + w + j] = src.at(r, cols - 1);
    for (int i = 0; i < cols; ++i) {
      float a = 0;
      for (int j = 0; j < ks; ++j) a += buf[i + j] * k[j];
      tmp.at(r, i) = a;
    }
  }
  if (dst.rows != rows || dst.cols != cols) dst = Img(rows, cols);
  for (int c = 0; c < cols; ++c) {
    for (int i = 0; i < w; ++i) buf[i] = tmp.at(0, c);
    for (int i = 0; i < rows; ++i) buf[w + i] = tmp.at(i, c);
    for (int i = 0; i < w; ++i) buf[rows + w + i] = tmp.at(rows - 1, c);
    for (int i = 0; i < rows; ++i) {
      float a = 0;
      for (int j = 0; j < ks; ++j) a += buf[i + j] * k[j];
      dst.at(i, c) = a;
    }
  }
}

// GradOriImages' two differences at one pixel (:959-992), in T on the float pixels (T = double: describe mode f64)
template <class T>
void grad_at(const Img& im, int i, int j, T& dc, T& dr) {
  const int rows = im.rows, cols = im.cols;
  if (j == 0) dc = T(2) * ((T)im.at(i, 1) - (T)im.at(i, 0));
  else if (j == cols - 1) dc = T(2) * ((T)im.at(i, j) - (T)im.at(i, j - 1));
  else dc = (T)im.at(i, j + 1) - (T)im.at(i, j - 1);
  if (i == 0) dr = T(2) * ((T)im.at(0, j) - (T)im.at(1, j));
  else if (i == rows - 1) dr = T(2) * ((T)im.at(i - 1, j) - (T)im.at(i, j));
  else dr = (T)im.at(i - 1, j) - (T)im.at(i + 1, j);
}

// GradOriImages (:959-992)
void grad_ori(const Img& im, Img& grad, Img& ori) {
  const int rows = im.rows, cols = im.cols;
  grad = Img(rows, cols);
  ori = Img(rows, cols);
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      float dc, dr;
      grad_at(im, i, j, dc, dr);
      grad.at(i, j) = sqrtf(dc * dc + dr * dr);
      ori.at(i, j) = atan2f(dr, dc);
    }
}

// LocalMaxMin (:1126-1147)
bool local_extremum(float v, const Img& d, int r, int c) {
  for (int rr = r - 1; rr <= r + 1; ++rr)
    for (int cc = c - 1; cc <= c + 1; ++cc) {
      const float o = d.at(rr, cc);
      if (v > 0 ? o > v : v > o) return false;
    }
  return true;
}

// NotOnEdge (:1149-1162)
bool not_on_edge(const Img& d, int r, int c) {
  const float f1 = d.at(r - 1, c) - d.at(r, c) * 2 + d.at(r + 1, c);
  const float f2 = d.at(r, c - 1) - d.at(r, c) * 2 + d.at(r, c + 1);
  const float f3 = d.at(r + 1, c + 1) - d.at(r + 1, c - 1);
  const float f4 = d.at(r - 1, c + 1) - d.at(r - 1, c - 1);
  const float f5 = (f3 - f4) * 0.25f;
  const float f6 = f1 * f2 - f5 * f5;
  const float f8 = f1 + f2;
  return f6 * 11 * 11 > f8 * f8 * 10;
}

// SolveLinearSystem (:1235-1272): Gaussian elimination with row pivoting, 3x3
void solve3(float* Y, float* H) {
  const int dim = 3;
  int best = 0;
  for (int i = 0; i < dim - 1; ++i) {
    float fmax = -1;
    for (int j = i; j < dim; ++j) {
      float f = H[j * dim + i];
      if (f < 0) f = -f;
      if (f > fmax) {
        fmax = f;
        best = j;
      }
    }
    if (best != i) {
      for (int j = 0; j < dim; ++j) std::swap(H[best * dim + j], H[i * dim + j]);
      std::swap(Y[best], Y[i]);
    }
    for (int j = i + 1; j < dim; ++j) {
      const float f = H[j * dim + i] / H[i * dim + i];
      for (int k = i; k < dim; ++k) H[j * dim + k] -= f * H[i * dim + k];
      Y[j] -= Y[i] * f;
    }
  }
  for (int i = dim - 1; i >= 0; --i) {
    for (int j = dim - 1; j > i; --j) Y[i] -= Y[j] * H[i * dim + j];
    Y[i] /= H[i * dim + i];
  }
}

// FitQuadratic (:1208-1231)
float fit_quadratic(float* X, const Img* dog, int index, int r, int c) {
  const Img &p0 = dog[index - 1], &p1 = dog[index], &p2 = dog[index + 1];
  float Y[3], H[9];
  Y[0] = 0.5f * (p2.at(r, c) - p0.at(r, c));
  Y[1] = 0.5f * (p1.at(r + 1, c) - p1.at(r - 1, c));
  Y[2] = 0.5f * (p1.at(r, c + 1) - p1.at(r, c - 1));
  H[0] = p0.at(r, c) - 2.0f * p1.at(r, c) + p2.at(r, c);
  H[4] = p1.at(r - 1, c) - 2.0f * p1.at(r, c) + p1.at(r + 1, c);
  H[8] = p1.at(r, c - 1) - 2.0f * p1.at(r, c) + p1.at(r, c + 1);
  H[3] = H[1] = 0.25f * ((p2.at(r + 1, c) - p2.at(r - 1, c)) - (p0.at(r + 1, c) - p0.at(r - 1, c)));
  H[6] = H[2] = 0.25f * ((p2.at(r, c + 1) - p2.at(r, c - 1)) - (p0.at(r, c + 1) - p0.at(r, c - 1)));
  H[7] = H[5] = 0.25f * ((p1.at(r + 1, c + 1) - p1.at(r + 1, c - 1)) - (p1.at(r - 1, c + 1) - p1.at(r - 1, c - 1)));
  X[0] = -Y[0];
  X[1] = -Y[1];
  X[2] = -Y[2];
  solve3(X, H);
  return p1.at(r, c) + 0.5f * (X[0] * Y[0] + X[1] * Y[1] + X[2] * Y[2]);
}

struct Key {
  float row, col, scale, ori;
  float desc[128];
};

// PlaceInIndex (:1609-1668); T = float is the library's arithmetic, T = double describe mode f64
template <class T>
void place(T* fdesc, T mag, T ori, T rx, T cx) {
  const T oribin = ori * (T)(8.0f / (2 * (float)kPi));
  const int nr = rx < 0 ? (int)(rx - 1) : (int)rx;
  const T rf = rx - (T)nr;
  const int nc = cx < 0 ? (int)(cx - 1) : (int)cx;
  const T cf = cx - (T)nc;
  const int no = oribin < 0 ? (int)(oribin - 1) : (int)oribin;
  const T of = oribin - (T)no;
  for (int i = 0; i < 2; ++i) {
    if ((unsigned)(i + nr) >= 4) continue;
    const T rg = i == 0 ? mag * (1 - rf) : mag * rf;
    for (int j = 0; j < 2; ++j) {
      if ((unsigned)(j + nc) >= 4) continue;
      const T cg = j == 0 ? rg * (1 - cf) : rg * cf;
      T* cell = fdesc + 8 * (4 * (i + nr) + j + nc);
      for (int k = 0; k < 2; ++k) cell[(no + k) & 7] += k == 0 ? cg * (1 - of) : cg * of;
    }
  }
}

// NormalizeVec (:1519-1527)
template <class T>
void normalize_vec(T* pf, int num) {
  T acc = 0;
  for (int i = 0; i < num; ++i) acc += pf[i] * pf[i];
  acc = 1 / std::sqrt(acc);
  for (int i = 0; i < num; ++i) pf[i] *= acc;
}

// What orc_sift_run_describe may change about the library's arithmetic (make_key itself changes nothing):
struct Tweak {
  int ulps = 0;     // mode pert: every result of sinf / cosf / expf and of the gradient image's atan2f moved this many floats
  int dir = 0;      //   up (+1), down (-1) or where a hash of (seed, key, sample, function) says (0)
  uint32_t seed = 0, key = 0;
  long drop = -1;   // mode drop: the selected sample (counted in raster order) that is left out; -2 = the one with the largest mag
};
enum { FN_SIN, FN_COS, FN_EXP, FN_ATAN2 };

float moved(float v, const Tweak* tw, int sample, int fn) {
  if (!tw || tw->ulps == 0) return v;
  int dir = tw->dir;
  if (dir == 0) {
    uint32_t h = (tw->seed + 1u) * 0x9E3779B1u ^ (tw->key + 1u) * 0x85EBCA6Bu ^ ((uint32_t)sample + 2u) * 0xC2B2AE35u ^
                 ((uint32_t)fn + 1u) * 0x27D4EB2Fu;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    dir = (h & 1u) ? 1 : -1;
  }
  for (int i = 0; i < tw->ulps; ++i) v = nextafterf(v, dir > 0 ? INFINITY : -INFINITY);
  return v;
}

// MakeKeypointSample / KeySample / AddSample (:1497-1607), plain-C branch: the descriptor of one key, 128 values.
//   T = float, tw = null   the library's arithmetic, operation for operation (make_key)
//   T = double             the samples the float tests select (rx, cx, the pixel inside the image: selection is float in
//                          every mode), and from there on everything in double on the same float pixels `im`: gradient,
//                          atan2, sin / cos of the orientation, exp, the trilinear weights, the sums, NormalizeVec, the clamp
//   tw                     float with the tweaks above; a moved sinf / cosf moves the selection too
// Returns the number of selected samples; sel_rows (optional) gets every selected sample's window row, in raster order.
template <class T>
int describe_key(T* desc, const Img* im, const Img& grad, const Img& orim, float fSize, float frow, float fcol,
                 float forient, const Tweak* tw = nullptr, std::vector<int>* sel_rows = nullptr) {
  constexpr bool wide = !std::is_same<T, float>::value;
  for (int i = 0; i < 128; ++i) desc[i] = 0;
  const int rowstart = (int)(frow + 0.5f), colstart = (int)(fcol + 0.5f);
  const float sinang = moved(sinf(forient), tw, -1, FN_SIN), cosang = moved(cosf(forient), tw, -1, FN_COS);
  const float fdrow = frow - (float)rowstart, fdcol = fcol - (float)colstart;
  const float frealsize = 3.0f * fSize, firealsize = 1.0f / (3.0f * fSize);
  const int win = (int)(frealsize * kSqrt2 * 5.0f * 0.5f + 0.5f);
  const float fsr = sinang * firealsize, fcr = cosang * firealsize, fdrr = -fdrow * firealsize,
              fdcr = -fdcol * firealsize;
  // (wide only) the same four in T from the key's floats
  [[maybe_unused]] const T wir = (T)1 / ((T)3 * (T)fSize);
  [[maybe_unused]] const T wsr = std::sin((T)forient) * wir, wcr = std::cos((T)forient) * wir;
  [[maybe_unused]] const T wdrr = -((T)frow - (T)rowstart) * wir, wdcr = -((T)fcol - (T)colstart) * wir;
  long drop = tw ? tw->drop : -1;
  int selected = 0;
  // pass 0 (drop == -2 only) finds the selected sample with the largest mag, pass 1 describes
  for (int pass = drop == -2 ? 0 : 1; pass < 2; ++pass) {
    long sel = 0, best_at = -1;
    float best = -1;
    for (int row = -win; row <= win; ++row) {
      const float fr = (float)row;
      float fc = -(float)win;
      for (int col = -win; col <= win; ++col, fc += 1) {
        const float rpos = fsr * fc + fcr * fr + fdrr;
        const float cpos = fcr * fc - fsr * fr + fdcr;
        const float rx = rpos + (2.0f - 0.5f), cx = cpos + (2.0f - 0.5f);
        if (!(rx > -0.9999f && rx < 3.9999f && cx > -0.9999f && cx < 3.9999f)) continue;
        const int r = rowstart + row, c = colstart + col;
        if (r < 0 || r >= grad.rows || c < 0 || c >= grad.cols) continue;
        const long at = sel++;
        const int sample = (row + win) * (2 * win + 1) + (col + win);
        const float g = grad.at(r, c) * moved(expf(-0.125f * (rpos * rpos + cpos * cpos)), tw, sample, FN_EXP);
        if (pass == 0) {
          if (g > best) {
            best = g;
            best_at = at;
          }
          continue;
        }
        if (sel_rows) sel_rows->push_back(row);
        if (at == drop) continue;
        if constexpr (wide) {
          const T wfc = (T)col, wfr = (T)row;
          const T wrpos = wsr * wfc + wcr * wfr + wdrr, wcpos = wcr * wfc - wsr * wfr + wdcr;
          T dc, dr;
          grad_at(*im, r, c, dc, dr);
          const T wg = std::sqrt(dc * dc + dr * dr) * std::exp((T)-0.125 * (wrpos * wrpos + wcpos * wcpos));
          T o = std::atan2(dr, dc) - (T)forient;
          while (o > (T)(2 * kPi)) o -= (T)(2 * kPi);
          while (o < 0) o += (T)(2 * kPi);
          place<T>(desc, wg, o, wrpos + (T)1.5, wcpos + (T)1.5);
        } else {
          float o = moved(orim.at(r, c), tw, sample, FN_ATAN2) - forient;
          while (o > 2 * kPi) o -= 2 * kPi;
          while (o < 0) o += 2 * kPi;
          place<float>(desc, g, o, rx, cx);
        }
      }
    }
    if (pass == 0) drop = best_at;
    selected = (int)sel;
  }
  normalize_vec(desc, 128);
  bool again = false;
  for (int i = 0; i < 128; ++i)
    if (desc[i] > (T)0.2f) {
      desc[i] = (T)0.2f;
      again = true;
    }
  if (again) normalize_vec(desc, 128);
  return selected;
}

// MakeKeypoint (:1424-1495)
void make_key(std::vector<Key>& out, const Img& grad, const Img& orim, float fscale, float fSize, float frow,
              float fcol, float forient) {
  Key k;
  k.ori = forient;
  k.row = fscale * frow;
  k.col = fscale * fcol;
  k.scale = fscale * fSize;
  describe_key<float>(k.desc, nullptr, grad, orim, fSize, frow, fcol, forient);
  out.push_back(k);
}

// SmoothHistogram (:1395-1408) incl. its different constants for the last bin
void smooth_hist(float* h, int n) {
  const float first = h[0];
  float prev = h[n - 1];
  for (int i = 0; i < n - 1; ++i) {
    const float org = h[i];
    h[i] = (prev + org + h[i + 1]) * 0.33333333f;
    prev = org;
  }
  h[n - 1] = (prev + h[n - 1] + first) * 0.3333333f;
}

// What a run shows of its stages (orc_sift_run): every scan hit that reached interp_key, in generation order, and the
// orientation peaks of the ones that took their pixel, in the order assign_ori emits them.
struct Hit {
  int octave, index, r0, c0, r, c, passed, took, first_peak, n_peaks;
  float X[3], val, fsize, frow, fcol;
};
struct Peak {
  int hit, bin;
  float ang;
};
struct Trace {
  std::vector<Hit> hits;
  std::vector<Peak> peaks;
};

// AssignOriHist (:1274-1382)
void assign_ori(std::vector<Key>& out, const Img& grad, const Img& orim, float fscale, float fSize, float frow,
                float fcol, Trace* trace) {
  const int rowstart = (int)(frow + 0.5f), colstart = (int)(fcol + 0.5f);
  const int rows = grad.rows, cols = grad.cols;
  float hist[36];
  memset(hist, 0, sizeof hist);
  const float fexpmult = -1.0f / (2.0f * 1.5f * 1.5f * fSize * fSize);
  const float fbinmult = 36.0f / (2 * kPi);
  const float fbinadd = (float)(kPi + 0.001f) * fbinmult;
  const int win = (int)(fSize * 1.5f * 3.0f);
  for (int r = rowstart - win; r <= rowstart + win; ++r) {
    if (r < 0 || r >= rows - 2) continue;
    for (int c = colstart - win; c <= colstart + win; ++c) {
      if (c < 0 || c >= cols - 2) continue;
      const float g = grad.at(r, c);
      if (!(g > 0)) continue;
      const float dr = (float)r - frow, dc = (float)c - fcol;
      const float rad2 = dr * dr + dc * dc;
      if (!((float)(win * win) + 0.5f > rad2)) continue;
      const float w = expf(rad2 * fexpmult);
      int bin = (int)(orim.at(r, c) * fbinmult + fbinadd);
      if (bin > 36) bin = 0;
      if (bin == 36) bin = 35;
      hist[bin] += g * w;
    }
  }
  for (int i = 0; i < 6; ++i) smooth_hist(hist, 36);
  float fmax = 0;
  for (int i = 0; i < 36; ++i)
    if (hist[i] > fmax) fmax = hist[i];
  fmax *= 0.8f;
  const float foriadd = 0.5f * 2 * kPi / 36.0f - kPi, forimult = 2 * kPi / 36.0f;
  for (int i = 0; i < 36; ++i) {
    const int prev = i == 0 ? 35 : i - 1, next = i == 35 ? 0 : i + 1;
    if (hist[i] <= hist[prev] || hist[i] <= hist[next] || hist[i] < fmax) continue;
    float f0 = hist[prev], f1 = hist[i], f2 = hist[next];   // InterpPeak (:1384-1393)
    if (f1 < 0) {
      f0 = -f0;
      f1 = -f1;
      f2 = -f2;
    }
    const float peak = 0.5f * (f0 - f2) / (f0 - 2.0f * f1 + f2);
    const float forient = (i + peak) * forimult + foriadd;
    if (trace) {
      trace->peaks.push_back(Peak{(int)trace->hits.size() - 1, i, forient});
      ++trace->hits.back().n_peaks;
    }
    make_key(out, grad, orim, fscale, fSize, frow, fcol, forient);
  }
}

// InterpKeyPoint (:1164-1206): the recursion as a loop
void interp_key(std::vector<Key>& out, const Img* dog, int index, int r, int c, const Img& grad, const Img& orim,
                std::vector<char>& taken, float fscale, float peak_thresh, int octave, Trace* trace) {
  const int rows = dog[0].rows, cols = dog[0].cols;
  const int r_start = r, c_start = c;
  float X[3], val = 0;
  for (int steps = 5;; --steps) {
    val = fit_quadratic(X, dog, index, r, c);
    int nr = r, nc = c;
    if (X[1] > 0.6f && r < rows - 3) nr++;
    if (X[1] < -0.6f && r > 3) nr--;
    if (X[2] > 0.6f && c < cols - 3) nc++;
    if (X[2] < -0.6f && c > 3) nc--;
    if (steps > 0 && (nr != r || nc != c)) {
      r = nr;
      c = nc;
      continue;
    }
    break;
  }
  if (trace) {
    Hit h;
    memset(&h, 0, sizeof h);
    h.octave = octave;
    h.index = index;
    h.r0 = r_start;
    h.c0 = c_start;
    h.r = r;
    h.c = c;
    h.X[0] = X[0];
    h.X[1] = X[1];
    h.X[2] = X[2];
    h.val = val;
    h.first_peak = (int)trace->peaks.size();
    trace->hits.push_back(h);
  }
  if (fabsf(X[0]) <= 1.5f && fabsf(X[1]) <= 1.5f && fabsf(X[2]) <= 1.5f && fabsf(val) >= peak_thresh) {
    if (trace) trace->hits.back().passed = 1;
    char& t = taken[(size_t)r * cols + c];
    if (!t) {
      t = 1;
      const float fSize = kInitSigma * powf(2.0f, ((float)index + X[0]) / (float)kScales);
      if (trace) {
        Hit& h = trace->hits.back();
        h.took = 1;
        h.fsize = fSize;
        h.frow = (float)r + X[1];
        h.fcol = (float)c + X[2];
      }
      assign_ori(out, grad, orim, fscale, fSize, (float)r + X[1], (float)c + X[2], trace);
    }
  }
}

struct Pyramid {
  std::vector<std::vector<Img>> gaus, dog;  // [octave][i]
};

// HalfImageSize (:390-408)
Img half_size(const Img& src) {
  Img half(src.rows >> 1, src.cols >> 1);
  for (int r = 0; r < half.rows; ++r)
    for (int c = 0; c < half.cols; ++c) half.at(r, c) = src.at(2 * r, 2 * c);
  return half;
}

// GetKeypoints / OctaveKeypoints / FindMaxMin (:301-361, :410-438, :891-957).  Keypoints come
// out in GENERATION order (octave, scale index, row, column, histogram peak ascending); the
// reference's linked list is that order reversed (every new key is pushed on the front).
void run_sift(const uint8_t* gray, int w, int h, int double_size, std::vector<Key>& keys, Pyramid* pyr,
              Trace* trace = nullptr) {
  const float peak_thresh = 0.04f / (float)kScales;
  Img org(h, w);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) org.at(y, x) = ((float)gray[(size_t)w * y + x]) * 1. / 255.;  // FEAT_SIFT_CPU.hpp:91
  Img cur;
  float fscale = 1.0f;
  if (double_size) {  // SiftDoubleSize (:363-380)
    cur = Img(2 * h - 2, 2 * w - 2);
    for (int i = 0; i < h - 1; ++i)
      for (int j = 0; j < w - 1; ++j) {
        cur.at(2 * i, 2 * j) = org.at(i, j);
        cur.at(2 * i + 1, 2 * j) = 0.5f * (org.at(i, j) + org.at(i + 1, j));
        cur.at(2 * i, 2 * j + 1) = 0.5f * (org.at(i, j) + org.at(i, j + 1));
        cur.at(2 * i + 1, 2 * j + 1) = 0.25f * (org.at(i, j) + org.at(i, j + 1) + org.at(i + 1, j) + org.at(i + 1, j + 1));
      }
    fscale = 0.5f;
  } else {
    cur = org;
  }
  const float fnew = double_size ? 1.0f : 0.5f;
  if (kInitSigma > fnew) {
    Img tmp;
    blur(tmp, cur, sqrtf(kInitSigma * kInitSigma - fnew * fnew));
    cur = tmp;
  }
  const float fwidth = powf(2.0f, 1.0f / (float)kScales);
  const float fincsigma = sqrtf(fwidth * fwidth - 1.0f);
  int octave = 0;
  while (cur.rows > 12 && cur.cols > 12) {
    std::vector<Img> gaus(kScales + 3), dog(kScales + 2);
    gaus[0] = cur;
    float sigma = kInitSigma;
    for (int i = 1; i < kScales + 3; ++i) {
      blur(gaus[i], gaus[i - 1], fincsigma * sigma);
      dog[i - 1] = Img(cur.rows, cur.cols);
      for (size_t p = 0; p < dog[i - 1].px.size(); ++p) dog[i - 1].px[p] = gaus[i - 1].px[p] - gaus[i].px[p];
      sigma *= fwidth;
    }
    const int rows = cur.rows, cols = cur.cols;
    std::vector<char> taken((size_t)rows * cols, 0);
    for (int index = 1; index < kScales + 1; ++index) {
      Img grad, orim;
      grad_ori(gaus[index], grad, orim);
      for (int r = 5; r < rows - 5; ++r)
        for (int c = 5; c < cols - 5; ++c) {
          const float v = dog[index].at(r, c);
          if (fabsf(v) > peak_thresh * 0.8f && local_extremum(v, dog[index], r, c) &&
              local_extremum(v, dog[index - 1], r, c) && local_extremum(v, dog[index + 1], r, c) &&
              not_on_edge(dog[index], r, c))
            interp_key(keys, dog.data(), index, r, c, grad, orim, taken, fscale, peak_thresh, octave, trace);
        }
    }
    Img half = half_size(gaus[kScales]);
    if (pyr) {
      pyr->gaus.push_back(gaus);
      pyr->dog.push_back(dog);
    }
    cur = half;
    fscale += fscale;
    ++octave;
  }
}

}  // namespace

extern "C" {

int orc_sift(const uint8_t* gray, int w, int h, int double_size, float* xy, float* scale_ori, float* desc, int cap) {
  std::vector<Key> keys;
  run_sift(gray, w, h, double_size, keys, nullptr);
  const int n = (int)keys.size();
  // list order of the reference = generation order reversed
  for (int i = 0; i < n && i < cap; ++i) {
    const Key& k = keys[n - 1 - i];
    xy[2 * i] = k.col;          // coord2D = (col, row), FEAT_SIFT_CPU.hpp:103-104
    xy[2 * i + 1] = k.row;
    if (scale_ori) {
      scale_ori[2 * i] = k.scale;
      scale_ori[2 * i + 1] = k.ori;
    }
    memcpy(desc + (size_t)i * 128, k.desc, sizeof k.desc);
  }
  return n;
}

// Pyramid images for stage-by-stage checks of the HIP path: kind 0 = Gaussian i (0..5),
// 1 = DoG i (0..4) of `octave`.  Returns rows*cols (0 if the octave does not exist) and the size.
int orc_sift_image(const uint8_t* gray, int w, int h, int double_size, int octave, int kind, int i, float* out,
                   int* rows, int* cols) {
  std::vector<Key> keys;
  Pyramid p;
  run_sift(gray, w, h, double_size, keys, &p);
  if (octave < 0 || octave >= (int)p.gaus.size()) return 0;
  const std::vector<Img>& v = kind == 0 ? p.gaus[octave] : p.dog[octave];
  if (i < 0 || i >= (int)v.size()) return 0;
  *rows = v[i].rows;
  *cols = v[i].cols;
  if (out) memcpy(out, v[i].px.data(), v[i].px.size() * sizeof(float));
  return (int)v[i].px.size();
}

// ---- one run, every stage (tests/test_sift_stages_cpu.py, tests/test_gpu_sift_stages.py) ----
struct SiftRun {
  Pyramid pyr;
  Trace trace;
  std::vector<Key> keys;
  std::map<std::pair<int, int>, std::pair<Img, Img>> grads;   // (octave, index) -> GradOriImages of that level, made on demand
};

// the gradient images of Gaussian level `index` (1..kScales: the levels keys come from) of `octave`, or null
static const std::pair<Img, Img>* run_grads(SiftRun* R, int octave, int index) {
  if (octave < 0 || octave >= (int)R->pyr.gaus.size() || index < 1 || index > kScales) return nullptr;
  auto it = R->grads.find({octave, index});
  if (it == R->grads.end()) {
    it = R->grads.emplace(std::make_pair(octave, index), std::pair<Img, Img>()).first;
    grad_ori(R->pyr.gaus[octave][index], it->second.first, it->second.second);
  }
  return &it->second;
}

// Descriptors of caller-supplied keys on the run's own pyramid (describe_key).  mode 0 f32: make_key's arithmetic ->
// out float [n][128]; 1 f64 -> out double [n][128]; 2 pert (ulps, dir, seed: Tweak) -> float; 3 drop (drop[n]: Tweak::drop
// per key) -> float.  totals (optional) [n]: selected samples per key, the dropped one included.  Returns 0, or -1 --
// nothing written -- when a key's octave / index is not a level keys come from or the mode does not exist.
int orc_sift_run_describe(void* run, int n, const int32_t* octave, const int32_t* index, const float* fsize,
                          const float* frow, const float* fcol, const float* ori, int mode, int ulps, int dir,
                          uint32_t seed, const int64_t* drop, void* out, int32_t* totals) {
  SiftRun* R = static_cast<SiftRun*>(run);
  if (mode < 0 || mode > 3 || (mode == 3 && !drop)) return -1;
  for (int i = 0; i < n; ++i)
    if (!run_grads(R, octave[i], index[i])) return -1;
  for (int i = 0; i < n; ++i) {
    const std::pair<Img, Img>& g = *run_grads(R, octave[i], index[i]);
    int total;
    if (mode == 1) {
      total = describe_key<double>(static_cast<double*>(out) + (size_t)128 * i, &R->pyr.gaus[octave[i]][index[i]], g.first,
                                   g.second, fsize[i], frow[i], fcol[i], ori[i]);
    } else {
      Tweak tw;
      if (mode == 2) {
        tw.ulps = ulps;
        tw.dir = dir;
        tw.seed = seed;
        tw.key = (uint32_t)i;
      }
      if (mode == 3) tw.drop = (long)drop[i];
      total = describe_key<float>(static_cast<float*>(out) + (size_t)128 * i, nullptr, g.first, g.second, fsize[i], frow[i],
                                  fcol[i], ori[i], mode == 0 ? nullptr : &tw);
    }
    if (totals) totals[i] = total;
  }
  return 0;
}

// Mode drop for the samples an off-by-one in a window row's interval loses: for every key and every window row with a
// selected sample, the row's first (which 0) and -- where the row has two or more -- last (which 1) selected sample is
// left out in turn, and the result compared with the key's f64 descriptor `ref` [n][128]: tried / detected [n][2] count
// the samples and those with max |drop - f64| > bar[key].  Returns 0, -1 as above.
int orc_sift_run_drop_row_ends(void* run, int n, const int32_t* octave, const int32_t* index, const float* fsize,
                               const float* frow, const float* fcol, const float* ori, const double* ref,
                               const double* bar, int32_t* tried, int32_t* detected) {
  SiftRun* R = static_cast<SiftRun*>(run);
  for (int i = 0; i < n; ++i)
    if (!run_grads(R, octave[i], index[i])) return -1;
  std::vector<int> rows;
  float d[128];
  for (int i = 0; i < n; ++i) {
    const std::pair<Img, Img>& g = *run_grads(R, octave[i], index[i]);
    rows.clear();
    describe_key<float>(d, nullptr, g.first, g.second, fsize[i], frow[i], fcol[i], ori[i], nullptr, &rows);
    tried[2 * i] = tried[2 * i + 1] = detected[2 * i] = detected[2 * i + 1] = 0;
    const long m = (long)rows.size();
    for (long t = 0; t < m; ++t) {
      const bool first = t == 0 || rows[t - 1] != rows[t], last = t + 1 == m || rows[t + 1] != rows[t];
      if (!first && !last) continue;
      const int which = first ? 0 : 1;
      Tweak tw;
      tw.drop = t;
      describe_key<float>(d, nullptr, g.first, g.second, fsize[i], frow[i], fcol[i], ori[i], &tw);
      double worst = 0;
      for (int e = 0; e < 128; ++e) worst = std::max(worst, std::fabs((double)d[e] - ref[(size_t)128 * i + e]));
      ++tried[2 * i + which];
      if (worst > bar[i]) ++detected[2 * i + which];
    }
  }
  return 0;
}

void* orc_sift_run(const uint8_t* gray, int w, int h, int double_size) {
  SiftRun* R = new SiftRun;
  run_sift(gray, w, h, double_size, R->keys, &R->pyr, &R->trace);
  return R;
}

void orc_sift_run_free(void* run) { delete static_cast<SiftRun*>(run); }

int orc_sift_run_octaves(const void* run, int* rows, int* cols, int cap) {
  const SiftRun* R = static_cast<const SiftRun*>(run);
  const int n = (int)R->pyr.gaus.size();
  for (int o = 0; o < n && o < cap; ++o) {
    rows[o] = R->pyr.gaus[o][0].rows;
    cols[o] = R->pyr.gaus[o][0].cols;
  }
  return n;
}

int orc_sift_run_level(const void* run, int octave, int kind, int i, float* out) {
  const SiftRun* R = static_cast<const SiftRun*>(run);
  if (octave < 0 || octave >= (int)R->pyr.gaus.size()) return 0;
  const std::vector<Img>& v = kind == 0 ? R->pyr.gaus[octave] : R->pyr.dog[octave];
  if (i < 0 || i >= (int)v.size()) return 0;
  memcpy(out, v[i].px.data(), v[i].px.size() * sizeof(float));
  return (int)v[i].px.size();
}

int orc_sift_run_hits(const void* run, int32_t* ints, float* floats, int cap) {
  const SiftRun* R = static_cast<const SiftRun*>(run);
  const int n = (int)R->trace.hits.size();
  for (int i = 0; i < n && i < cap; ++i) {
    const Hit& h = R->trace.hits[i];
    const int32_t iv[10] = {h.octave, h.index, h.r0, h.c0, h.r, h.c, h.passed, h.took, h.first_peak, h.n_peaks};
    const float fv[7] = {h.X[0], h.X[1], h.X[2], h.val, h.fsize, h.frow, h.fcol};
    memcpy(ints + (size_t)10 * i, iv, sizeof iv);
    memcpy(floats + (size_t)7 * i, fv, sizeof fv);
  }
  return n;
}

int orc_sift_run_peaks(const void* run, int32_t* hit_bin, float* ang, int cap) {
  const SiftRun* R = static_cast<const SiftRun*>(run);
  const int n = (int)R->trace.peaks.size();
  for (int i = 0; i < n && i < cap; ++i) {
    hit_bin[2 * i] = R->trace.peaks[i].hit;
    hit_bin[2 * i + 1] = R->trace.peaks[i].bin;
    ang[i] = R->trace.peaks[i].ang;
  }
  return n;
}

int orc_sift_taps(float sigma) { return (int)gauss_kernel(sigma).size(); }

void orc_sift_blur(const float* src, int rows, int cols, float sigma, float* dst) {
  Img s(rows, cols), d;
  memcpy(s.px.data(), src, s.px.size() * sizeof(float));
  blur(d, s, sigma);
  memcpy(dst, d.px.data(), d.px.size() * sizeof(float));
}

void orc_sift_half(const float* src, int rows, int cols, float* dst) {
  Img s(rows, cols);
  memcpy(s.px.data(), src, s.px.size() * sizeof(float));
  const Img d = half_size(s);
  memcpy(dst, d.px.data(), d.px.size() * sizeof(float));
}

}  // extern "C"
