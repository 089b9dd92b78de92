// CLUSTER_LINKAGE's per-pair expressions (CLUSTER_LINKAGE_CPU.hpp; line numbers are that file's), shared by the two
// forms of the clusterer -- linkage.hip (MH_LINKAGE_SCAN: one workgroup per problem) and linkage_rowmax.hip
// (MH_LINKAGE_ROWMAX: the matrix stage on the whole grid) -- so that both compute every matrix element with the same
// roundings: Float = float, unsuffixed literals = double, the reference's expression order.
#pragma once
#include "steps.h"

namespace mh {
namespace {

__device__ __forceinline__ float sq_dist(const float* a, const float* b, int n) {   // Pt::sqEuclDist: d = pt - this
  float r = 0.f;
  for (int x = 0; x < n; ++x) {
    const float d = __fsub_rn(b[x], a[x]);
    r = __fadd_rn(r, __fmul_rn(d, d));
  }
  return r;
}

__device__ __forceinline__ void saturate(int& x, int& y, int w, int h) {
  x = x < 0 ? 0 : (x >= w ? w - 1 : x);
  y = y < 0 ? 0 : (y >= h ? h - 1 : y);
}

// getDiscontinuityMatrix's element (:244-283): the largest difference between the slope of the
// straight depth line from p to q and the slopes between consecutive Bresenham samples (:176-220).
__device__ float discontinuity(const DepthImage& D, int px, int py, int qx, int qy) {
  const float depthStart = D.img[(size_t)py * D.w + px].z, depthEnd = D.img[(size_t)qy * D.w + qx].z;
  const int xDiff = px - qx, yDiff = py - qy;
  const float imagePlaneDist = sqrtf((float)(xDiff * xDiff + yDiff * yDiff));
  const float directAngle = atan2f(__fsub_rn(depthEnd, depthStart), imagePlaneDist);
  int x0 = px, y0 = py, x1 = qx, y1 = qy, t;
  const bool steep = abs(y1 - y0) > abs(x1 - x0);
  if (steep) {
    t = x0; x0 = y0; y0 = t;
    t = x1; x1 = y1; y1 = t;
  }
  if (x0 > x1) {
    t = x0; x0 = x1; x1 = t;
    t = y0; y0 = y1; y1 = t;
  }
  const float deltaX = __fsub_rn((float)x1, (float)x0), deltaY = fabsf(__fsub_rn((float)y1, (float)y0));
  const int yStep = (y0 < y1) ? 1 : -1;
  int perStep = (x1 - x0) / 20;
  if (perStep < 1) perStep = 1;
  float error = 0.f;
  const float deltaError = __fdiv_rn(deltaY, deltaX);
  int y = y0;
  float maxAngleDiff = -1.f;
  int pax = 0, pay = 0;
  bool have = false;
  for (int x = x0; x <= x1;) {
    const int cx = steep ? y : x, cy = steep ? x : y;
    if (have) {
      int ax = pax, ay = pay, bx = cx, by = cy;
      saturate(ax, ay, D.w, D.h);
      saturate(bx, by, D.w, D.h);
      const float depth1 = D.img[(size_t)ay * D.w + ax].z, depth2 = D.img[(size_t)by * D.w + bx].z;
      const float dx = (float)(pax - cx), dy = (float)(pay - cy);
      const float pixDistance = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
      const float pixAngle = atan2f(__fsub_rn(depth2, depth1), pixDistance);
      const float angleDiff = fabsf(__fsub_rn(directAngle, pixAngle));
      if (angleDiff > maxAngleDiff) maxAngleDiff = angleDiff;
    }
    pax = cx;
    pay = cy;
    have = true;
    x += perStep;
    if (x > x1) break;   // the values below are not used any more (and are NaN when p == q)
    error = __fadd_rn(error, __fmul_rn(__fmul_rn(deltaError, (float)perStep), (float)yStep));
    float intPart;
    error = modff(error, &intPart);
    y = (int)__fadd_rn((float)y, intPart);
  }
  const float discontinuityDiv = (float)(-2 * (M_PI / 128) * (M_PI / 128));
  return expf(__fdiv_rn(__fmul_rn(maxAngleDiff, maxAngleDiff), discontinuityDiv));
}

// getAverageNNDistances' distances of one pair (:97-123)
__device__ __forceinline__ void lk_nn_pair(const float* uv_i, const float* uv_j, const float* mx_i, const float* mx_j,
                                           float& d2, float& d3) {
  d2 = sqrtf(sq_dist(uv_i, uv_j, 2));
  d3 = sqrtf(sq_dist(mx_i, mx_j, 3));
}

// fill weight of adaptiveWeightSum (:331-337): 1.0 / (1 + (d*d/gammaSq)), gamma = 25
__device__ __forceinline__ float lk_fill_weight(const DepthImage& D, const float* uv) {
  int x = (int)uv[0], y = (int)uv[1];
  saturate(x, y, D.w, D.h);
  const float d = D.fill ? D.fill[(size_t)y * D.w + x] : 0.f;
  return (float)(1.0 / (double)__fadd_rn(1.f, __fdiv_rn(__fmul_rn(d, d), 625.f)));
}

__device__ __forceinline__ float lk_two_sigma_sq(float sigma) { return __fmul_rn(__fmul_rn(2.f, sigma), sigma); }

// pass 1 (:133-149, 231-285, 681-682): K2D's element -> v2, K3D + the discontinuity kernel -> the return value
__device__ __forceinline__ float lk_pass1(const DepthImage& D, const float* uv_i, const float* uv_j, const float* wx_i,
                                          const float* wx_j, float two2, float two3, float& v2) {
  v2 = expf(__fdiv_rn(__fmul_rn(-1.f, sq_dist(uv_i, uv_j, 2)), two2));
  const float v3 = expf(__fdiv_rn(__fmul_rn(-1.f, sq_dist(wx_i, wx_j, 3)), two3));
  int ax = (int)uv_i[0], ay = (int)uv_i[1], bx = (int)uv_j[0], by = (int)uv_j[1];
  saturate(ax, ay, D.w, D.h);
  saturate(bx, by, D.w, D.h);
  return __fadd_rn(v3, discontinuity(D, ax, ay, bx, by));
}

// pass 2 (:151-173, 683-692): the element normalised by pass 1's maximum, x / + K3F
__device__ __forceinline__ float lk_pass2(int use3d_filter, bool diagonal, const float* mx_i, const float* mx_j,
                                          const float* wx_i, const float* wx_j, float a, float max1) {
  const float sigma = 0.1f;
  const float twoSigmaSq = __fmul_rn(__fmul_rn(2.f, sigma), sigma);
  float val = 1.f;
  if (!diagonal) {
    const float dm = sqrtf(sq_dist(mx_i, mx_j, 3)), dr = sqrtf(sq_dist(wx_i, wx_j, 3));
    const float de = __fdiv_rn(fabsf(__fsub_rn(dm, dr)), dm);
    val = expf(__fdiv_rn(__fmul_rn(__fmul_rn(-1.f, de), de), twoSigmaSq));
  }
  const float e = __fdiv_rn(a, max1);
  return use3d_filter == 1 ? __fadd_rn(e, val) : __fmul_rn(e, val);
}

// pass 3 (:339-365): the final similarity from K2D's element, the 3-D side's and the two fill weights
__device__ __forceinline__ float lk_pass3(float K2De, float a, float max2, float w_i, float w_j) {
  const float K3De = __fdiv_rn(a, max2);
  const float jointWeight = __fmul_rn(w_i, w_j);
  const float w2D = (float)(0.5 + 0.5 * (1.0 - (double)jointWeight));   // alpha + alphaBar*(1.0 - jointWeight)
  const float w3D = __fmul_rn(0.5f, jointWeight);
  return __fadd_rn(__fmul_rn(w2D, K2De), __fmul_rn(w3D, K3De));
}

// The average / minimum / maximum linkage value of row `first` at column i after the merge (first, second)
// (:506-526), from the two rows' entries da = Dm[first][i], db = Dm[second][i] and the sizes before the merge.
// Minimum / maximum linkage: the reference recomputes min / max of K over the merged cluster's pairs (minimumLinkage
// :404-413, maximumLinkage :390-399); min over a union is the min of the two clusters' minima -- the row entries hold
// exactly those (singletons start as K itself) -- so the update is exact, no arithmetic.  A cluster i that is EMPTY
// (absorbed earlier) gets the reference's empty-loop value.  (`second` is empty by the time the reference's loop runs; a
// merge may also have absorbed a cluster that was empty already -- the stale list entry of the scan, S2 = 0 -- and then
// changes nothing.)  The reference's loops compare with `<` / `>` from 1e20 / -1: a NaN similarity never becomes the
// minimum / maximum (fminf / fmaxf skip one NaN the same way), and over nothing but NaN the start value stays.
__device__ __forceinline__ float lk_merged_value(int linkage_type, float da, float db, int S1, int S2, bool empty) {
  if (linkage_type == 1) {
    const float a = __fmul_rn((float)S1, da), b = __fmul_rn((float)S2, db);
    return (float)((1.0 / (double)(S1 + S2)) * (double)__fadd_rn(a, b));
  }
  const float start = linkage_type == 0 ? 1e20f : -1.f;
  float v = start;
  if (!empty) v = S2 == 0 ? da : (linkage_type == 0 ? fminf(da, db) : fmaxf(da, db));
  return v != v ? start : v;
}

}  // namespace
}  // namespace mh
