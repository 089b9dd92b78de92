// FILTER, depth class, as device code shared by filter_depth_kernel / filter_depth_wave_kernel (filter_depth.hip) and
// the fused tails of pose_kernel / pose_refine_kernel (pose.hip): see filter_depth.hip for what the class computes.
// One function per piece of the arithmetic -- a test point's term, the :260-270 step -- so that the workgroup form
// (filter_depth_score: lane 0 adds out of LDS) and the wave form (filter_depth_score_wave: no LDS at all) cannot diverge.
#pragma once
#include "filter_dev.h"

namespace mh {

namespace {

// (int) p of :226 where the reference defines it; false: NaN, infinite or outside int -- off the image
__device__ __forceinline__ bool pixel_of(float p, int& i) {
  if (!(p >= -2147483648.f && p < 2147483648.f)) return false;
  i = (int)p;   // truncation toward zero: (-1, 0) -> 0, inside the image as in the reference
  return true;
}

// (int)(MinKeypointFraction * keypoints.size()) of :260; outside int (undefined in the reference): the nearest int, NaN: 0
__device__ __forceinline__ int int_of(float v) {
  if (!(v < 2147483648.f)) return v != v ? 0 : 0x7FFFFFFF;
  return v < -2147483648.f ? (int)0x80000000 : (int)v;
}

// One test point of the incorrect score (:218-255), by the lane that owns it.  k: the point in model coordinates, or
// nullptr for a lane past the list's end.  `use`: the point fell on a measured pixel of the map (usedKeypointCount, :237).
// Returns what :254 adds to IS -- 0. for a point that is skipped, off the list, or occluded (:244).
__device__ __forceinline__ double filter_depth_point_term(const TM& T, const FilterDepthArgs& da, const float* k, bool& use) {
  const float* const zmap = reinterpret_cast<const float*>(da.img);
  bool on = false;          // the point falls on a pixel of the map
  int px = 0;
  float zp = 0.f;           // putativeDepth
  if (k) {
    float wx, wy, wz, cx, cy, cz;
    tm_apply(T.r, T.t, k[0], k[1], k[2], wx, wy, wz);                       // PoseTM.transform (:220)
    tm_apply_inv(da.dcam.Rc, da.dcam.tc, wx, wy, wz, cx, cy, cz);           // depthmap->TM.inverseTransform (:221)
    const float pu = __fadd_rn(__fmul_rn(__fdiv_rn(cx, cz), da.dcam.K[0]), da.dcam.K[2]);   // :223
    const float pv = __fadd_rn(__fmul_rn(__fdiv_rn(cy, cz), da.dcam.K[1]), da.dcam.K[3]);   // :224
    int ix = 0, iy = 0;
    on = pixel_of(pu, ix) && pixel_of(pv, iy) && ix >= 0 && ix < da.w && iy >= 0 && iy < da.h;   // :226-231
    px = iy * da.w + ix;
    zp = cz;
  }
  // both gathers of the step before either is used: their addresses are the lane's own arithmetic
  float dist = 0.f, zk = 0.f;
  if (on) {
    if (da.fill) dist = da.fill[px];        // distanceMap->getProb (:233)
    zk = zmap[4 * (size_t)px + 2];          // depthmap->getDepth (:239)
  }
  use = on && !(dist > 0.f);                // :234-237
  double term = 0.;
  if (use && !(zk < zp)) {                  // :244: the sensor saw something in front: an occlusion, nothing added
    const float cauchy = __fmul_rn(da.depth_fraction, zk);   // :248
    float t = __fdiv_rn(__fsub_rn(zp, zk), cauchy);          // :250
    t = __fmul_rn(t, t);                                     // :251
    term = 1.0 - (1.0 / (1.0 + (double)t));                  // :254
  }
  return term;
}

// :260-270 (one lane): the IS that is subtracted, obj_score = score - IS, the optional per-slot outputs
__device__ __forceinline__ void filter_depth_close(const FilterBuffers& fb, const FilterDepthArgs& da, int o, float score, float IS,
                                                   int used, int plausible, int np) {
  if (used <= int_of(__fmul_rn(da.min_keypoint_fraction, (float)np)))   // :260
    IS = 0.f;
  else
    IS = __fmul_rn(IS, __fdiv_rn((float)plausible, (float)used));
  fb.obj_score[o] = __fsub_rn(score, IS);
  if (da.out_is) da.out_is[o] = IS;
  if (da.out_used) da.out_used[o] = used;
  if (da.out_plausible) da.out_plausible[o] = plausible;
}

// F1 of the depth class for ONE object by one wavefront: what filter_score_wave (filter_dev.h) is to filter_score.  No
// FilterLds, no LDS, no workgroup barrier.  `quat` / `trans`: the pose as obj_pose holds it (all lanes); fb: the frame's
// buffers; da: the frame's own map, its camera, the class's parameters and the test points.  One image.
__device__ __forceinline__ void filter_depth_score_wave(const FilterBuffers& fb, const DevCam& cam, float feature_distance,
                                                        const FilterDepthArgs& da, int o, int m, const float* quat,
                                                        const float* trans, int lane) {
  const int b = fb.model_off[m];
  const int n = fb.model_off[m + 1] - b;
  TM T;
  tm_from_pose(T, quat, trans);
  // ---- the projection score (:191-205) ----
  float score = 0.f;
  unsigned inl_bits = 0u;     // this lane's in-cluster flags of the first 32 steps
  int plausible = 0;          // clusterSize
  for (int base = 0, step = 0; base < n; base += 64, ++step) {
    const int i = base + lane;
    float e = __builtin_inff();
    if (i < n) {
      const mh_corr c = fb.corr[b + i];
      e = reproj_err2(T.r, T.t, cam, c.x, c.y, c.z, c.u, c.v);
    }
    const bool in = e < feature_distance;
    if (in && step < 32) inl_bits |= 1u << step;
    plausible += __popcll(__ballot(i < n && e < da.plausible_sq_distance));
    score = filter_chain_wave(score, in ? 1. / ((double)e + 1.) : 0., min(64, n - base));
  }
  // ---- the incorrect score over the model's test points (:207-255) ----
  const int pb = da.pts_off[m], np = da.pts_off[m + 1] - pb;
  float IS = 0.f;
  int used = 0;               // usedKeypointCount
  for (int base = 0; base < np; base += 64) {
    const int j = base + lane;
    bool use;
    const double term = filter_depth_point_term(T, da, j < np ? da.pts + 3 * (size_t)(pb + j) : nullptr, use);
    used += __popcll(__ballot(use));
    IS = filter_chain_wave(IS, term, min(64, np - base));
  }
  if (lane == 0) filter_depth_close(fb, da, o, score, IS, used, plausible, np);
  // ---- the claims, by the projection score (:274-286) ----
  if (!(score > 0.f)) return;
  const unsigned long long key = pack_best(score, o);
  for (int base = 0, step = 0; base < n; base += 64, ++step) {
    const int i = base + lane;
    if (i >= n) continue;
    bool in;
    if (step < 32) {
      in = (inl_bits >> step) & 1u;
    } else {
      const mh_corr c = fb.corr[b + i];
      in = reproj_err2(T.r, T.t, cam, c.x, c.y, c.z, c.u, c.v) < feature_distance;
    }
    if (in) atomicMax(&fb.best[fb.m_rep[b + i]], key);
  }
}

}  // namespace

}  // namespace mh
