// FILTER, depth class: FILTER_PROJECTION_DEPTH_CPU::process on gfx950
// (moped3d/libmoped/src/filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329).
//
// FILTER_PROJECTION_CPU (filter.hip: F1..F4) plus a test of every object's pose against the frame's depth map:
//  F1  per object, one wavefront: the projection score and the in-cluster flags exactly as filter_score forms them
//      (:193-201), clusterSize = matches with err2 < PlausibleSqDistance (:202-204); then the "incorrect score" IS over
//      the model's test points in list order (:213-255): the point through the object's pose into the depth camera,
//      truncated to a pixel; off the image or on a FILLED pixel (fill distance > 0) it is skipped, else it is used; a
//      sensor reading in front of the point (an occlusion) adds nothing, one behind it the Cauchy term
//      1 - 1/(1 + ((z - zk) / (DepthFraction zk))^2) in double, added into the float IS by the reference's
//      Float += double chain; :260-267 in float; obj_score = score - IS (:270).
//      The keypoint claims carry the PROJECTION score (:277 compares the local `score`), only the erase test
//      `object->score < MinScore` (:309) sees the penalty.
//  F2..F4  filter_finish (filter_dev.h), unchanged: it reads the claims' object ids and obj_score, never the claims'
//      scores, so obj_score = score - IS and a claim key made of `score` need no second array.
// The (int) of a projected coordinate that is NaN, infinite or outside int's range is undefined in the reference: here
// such a point is off the image.  One image per frame (the reference projects the matches through their own image; the
// callers refuse several).
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

// F1 of the depth class for the object slots first, first + stride, ... (every thread of the workgroup calls it): the
// slot walk, the score chain and the claims are filter_score's (filter_dev.h), one image.
__device__ __forceinline__ void filter_depth_score(FilterLds& S, const FilterBuffers& fb, const DevCam& cam, float feature_distance,
                                                   const FilterDepthArgs& da, int n_slots, int first, int stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  filter_load_slots(S, fb, n_slots, false);
  const int tw = 64 * wave;   // the wavefront's 64 words of term_s
  const float* const zmap = reinterpret_cast<const float*>(da.img);
  const int n_listed = S.cnt_s, n_low = min(n_slots, FL_SLOTS);
  for (int idx = first + stride * wave; idx < n_listed + (n_slots - n_low); idx += stride * (FT / 64)) {
    const int o = idx < n_listed ? S.vlist_s[idx] : n_low + (idx - n_listed);
    int m, b, n;
    if (!filter_slot(S, fb, o, m, b, n)) continue;
    TM T;
    tm_from_pose(T, fb.obj_pose + 7 * (size_t)o, fb.obj_pose + 7 * (size_t)o + 4);
    // ---- the projection score (:191-205) ----
    float score = 0.f;          // lane 0 only
    unsigned inl_bits = 0u;     // this lane's in-cluster flags of the first 32 steps
    int plausible = 0;          // clusterSize (all lanes)
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
      S.term_s[tw + lane] = in ? 1. / ((double)e + 1.) : 0.;
      filter_wave_sync();
      if (lane == 0) {
        const int cnt = min(64, n - base);
        for (int j = 0; j < cnt; ++j) score = (float)((double)score + S.term_s[tw + j]);
      }
      filter_wave_sync();
    }
    // ---- the incorrect score over the model's test points (:207-255) ----
    const int pb = da.pts_off[m], np = da.pts_off[m + 1] - pb;
    float IS = 0.f;             // lane 0 only
    int used = 0;               // usedKeypointCount (all lanes)
    for (int base = 0; base < np; base += 64) {
      const int j = base + lane;
      bool on = false;          // the point falls on a pixel of the map
      int px = 0;
      float zp = 0.f;           // putativeDepth
      if (j < np) {
        const float* k = da.pts + 3 * (size_t)(pb + j);
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
      const bool use = on && !(dist > 0.f);     // :234-237
      used += __popcll(__ballot(use));
      double term = 0.;
      if (use && !(zk < zp)) {                  // :244: the sensor saw something in front: an occlusion, nothing added
        const float cauchy = __fmul_rn(da.depth_fraction, zk);   // :248
        float t = __fdiv_rn(__fsub_rn(zp, zk), cauchy);          // :250
        t = __fmul_rn(t, t);                                     // :251
        term = 1.0 - (1.0 / (1.0 + (double)t));                  // :254
      }
      S.term_s[tw + lane] = term;
      filter_wave_sync();
      if (lane == 0) {
        const int cnt = min(64, np - base);
        for (int jj = 0; jj < cnt; ++jj) IS = (float)((double)IS + S.term_s[tw + jj]);
      }
      filter_wave_sync();
    }
    // ---- :260-270 ----
    if (lane == 0) {
      if (used <= int_of(__fmul_rn(da.min_keypoint_fraction, (float)np)))   // :260
        IS = 0.f;
      else
        IS = __fmul_rn(IS, __fdiv_rn((float)plausible, (float)used));
      fb.obj_score[o] = __fsub_rn(score, IS);
      if (da.out_is) da.out_is[o] = IS;
      if (da.out_used) da.out_used[o] = used;
      if (da.out_plausible) da.out_plausible[o] = plausible;
    }
    // ---- the claims, by the projection score (:274-286) ----
    score = __shfl(score, 0);
    if (!(score > 0.f)) continue;
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
}

// filter_kernel with the depth term: F1 in every workgroup, F2..F4 in the last one to finish
__global__ __launch_bounds__(FT) void filter_depth_kernel(FilterBuffers fb, DevCam cam, float feature_distance,
                                                          int min_points, float min_score, FilterDepthArgs da,
                                                          int32_t* n_slots_dev, int32_t* n_clusters_dev,
                                                          FrameCounts* counts, FilterTail tail) {
  __shared__ FilterLds S;
  const int n_slots = *n_slots_dev;
  filter_depth_score(S, fb, cam, feature_distance, da, n_slots, blockIdx.x, gridDim.x);
  if (!last_workgroup(tail.ticket)) return;
  filter_finish(S, fb, min_points, min_score, n_slots, n_slots_dev, n_clusters_dev, counts, tail);
}

}  // namespace

void launch_filter_depth(const FilterBuffers& fb, const DevCam& cam, int min_points, float feature_distance,
                         float min_score, const FilterDepthArgs& da, int32_t* n_slots_dev, int32_t* n_clusters_dev,
                         FrameCounts* counts, const FilterTail& tail, hipStream_t s) {
  const int grid_cap = tail.grid > 0 ? (tail.grid < FILTER_GRID ? tail.grid : FILTER_GRID) : FILTER_GRID;
  const int grid = fb.max_objects < grid_cap ? (fb.max_objects > 0 ? fb.max_objects : 1) : grid_cap;
  hipLaunchKernelGGL(filter_depth_kernel, dim3(grid), dim3(FT), 0, s, fb, cam, feature_distance, min_points,
                     min_score, da, n_slots_dev, n_clusters_dev, counts, tail);
}

}  // namespace mh
