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
// The arithmetic lives in filter_depth_dev.h, in two forms of one F1: filter_depth_score (below; a workgroup walks the
// slots, lane 0 adds out of LDS) for the launch of its own, filter_depth_score_wave (one object, one wavefront, no LDS)
// for the POSE tails of a fused frame (pose.hip) and for filter_depth_wave_kernel.
// The (int) of a projected coordinate that is NaN, infinite or outside int's range is undefined in the reference: here
// such a point is off the image.  One image per frame (the reference projects the matches through their own image; the
// callers refuse several).
#include "filter_depth_dev.h"

namespace mh {

namespace {

// F1 of the depth class for the object slots first, first + stride, ... (every thread of the workgroup calls it): the
// slot walk, the score chain and the claims are filter_score's (filter_dev.h), one image.
__device__ __forceinline__ void filter_depth_score(FilterLds& S, const FilterBuffers& fb, const DevCam& cam, float feature_distance,
                                                   const FilterDepthArgs& da, int n_slots, int first, int stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  filter_load_slots(S, fb, n_slots, false);
  const int tw = 64 * wave;   // the wavefront's 64 words of term_s
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
      bool use;
      const double term = filter_depth_point_term(T, da, j < np ? da.pts + 3 * (size_t)(pb + j) : nullptr, use);
      used += __popcll(__ballot(use));
      S.term_s[tw + lane] = term;
      filter_wave_sync();
      if (lane == 0) {
        const int cnt = min(64, np - base);
        for (int jj = 0; jj < cnt; ++jj) IS = (float)((double)IS + S.term_s[tw + jj]);
      }
      filter_wave_sync();
    }
    // ---- :260-270 ----
    if (lane == 0) filter_depth_close(fb, da, o, score, IS, used, plausible, np);
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

// The same through filter_depth_score_wave (mh_filter_depth_debug_form 1): every wavefront one object slot at a time --
// the arithmetic the fused POSE tails run, under the stage-level entry without POSE in between
__global__ __launch_bounds__(FT) void filter_depth_wave_kernel(FilterBuffers fb, DevCam cam, float feature_distance,
                                                               int min_points, float min_score, FilterDepthArgs da,
                                                               int32_t* n_slots_dev, int32_t* n_clusters_dev,
                                                               FrameCounts* counts, FilterTail tail) {
  __shared__ FilterLds S;
  const int n_slots = *n_slots_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = (int)blockIdx.x * (FT / 64) + wave; o < n_slots; o += (int)gridDim.x * (FT / 64))
    if (fb.obj_valid[o])   // (wave-uniform)
      filter_depth_score_wave(fb, cam, feature_distance, da, o, fb.obj_model[o], fb.obj_pose + 7 * (size_t)o,
                              fb.obj_pose + 7 * (size_t)o + 4, lane);
  if (!last_workgroup(tail.ticket)) return;
  filter_finish(S, fb, min_points, min_score, n_slots, n_slots_dev, n_clusters_dev, counts, tail);
}

}  // namespace

void launch_filter_depth_wave(const FilterBuffers& fb, const DevCam& cam, int min_points, float feature_distance,
                              float min_score, const FilterDepthArgs& da, int32_t* n_slots_dev, int32_t* n_clusters_dev,
                              FrameCounts* counts, const FilterTail& tail, hipStream_t s) {
  const int want = (fb.max_objects + FT / 64 - 1) / (FT / 64);
  const int grid = want < 1 ? 1 : (want < FILTER_GRID ? want : FILTER_GRID);
  hipLaunchKernelGGL(filter_depth_wave_kernel, dim3(grid), dim3(FT), 0, s, fb, cam, feature_distance, min_points,
                     min_score, da, n_slots_dev, n_clusters_dev, counts, tail);
}

void launch_filter_depth(const FilterBuffers& fb, const DevCam& cam, int min_points, float feature_distance,
                         float min_score, const FilterDepthArgs& da, int32_t* n_slots_dev, int32_t* n_clusters_dev,
                         FrameCounts* counts, const FilterTail& tail, hipStream_t s) {
  const int grid_cap = tail.grid > 0 ? (tail.grid < FILTER_GRID ? tail.grid : FILTER_GRID) : FILTER_GRID;
  const int grid = fb.max_objects < grid_cap ? (fb.max_objects > 0 ? fb.max_objects : 1) : grid_cap;
  hipLaunchKernelGGL(filter_depth_kernel, dim3(grid), dim3(FT), 0, s, fb, cam, feature_distance, min_points,
                     min_score, da, n_slots_dev, n_clusters_dev, counts, tail);
}

}  // namespace mh
