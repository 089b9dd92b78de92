// DEPTH_VERIFY: DEPTH_VERIFY_CPU::process on gfx950 (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp:86-208).
//
// The reference's sanity check of every object that left FILTER2 against the Kinect map.  Per object:
//  QS  the quality score (:123-137): over ALL matches of the object's model in list order, the pinned project()
//      (reproj_err2: z < 0.001 gives an infinite error and a quotient of 0.), `QS += 1.0 / (1.0 + projectionError)`;
//      plausibleMatchCount = matches with projectionError < FeatureDistance.
//  IS  the incorrect score (:142-189): over ALL keypoints of the model -- the rows the store holds for it, in row
//      order -- the keypoint through the object's pose into the depth camera, truncated to a pixel (:164-167).  A
//      keypoint whose fill distance is above MaxDistance is skipped (:168), else it is used (:171); a sensor reading in
//      front of it is an occlusion and adds nothing (:178), one behind it the Cauchy term
//      `IS += 1.0 - (1.0 / (1.0 + term))` (:182-188).
//  :191-206  multiplier = (Float)keypointCount / usedKeypointCount, capped by MaxMultiplier; IS *= multiplier;
//      QS /= plausibleMatchCount; IS /= keypointCount; the object is erased if IS > QS.
// Float is float: QS, IS, multiplier, cauchyScale and term are floats; the literals 1.0 make every added quotient a
// double that is rounded into the float accumulator at each step.  Both sums are therefore ORDERED CHAINS, QS in match
// order and IS in keypoint order, and the device gives the same words.  The one reordering used: a term that is exactly
// 0. (a skipped keypoint, a `continue`, a lane past the end) may be added or left out, `float + 0.` being the float.
// The divisors are ints converted to float, zero included: x/0 = inf is capped by MaxMultiplier, 0/0 = NaN passes the
// cap and makes IS > QS false -- the object stays.
// Readings settled here:
//  - modelNum is the object's model index; matches[m] the model's slice of the match list; one image.
//  - The reference does not test the pixel: a keypoint off the map reads outside the buffer there.  Here it is counted
//    in keypointCount and not used; the same for a coordinate that is NaN, infinite or outside int (pixel_of's rule,
//    truncation toward zero inside (-1, 0) included).
//  - Everything else as written: a keypoint behind the depth camera projects like any other, a NaN depth gives a NaN
//    term, a NaN distance is used (`distance > MaxDistance` is false).
//  - No distance map (the reference would dereference null): no distance test, every on-map pixel is used.
//
// Two forms of one arithmetic (depth_verify_dev.h; mh_depth_verify_debug_form):
//  0  one workgroup per object, grid-strided.  The per-point work feeds two serial chains; the chains are the critical
//     path (a dependent cvt / add / cvt per term), so wavefronts 1..3 produce the terms of round r -- DV_CHUNK matches or
//     keypoints, the transform, the projection and both gathers issued together -- into one half of an LDS ring while
//     wavefront 0 chains the terms of round r - 1 out of the other half; one barrier per round.  The counts are ballots
//     of the producing wavefronts, summed by the closing thread.
//  1  one wavefront per object, no LDS: depth_verify_object_wave.
// No floating-point atomics, no scratch.
#include "depth_verify_dev.h"

namespace mh {

namespace {

struct DepthVerifyLds {
  double term_s[2][DV_CHUNK];
  int cnt_s[DV_THREADS / 64][2];   // per producing wavefront: plausible, used
};

// form 0 for one object: every thread of the workgroup calls it; ends behind a barrier
__device__ __forceinline__ void depth_verify_object(DepthVerifyLds& S, const DepthVerifyArgs& a, const mh_corr* corr,
                                                    const int32_t* model_off, int m, const float* pose, mh_verify_record* rec) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int p = tid - 64;   // the producing thread's place in a round
  TM T;
  tm_from_pose(T, pose, pose + 4);
  const int b = model_off[m], n = model_off[m + 1] - b;
  const int kb = a.model_begin[m], nk = a.model_begin[m + 1] - kb;
  const int rq = (n + DV_CHUNK - 1) / DV_CHUNK, rk = (nk + DV_CHUNK - 1) / DV_CHUNK;
  float QS = 0.f, IS = 0.f;        // wavefront 0
  int plausible = 0, used = 0;     // the producing wavefronts: their own share
  for (int r = 0; r <= rq + rk; ++r) {
    if (wave > 0) {
      if (r < rq) {                // matches r * DV_CHUNK ...
        const int i = r * DV_CHUNK + p;
        bool pl;
        S.term_s[r & 1][p] = depth_verify_match_term(T, a, i < n ? corr + b + i : nullptr, pl);
        plausible += __popcll(__ballot(pl));
      } else if (r < rq + rk) {    // keypoints (r - rq) * DV_CHUNK ...
        const int j = (r - rq) * DV_CHUNK + p;
        bool use;
        S.term_s[r & 1][p] = depth_verify_point_term(T, a, j < nk ? a.xyz + 3 * (size_t)(kb + j) : nullptr, use);
        used += __popcll(__ballot(use));
      }
    } else if (r > 0) {            // the chain of round r - 1 (every lane of wavefront 0 the same: LDS broadcasts)
      const int q = r - 1;
      const double* const t = S.term_s[q & 1];
      if (q < rq) {
        const int cnt = min(DV_CHUNK, n - q * DV_CHUNK);
        for (int j = 0; j < cnt; ++j) QS = (float)((double)QS + t[j]);
      } else {
        const int cnt = min(DV_CHUNK, nk - (q - rq) * DV_CHUNK);
        for (int j = 0; j < cnt; ++j) IS = (float)((double)IS + t[j]);
      }
    }
    __syncthreads();
  }
  if ((tid & 63) == 0) {
    S.cnt_s[wave][0] = plausible;
    S.cnt_s[wave][1] = used;
  }
  __syncthreads();
  if (tid == 0) {
    int pl = 0, us = 0;
    for (int w = 1; w < DV_THREADS / 64; ++w) {
      pl += S.cnt_s[w][0];
      us += S.cnt_s[w][1];
    }
    depth_verify_close(a, rec, QS, IS, pl, us, nk);
  }
  __syncthreads();   // (cnt_s and the ring are the next object's)
}

// mh_depth_verify, form 0: workgroup x walks the objects x, x + gridDim.x, ...
__global__ __launch_bounds__(DV_THREADS) void depth_verify_kernel(DepthVerifyListArgs a) {
  __shared__ DepthVerifyLds S;
  for (int o = blockIdx.x; o < a.n_obj; o += gridDim.x)
    depth_verify_object(S, a.core, a.corr, a.model_off, a.obj_model[o], a.obj_pose + 7 * (size_t)o, a.rec + o);
}

// ... form 1: every wavefront one object at a time
__global__ __launch_bounds__(DV_THREADS) void depth_verify_wave_kernel(DepthVerifyListArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = (int)blockIdx.x * (DV_THREADS / 64) + wave; o < a.n_obj; o += (int)gridDim.x * (DV_THREADS / 64))
    depth_verify_object_wave(a.core, a.corr, a.model_off, a.obj_model[o], a.obj_pose + 7 * (size_t)o, a.rec + o, lane);
}

// Frames: workgroup (x, f) scores the objects x, x + gridDim.x, ... of result slot first_slot + f (form 0); the frame's
// last workgroup erases
__global__ __launch_bounds__(DV_THREADS) void depth_verify_frame_kernel(DepthVerifyFrameArgs a) {
  __shared__ DepthVerifyLds S;
  const int f = blockIdx.y, slot = a.first_slot + f;
  unsigned char* const result = a.result + (size_t)slot * a.result_bytes;
  int32_t* const head = reinterpret_cast<int32_t*>(a.block + (size_t)slot * a.slot_bytes);
  mh_verify_record* const rec = reinterpret_cast<mh_verify_record*>(head + 4);
  const int n = min(max(*reinterpret_cast<const int32_t*>(result), 0), a.max_objects);
  mh_object* const obj = reinterpret_cast<mh_object*>(result + 16);
  DepthVerifyArgs core = a.core;
  if (a.maps_on) {
    core.img = a.maps.img[f];
    core.fill = a.maps.fill[f];
  }
  const mh_corr* const corr = reinterpret_cast<const mh_corr*>(reinterpret_cast<const unsigned char*>(a.corr) + (size_t)f * a.arena_bytes);
  const int32_t* const model_off =
      reinterpret_cast<const int32_t*>(reinterpret_cast<const unsigned char*>(a.model_off) + (size_t)f * a.arena_bytes);
  for (int o = blockIdx.x; o < n; o += gridDim.x) depth_verify_object(S, core, corr, model_off, obj[o].model, obj[o].pose, rec + o);
  if (!last_workgroup(a.tickets + slot)) return;
  // :204-206 for the whole list by one thread: ascending, so a move never overwrites an unread object
  if (threadIdx.x == 0) {
    int k = 0;
    for (int o = 0; o < n; ++o) {
      if (!rec[o].keep) continue;
      if (k != o) obj[k] = obj[o];
      ++k;
    }
    head[0] = n;
    head[1] = k;
    head[2] = head[3] = 0;
    *reinterpret_cast<int32_t*>(result) = k;
  }
}

}  // namespace

void launch_frame_depth_verify(const DepthVerifyFrameArgs& a, int n_frames, hipStream_t s) {
  hipLaunchKernelGGL(depth_verify_frame_kernel, dim3(DV_FRAME_GRID, n_frames), dim3(DV_THREADS), 0, s, a);
}

void launch_depth_verify(const DepthVerifyListArgs& a, int form, hipStream_t s) {
  if (a.n_obj <= 0) return;
  if (form == 1) {
    const int want = (a.n_obj + DV_THREADS / 64 - 1) / (DV_THREADS / 64);
    hipLaunchKernelGGL(depth_verify_wave_kernel, dim3(want < DV_GRID ? want : DV_GRID), dim3(DV_THREADS), 0, s, a);
  } else {
    hipLaunchKernelGGL(depth_verify_kernel, dim3(a.n_obj < DV_GRID ? a.n_obj : DV_GRID), dim3(DV_THREADS), 0, s, a);
  }
}

}  // namespace mh
