// Device code the kernels of the Kinect-view models share (view_rows.hip: the selection; view_merge.hip: the merge of
// re-seen points): a keypoint's verdict under rules 1 .. 7 of the block above mh_view_spec (moped_hip.h) with its model
// coordinates, and the bounding box's accumulator.  The verdict lives here and nowhere else.
#pragma once
#include "context.h"
#include "geom.h"
#include "steps.h"

namespace mh {

enum { VR_KEEP = 0, VR_PIXEL, VR_DEPTH, VR_FILL, VR_ROI, VR_BOX, VR_DUP, VR_LIMIT, VR_NONE };   // 1 .. 7 = the stats word

struct Box6 {
  float mn0, mn1, mn2, mx0, mx1, mx2;
  // Pt::min / Pt::max (moped.hpp): a NaN coordinate leaves the box as it is
  __device__ __forceinline__ void add(float x, float y, float z) {
    mn0 = x < mn0 ? x : mn0;
    mn1 = y < mn1 ? y : mn1;
    mn2 = z < mn2 ? z : mn2;
    mx0 = x > mx0 ? x : mx0;
    mx1 = y > mx1 ? y : mx1;
    mx2 = z > mx2 ? z : mx2;
  }
  // over the wavefront (the accumulators hold no NaN)
  __device__ __forceinline__ void wave_reduce() {
    for (int off = 32; off >= 1; off >>= 1) {
      mn0 = fminf(mn0, __shfl_xor(mn0, off));
      mn1 = fminf(mn1, __shfl_xor(mn1, off));
      mn2 = fminf(mn2, __shfl_xor(mn2, off));
      mx0 = fmaxf(mx0, __shfl_xor(mx0, off));
      mx1 = fmaxf(mx1, __shfl_xor(mx1, off));
      mx2 = fmaxf(mx2, __shfl_xor(mx2, off));
    }
  }
};
__device__ __forceinline__ Box6 box6_empty() {
  const float big = 10E10f;   // moped.cpp:107-108
  const Box6 b = {big, big, big, -big, -big, -big};
  return b;
}

// what one view's keypoints are judged with (uniform over the workgroup)
struct ViewJudge {
  const float2* xy;
  const float4* map;
  const float* fill;      // nullptr: no fill test
  const int32_t* m_idx;   // nullptr: no duplicate test
  const float* m_d1;
  const float* m_d2;
  TM T;
  float r0, r1, r2, r3, wf, hf, far2;
};

__device__ __forceinline__ void view_judge_init(ViewJudge& J, const ViewArgs& a, int view) {
  J.xy = reinterpret_cast<const float2*>(a.xy) + (size_t)view * a.cap;
  J.map = a.v[view].map;
  J.fill = a.spec.max_fill_distance >= 0.f ? a.v[view].fill : nullptr;
  J.m_idx = a.dup_on ? a.dup.idx_dev + (size_t)view * a.cap : nullptr;
  J.m_d1 = a.dup_on ? a.dup.d1_dev + (size_t)view * a.cap : nullptr;
  J.m_d2 = a.dup_on ? a.dup.d2_dev + (size_t)view * a.cap : nullptr;
  tm_from_pose(J.T, a.v[view].pose, a.v[view].pose + 4);
  J.r0 = a.spec.roi[0];
  J.r1 = a.spec.roi[1];
  J.r2 = a.spec.roi[2];
  J.r3 = a.spec.roi[3];
  J.wf = (float)a.w;
  J.hf = (float)a.h;
  J.far2 = __fmul_rn(a.spec.merge_dist, a.spec.merge_dist);
}

// keypoint i of the list: VR_KEEP or the rule that drops it; (x, y, z) = X_model where rule 5 was reached.  A VR_DUP
// verdict's row is J.m_idx[i].
__device__ __forceinline__ int view_verdict(const ViewArgs& a, const ViewJudge& J, int i, float& x, float& y, float& z) {
  const float2 p = J.xy[i];
  const float u = p.x, v = p.y;
  // 1: NaN fails the comparisons, +-inf the bounds
  if (!(u > -1.f && u < J.wf && v > -1.f && v < J.hf)) return VR_PIXEL;
  const size_t px = (size_t)(int)v * a.w + (int)u;   // (int): truncation, -0.5 -> 0 (DEPTHMAP_PROP_CPU.hpp:103)
  const float4 m = J.map[px];
  if (!(m.w >= 0.f)) return VR_DEPTH;                                                   // 2 (:131)
  if (J.fill && !(J.fill[px] <= a.spec.max_fill_distance)) return VR_FILL;              // 3 (DEPTH_VERIFY_CPU.hpp:167-170)
  if (!a.roi_all && !(u >= J.r0 && u < J.r2 && v >= J.r1 && v < J.r3)) return VR_ROI;   // 4
  tm_apply_inv(J.T.r, J.T.t, m.x, m.y, m.z, x, y, z);                                   // 5
  if (!a.box_all && !(x >= a.spec.box[0] && x <= a.spec.box[3] && y >= a.spec.box[1] && y <= a.spec.box[4] &&
                      z >= a.spec.box[2] && z <= a.spec.box[5]))
    return VR_BOX;                                                                      // 6
  if (J.m_idx) {                                                                        // 7
    const int32_t j = J.m_idx[i];
    if (match_accepted(j, J.m_d1[i], J.m_d2[i], a.spec.merge_ratio) && j < a.dup.n_db_rows && a.dup.model_of_dev[j] == a.dup.model) {
      const float* o = a.dup.xyz_dev + (size_t)j * 3;
      const float dx = __fsub_rn(x, o[0]), dy = __fsub_rn(y, o[1]), dz = __fsub_rn(z, o[2]);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      if (d2 <= J.far2) return VR_DUP;
    }
  }
  return VR_KEEP;
}

}  // namespace mh
