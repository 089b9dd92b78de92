// DEPTH_VERIFY as device code (depth_verify.hip): see there for what the class computes.  One function per piece of the
// arithmetic -- a match's quotient, a keypoint's term, the closing lines -- so that the workgroup form (terms through
// LDS, one wavefront chains) and the wave form (no LDS, the chain by readlanes) cannot diverge.
#pragma once
#include "depth_verify.h"
#include "filter_depth_dev.h"

namespace mh {

namespace {

// One match of the quality score (:129-135), by the lane that owns it.  c: the match, or nullptr for a lane past the
// list's end.  `plausible`: projectionError < FeatureDistance (:132).  Returns what :135 adds to QS: 0. past the end
// (and for a point project() refuses: its error is infinite).
__device__ __forceinline__ double depth_verify_match_term(const TM& T, const DepthVerifyArgs& a, const mh_corr* c, bool& plausible) {
  plausible = false;
  if (!c) return 0.;
  const mh_corr m = *c;
  const float e = reproj_err2(T.r, T.t, a.cam, m.x, m.y, m.z, m.u, m.v);   // :129-131
  plausible = e < a.feature_distance;                                       // :132
  return 1.0 / (1.0 + (double)e);                                           // :135
}

// One keypoint of the incorrect score (:156-188), by the lane that owns it.  k: the store's row in model coordinates,
// or nullptr for a lane past the model's end.  `use`: the keypoint passed :168 (usedKeypointCount, :171).  Returns what
// :188 adds to IS -- 0. for a keypoint that is off the map, skipped, past the end, or occluded (:178).
__device__ __forceinline__ double depth_verify_point_term(const TM& T, const DepthVerifyArgs& a, const float* k, bool& use) {
  const float* const zmap = reinterpret_cast<const float*>(a.img);
  bool on = false;          // the keypoint falls on a pixel of the map
  int px = 0;
  float zp = 0.f;           // putativeDepth
  if (k) {
    float wx, wy, wz, cx, cy, cz;
    tm_apply(T.r, T.t, k[0], k[1], k[2], wx, wy, wz);                       // PoseTM.transform (:161)
    tm_apply_inv(a.dcam.Rc, a.dcam.tc, wx, wy, wz, cx, cy, cz);             // depthmap->TM.inverseTransform (:162)
    const float pu = __fadd_rn(__fmul_rn(__fdiv_rn(cx, cz), a.dcam.K[0]), a.dcam.K[2]);   // :164
    const float pv = __fadd_rn(__fmul_rn(__fdiv_rn(cy, cz), a.dcam.K[1]), a.dcam.K[3]);   // :165
    int ix = 0, iy = 0;
    on = pixel_of(pu, ix) && pixel_of(pv, iy) && ix >= 0 && ix < a.w && iy >= 0 && iy < a.h;   // (the reference reads outside)
    px = iy * a.w + ix;
    zp = cz;                                                                // :174
  }
  // both gathers of the step before either is used: their addresses are the lane's own arithmetic
  float dist = 0.f, zk = 0.f;
  if (on) {
    if (a.fill) dist = a.fill[px];          // distanceMap->getProb (:167)
    zk = zmap[4 * (size_t)px + 2];          // depthmap->getDepth (:173)
  }
  use = on && !(dist > a.max_distance);     // :168-171 (a NaN distance is used; no distance map: no test)
  double term = 0.;
  if (use && !(zk < zp)) {                  // :178: the sensor saw something in front: an occlusion, nothing added
    const float cauchy = __fmul_rn(a.depth_fraction, zk);    // :182
    float t = __fdiv_rn(__fsub_rn(zp, zk), cauchy);          // :184
    t = __fmul_rn(t, t);                                     // :185
    term = 1.0 - (1.0 / (1.0 + (double)t));                  // :188
  }
  return term;
}

// :191-204 (one lane): the multiplier and its cap, both quotients, the verdict
__device__ __forceinline__ void depth_verify_close(const DepthVerifyArgs& a, mh_verify_record* rec, float QS, float IS,
                                                   int plausible, int used, int keypoints) {
  mh_verify_record r;
  r.qs_raw = QS;
  r.is_raw = IS;
  float mult = __fdiv_rn((float)keypoints, (float)used);   // :191 (x/0 = inf, 0/0 = NaN)
  if (mult > a.max_multiplier) mult = a.max_multiplier;    // :194-196 (NaN passes)
  r.multiplier = mult;
  IS = __fmul_rn(IS, mult);                                // :197
  QS = __fdiv_rn(QS, (float)plausible);                    // :200
  IS = __fdiv_rn(IS, (float)keypoints);
  r.qs = QS;
  r.is = IS;
  r.plausible = plausible;
  r.used = used;
  r.keypoints = keypoints;
  r.keep = IS > QS ? 0 : 1;                                // :204
  *rec = r;
}

// DEPTH_VERIFY of ONE object by one wavefront, as filter_depth_score_wave scores one: no LDS, no workgroup barrier; both
// chains by filter_chain_wave.  pose: the seven words as mh_object holds them (all lanes).
__device__ __forceinline__ void depth_verify_object_wave(const DepthVerifyArgs& a, const mh_corr* corr, const int32_t* model_off,
                                                         int m, const float* pose, mh_verify_record* rec, int lane) {
  TM T;
  tm_from_pose(T, pose, pose + 4);
  // ---- the quality score (:123-137) ----
  const int b = model_off[m], n = model_off[m + 1] - b;
  float QS = 0.f;
  int plausible = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool pl;
    const double term = depth_verify_match_term(T, a, i < n ? corr + b + i : nullptr, pl);
    plausible += __popcll(__ballot(pl));
    QS = filter_chain_wave(QS, term, min(64, n - base));
  }
  // ---- the incorrect score over the model's rows (:152-189) ----
  const int kb = a.model_begin[m], nk = a.model_begin[m + 1] - kb;
  float IS = 0.f;
  int used = 0;
  for (int base = 0; base < nk; base += 64) {
    const int j = base + lane;
    bool use;
    const double term = depth_verify_point_term(T, a, j < nk ? a.xyz + 3 * (size_t)(kb + j) : nullptr, use);
    used += __popcll(__ballot(use));
    IS = filter_chain_wave(IS, term, min(64, nk - base));
  }
  if (lane == 0) depth_verify_close(a, rec, QS, IS, plausible, used, nk);
}

}  // namespace

}  // namespace mh
