// POSE's LM refine as device code shared by pose.hip (pose_refine) and pose_debug.hip (the verification hooks
// mh_pose_debug_rows / mh_pose_debug_step): residual rows and their Jacobians, the wave-wide sum, the cost, the 6 x 6
// solve, the pose update and lm_refine itself.  One definition each, so that what the hooks show is what ships.
// (Splitting lm_refine's accumulation into a function of its own changed the register allocation of every kernel that
// refines; an observer argument that is empty in the product does not: scripts/asm_kernel_diff.py.)
#pragma once
#include "steps.h"

namespace mh {

namespace {

// ---- LM refine, one wavefront ----------------------------------------------------
// 6-DoF local update (omega, dt): R <- exp(omega) R, t <- t + dt.
//
// KIND selects the residual model (what the reference class minimises):
//   0  POSE_RANSAC_LM_DIFF_REPROJECTION_CPU   (moped2 …REPROJECTION_CPU.hpp:100-138)
//   1  POSE_RANSAC_LM_DIFF_BACKPROJECTION_DEPTH_CPU (moped3d …BACKPROJECTION_DEPTH_CPU.hpp:108-190)
//   2  POSE_RANSAC_LM_DIFF_REPROJECTION_DEPTH_CPU   (moped3d …REPROJECTION_DEPTH_CPU.hpp:106-216)
// phase 0 minimises the plain (un-squared) errors for fast convergence, phase 1 the
// reference's squared errors so the result sits at the minimiser levmar converges to.
// A point is pts[PS*i ..] = u,v, x,y,z [, wx,wy,wz, cauchyWeight].
constexpr int MAX_ROWS = 4;
// KIND 3 = KIND 0's residuals with every correspondence in its own image (several cameras): a point carries
// its image number behind x,y,z and every projection goes through that image's camera (LmData::image,
// …REPROJECTION_CPU.hpp:213-237).
template <int KIND> struct PointStride { static constexpr int value = (KIND == 0) ? 5 : ((KIND == 3) ? 6 : 9); };
// the camera of a point: `cams` is ONE camera for KIND 0..2, the frame's camera table for KIND 3
template <int KIND>
__device__ __forceinline__ const DevCam& cam_of(const DevCam* cams, const float* p) {
  return KIND == 3 ? cams[__float_as_int(p[5])] : cams[0];
}

struct Accum {
  float H[21];  // upper triangle of J^T J
  float g[6];   // J^T r
};

// J row for a residual whose gradient w.r.t. the camera-frame point is gc:
// dc/dw = Rc^T, dw/d(dt) = I, dw/d(omega) = -[y]_x with y the rotated model point
// ->  translation part = Rc gc (world frame), rotation part = y x (Rc gc).
__device__ __forceinline__ void row_from_grad(const DevCam& cam, const float* y, const float* gc, float* J) {
  float gw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gw[k] = gc[0] * cam.Rc[k * 3 + 0] + gc[1] * cam.Rc[k * 3 + 1] + gc[2] * cam.Rc[k * 3 + 2];
  J[0] = y[1] * gw[2] - y[2] * gw[1];
  J[1] = y[2] * gw[0] - y[0] * gw[2];
  J[2] = y[0] * gw[1] - y[1] * gw[0];
  J[3] = gw[0];
  J[4] = gw[1];
  J[5] = gw[2];
}

// The third row of KIND 2 and its J: depthError = | p (p.W) - p | = |p| |p.W - 1| with p the camera-frame point
// (…REPROJECTION_DEPTH_CPU.hpp:176-186), x50, weight3D -- whatever the sign of the depth (:180-213 run for every point).
__device__ __forceinline__ void depth_row(const DevCam& cam, const float* y, const float* c, const float* p, float w3, int phase,
                                          float* r, float (*J)[6], bool want_j) {
  const float* W = p + 5;
  const float pw = c[0] * W[0] + c[1] * W[1] + c[2] * W[2] - 1.f;
  const float n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  const float nn = sqrtf(n2);
  float g[3];
  if (phase == 0) {
    const float s3 = sqrtf(50.f * w3);
    r[2] = s3 * nn * pw;
    if (want_j) {
      for (int k = 0; k < 3; ++k) g[k] = s3 * (c[k] / nn * pw + nn * W[k]);
      row_from_grad(cam, y, g, J[2]);
    }
  } else {
    r[2] = 50.f * w3 * n2 * pw * pw;
    if (want_j) {
      for (int k = 0; k < 3; ++k) g[k] = 50.f * w3 * (2.f * c[k] * pw * pw + n2 * 2.f * pw * W[k]);
      row_from_grad(cam, y, g, J[2]);
    }
  }
}

// Residual rows of one correspondence.  Returns the row count; r[], and J[][6] when want_j.
template <int KIND>
__device__ __forceinline__ int residual_rows(const float* R, const float* t, const DevCam& cam, const float* p,
                                             float alpha, int phase, float* r, float (*J)[6], bool want_j) {
  const float X = p[2], Y = p[3], Z = p[4];
  float y[3];  // rotated model point
  y[0] = R[0] * X + R[1] * Y + R[2] * Z;
  y[1] = R[3] * X + R[4] * Y + R[5] * Z;
  y[2] = R[6] * X + R[7] * Y + R[8] * Z;
  const float wx = y[0] + t[0] - cam.tc[0], wy = y[1] + t[1] - cam.tc[1], wz = y[2] + t[2] - cam.tc[2];
  float c[3];  // camera-frame point
  c[0] = wx * cam.Rc[0] + wy * cam.Rc[3] + wz * cam.Rc[6];
  c[1] = wx * cam.Rc[1] + wy * cam.Rc[4] + wz * cam.Rc[7];
  c[2] = wx * cam.Rc[2] + wy * cam.Rc[5] + wz * cam.Rc[8];
  constexpr int NR = (KIND == 0 || KIND == 3) ? 2 : ((KIND == 1) ? 4 : 3);      // rows in phase 0
  const int nrows = (phase == 0) ? NR : ((KIND == 2) ? 3 : 2);   // the reference's row count in phase 1
  float w3 = 0.f, w2 = 1.f;
  if (KIND == 1 || KIND == 2) {
    w3 = (1.f - alpha) * p[8];
    w2 = 1.f - w3;
  }
  if (c[2] < 0.f || !(fabsf(c[2]) > 1e-9f)) {  // behind the camera: the reference's penalty, no gradient
    // (within 1e-9 of the camera's plane as well, where the reference divides by zero: this project's departure)
    const float pen = -c[2] + 10.f;
    for (int a = 0; a < nrows; ++a) {
      float wgt = 1.f;
      if (KIND == 1) wgt = (a == nrows - 1) ? w3 : w2;
      if (KIND == 2) wgt = (a == 2) ? w3 : w2;
      r[a] = pen * ((phase == 0) ? sqrtf(wgt) : wgt);
      if (want_j)
        for (int k = 0; k < 6; ++k) J[a][k] = 0.f;
    }
    // KIND 2: the reference guards only the 2-D pair (…REPROJECTION_DEPTH_CPU.hpp:132-136); its depth row (:180-213) is
    // computed for every point and overwrites the penalty written there -- as here, with its Jacobian
    if (KIND == 2) depth_row(cam, y, c, p, w3, phase, r, J, want_j);
    return nrows;
  }
  if (KIND == 0 || KIND == 2 || KIND == 3) {
    const float iz = 1.f / c[2];
    const float du = c[0] * iz * cam.K[0] + cam.K[2] - p[0];
    const float dv = c[1] * iz * cam.K[1] + cam.K[3] - p[1];
    const float gu[3] = {cam.K[0] * iz, 0.f, -cam.K[0] * c[0] * iz * iz};
    const float gv[3] = {0.f, cam.K[1] * iz, -cam.K[1] * c[1] * iz * iz};
    const float s0 = (phase == 0) ? sqrtf(w2) : w2;
    float g[3];
    if (phase == 0) {
      r[0] = s0 * du;
      r[1] = s0 * dv;
    } else {
      r[0] = s0 * du * du;
      r[1] = s0 * dv * dv;
    }
    if (want_j) {
      const float fu = (phase == 0) ? s0 : 2.f * s0 * du, fv = (phase == 0) ? s0 : 2.f * s0 * dv;
      for (int k = 0; k < 3; ++k) g[k] = fu * gu[k];
      row_from_grad(cam, y, g, J[0]);
      for (int k = 0; k < 3; ++k) g[k] = fv * gv[k];
      row_from_grad(cam, y, g, J[1]);
    }
    if (KIND == 2) depth_row(cam, y, c, p, w3, phase, r, J, want_j);
    return nrows;
  }
  // KIND == 1: back-projection onto the ray through the depth-map point W
  {
    const float* W = p + 5;
    const float wn = sqrtf(W[0] * W[0] + W[1] * W[1] + W[2] * W[2]);
    const float n[3] = {W[0] / wn, W[1] / wn, W[2] / wn};
    const float sp = n[0] * c[0] + n[1] * c[1] + n[2] * c[2];
    const float e[3] = {c[0] - n[0] * sp, c[1] - n[1] * sp, c[2] - n[2] * sp};  // p - pHat
    const float ez = wn - sp;                                                     // along the ray
    float g[3];
    if (phase == 0) {
      const float s2 = sqrtf(w2), s3 = sqrtf(w3);
      for (int a = 0; a < 3; ++a) {
        r[a] = s2 * e[a];
        if (want_j) {
          for (int k = 0; k < 3; ++k) g[k] = s2 * ((a == k ? 1.f : 0.f) - n[a] * n[k]);
          row_from_grad(cam, y, g, J[a]);
        }
      }
      r[3] = s3 * ez;
      if (want_j) {
        for (int k = 0; k < 3; ++k) g[k] = -s3 * n[k];
        row_from_grad(cam, y, g, J[3]);
      }
    } else {
      r[0] = w2 * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);  // weight2D * dxy^2
      r[1] = w3 * ez * ez;                                    // weight3D * dz^2
      if (want_j) {
        for (int k = 0; k < 3; ++k) g[k] = 2.f * w2 * e[k];
        row_from_grad(cam, y, g, J[0]);
        for (int k = 0; k < 3; ++k) g[k] = -2.f * w3 * ez * n[k];
        row_from_grad(cam, y, g, J[1]);
      }
    }
    return nrows;
  }
}

// Wave-wide sum, the same value in every lane: four DPP steps inside the rows of 16 lanes
// (quad swaps, half-row mirror, row mirror), then the four row totals through scalar
// registers -- no LDS round trips (a __shfl_xor butterfly is six dependent ds_bpermutes).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror
  v = dpp_add<0x140>(v);   // row_mirror
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}

// Sum of squared residuals over the inlier list at pose (R,t); all 64 lanes return it.
// KIND = the points' layout (PointStride, the camera of a point); RES = the residual model (default: KIND's own; 0 on a depth
// layout = plain reprojection residuals of the same points, the 2-D polish before the depth refine)
template <int KIND, int RES = KIND>
__device__ float lm_cost(const float* R, const float* t, const DevCam* cams, const float* pts,
                         const int* list, int n, float alpha, int phase, int lane) {
  constexpr int PS = PointStride<KIND>::value;
  float c = 0.f;
  for (int i = lane; i < n; i += 64) {
    float r[MAX_ROWS];
    const float* p = pts + PS * list[i];
    const int nr = residual_rows<RES>(R, t, cam_of<KIND>(cams, p), p, alpha, phase, r, nullptr, false);
    for (int a = 0; a < nr; ++a) c += r[a] * r[a];
  }
  return wave_sum(c);
}

// exp(omega) R
__device__ void rotate_left(const float* w, const float* R, float* out) {
  const float th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const float th = sqrtf(th2);
  float a, b;  // exp = I + a [w]x + b [w]x^2
  if (th < 1e-4f) {
    a = 1.f - th2 / 6.f;
    b = 0.5f - th2 / 24.f;
  } else {
    a = sinf(th) / th;
    b = (1.f - cosf(th)) / th2;
  }
  const float K[9] = {0.f, -w[2], w[1], w[2], 0.f, -w[0], -w[1], w[0], 0.f};
  float K2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K2[r * 3 + c] = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
  float E[9];
  for (int i = 0; i < 9; ++i) E[i] = a * K[i] + b * K2[i];
  E[0] += 1.f;
  E[4] += 1.f;
  E[8] += 1.f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[r * 3 + c] = E[r * 3] * R[c] + E[r * 3 + 1] * R[3 + c] + E[r * 3 + 2] * R[6 + c];
}

// Solve (H + mu I) x = -g for symmetric positive H (6x6, upper triangle packed) by Cholesky.
__device__ bool solve6(const float* Hp, const float* g, float mu, float* x) {
  float A[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = Hp[k];
      A[j][i] = Hp[k];
      ++k;
    }
  for (int i = 0; i < 6; ++i) A[i][i] += mu;
  // L with the reciprocals of its diagonal kept beside it: one v_rsq per pivot, no divisions
  float Lm[6][6], inv[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      float s = A[i][j];
      for (int m = 0; m < j; ++m) s -= Lm[i][m] * Lm[j][m];
      if (i == j) {
        if (!(s > 0.f)) return false;
        inv[i] = __frsqrt_rn(s);
        Lm[i][i] = s * inv[i];
      } else {
        Lm[i][j] = s * inv[j];
      }
    }
  float y[6];
  for (int i = 0; i < 6; ++i) {
    float s = -g[i];
    for (int m = 0; m < i; ++m) s -= Lm[i][m] * y[m];
    y[i] = s * inv[i];
  }
  for (int i = 5; i >= 0; --i) {
    float s = y[i];
    for (int m = i + 1; m < 6; ++m) s -= Lm[m][i] * x[m];
    x[i] = s * inv[i];
  }
  return true;
}

#ifdef POSE_PROF   // phase timing build (make EXTRA=-DPOSE_PROF): cycles of thread 0 per phase, summed over tasks;
__device__ unsigned long long g_pose_prof[32];   // [6] = LM iterations (accepted or not) over all refines;
// inside an iteration: [8] Jacobian pass, [9] the 27 wave sums, [10] solve + pose update, [11] cost of the new pose,
// [12] attempts, [13] the cost before the first iteration; [16 + 4 * phase + e] = refines of that phase that ended by
// e = 0 iteration cap, 1 eight rejections, 2 converged (or nothing promised), 3 zero gradient; [24 + phase] iterations, [26 + phase] attempts
#define LP_T(k) do { if (lane == 0) { const unsigned long long now_ = clock64(); atomicAdd(&g_pose_prof[k], now_ - t_lm); t_lm = now_; } } while (0)
#define LP_N(k) do { if (lane == 0) atomicAdd(&g_pose_prof[k], 1ull); } while (0)
#else
#define LP_T(k) do { } while (0)
#define LP_N(k) do { } while (0)
#endif

// What lm_refine shows of every iteration: its normal equations (H scaled, both summed over the wavefront), as the
// iteration is about to use them.  The product's observer is empty; mh_pose_debug_rows' keeps a copy.
struct LmNoObserver {
  __device__ __forceinline__ void operator()(const Accum&) const {}
};
// Runs on one full wavefront; pose in/out is wave-uniform.
template <int KIND, int RES = KIND, class OBS = LmNoObserver>
__device__ float lm_refine(float* R, float* t, const DevCam* cams, const float* pts, const int* list,
                           int n, float alpha, int phase, int iters, int lane, OBS observe = OBS()) {
  constexpr int PS = PointStride<KIND>::value;
#ifdef POSE_PROF
  unsigned long long t_lm = clock64();
#endif
  float cost = lm_cost<KIND, RES>(R, t, cams, pts, list, n, alpha, phase, lane);
  LP_T(13);
  float mu = -1.f, nu = 2.f;
  // Phase 1's residuals are squares, r = d^2 (KIND 0 / 3: d = du, dv): the Hessian of sum r^2 = sum d^4 is
  // 12 d^2 grad d grad d^T, Gauss-Newton's 2 J^T J (J = 2 d grad d) is 8 d^2 grad d grad d^T -- two thirds of it, so every
  // Gauss-Newton step overshoots by half and the iteration converges linearly (error x -1/2 per step: 7.8 iterations
  // per refine measured, a third of them ending in eight rejected attempts).  With J^T J scaled by 3/2 the step is
  // Newton's for these residuals: same minimiser, quadratic convergence.  (The depth classes' phase-1 rows are sums of
  // squares of several terms; they keep Gauss-Newton.)
#ifndef LM_HS
#define LM_HS 1.5f
#endif
#ifndef LM_TOL0
#define LM_TOL0 1e-4f
#endif
#ifndef LM_TOL1
#define LM_TOL1 1e-5f
#endif
#ifndef LM_STOP
#define LM_STOP 1
#endif
#ifndef DRAW_MULHI
#define DRAW_MULHI 1
#endif
  const float hs = (phase == 1 && (RES == 0 || RES == 3)) ? LM_HS : 1.f;
  // Phase 0 only hands phase 1 a start: it stops at a relative gain of 1e-4 per step (1e-6 cost two more iterations per
  // refine and moved phase 1's end state by nothing); phase 1 at 1e-5, the resolution of its cost (below)
  // (the depth classes keep 1e-6 in both phases: their cost can hold a large constant, see the stop rule below)
  const float tol = (RES == 1 || RES == 2) ? 1e-6f : (phase == 0 ? LM_TOL0 : LM_TOL1);
  for (int it = 0; it < iters; ++it) {
#ifdef POSE_PROF
    if (lane == 0) atomicAdd(&g_pose_prof[6], 1ull);
    LP_N(24 + phase);
    t_lm = clock64();
#endif
    Accum acc;
    for (int i = 0; i < 21; ++i) acc.H[i] = 0.f;
    for (int i = 0; i < 6; ++i) acc.g[i] = 0.f;
    for (int i = lane; i < n; i += 64) {
      float r[MAX_ROWS], J[MAX_ROWS][6];
      const float* p = pts + PS * list[i];
      const int nr = residual_rows<RES>(R, t, cam_of<KIND>(cams, p), p, alpha, phase, r, J, true);
      for (int row = 0; row < nr; ++row) {
        int k = 0;
        for (int a = 0; a < 6; ++a) {
          for (int b = a; b < 6; ++b) acc.H[k++] += J[row][a] * J[row][b];
          acc.g[a] += J[row][a] * r[row];
        }
      }
    }
    LP_T(8);
    for (int i = 0; i < 21; ++i) acc.H[i] = hs * wave_sum(acc.H[i]);
    for (int i = 0; i < 6; ++i) acc.g[i] = wave_sum(acc.g[i]);
    LP_T(9);
    observe(acc);
    if (mu < 0.f) {  // tau * max diagonal (lm_core.c:672-676)
      float mx = 0.f;
      const int di[6] = {0, 6, 11, 15, 18, 20};
      for (int i = 0; i < 6; ++i) mx = fmaxf(mx, acc.H[di[i]]);
      mu = 1e-3f * mx;
    }
    float ginf = 0.f;
    for (int i = 0; i < 6; ++i) ginf = fmaxf(ginf, fabsf(acc.g[i]));
    if (!(ginf > 0.f)) { LP_N(16 + 4 * phase + 3); return cost; }
    bool accepted = false, converged = false;
    for (int attempt = 0; attempt < 8 && !accepted; ++attempt) {
      float dx[6];
#ifdef POSE_PROF
      if (lane == 0) atomicAdd(&g_pose_prof[12], 1ull);
      LP_N(26 + phase);
      t_lm = clock64();
#endif
      if (solve6(acc.H, acc.g, mu, dx)) {
        float Rn[9], tn[3];
        rotate_left(dx, R, Rn);
        for (int i = 0; i < 3; ++i) tn[i] = t[i] + dx[3 + i];
        LP_T(10);
        const float c2 = lm_cost<KIND, RES>(Rn, tn, cams, pts, list, n, alpha, phase, lane);
        LP_T(11);
        float dL = 0.f;
        for (int i = 0; i < 6; ++i) dL += dx[i] * (mu * dx[i] - acc.g[i]);
        const float dF = cost - c2;
        if (dF > 0.f && dL > 0.f) {
          for (int i = 0; i < 9; ++i) R[i] = Rn[i];
          for (int i = 0; i < 3; ++i) t[i] = tn[i];
          // nothing left at fp32 resolution: the next steps would only be rejected.  Only a step taken at the damping
          // the iteration started with says so: one that needed rejections first is short because mu grew, not
          // because the minimum is near (tests/tools/frame_stress.py: two objects in 600 frames stopped 1 degree short
          // of the optimum in a narrow valley, FILTER2 score 10-15% under the oracle's)
          converged = attempt == 0 && dF <= tol * cost;
          cost = c2;
          float tt = 2.f * dF / dL - 1.f;
          tt = 1.f - tt * tt * tt;
          mu *= fmaxf(tt, 1.f / 3.f);
          nu = 2.f;
          accepted = true;
          break;
        }
        // At the minimum, at fp32 resolution: the step of the damping this iteration started with was rejected, it is
        // itself below anything the 1 px bar could notice (2e-5 rad / 2e-5 m: 0.03 px at this geometry; at 2e-6, the pose's
        // own resolution, three refines in sixteen still burnt their eight attempts), and so is the UNDAMPED
        // Gauss-Newton step (one more 6 x 6 solve, once per refine).  Heavier damping only shortens the step: the seven
        // further attempts the loop used to make here -- a solve, a pose update and a pass over the points each, all
        // rejected -- were two thirds of a refine's time (POSE_PROF: 2.0 attempts per iteration, the last iteration of
        // most refines nothing but eight rejections).  The test is on the STEP, not on its promised gain relative to the
        // cost: a correspondence with a wrong depth attribute (or behind the camera) puts a constant into the depth
        // classes' cost that dwarfs everything the inliers can still gain, and a refine that stopped on "gain < 1e-6
        // of the cost" left frame 6 of the 50-model pool without one of its objects.
        auto tiny = [](const float* d) {
          float m = 0.f;
          for (int i = 0; i < 6; ++i) m = fmaxf(m, fabsf(d[i]));
          return m < 2e-5f;
        };
        if (LM_STOP && attempt == 0 && tiny(dx)) {
          float dx0[6], mxd = 0.f;
          const int di[6] = {0, 6, 11, 15, 18, 20};
          for (int i = 0; i < 6; ++i) mxd = fmaxf(mxd, acc.H[di[i]]);
          if (solve6(acc.H, acc.g, 1e-7f * mxd, dx0) && tiny(dx0)) {
            converged = true;
            break;
          }
        }
      }
      mu *= nu;
      nu *= 2.f;
    }
    if (converged) { LP_N(16 + 4 * phase + 2); return cost; }
    if (!accepted) { LP_N(16 + 4 * phase + 1); return cost; }
  }
  LP_N(16 + 4 * phase + 0);
  return cost;
}

}  // namespace

}  // namespace mh
