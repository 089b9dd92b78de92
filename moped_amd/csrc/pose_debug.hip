// Verification hooks of POSE's LM refine (mh_pose_debug_rows, mh_pose_debug_step): the shipped device functions of
// pose_lm_dev.h -- residual_rows, lm_cost, lm_accumulate / lm_reduce, solve6, rotate_left -- on one wavefront, with
// everything they compute written out.  No code of its own on the arithmetic's path: tests/pose_ref.py restates what
// these functions do and tests/test_gpu_pose_rows.py holds the device to it word for word.  In a translation unit of
// its own so that the kernels of pose.hip see no second caller of their functions (the inliner's choices, and with
// them the register budget of pose_kernel, stay what they were).
#include <cstring>
#include <vector>

#include "frame.h"
#include "pose_lm_dev.h"

MH_TRACE_TU()

using namespace mh;

namespace {

constexpr uint32_t POSE_DEBUG_FILL = MH_POSE_DEBUG_FILL;   // rows a residual model does not have, a step not taken
static_assert(POSE_MAX_PTS == MH_POSE_MAX_PTS, "the header's bound is the kernels'");

struct KeepAccum {   // lm_refine's observer: the normal equations of an iteration, as the iteration uses them
  Accum* out;
  __device__ __forceinline__ void operator()(const Accum& a) const { *out = a; }
};

// One wavefront.  Per list entry i (lane i % 64, as lm_cost / lm_accumulate walk the list): the rows and Jacobians of
// residual_rows<RES> through cam_of<KIND>; then lm_cost and the normal equations of the same list.
// sums: cost | H [21] | g [6].
template <int KIND, int RES>
__global__ __launch_bounds__(64) void pose_debug_rows_kernel(const float* __restrict__ pose, const DevCam* __restrict__ cams,
                                                             const float* __restrict__ pts, const int* __restrict__ list, int n,
                                                             float alpha, int phase, int32_t* __restrict__ nrows,
                                                             uint32_t* __restrict__ r_out, uint32_t* __restrict__ J_out,
                                                             float* __restrict__ sums) {
  constexpr int PS = PointStride<KIND>::value;
  const int lane = threadIdx.x;
  float R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = pose[i];
  for (int i = 0; i < 3; ++i) t[i] = pose[9 + i];
  for (int i = lane; i < n; i += 64) {
    float r[MAX_ROWS], J[MAX_ROWS][6];
    const float* p = pts + PS * list[i];
    const int nr = residual_rows<RES>(R, t, cam_of<KIND>(cams, p), p, alpha, phase, r, J, true);
    nrows[i] = nr;
    for (int a = 0; a < MAX_ROWS; ++a) {
      r_out[i * MAX_ROWS + a] = a < nr ? __float_as_uint(r[a]) : POSE_DEBUG_FILL;
      for (int k = 0; k < 6; ++k) J_out[(i * MAX_ROWS + a) * 6 + k] = a < nr ? __float_as_uint(J[a][k]) : POSE_DEBUG_FILL;
    }
  }
  const float cost = lm_cost<KIND, RES>(R, t, cams, pts, list, n, alpha, phase, lane);
  // H, g: lm_refine's own, seen through its observer in the first (here: only) iteration.  What the iteration then does
  // with them -- a solve, a step, a cost -- moves the local copy of the pose and is dropped.
  Accum acc;
  for (int i = 0; i < 21; ++i) acc.H[i] = __uint_as_float(POSE_DEBUG_FILL);
  for (int i = 0; i < 6; ++i) acc.g[i] = __uint_as_float(POSE_DEBUG_FILL);
  lm_refine<KIND, RES>(R, t, cams, pts, list, n, alpha, phase, 1, lane, KeepAccum{&acc});
  if (lane == 0) {
    sums[0] = cost;
    for (int i = 0; i < 21; ++i) sums[1 + i] = acc.H[i];
    for (int i = 0; i < 6; ++i) sums[22 + i] = acc.g[i];
  }
}

// One wavefront, every lane the same work: in = H [21] | g [6] | mu | R [9] | t [3]; out = dx [6] | Rn [9] | tn [3]
// (the fill word when solve6 refuses); flags = solve6's answer | 1 when all 64 lanes hold the same 19 words.
__global__ __launch_bounds__(64) void pose_debug_step_kernel(const float* __restrict__ in, uint32_t* __restrict__ out,
                                                             int32_t* __restrict__ flags) {
  float H[21], g[6], R[9], t[3], dx[6], Rn[9], tn[3];
  for (int i = 0; i < 21; ++i) H[i] = in[i];
  for (int i = 0; i < 6; ++i) g[i] = in[21 + i];
  const float mu = in[27];
  for (int i = 0; i < 9; ++i) R[i] = in[28 + i];
  for (int i = 0; i < 3; ++i) t[i] = in[37 + i];
  uint32_t w[19];
  const bool ok = solve6(H, g, mu, dx);
  if (ok) {
    rotate_left(dx, R, Rn);
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + dx[3 + i];
    for (int i = 0; i < 6; ++i) w[i] = __float_as_uint(dx[i]);
    for (int i = 0; i < 9; ++i) w[6 + i] = __float_as_uint(Rn[i]);
    for (int i = 0; i < 3; ++i) w[15 + i] = __float_as_uint(tn[i]);
  } else {
    for (int i = 0; i < 18; ++i) w[i] = POSE_DEBUG_FILL;
  }
  w[18] = ok;
  bool differs = false;
  for (int i = 0; i < 19; ++i) differs |= w[i] != (uint32_t)__builtin_amdgcn_readfirstlane((int)w[i]);
  const bool agree = __ballot(differs) == 0ull;
  if (threadIdx.x == 0) {
    for (int i = 0; i < 18; ++i) out[i] = w[i];
    flags[0] = ok;
    flags[1] = agree;
  }
}

template <int KIND, int RES>
void launch_rows(const float* pose, const DevCam* cams, const float* pts, const int* list, int n, float alpha, int phase,
                 int32_t* nrows, uint32_t* r, uint32_t* J, float* sums, hipStream_t s) {
  hipLaunchKernelGGL((pose_debug_rows_kernel<KIND, RES>), dim3(1), dim3(64), 0, s, pose, cams, pts, list, n, alpha, phase, nrows,
                     r, J, sums);
}

int refuse(mh_ctx* ctx, const char* who, const std::string& what) {
  ctx->err = std::string(who) + ": " + what;
  return MH_ERR_ARG;
}

constexpr size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int mh_pose_debug_rows(mh_ctx* ctx, int kind, int res, int phase, float alpha, const float R[9], const float t[3],
                       const mh_cam* cams, int n_images, const float* pts, int n_pts, const int32_t* list, int n,
                       int32_t* nrows, float* r, float* J, float* cost, float* H, float* g, float* devcams) {
  const char* const who = "mh_pose_debug_rows";
  if (!ctx) return MH_ERR_ARG;
  if (!R || !t || !cams || !pts || !list || !nrows || !r || !J || !cost || !H || !g || !devcams)
    return refuse(ctx, who, "a pointer is null");
  const bool pair = (kind == res && kind >= 0 && kind <= 3) || (res == 0 && (kind == 1 || kind == 2));
  if (!pair) return refuse(ctx, who, "(kind, res) must be one of (0,0) (1,1) (2,2) (3,3) (1,0) (2,0)");
  if (phase != 0 && phase != 1) return refuse(ctx, who, "phase must be 0 or 1");
  if (n_images < 1 || n_images > MH_MAX_IMAGES) return refuse(ctx, who, "n_images outside 1 .. MH_MAX_IMAGES");
  if (n_pts < 1 || n_pts > POSE_MAX_PTS) return refuse(ctx, who, "n_pts outside 1 .. 2048");
  if (n < 1 || n > POSE_MAX_PTS) return refuse(ctx, who, "n outside 1 .. 2048");
  for (int i = 0; i < n; ++i)
    if (list[i] < 0 || list[i] >= n_pts) return refuse(ctx, who, "list[" + std::to_string(i) + "] outside [0, n_pts)");
  const int ps = kind == 0 ? 5 : (kind == 3 ? 6 : 9);
  if (kind == 3)
    for (int i = 0; i < n_pts; ++i) {
      int32_t img;
      std::memcpy(&img, pts + (size_t)6 * i + 5, 4);
      if (img < 0 || img >= n_images) return refuse(ctx, who, "point " + std::to_string(i) + ": image word outside [0, n_images)");
    }
  if (int rc = mh::enter(ctx)) return rc;
  hipStream_t s = ctx->stream;
  const size_t un = (size_t)n;
  // one temporary block: pose [12] | cams | pts | list || nrows | r | J | sums [28]
  const size_t o_cam = pad16(12 * 4), o_pts = o_cam + pad16((size_t)n_images * sizeof(DevCam)),
               o_list = o_pts + pad16((size_t)n_pts * ps * 4), o_nr = o_list + pad16(un * 4), o_r = o_nr + pad16(un * 4),
               o_J = o_r + pad16(un * MAX_ROWS * 4), o_sum = o_J + pad16(un * MAX_ROWS * 6 * 4), bytes = o_sum + pad16(28 * 4);
  std::vector<unsigned char> h(o_nr);
  std::memcpy(h.data(), R, 36);
  std::memcpy(h.data() + 36, t, 12);
  std::vector<DevCam> dc(n_images);
  for (int i = 0; i < n_images; ++i) dc[i] = make_devcam(cams[i]);
  std::memcpy(h.data() + o_cam, dc.data(), (size_t)n_images * sizeof(DevCam));
  std::memcpy(h.data() + o_pts, pts, (size_t)n_pts * ps * 4);
  std::memcpy(h.data() + o_list, list, un * 4);
  DevBuf<unsigned char> buf;
  std::vector<unsigned char> down(bytes - o_nr);
  hipError_t e = buf.ensure(bytes, s);
  if (e == hipSuccess) e = hipMemcpyAsync(buf, h.data(), o_nr, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    unsigned char* const b = buf;
    const float* d_pose = reinterpret_cast<const float*>(b);
    const DevCam* d_cams = reinterpret_cast<const DevCam*>(b + o_cam);
    const float* d_pts = reinterpret_cast<const float*>(b + o_pts);
    const int* d_list = reinterpret_cast<const int*>(b + o_list);
    int32_t* d_nr = reinterpret_cast<int32_t*>(b + o_nr);
    uint32_t* d_r = reinterpret_cast<uint32_t*>(b + o_r);
    uint32_t* d_J = reinterpret_cast<uint32_t*>(b + o_J);
    float* d_sum = reinterpret_cast<float*>(b + o_sum);
#define MH_ROWS(K_, R_) launch_rows<K_, R_>(d_pose, d_cams, d_pts, d_list, n, alpha, phase, d_nr, d_r, d_J, d_sum, s)
    if (kind == 0) MH_ROWS(0, 0);
    else if (kind == 3) MH_ROWS(3, 3);
    else if (kind == 1 && res == 1) MH_ROWS(1, 1);
    else if (kind == 1) MH_ROWS(1, 0);
    else if (res == 2) MH_ROWS(2, 2);
    else MH_ROWS(2, 0);
#undef MH_ROWS
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(down.data(), buf + o_nr, bytes - o_nr, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);   // (before the block goes)
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    ctx->err = std::string(who) + ": " + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  const unsigned char* const d = down.data() - o_nr;
  std::memcpy(nrows, d + o_nr, un * 4);
  std::memcpy(r, d + o_r, un * MAX_ROWS * 4);
  std::memcpy(J, d + o_J, un * MAX_ROWS * 6 * 4);
  const float* sums = reinterpret_cast<const float*>(d + o_sum);
  *cost = sums[0];
  std::memcpy(H, sums + 1, 21 * 4);
  std::memcpy(g, sums + 22, 6 * 4);
  std::memcpy(devcams, dc.data(), (size_t)n_images * sizeof(DevCam));
  return MH_OK;
}

int mh_pose_debug_step(mh_ctx* ctx, const float H[21], const float g[6], float mu, const float R[9], const float t[3],
                       int32_t* solved, float dx[6], float Rn[9], float tn[3], int32_t* lanes_agree) {
  const char* const who = "mh_pose_debug_step";
  if (!ctx) return MH_ERR_ARG;
  if (!H || !g || !R || !t || !solved || !dx || !Rn || !tn || !lanes_agree) return refuse(ctx, who, "a pointer is null");
  if (int rc = mh::enter(ctx)) return rc;
  hipStream_t s = ctx->stream;
  float in[40];
  std::memcpy(in, H, 21 * 4);
  std::memcpy(in + 21, g, 6 * 4);
  in[27] = mu;
  std::memcpy(in + 28, R, 9 * 4);
  std::memcpy(in + 37, t, 3 * 4);
  uint32_t out[20] = {};   // dx | Rn | tn | solved, lanes_agree
  DevBuf<uint32_t> buf;    // in [40] | out [20]
  hipError_t e = buf.ensure(60, s);
  if (e == hipSuccess) e = hipMemcpyAsync(buf, in, sizeof in, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pose_debug_step_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const float*>(buf.p), buf.p + 40,
                       reinterpret_cast<int32_t*>(buf.p + 58));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, buf.p + 40, sizeof out, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    ctx->err = std::string(who) + ": " + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  std::memcpy(dx, out, 6 * 4);
  std::memcpy(Rn, out + 6, 9 * 4);
  std::memcpy(tn, out + 15, 3 * 4);
  *solved = (int32_t)out[18];
  *lanes_agree = (int32_t)out[19];
  return MH_OK;
}

}  // extern "C"
