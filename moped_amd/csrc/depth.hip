// moped3d's depth front end on the device, the parts that decide which
// features and matches reach CLUSTER:
//   DEPTHFILTER_CPU   (moped3d/libmoped/src/depthfilter/DEPTHFILTER_CPU.hpp:117-254): features
//                     (ToFilter = 1) or a model's matches (ToFilter = 2) survive only where their
//                     density per square metre of scene surface, taken over image patches and
//                     dilated 3x3, exceeds Density;
//   MATCH_ADAPTIVE_FLANN_CPU's ratio (moped3d/.../match/MATCH_ADAPTIVE_FLANN_CPU.hpp:193-215,
//                     361-376): the ratio-test threshold of a query depends on the depth under it
//                     and on the model of its nearest neighbour.
// Arithmetic follows the reference's expressions literally (float / double mix included); the
// build has -ffp-contract=off.  The per-match parts live in group_kernel (group.hip).
#include <algorithm>

#include "steps.h"

namespace mh {

namespace {

constexpr int DP_THREADS = 256;

// projectPoint (:38-43): Float x = (u - K[2]) / K[0]*depth
__device__ __forceinline__ void project_point(float u, float v, float depth, const float* K, float* o) {
  o[0] = __fmul_rn(__fdiv_rn(__fsub_rn(u, K[2]), K[0]), depth);
  o[1] = __fmul_rn(__fdiv_rn(__fsub_rn(v, K[3]), K[1]), depth);
  o[2] = depth;
}
// Pt<3>::euclDist (include/moped.hpp:125-126): d = pt[x] - this[x]; r += d*d; sqrt
__device__ __forceinline__ float eucl_dist(const float* a, const float* b) {
  float r = 0.f;
  for (int x = 0; x < 3; ++x) {
    const float d = __fsub_rn(b[x], a[x]);
    r = __fadd_rn(r, __fmul_rn(d, d));
  }
  return sqrtf(r);
}

// One workgroup per patch: minimum depth (:157-166, std::min semantics: NaN never wins), then
// the patch's area at that depth (getArea :50-61, with the reference's `y1 = min(.., width)`)
// and 1.0 / area as the double every feature of the patch adds to its density.
// blockIdx.y = frame of a batch: its own depth map (DepthMaps), its own patch map behind the frames' before it.
__global__ __launch_bounds__(DP_THREADS) void depth_patch_kernel(const float4* __restrict__ img, int w, int h,
                                                                 float k0, float k1, float k2, float k3, int patch,
                                                                 int pw, double* __restrict__ inv_size, DepthMaps maps) {
  __shared__ float red[DP_THREADS];
  if (blockIdx.y) {
    img = maps.img[blockIdx.y];
    inv_size += (size_t)blockIdx.y * gridDim.x;
  }
  const int p = blockIdx.x, px = p % pw, py = p / pw;
  const int x0 = px * patch, y0 = py * patch;
  const int x1 = min((px + 1) * patch, w), y1 = min((py + 1) * patch, h);
  float m = 1e10f;
  for (int i = threadIdx.x; i < (x1 - x0) * (y1 - y0); i += DP_THREADS) {
    const int x = x0 + i % (x1 - x0), y = y0 + i / (x1 - x0);
    const float d = img[(size_t)y * w + x].z;   // Image::getDepth (include/moped.hpp:279-284)
    m = d < m ? d : m;
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = DP_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      const float o = red[threadIdx.x + s];
      red[threadIdx.x] = o < red[threadIdx.x] ? o : red[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float K[4] = {k0, k1, k2, k3};
    const int y1ref = min((py + 1) * patch, w);   // :170, as written
    float c0[3], c1[3], c2[3];
    project_point((float)x0, (float)y0, red[0], K, c0);
    project_point((float)x0, (float)y1ref, red[0], K, c1);
    project_point((float)x1, (float)y0, red[0], K, c2);
    const float area = __fmul_rn(eucl_dist(c0, c2), eucl_dist(c0, c1));
    inv_size[p] = 1.0 / (double)area;   // `1.0 / sizeMap[..]` (:189)
  }
}

}  // namespace

namespace {

constexpr int DF_MAX_PATCHES = 4096;

// DEPTHFILTER with ToFilter = 1 (:181-211): keep[q] = 1 where the dilated density of the
// feature's patch exceeds `filter`.  Single workgroup per frame; q_count: the frames' keypoint counts on the device, one
// word per frame (rows past a frame's count are whatever the buffer held before: they count for nothing).
__global__ __launch_bounds__(1024) void feature_density_kernel(const float* __restrict__ q_uv, int Q,
                                                               const int32_t* __restrict__ q_count, int patch, int pw,
                                                               int ph, const double* __restrict__ inv_size,
                                                               float filter, uint8_t* __restrict__ keep) {
  __shared__ int cnt[DF_MAX_PATCHES];
  __shared__ float val[DF_MAX_PATCHES];
  const int P = pw * ph;
  if (blockIdx.y) {   // frame of a batch: keypoints and flags frame after frame, the patch maps too
    q_uv += 2 * (size_t)blockIdx.y * Q;
    keep += (size_t)blockIdx.y * Q;
    inv_size += (size_t)blockIdx.y * P;
  }
  if (q_count) Q = min(Q, q_count[blockIdx.y]);
  for (int p = threadIdx.x; p < P; p += blockDim.x) cnt[p] = 0;
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += blockDim.x) atomicAdd(&cnt[patch_of(q_uv[2 * q], q_uv[2 * q + 1], patch, pw, ph)], 1);
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x) val[p] = density_replay(cnt[p], inv_size[p]);
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += blockDim.x) {
    const int p = patch_of(q_uv[2 * q], q_uv[2 * q + 1], patch, pw, ph);
    keep[q] = dilated(val, p, pw, ph) > filter;
  }
}

// DEPTHFILTER as a step of its own (mh_depth_filter) on the step's own lists: group g = points [group_off[g],
// group_off[g + 1]) -- ONE group is ToFilter = 1 (:180-214, the detected features), one group per model ToFilter = 2
// (:215-251, every model's matches with a countMap of their own).  One workgroup per group.  The reference adds the
// double `1.0 / sizeMap[p]` to the Float countMap[p] once per point, in list order; every addition into one patch adds
// the same double, so the patch's value depends on how many points it has and not on where they stand in the list:
// LDS holds the count, density_replay redoes the additions -- the arithmetic of feature_density_kernel and of
// group_kernel's (a'), whose verdicts these are bit for bit.
__global__ __launch_bounds__(1024) void group_density_kernel(const float* __restrict__ uv,
                                                             const int32_t* __restrict__ group_off, int patch, int pw,
                                                             int ph, const double* __restrict__ inv_size, float filter,
                                                             uint8_t* __restrict__ keep) {
  __shared__ int cnt[DF_MAX_PATCHES];
  __shared__ float val[DF_MAX_PATCHES];
  const int P = pw * ph;
  const int a = group_off[blockIdx.x], b = group_off[blockIdx.x + 1];
  if (b <= a) return;   // (the whole workgroup: an empty model)
  for (int p = threadIdx.x; p < P; p += blockDim.x) cnt[p] = 0;
  __syncthreads();
  for (int i = a + threadIdx.x; i < b; i += blockDim.x) atomicAdd(&cnt[patch_of(uv[2 * i], uv[2 * i + 1], patch, pw, ph)], 1);
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x) val[p] = density_replay(cnt[p], inv_size[p]);
  __syncthreads();
  for (int i = a + threadIdx.x; i < b; i += blockDim.x)
    keep[i] = dilated(val, patch_of(uv[2 * i], uv[2 * i + 1], patch, pw, ph), pw, ph) > filter;
}

// DEPTHMAP_PROP as a step of its own (mh_depth_prop; DEPTHMAP_PROP_CPU.hpp:101-132): the pixel (int) u, (int) v of the
// map -- truncated, no interpolation, clamped to the map where the reference reads out of bounds -- gives coord3D, depth
// = its z and depthValid = (norm >= 0); fillDistance from the distance map, or -1 without one (:107-111).
__global__ __launch_bounds__(256) void depth_prop_kernel(const float4* __restrict__ img, const float* __restrict__ fill,
                                                         int w, int h, const float* __restrict__ uv, int n,
                                                         mh_depth_info* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int ix = (int)uv[2 * i], iy = (int)uv[2 * i + 1];
  ix = ix < 0 ? 0 : (ix >= w ? w - 1 : ix);
  iy = iy < 0 ? 0 : (iy >= h ? h - 1 : iy);
  const size_t px = (size_t)iy * w + ix;
  const float4 d = img[px];
  mh_depth_info o;
  o.depth_valid = d.w >= 0.f ? 1 : 0;
  o.coord3d[0] = d.x;
  o.coord3d[1] = d.y;
  o.coord3d[2] = d.z;
  o.depth = d.z;
  o.fill_distance = fill ? fill[px] : -1.f;
  out[i] = o;
}

}  // namespace

int depth_filter_max_patches() { return DF_MAX_PATCHES; }

void launch_group_density(const float* uv, const int32_t* group_off, int n_groups, int patch, int pw, int ph,
                          const double* inv_size, float filter, uint8_t* keep, hipStream_t s) {
  if (n_groups <= 0) return;
  hipLaunchKernelGGL(group_density_kernel, dim3(n_groups), dim3(1024), 0, s, uv, group_off, patch, pw, ph, inv_size, filter,
                     keep);
}

void launch_depth_prop(const DepthImage& dimg, const float* uv, int n, mh_depth_info* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(depth_prop_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dimg.img, dimg.fill, dimg.w, dimg.h, uv, n,
                     out);
}

void launch_depth_patches(const DepthImage& dimg, const float K[4], int patch, double* inv_size, hipStream_t s,
                          const DepthMaps* maps, int n_frames) {
  const int pw = (dimg.w + patch - 1) / patch, ph = (dimg.h + patch - 1) / patch;
  const bool batch = maps && n_frames > 1;
  hipLaunchKernelGGL(depth_patch_kernel, dim3(pw * ph, batch ? n_frames : 1), dim3(DP_THREADS), 0, s, dimg.img, dimg.w,
                     dimg.h, K[0], K[1], K[2], K[3], patch, pw, inv_size, batch ? *maps : DepthMaps());
}

void launch_feature_density(const float* q_uv, int Q, const int32_t* q_count, int patch, int pw, int ph,
                            const double* inv_size, float filter, uint8_t* keep, hipStream_t s, int n_frames) {
  if (Q <= 0) return;
  hipLaunchKernelGGL(feature_density_kernel, dim3(1, std::max(1, n_frames)), dim3(1024), 0, s, q_uv, Q, q_count, patch, pw,
                     ph, inv_size, filter, keep);
}

}  // namespace mh
