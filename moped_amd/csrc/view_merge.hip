// 3-D models from Kinect views: the keypoints of a further view that the model already holds (rule 7 of mh_view_spec, the
// duplicates mh_db_append_view drops) are folded into the rows they re-observe.  The arithmetic is the block above
// mh_view_merge_dev in moped_hip.h: per touched row the plain mean of its observations in list order, then
// old * (float)views + mean, every operation one float32 rounding (__fadd_rn / __fmul_rn / __fdiv_rn, as geom.h), no
// floating-point atomics: a row's sum is one wavefront's, taken in list order, so neither the grid nor the order in
// which workgroups run can change a bit.
//
// Two launches.  (1) view_merge_mark_kernel, one workgroup of 1024 threads like the selection's: every keypoint's verdict
// by the selection's own device code (view_rows_dev.h); a duplicate notes its row and its X_model and marks the row
// (integer atomicOr); then a stable compaction of the marks, ballot + popcount + the 16 wavefront counts through LDS, so
// that merged rows come out in ascending row order; the view counts.  (2) view_merge_fold_kernel, one wavefront per
// merged row: the list in chunks of 64, __ballot's 64-bit mask of "observes my row", the set bits taken lowest first,
// each lane holding 2 of the 128 components.
#include "context.h"
#include "view_check.h"
#include "view_rows_dev.h"

using namespace mh;

namespace {

constexpr int VM_THREADS = 1024;
constexpr int VM_WAVES = VM_THREADS / 64;
constexpr int VM_FOLD_WAVES = 4;

__global__ __launch_bounds__(VM_THREADS) void view_merge_mark_kernel(const MergeArgs m) {
  __shared__ int wcnt[VM_WAVES];
  const ViewArgs& a = m.v;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  ViewJudge J;
  view_judge_init(J, a, 0);
  const int n = min(max(a.n[0], 0), a.cap);
  const int rows = a.dup.row_end - a.dup.row_begin;
  // the verdicts (m.touched is zero when the kernel starts)
  for (int i = t; i < n; i += VM_THREADS) {
    float x = 0.f, y = 0.f, z = 0.f;
    int r = -1;
    if (view_verdict(a, J, i, x, y, z) == VR_DUP) {
      r = J.m_idx[i] - a.dup.row_begin;
      if (r < 0 || r >= rows) r = -1;   // (a store whose model_of disagrees with [row_begin, row_end): no row of ours)
    }
    m.obs_row[i] = r;
    if (r >= 0) {
      m.obs_xyz[(size_t)i * 3] = x;
      m.obs_xyz[(size_t)i * 3 + 1] = y;
      m.obs_xyz[(size_t)i * 3 + 2] = z;
      atomicOr(&m.touched[r], 1);
    }
  }
  __syncthreads();
  // the marks, compacted in row order; the counts
  int base = 0;   // merged rows so far (uniform)
  for (int c0 = 0; c0 < rows; c0 += VM_THREADS) {
    const int r = c0 + t;
    const bool hit = r < rows && __hip_atomic_load(&m.touched[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < VM_WAVES; ++w) {
      const int c = wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int at = base + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (hit && at < m.merged_cap) m.merged_idx[at] = r;
    if (r < rows) m.views_out[r] = (m.views_in ? m.views_in[r] : 1) + (hit ? 1 : 0);
    base += total;
    __syncthreads();   // wcnt is the next chunk's
  }
  if (t == 0) *m.n_merged = base;
}

__global__ __launch_bounds__(VM_FOLD_WAVES * 64) void view_merge_fold_kernel(const MergeArgs m) {
  const ViewArgs& a = m.v;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * VM_FOLD_WAVES + (threadIdx.x >> 6);   // (uniform over the wavefront)
  if (k >= min(*m.n_merged, m.merged_cap)) return;
  const int r = m.merged_idx[k];
  const int n = min(max(a.n[0], 0), a.cap);
  const float2* qn = reinterpret_cast<const float2*>(m.qn);
  float2 acc = make_float2(0.f, 0.f);
  float bx = 0.f, by = 0.f, bz = 0.f;
  int cnt = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int i = c0 + lane;
    unsigned long long mask = __ballot(i < n && m.obs_row[i] == r);
    while (mask) {   // list order: the lowest set bit first
      const int o = c0 + __ffsll((long long)mask) - 1;
      mask &= mask - 1ull;
      const float2 q = qn[(size_t)o * (DIM / 2) + lane];
      const float x = m.obs_xyz[(size_t)o * 3], y = m.obs_xyz[(size_t)o * 3 + 1], z = m.obs_xyz[(size_t)o * 3 + 2];
      if (cnt == 0) {
        acc = q;
        bx = x;
        by = y;
        bz = z;
      } else {
        acc.x = __fadd_rn(acc.x, q.x);
        acc.y = __fadd_rn(acc.y, q.y);
        bx = __fadd_rn(bx, x);
        by = __fadd_rn(by, y);
        bz = __fadd_rn(bz, z);
      }
      ++cnt;
    }
  }
  if (cnt > 1) {
    const float kf = (float)cnt;
    acc.x = __fdiv_rn(acc.x, kf);
    acc.y = __fdiv_rn(acc.y, kf);
    bx = __fdiv_rn(bx, kf);
    by = __fdiv_rn(by, kf);
    bz = __fdiv_rn(bz, kf);
  }
  const int c = m.views_in ? m.views_in[r] : 1;
  const float cf = (float)c, c1 = (float)(c + 1);
  const size_t row = (size_t)a.dup.row_begin + r;
  const float2 d = reinterpret_cast<const float2*>(m.old_desc)[row * (DIM / 2) + lane];
  float2 s;
  s.x = __fadd_rn(__fmul_rn(d.x, cf), acc.x);
  s.y = __fadd_rn(__fmul_rn(d.y, cf), acc.y);
  reinterpret_cast<float2*>(m.merged_desc)[(size_t)k * (DIM / 2) + lane] = s;
  if (m.merged_desc_copy) reinterpret_cast<float2*>(m.merged_desc_copy)[(size_t)k * (DIM / 2) + lane] = s;
  if (lane < 3) {
    const float b = lane == 0 ? bx : lane == 1 ? by : bz;
    m.merged_xyz[(size_t)k * 3 + lane] = __fdiv_rn(__fadd_rn(__fmul_rn(a.dup.xyz_dev[row * 3 + lane], cf), b), c1);
  }
}

// the edit's staging block: merged row k (normalised, with its norm term and point) over staged row idx[k]
__global__ __launch_bounds__(256) void view_merge_scatter_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ n_merged,
                                                                 int cap, const float* __restrict__ desc,
                                                                 const float* __restrict__ norm, const float* __restrict__ xyz,
                                                                 float* __restrict__ stage_desc, float* __restrict__ stage_norm,
                                                                 float* __restrict__ stage_xyz) {
  const int k = blockIdx.x * 8 + (threadIdx.x >> 5), c = threadIdx.x & 31;
  if (k >= min(*n_merged, cap)) return;
  const size_t r = (size_t)idx[k];
  reinterpret_cast<float4*>(stage_desc + r * DIM)[c] = reinterpret_cast<const float4*>(desc + (size_t)k * DIM)[c];
  if (c == 0) stage_norm[r] = norm[k];
  if (c < 3) stage_xyz[r * 3 + c] = xyz[(size_t)k * 3 + c];
}

// Model::boundingBox over xyz[0, n_fixed + *n_more) with the selection's `<` / `>` rule
__global__ __launch_bounds__(VM_THREADS) void view_box_kernel(const float* __restrict__ xyz, int n_fixed, const int32_t* __restrict__ n_more,
                                                              float* __restrict__ bbox) {
  __shared__ float red[VM_WAVES][6];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = n_fixed + (n_more ? max(*n_more, 0) : 0);
  Box6 bb = box6_empty();
  for (int r = t; r < n; r += VM_THREADS) bb.add(xyz[(size_t)r * 3], xyz[(size_t)r * 3 + 1], xyz[(size_t)r * 3 + 2]);
  bb.wave_reduce();
  if (lane == 0) {
    red[wave][0] = bb.mn0;
    red[wave][1] = bb.mn1;
    red[wave][2] = bb.mn2;
    red[wave][3] = bb.mx0;
    red[wave][4] = bb.mx1;
    red[wave][5] = bb.mx2;
  }
  __syncthreads();
  if (t < 6) {
    float v = red[0][t];
    for (int w = 1; w < VM_WAVES; ++w) v = t < 3 ? fminf(v, red[w][t]) : fmaxf(v, red[w][t]);
    bbox[t] = v;
  }
}

// mh_db_keep_rows: rows [b, b + rows) of the store whose flag is set, packed in order into the staging block with their
// norm terms and points (one workgroup; the compaction of the kernels above)
__global__ __launch_bounds__(VM_THREADS) void view_keep_kernel(const uint8_t* __restrict__ keep, int b, int rows,
                                                               const float* __restrict__ desc, const float* __restrict__ norm,
                                                               const float* __restrict__ xyz, float* __restrict__ stage_desc,
                                                               float* __restrict__ stage_norm, float* __restrict__ stage_xyz,
                                                               float* __restrict__ bbox) {
  __shared__ int wcnt[VM_WAVES];
  __shared__ int src_s[VM_THREADS];
  __shared__ float red[VM_WAVES][6];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  Box6 bb = box6_empty();
  int base = 0;
  for (int c0 = 0; c0 < rows; c0 += VM_THREADS) {
    const int r = c0 + t;
    const bool hit = r < rows && keep[r] != 0;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < VM_WAVES; ++w) {
      const int c = wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int at = before + __popcll(bal & ((1ull << lane) - 1ull));
    if (hit) {
      const float* x = xyz + (size_t)(b + r) * 3;
      float* o = stage_xyz + (size_t)(base + at) * 3;
      o[0] = x[0];
      o[1] = x[1];
      o[2] = x[2];
      bb.add(x[0], x[1], x[2]);
      stage_norm[base + at] = norm[b + r];
      src_s[at] = b + r;
    }
    __syncthreads();
    for (int k = t; k < total * (DIM / 4); k += VM_THREADS) {
      const int row = k >> 5, c = k & 31;
      reinterpret_cast<float4*>(stage_desc + (size_t)(base + row) * DIM)[c] =
          reinterpret_cast<const float4*>(desc + (size_t)src_s[row] * DIM)[c];
    }
    base += total;
    __syncthreads();   // wcnt and src_s are the next chunk's
  }
  bb.wave_reduce();
  if (lane == 0) {
    red[wave][0] = bb.mn0;
    red[wave][1] = bb.mn1;
    red[wave][2] = bb.mn2;
    red[wave][3] = bb.mx0;
    red[wave][4] = bb.mx1;
    red[wave][5] = bb.mx2;
  }
  __syncthreads();
  if (t < 6) {
    float v = red[0][t];
    for (int w = 1; w < VM_WAVES; ++w) v = t < 3 ? fminf(v, red[w][t]) : fmaxf(v, red[w][t]);
    bbox[t] = v;
  }
}

}  // namespace

namespace mh {

int launch_view_merge(mh_ctx* ctx, const MergeArgs& m) {
  const int rows = m.v.dup.row_end - m.v.dup.row_begin;
  hipStream_t s = ctx->stream;
  if (rows > 0) MH_HIP(ctx, hipMemsetAsync(m.touched, 0, (size_t)rows * sizeof(int32_t), s));
  hipLaunchKernelGGL(view_merge_mark_kernel, dim3(1), dim3(VM_THREADS), 0, s, m);
  const int most = std::min(std::min(rows, m.v.cap), m.merged_cap);   // a row has an observation of its own
  if (most > 0)
    hipLaunchKernelGGL(view_merge_fold_kernel, dim3((most + VM_FOLD_WAVES - 1) / VM_FOLD_WAVES), dim3(VM_FOLD_WAVES * 64), 0, s, m);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

void launch_view_merge_scatter(const int32_t* idx, const int32_t* n_merged, int cap, const float* desc, const float* norm,
                               const float* xyz, float* stage_desc, float* stage_norm, float* stage_xyz, hipStream_t s) {
  if (cap <= 0) return;
  hipLaunchKernelGGL(view_merge_scatter_kernel, dim3((cap + 7) / 8), dim3(256), 0, s, idx, n_merged, cap, desc, norm, xyz,
                     stage_desc, stage_norm, stage_xyz);
}

void launch_view_box(const float* xyz, int n_fixed, const int32_t* n_more, float* bbox, hipStream_t s) {
  hipLaunchKernelGGL(view_box_kernel, dim3(1), dim3(VM_THREADS), 0, s, xyz, n_fixed, n_more, bbox);
}

void launch_view_keep(const uint8_t* keep, int b, int rows, const float* desc, const float* norm, const float* xyz,
                      float* stage_desc, float* stage_norm, float* stage_xyz, float* bbox, hipStream_t s) {
  hipLaunchKernelGGL(view_keep_kernel, dim3(1), dim3(VM_THREADS), 0, s, keep, b, rows, desc, norm, xyz, stage_desc, stage_norm,
                     stage_xyz, bbox);
}

int ensure_view_merge(mh_ctx* ctx, int cap, int rows) {
  mh_ctx::Planar& p = ctx->planar;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, p.mg_obs_row.ensure((size_t)cap, s));
  MH_HIP(ctx, p.mg_obs_xyz.ensure((size_t)cap * 3, s));
  MH_HIP(ctx, p.mg_touched.ensure((size_t)std::max(rows, 1), s));
  return MH_OK;
}

}  // namespace mh

extern "C" int mh_view_merge_dev(mh_ctx* ctx, const float* desc_dev, const float* qn_desc_dev, const float* xy_dev,
                                 const int32_t* n_dev, int cap, const mh_view* view, int width, int height,
                                 const mh_view_spec* spec, const mh_view_dup* dup, const float* old_desc_dev,
                                 const int32_t* views_in_dev, int32_t* merged_idx_dev, float* merged_desc_dev,
                                 float* merged_xyz_dev, int merged_cap, int32_t* n_merged_dev, int32_t* views_out_dev) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_view_merge_dev";
  if (const char* why = view_merge_why(desc_dev, qn_desc_dev, xy_dev, n_dev, cap, dup, old_desc_dev, views_in_dev, merged_idx_dev,
                                       merged_desc_dev, merged_xyz_dev, merged_cap, n_merged_dev, views_out_dev)) {
    ctx->err = std::string(who) + ": " + why;
    return MH_ERR_ARG;
  }
  MergeArgs m = {};
  if (int rc = view_args_check(ctx, who, view, 1, width, height, spec, &m.v)) return rc;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  if (int rc = ensure_view_merge(ctx, cap, dup->row_end - dup->row_begin)) return rc;
  m.v.desc = desc_dev;
  m.v.xy = xy_dev;
  m.v.n = n_dev;
  m.v.cap = cap;
  m.v.dup = *dup;
  m.v.dup_on = spec->merge_ratio > 0.f && spec->merge_dist >= 0.f;
  m.qn = qn_desc_dev;
  m.old_desc = old_desc_dev;
  m.views_in = views_in_dev;
  m.obs_row = ctx->planar.mg_obs_row;
  m.obs_xyz = ctx->planar.mg_obs_xyz;
  m.touched = ctx->planar.mg_touched;
  m.merged_idx = merged_idx_dev;
  m.merged_desc = merged_desc_dev;
  m.merged_desc_copy = nullptr;
  m.merged_xyz = merged_xyz_dev;
  m.merged_cap = merged_cap;
  m.n_merged = n_merged_dev;
  m.views_out = views_out_dev;
  return launch_view_merge(ctx, m);
}
