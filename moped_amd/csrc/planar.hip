// Planar models from FEAT's lists: the back half of Moped::createPlanarModelsFromImages (moped2/libmoped/src/moped.cpp:
// 196-236).  The reference turns every detected feature of an image into a model point at (u scale, v scale, 0) and
// keeps detectedFeatures order (:220-232).  Here ONE launch takes FEAT's output as it lies on the device -- desc [cap][128],
// xy [cap][2], the count in a device word -- selects the keypoints inside a region of interest, writes them densely
// packed in list order (a stable compaction: mh_db_splice's byte-equality with an upload depends on row order) with
// their model coordinates, and reduces Model::boundingBox (moped.cpp:107-125) over what it wrote.
//
// One workgroup of 1024 threads per image; the list is walked in chunks of 1024 keypoints: ballot + popcount inside a
// wavefront, the 16 wavefront counts through LDS, the chunk's base carried from chunk to chunk.  The descriptors of a
// chunk's kept rows are then copied by all threads, 32 float4 per row.  Coordinates: one rounding per operation, in the
// order written (the build has -ffp-contract=off; `/` is the correctly rounded division), so both forms equal numpy's
// float32 expression bit for bit.
#include <cmath>

#include "context.h"

using namespace mh;

namespace {

constexpr int PL_THREADS = 1024;
constexpr int PL_WAVES = PL_THREADS / 64;

__global__ __launch_bounds__(PL_THREADS) void planar_rows_kernel(const PlanarArgs a) {
  __shared__ int wcnt[PL_WAVES];
  __shared__ int src_s[PL_THREADS];
  __shared__ float red[PL_WAVES][6];
  const int img = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* desc = a.desc + (size_t)img * a.cap * DIM;
  const float2* xy = reinterpret_cast<const float2*>(a.xy) + (size_t)img * a.cap;
  float* desc_out = a.desc_out + (size_t)img * a.out_pitch * DIM;
  float* desc_copy = a.desc_copy ? a.desc_copy + (size_t)img * a.out_pitch * DIM : nullptr;
  float* xyz_out = a.xyz_out + (size_t)img * a.out_pitch * 3;
  const int n = min(max(a.n[img], 0), a.cap);
  const int limit = a.spec.max_rows > 0 ? min(a.out_cap, a.spec.max_rows) : a.out_cap;
  const float r0 = a.spec.roi[0], r1 = a.spec.roi[1], r2 = a.spec.roi[2], r3 = a.spec.roi[3];
  const float big = 10E10f;   // moped.cpp:107-108
  float mn0 = big, mn1 = big, mn2 = big, mx0 = -big, mx1 = -big, mx2 = -big;
  int base = 0;   // rows written so far (uniform)
  for (int c0 = 0; c0 < n && base < limit; c0 += PL_THREADS) {
    const int i = c0 + t;
    bool keep = false;
    float u = 0.f, v = 0.f;
    if (i < n) {
      const float2 p = xy[i];
      u = p.x;
      v = p.y;
      keep = a.all || (u >= r0 && u < r2 && v >= r1 && v < r3);   // half-open; a NaN fails every comparison
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PL_WAVES; ++w) {
      const int c = wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int at = before + __popcll(bal & ((1ull << lane) - 1ull));   // place among the chunk's kept rows
    if (keep && base + at < limit) {
      float x, y, z;
      if (a.spec.form == 0) {   // moped.cpp:225
        x = u * a.spec.scale;
        y = v * a.spec.scale;
        z = 0.f;
      } else {   // the plane z = const in front of a camera with K = (fx, fy, cx, cy)
        z = a.spec.z;
        x = (u - a.spec.K[2]) / a.spec.K[0];
        x = x * z;
        y = (v - a.spec.K[3]) / a.spec.K[1];
        y = y * z;
      }
      float* o = xyz_out + (size_t)(base + at) * 3;
      o[0] = x;
      o[1] = y;
      o[2] = z;
      // Pt::min / Pt::max (moped.hpp): a NaN coordinate leaves the box as it is
      mn0 = x < mn0 ? x : mn0;
      mn1 = y < mn1 ? y : mn1;
      mn2 = z < mn2 ? z : mn2;
      mx0 = x > mx0 ? x : mx0;
      mx1 = y > mx1 ? y : mx1;
      mx2 = z > mx2 ? z : mx2;
      src_s[at] = i;
    }
    __syncthreads();
    const int rows = min(total, limit - base);
    for (int k = t; k < rows * (DIM / 4); k += PL_THREADS) {
      const int r = k >> 5, c = k & 31;
      const float4 d = reinterpret_cast<const float4*>(desc + (size_t)src_s[r] * DIM)[c];
      reinterpret_cast<float4*>(desc_out + (size_t)(base + r) * DIM)[c] = d;
      if (desc_copy) reinterpret_cast<float4*>(desc_copy + (size_t)(base + r) * DIM)[c] = d;
    }
    base += rows;
    __syncthreads();   // wcnt and src_s are the next chunk's
  }
  // the box: wavefront, then workgroup (the accumulators hold no NaN)
  for (int off = 32; off >= 1; off >>= 1) {
    mn0 = fminf(mn0, __shfl_xor(mn0, off));
    mn1 = fminf(mn1, __shfl_xor(mn1, off));
    mn2 = fminf(mn2, __shfl_xor(mn2, off));
    mx0 = fmaxf(mx0, __shfl_xor(mx0, off));
    mx1 = fmaxf(mx1, __shfl_xor(mx1, off));
    mx2 = fmaxf(mx2, __shfl_xor(mx2, off));
  }
  if (lane == 0) {
    red[wave][0] = mn0;
    red[wave][1] = mn1;
    red[wave][2] = mn2;
    red[wave][3] = mx0;
    red[wave][4] = mx1;
    red[wave][5] = mx2;
  }
  __syncthreads();
  if (t < 6) {
    float m = red[0][t];
    for (int w = 1; w < PL_WAVES; ++w) m = t < 3 ? fminf(m, red[w][t]) : fmaxf(m, red[w][t]);
    a.bbox[(size_t)img * 6 + t] = m;
  }
  if (t == 0) a.n_out[img] = base;
}

bool finite4(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3]); }

}  // namespace

namespace mh {

void launch_planar_rows(const PlanarArgs& a, int n_images, hipStream_t s) {
  if (n_images <= 0) return;
  hipLaunchKernelGGL(planar_rows_kernel, dim3(n_images), dim3(PL_THREADS), 0, s, a);
}

int planar_spec_check(mh_ctx* ctx, const char* who, const mh_planar_spec* spec, int* all) {
  const char* why = nullptr;
  if (!spec) why = "no mh_planar_spec";
  else if (spec->form != 0 && spec->form != 1) why = "form is 0 (u scale, v scale, 0) or 1 (a plane at z in front of K)";
  else if (!std::isfinite(spec->scale) || !std::isfinite(spec->z) || !finite4(spec->K)) why = "non-finite scale, z or K";
  else if (spec->form == 1 && (spec->K[0] == 0.f || spec->K[1] == 0.f)) why = "fx or fy is 0";
  else if (std::isnan(spec->roi[0]) || std::isnan(spec->roi[1]) || std::isnan(spec->roi[2]) || std::isnan(spec->roi[3]))
    why = "NaN in roi";
  else if (spec->max_rows < 0) why = "max_rows < 0";
  if (why) {
    ctx->err = std::string(who) + ": " + why;
    return MH_ERR_ARG;
  }
  *all = spec->roi[0] == 0.f && spec->roi[1] == 0.f && spec->roi[2] == 0.f && spec->roi[3] == 0.f;
  return MH_OK;
}

}  // namespace mh

// both entry points below; `who` names the one called in the error text
static int planar_rows_call(mh_ctx* ctx, const char* who, const float* desc_dev, const float* xy_dev, const int32_t* n_dev,
                            int n_images, int cap, const mh_planar_spec* spec, float* desc_out_dev, float* xyz_out_dev,
                            int out_cap, int32_t* n_out_dev, float* bbox_dev) {
  if (!ctx) return MH_ERR_ARG;
  if (!desc_dev || !xy_dev || !n_dev || n_images <= 0 || n_images > MH_MAX_BATCH || cap <= 0 || !desc_out_dev ||
      !xyz_out_dev || out_cap <= 0 || !n_out_dev || !bbox_dev || ((uintptr_t)desc_dev & 15) || ((uintptr_t)desc_out_dev & 15) ||
      ((uintptr_t)xy_dev & 7)) {
    ctx->err = std::string(who) + ": bad argument (descriptor arrays are 16-byte aligned, xy 8-byte)";
    return MH_ERR_ARG;
  }
  PlanarArgs a = {};
  if (int rc = planar_spec_check(ctx, who, spec, &a.all)) return rc;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  a.desc = desc_dev;
  a.xy = xy_dev;
  a.n = n_dev;
  a.cap = cap;
  a.spec = *spec;
  a.desc_out = desc_out_dev;
  a.desc_copy = nullptr;
  a.xyz_out = xyz_out_dev;
  a.out_pitch = (size_t)out_cap;
  a.out_cap = out_cap;
  a.n_out = n_out_dev;
  a.bbox = bbox_dev;
  launch_planar_rows(a, n_images, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

extern "C" {

int mh_planar_rows_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int cap,
                       const mh_planar_spec* spec, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                       int32_t* n_out_dev, float* bbox_dev) {
  return planar_rows_call(ctx, "mh_planar_rows_dev", desc_dev, xy_dev, n_dev, 1, cap, spec, desc_out_dev, xyz_out_dev, out_cap,
                          n_out_dev, bbox_dev);
}

int mh_planar_rows_batch_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int n_images,
                             int cap, const mh_planar_spec* spec, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                             int32_t* n_out_dev, float* bbox_dev) {
  return planar_rows_call(ctx, "mh_planar_rows_batch_dev", desc_dev, xy_dev, n_dev, n_images, cap, spec, desc_out_dev,
                          xyz_out_dev, out_cap, n_out_dev, bbox_dev);
}

}  // extern "C"
