// C ABI: moped3d's weighted mean-shift clusterer on host pointers (mh_cluster_wms, mh_wms_debug_state): one upload,
// one launch of wms_batch_kernel (wms.hip), one download.
#include <cmath>
#include <cstring>

#include "frame.h"

using namespace mh;

namespace {

// the checks both entries share; `who` names the call in the message
int wms_check(mh_ctx* ctx, const char* who, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
              const mh_wms_params* prm) {
  if (!ctx) return MH_ERR_ARG;
  const auto bad = [&](const char* what) {
    ctx->err = std::string(who) + ": " + what;
    return MH_ERR_ARG;
  };
  if (!prm) return bad("prm is null");
  if (n_problems < 0) return bad("n_problems < 0");
  if (!(prm->radius >= 0.f)) return bad("radius must be a number >= 0");
  if (!(prm->merge >= 0.f)) return bad("merge must be a number >= 0");
  if (!(prm->half_weight_distance >= 0.f)) return bad("half_weight_distance must be a number >= 0");
  if (prm->max_iter < 0) return bad("max_iter < 0");
  if (n_problems == 0) return MH_OK;
  if (!off) return bad("off is null");
  if (off[0] != 0) return bad("off must start at 0");
  for (int p = 0; p < n_problems; ++p) {
    if (off[p + 1] < off[p]) return bad("off must not decrease");
    if (off[p + 1] - off[p] > MS_CAP) return bad("more than 2048 points in one problem");
  }
  if (off[n_problems] > 0 && !xyz_host) return bad("xyz_host is null");
  if (off[n_problems] > 0 && !fill_host) return bad("fill_host is null");
  return MH_OK;
}

// Both entries once the arguments are checked (total > 0).  The download -- totals | per-problem kept clusters, members,
// iterations | cl_off | members -- lands in the context's pinned block behind the upload's staging; *down points at it.
// state_cw / state_active (optional): where the device keeps the final centres + weights and the active flags.
int wms_run(mh_ctx* ctx, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
            const mh_wms_params* prm, int cap_clusters, int cap_members, const unsigned char** down, float4** state_cw,
            int32_t** state_active) {
  const size_t total = (size_t)off[n_problems];
  if (int rc_enter = mh::enter(ctx)) return rc_enter;
  const auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
  // upload: ticket (zero) | off | xyz | fill
  const size_t u_off = 16, u_xyz = u_off + pad(((size_t)n_problems + 1) * 4), u_fill = u_xyz + pad(total * 12),
               b_up = u_fill + pad(total * 4);
  // download: totals [2] int64 | ncl, nmem, iters [n_problems] | cl_off [cap_clusters + 1] | members [cap_members]
  const size_t d_cnt = 16, d_cl = d_cnt + 3 * (size_t)n_problems * 4, d_mem = d_cl + ((size_t)cap_clusters + 1) * 4,
               b_down = pad(d_mem + (size_t)cap_members * 4);
  const size_t b_state = pad(wms_state_bytes(n_problems, total));
  int rc = ensure_scratch(ctx, b_up + b_state + b_down + 64);
  if (rc) return rc;
  if ((rc = ensure_pinned(ctx, b_up + b_down))) return rc;
  unsigned char* const h = reinterpret_cast<unsigned char*>(ctx->pinned.p);
  std::memset(h, 0, 16);
  std::memcpy(h + u_off, off, ((size_t)n_problems + 1) * 4);
  std::memcpy(h + u_xyz, xyz_host, total * 12);
  std::memcpy(h + u_fill, fill_host, total * 4);
  unsigned char* const base = ctx->scratch;
  unsigned char* const d_state = base + b_up;
  unsigned char* const d_down = d_state + b_state;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(base, h, b_up, hipMemcpyHostToDevice, s));
  WmsParams wp;
  wp.radius = prm->radius;
  wp.merge = prm->merge;
  wp.min_pts = prm->min_pts;
  wp.max_iter = prm->max_iter;
  wp.half_weight_distance = prm->half_weight_distance;
  int32_t *s_ncl = nullptr, *s_nmem = nullptr, *s_iters = nullptr;
  launch_wms_batch(reinterpret_cast<const float*>(base + u_xyz), reinterpret_cast<const float*>(base + u_fill),
                   reinterpret_cast<const int32_t*>(base + u_off), n_problems, (int)total, wp, d_state, state_cw, state_active,
                   &s_ncl, &s_nmem, &s_iters, reinterpret_cast<long long*>(d_down), reinterpret_cast<int32_t*>(d_down + d_cl),
                   cap_clusters, reinterpret_cast<int32_t*>(d_down + d_mem), cap_members, reinterpret_cast<unsigned int*>(base), s);
  MH_HIP(ctx, hipGetLastError());
  // the three per-problem arrays (contiguous in the state: ncl | nmem | iters) join the download block on the device
  MH_HIP(ctx, hipMemcpyAsync(d_down + d_cnt, s_ncl, 3 * (size_t)n_problems * 4, hipMemcpyDeviceToDevice, s));
  MH_HIP(ctx, hipMemcpyAsync(h + b_up, d_down, b_down, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  *down = h + b_up;
  return MH_OK;
}

}  // namespace

extern "C" {

int mh_cluster_wms(mh_ctx* ctx, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
                   const mh_wms_params* prm, int32_t* n_clusters, int32_t* cl_off, int cap_clusters, int32_t* members,
                   int cap_members, int64_t needed[2]) {
  if (int rc = wms_check(ctx, "mh_cluster_wms", xyz_host, fill_host, off, n_problems, prm)) return rc;
  if (cap_clusters < 0 || cap_members < 0) {
    ctx->err = "mh_cluster_wms: cap_clusters and cap_members must be >= 0";
    return MH_ERR_ARG;
  }
  const char* null_arg = !cl_off ? "cl_off" : (n_problems > 0 && !n_clusters) ? "n_clusters"
                         : (cap_members > 0 && !members) ? "members" : nullptr;
  if (null_arg) {
    ctx->err = std::string("mh_cluster_wms: ") + null_arg + " is null";
    return MH_ERR_ARG;
  }
  // what the device block and the download are sized by: the caller's caps, but no more than can exist -- a cluster per
  // point, n members per cluster of a problem of n points -- so that a generous cap costs nothing
  {
    long long most_k = 0, most_m = 0;
    for (int p = 0; p < n_problems; ++p) {
      const long long n = off[p + 1] - off[p];
      most_k += n;
      most_m += n * n;
    }
    cap_clusters = (int)std::min<long long>(cap_clusters, most_k);
    cap_members = (int)std::min<long long>(cap_members, most_m);
  }
  cl_off[0] = 0;
  if (needed) needed[0] = needed[1] = 0;
  for (int p = 0; p < n_problems; ++p) n_clusters[p] = 0;
  if (n_problems == 0 || off[n_problems] == 0) return MH_OK;
  const unsigned char* down = nullptr;
  if (int rc = wms_run(ctx, xyz_host, fill_host, off, n_problems, prm, cap_clusters, cap_members, &down, nullptr, nullptr))
    return rc;
  const long long* tot = reinterpret_cast<const long long*>(down);
  const int32_t* ncl = reinterpret_cast<const int32_t*>(down + 16);
  const int32_t* d_cl = ncl + 3 * (size_t)n_problems;
  const int32_t* d_mem = d_cl + (size_t)cap_clusters + 1;
  if (needed) {
    needed[0] = tot[0];
    needed[1] = tot[1];
  }
  // the clusters written: the longest prefix of the list inside both caps
  const long long listed = std::min<long long>(tot[0], cap_clusters);
  long long K = 0;
  while (K < listed && d_cl[K + 1] <= cap_members && d_cl[K + 1] >= d_cl[K]) ++K;
  std::memcpy(cl_off, d_cl, ((size_t)K + 1) * 4);
  if (d_cl[K] > 0) std::memcpy(members, d_mem, (size_t)d_cl[K] * 4);
  long long before = 0;
  for (int p = 0; p < n_problems; ++p) {
    n_clusters[p] = (int32_t)std::max<long long>(0, std::min<long long>(ncl[p], K - before));
    before += ncl[p];
  }
  if (K < tot[0]) {
    ctx->err = "mh_cluster_wms: " + std::to_string(tot[0]) + " clusters with " + std::to_string(tot[1]) +
               " members exist, the caps hold " + std::to_string(cap_clusters) + " / " + std::to_string(cap_members);
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_wms_debug_state(mh_ctx* ctx, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
                       const mh_wms_params* prm, float* weight, float* centre, int32_t* active, int32_t* iterations) {
  if (int rc = wms_check(ctx, "mh_wms_debug_state", xyz_host, fill_host, off, n_problems, prm)) return rc;
  if (n_problems == 0) return MH_OK;
  if (!iterations || (off[n_problems] > 0 && (!weight || !centre || !active))) {
    ctx->err = "mh_wms_debug_state: an output pointer is null";
    return MH_ERR_ARG;
  }
  for (int p = 0; p < n_problems; ++p) iterations[p] = 0;
  const size_t total = (size_t)off[n_problems];
  if (total == 0) return MH_OK;
  const unsigned char* down = nullptr;
  float4* d_cw = nullptr;
  int32_t* d_active = nullptr;
  if (int rc = wms_run(ctx, xyz_host, fill_host, off, n_problems, prm, 0, 0, &down, &d_cw, &d_active)) return rc;
  const int32_t* cnt = reinterpret_cast<const int32_t*>(down + 16);
  std::memcpy(iterations, cnt + 2 * (size_t)n_problems, (size_t)n_problems * 4);
  std::vector<float> cw(4 * total);
  MH_HIP(ctx, hipMemcpy(cw.data(), d_cw, total * sizeof(float4), hipMemcpyDeviceToHost));
  MH_HIP(ctx, hipMemcpy(active, d_active, total * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < total; ++i) {
    centre[3 * i] = cw[4 * i];
    centre[3 * i + 1] = cw[4 * i + 1];
    centre[3 * i + 2] = cw[4 * i + 2];
    weight[i] = cw[4 * i + 3];
  }
  return MH_OK;
}

}  // extern "C"
