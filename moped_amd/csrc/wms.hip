// CLUSTER: CLUSTER_WEIGHTED_MEAN_SHIFT_CPU::WeighedMeanShift<3> on gfx950
// (moped3d/libmoped/src/cluster/CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp:72-158).
//
// A true mean shift over the matches' camera-frame points: every point starts as an active canopy centred on itself;
// an iteration (1) moves every active canopy to the weighted mean of the POINTS within Radius of its centre -- the
// points never move, so the canopies are independent -- and (2) switches canopies off in a greedy ordered scan: for a
// ascending, active when reached, every b > a (active or not) whose centre is within Merge of a's goes inactive.  The
// clusters are the points within Radius of the surviving centres, so they MAY OVERLAP.  The kernel keeps the
// reference's fp32 operation order:
//
//  (1) one thread per active canopy (the active ones are kept as a list, so the waves that have none idle), the
//      inner loop over the points in list order reads wave-uniform LDS addresses (one float4 each for (x, y, z, w)
//      and the rounded products (xw, yw, zw)); no fused multiply-add, a true division;
//  (2) the closeness tests are independent: all wavefronts compute them as bit rows, 64 canopies at a time, for the
//      rows that are still active when their block starts; wavefront 0 holds the active set in registers (lane w =
//      word w) and resolves the ordered scan over those rows.  A hit against an inactive canopy still clears `done`.
//
// An iteration that changes neither an active centre's bits nor the active set is a fixed point: every later one is
// the same, so the loop leaves and reports the count the reference would reach (MaxIterations when something is
// still within Merge, else the next one).
//
// One workgroup per (model, image) problem; all state in LDS; <= MS_CAP points.  The workgroups leave their final
// centres, active flags and per-canopy cluster sizes in global memory; the LAST one to finish (common.h) gives every
// kept cluster its place in the call's CSR -- clusters in (problem, canopy) order -- and writes the members, descending
// (the reference's push_front), one wavefront per 64 canopies.  A cluster that does not fit the caps is not written
// at all; the totals tell the caller what to ask for.
#include "steps.h"

namespace mh {

namespace {

constexpr int WMS_THREADS = 1024;
constexpr int WMS_WAVES = WMS_THREADS / 64;
constexpr int WMS_ROWS = 64;             // canopies per block of the merge phase
constexpr int WMS_WORDS = MS_CAP / 64;   // 64-bit words of one bit row

struct WmsLds {
  float4 P[MS_CAP];     // x, y, z, weight
  float4 PW[MS_CAP];    // x * w, y * w, z * w (rounded products), -
  float C[3][MS_CAP];   // canopy centres (inactive ones stay frozen)
  unsigned long long rowbits[WMS_ROWS][WMS_WORDS];   // merge phase: closeness of the block's rows to the later canopies
  unsigned long long act[WMS_WORDS];                 // active canopies
  int alist[MS_CAP];    // the active canopies, ascending
  int na;
  int hit;              // a closeness test of this iteration's scan succeeded (`done = false`)
  int act_changed;
};
constexpr int WMS_LDS_BYTES = (int)sizeof(WmsLds);
static_assert(WMS_LDS_BYTES <= 160 * 1024 - 1024, "WmsLds must fit the CU's LDS");

__device__ __forceinline__ unsigned long long wms_readlane64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// Pt<3>::sqEuclDist: d = other[x] - this[x]; r += d * d over x = 0, 1, 2 (r starts at 0)
__device__ __forceinline__ float wms_sqdist(float tx, float ty, float tz, float ox, float oy, float oz) {
  const float d0 = __fsub_rn(ox, tx), d1 = __fsub_rn(oy, ty), d2 = __fsub_rn(oz, tz);
  float r = __fadd_rn(0.f, __fmul_rn(d0, d0));
  r = __fadd_rn(r, __fmul_rn(d1, d1));
  return __fadd_rn(r, __fmul_rn(d2, d2));
}

// cauchyWeight (:184-186): the quotient in float, the rest in double, rounded to float
__device__ __forceinline__ float wms_weight(float d, float g) {
  const float q = __fdiv_rn(__fmul_rn(d, d), __fmul_rn(g, g));
  return (float)(1.0 / (1.0 + (double)q));
}

struct WmsState {       // per point (problem p's points at off[p] ..), per problem
  float4* cw;           // final centre, weight
  int32_t* active;
  int32_t* size;        // points within Radius of an active canopy's centre
  int32_t* lk;          // place of its cluster among the problem's kept ones, or -1
  int32_t* lo;          // first member's place among the problem's members
  int32_t* ncl;         // per problem: kept clusters, their members, iterations
  int32_t* nmem;
  int32_t* iters;
  long long* base_k;    // per problem, by the last workgroup: clusters / members of the problems before
  long long* base_o;
};

// A frame's (model) problem writes its own clusters: its members' region is known without the other problems.
struct WmsOwn {
  int32_t* members = nullptr;   // the problem's region (member_cap words); nullptr: the last workgroup emits (wms_emit)
  int member_cap = 0;           // clusters are kept while they end inside it; the first that does not is dropped with the later ones
  int32_t member_base = 0;      // added to the problem-local index
  int32_t* cl_start = nullptr;  // [kept + 1]: where each kept cluster starts in the region
  int32_t* over = nullptr;      // set when a cluster was dropped for the cap
};

// load(i) -> (x, y, z, fill distance) of the problem's point i
template <typename Load>
__device__ __forceinline__ void wms_body(WmsLds& L, Load load, int b, int n, int p, float radius, float merge, int min_pts,
                                         int max_iter, float hwd, const WmsState& S, const WmsOwn& own) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float sq_radius = __fmul_rn(radius, radius);
  const float sq_merge = __fmul_rn(merge, merge);
  const int W = (n + 63) >> 6;

  for (int i = tid; i < n; i += WMS_THREADS) {
    const float4 in = load(i);
    const float x = in.x, y = in.y, z = in.z;
    const float w = wms_weight(in.w, hwd);
    L.P[i] = make_float4(x, y, z, w);
    L.PW[i] = make_float4(__fmul_rn(x, w), __fmul_rn(y, w), __fmul_rn(z, w), 0.f);
    L.C[0][i] = x;
    L.C[1][i] = y;
    L.C[2][i] = z;
    L.alist[i] = i;
  }
  if (tid < WMS_WORDS) {
    const int left = n - tid * 64;
    L.act[tid] = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1ull : 0ull;
  }
  if (tid == 0) L.na = n;
  __syncthreads();

  int it = 0;
  while (it < max_iter) {
    const int na = L.na;
    // ---- (1) shift (:108-127) ----
    int changed = 0;
    for (int kb = wave * 64; kb < na; kb += WMS_THREADS) {   // wave-uniform trip count
      const int k = kb + lane;
      const bool live = k < na;
      const int a = live ? L.alist[k] : 0;
      const float ox = L.C[0][a], oy = L.C[1][a], oz = L.C[2][a];
      float cx = 0.f, cy = 0.f, cz = 0.f, ws = 0.f;
#pragma unroll 4
      for (int i = 0; i < n; ++i) {
        const float4 q = L.P[i];
        const float4 qw = L.PW[i];
        if (wms_sqdist(ox, oy, oz, q.x, q.y, q.z) < sq_radius) {
          cx = __fadd_rn(cx, qw.x);
          cy = __fadd_rn(cy, qw.y);
          cz = __fadd_rn(cz, qw.z);
          ws = __fadd_rn(ws, q.w);
        }
      }
      if (live) {
        const float nx = __fdiv_rn(cx, ws), ny = __fdiv_rn(cy, ws), nz = __fdiv_rn(cz, ws);
        changed |= (__float_as_int(nx) ^ __float_as_int(ox)) | (__float_as_int(ny) ^ __float_as_int(oy)) |
                   (__float_as_int(nz) ^ __float_as_int(oz));
        L.C[0][a] = nx;
        L.C[1][a] = ny;
        L.C[2][a] = nz;
      }
    }
    if (tid == 0) {
      L.hit = 0;
      L.act_changed = 0;
    }
    __syncthreads();

    // ---- (2) merge (:130-141), in blocks of WMS_ROWS canopies ----
    unsigned long long actreg = lane < WMS_WORDS ? L.act[lane] : 0ull;   // used by wavefront 0: lane w = word w
    int hit = 0, act_changed = 0;
    constexpr int RPW = WMS_ROWS / WMS_WAVES;
    for (int i0 = 0; i0 < n; i0 += WMS_ROWS) {
      const int g = i0 >> 6;
      const unsigned long long rows = L.act[g];   // the rows still active as the block starts: the others are never reached
      if (rows == 0ull) continue;                 // (the same in every thread)
#pragma unroll
      for (int u = 0; u < RPW; ++u) {
        const int r = wave * RPW + u;
        if (!((rows >> r) & 1ull)) continue;
        const int a = i0 + r;
        const float ax = L.C[0][a], ay = L.C[1][a], az = L.C[2][a];
        unsigned long long mine = 0ull;
        for (int w = g; w < W; ++w) {
          const int j = w * 64 + lane;
          bool close = false;
          if (j > a && j < n) close = wms_sqdist(ax, ay, az, L.C[0][j], L.C[1][j], L.C[2][j]) < sq_merge;
          const unsigned long long bl = __ballot(close);
          if (lane == w) mine = bl;
        }
        if (lane >= g && lane < W) L.rowbits[r][lane] = mine;
      }
      __syncthreads();
      if (wave == 0) {
        // (Fetching eight rows per LDS round trip ahead of the scan was built and measured: 3% slower at n = 150, 586
        // and 2048 -- the scan is not what bounds an iteration.  Dropped.)
        for (unsigned long long m = rows; m; m &= m - 1ull) {
          const int r = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
          const unsigned long long row = (lane >= g && lane < W) ? L.rowbits[r][lane] : 0ull;   // (read before the test: one round trip per row)
          if (!((wms_readlane64(actreg, g) >> r) & 1ull)) continue;   // switched off by an earlier row of this block
          if (__ballot(row != 0ull) == 0ull) continue;
          hit = 1;
          const unsigned long long next = actreg & ~row;
          if (__ballot(next != actreg) != 0ull) act_changed = 1;
          actreg = next;
        }
        if (lane < WMS_WORDS) L.act[lane] = actreg;
      }
      __syncthreads();
    }
    // the list of active canopies, ascending
    if (wave == 0) {
      int base = 0;
      for (int w = 0; w < W; ++w) {
        const unsigned long long m = wms_readlane64(actreg, w);
        if ((m >> lane) & 1ull) L.alist[base + __popcll(m & ((1ull << lane) - 1ull))] = w * 64 + lane;
        base += __popcll(m);
      }
      if (lane == 0) {
        L.na = base;
        L.hit = hit;
        L.act_changed = act_changed;
      }
    }
    const int any_changed = __syncthreads_or(changed);
    ++it;
    if (!L.hit) break;   // `done` stayed true
    if (!any_changed && !L.act_changed) {   // a fixed point with something still within Merge: the reference runs on to MaxIterations
      it = max_iter;
      break;
    }
    __syncthreads();   // (L.hit is rewritten by the next iteration)
  }
  __syncthreads();

  // ---- sizes of the surviving canopies' clusters (:144-157), their places among the problem's kept ones ----
  const int na = L.na;
  int* const szk = reinterpret_cast<int*>(&L.PW[0]);   // by list position; the products are dead from here on
  int* const lkk = szk + MS_CAP;
  int* const lok = lkk + MS_CAP;
  static_assert(sizeof(L.PW) >= 3 * MS_CAP * sizeof(int), "the three lists live in PW");
  for (int k = wave; k < na; k += WMS_WAVES) {
    const int a = L.alist[k];
    const float ax = L.C[0][a], ay = L.C[1][a], az = L.C[2][a];
    int cnt = 0;
    for (int w = 0; w < W; ++w) {
      const int i = w * 64 + lane;
      bool in = false;
      if (i < n) {
        const float4 q = L.P[i];
        in = wms_sqdist(ax, ay, az, q.x, q.y, q.z) < sq_radius;
      }
      cnt += __popcll(__ballot(in));
    }
    if (lane == 0) szk[k] = cnt;
  }
  __syncthreads();
  if (wave == 0) {
    int nk = 0, nm = 0;
    bool full = false;   // own emission: a cluster has been dropped for the cap, and so are all later ones
    for (int k0 = 0; k0 < na; k0 += 64) {
      const int k = k0 + lane;
      const int sz = k < na ? szk[k] : 0;
      bool kept = k < na && sz > min_pts;
      int incl = kept ? sz : 0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      if (own.members) {   // (the ends ascend: the clusters that fit are a prefix, and the chunk is cut at the first that does not)
        const unsigned long long bad = __ballot(kept && (full || nm + incl > own.member_cap));
        if (bad) {
          if (!full && lane == 0 && own.over) *own.over = 1;
          full = true;
          const int first = __builtin_ctzll(bad);
          if (lane >= first) kept = false;
          const int fits = first > 0 ? __shfl(incl, first - 1) : 0;   // members of the chunk's clusters before the cut
          incl = lane < first ? incl : fits;
        }
      }
      const unsigned long long m = __ballot(kept);
      if (k < na) {
        lkk[k] = kept ? nk + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        lok[k] = nm + incl - (kept ? sz : 0);
      }
      nk += __popcll(m);
      nm += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) {
      S.ncl[p] = nk;
      S.nmem[p] = nm;
      S.iters[p] = it;
      if (own.cl_start) own.cl_start[nk] = nm;
    }
  }
  if (own.members) {   // this problem's own members, descending, one wavefront per cluster
    __syncthreads();
    for (int k = wave; k < na; k += WMS_WAVES) {
      const int ck = lkk[k];
      if (ck < 0) continue;
      const int a = L.alist[k], o = lok[k];
      const float ax = L.C[0][a], ay = L.C[1][a], az = L.C[2][a];
      if (lane == 0 && own.cl_start) own.cl_start[ck] = o;
      int run = 0;
      for (int w = W - 1; w >= 0; --w) {
        const int i = w * 64 + 63 - lane;
        bool in = false;
        if (i < n) {
          const float4 q = L.P[i];
          in = wms_sqdist(ax, ay, az, q.x, q.y, q.z) < sq_radius;
        }
        const unsigned long long mb = __ballot(in);
        if (in) own.members[o + run + __popcll(mb & ((1ull << lane) - 1ull))] = own.member_base + i;
        run += __popcll(mb);
      }
    }
  }
  for (int i = tid; i < n; i += WMS_THREADS) {
    S.cw[b + i] = make_float4(L.C[0][i], L.C[1][i], L.C[2][i], L.P[i].w);
    S.active[b + i] = (int)((L.act[i >> 6] >> (i & 63)) & 1ull);
    S.size[b + i] = 0;
    S.lk[b + i] = -1;
    S.lo[b + i] = 0;
  }
  __syncthreads();
  for (int k = tid; k < na; k += WMS_THREADS) {
    const int a = L.alist[k];
    S.size[b + a] = szk[k];
    S.lk[b + a] = lkk[k];
    S.lo[b + a] = lok[k];
  }
}

// By the last workgroup of the launch: the problems' clusters as one CSR, the members written.
// out_tot[0] / [1]: clusters / members that exist.  cl_off[k] (k <= cap_clusters): where cluster k starts; a cluster is
// written when it and its members lie inside the caps -- the clusters written are a prefix of the list.
__device__ void wms_emit(const float* __restrict__ xyz, const int32_t* __restrict__ off, int n_problems, float radius,
                         const WmsState& S, long long* out_tot, int32_t* cl_off, int cap_clusters, int32_t* members,
                         int cap_members, long long* scan_s) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float sq_radius = __fmul_rn(radius, radius);
  // ---- clusters / members before every problem ----
  long long run_k = 0, run_o = 0;
  for (int p0 = 0; p0 < n_problems; p0 += WMS_THREADS) {
    const int p = p0 + tid;
    const long long nk = p < n_problems ? S.ncl[p] : 0, nm = p < n_problems ? S.nmem[p] : 0;
    long long ik = nk, io = nm;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long uk = __shfl_up(ik, d), uo = __shfl_up(io, d);
      if (lane >= d) {
        ik += uk;
        io += uo;
      }
    }
    __syncthreads();   // (scan_s of the chunk before)
    if (lane == 63) {
      scan_s[2 * wave] = ik;
      scan_s[2 * wave + 1] = io;
    }
    __syncthreads();
    long long bk = 0, bo = 0, tk = 0, to = 0;
    for (int w = 0; w < WMS_WAVES; ++w) {
      const long long ck = scan_s[2 * w], co = scan_s[2 * w + 1];
      if (w < wave) {
        bk += ck;
        bo += co;
      }
      tk += ck;
      to += co;
    }
    if (p < n_problems) {
      S.base_k[p] = run_k + bk + ik - nk;
      S.base_o[p] = run_o + bo + io - nm;
    }
    run_k += tk;
    run_o += to;
  }
  if (tid == 0) {
    out_tot[0] = run_k;
    out_tot[1] = run_o;
    if (run_k <= cap_clusters) cl_off[run_k] = (int32_t)(run_o < 0x7fffffffLL ? run_o : 0x7fffffffLL);
  }
  __syncthreads();   // base_k / base_o: written and read by this workgroup
  // ---- one wavefront per 64 canopies, round robin over the problems' chunks ----
  long long q = 0;
  for (int p = 0; p < n_problems; ++p) {
    const int b = off[p], n = off[p + 1] - b;
    const int chunks = (n + 63) >> 6;
    if (n <= 0 || S.ncl[p] == 0) continue;
    const long long bk = S.base_k[p], bo = S.base_o[p];
    const int W = chunks;
    for (int c = 0; c < chunks; ++c, ++q) {
      if ((int)(q & (WMS_WAVES - 1)) != wave) continue;
      const int i0 = c * 64 + lane;
      const int lk = i0 < n ? S.lk[b + i0] : -1;
      const int lo = i0 < n ? S.lo[b + i0] : 0;
      const int sz = i0 < n ? S.size[b + i0] : 0;
      for (unsigned long long m = __ballot(lk >= 0); m; m &= m - 1ull) {
        const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
        const long long k = bk + __builtin_amdgcn_readlane(lk, l);
        const long long o = bo + __builtin_amdgcn_readlane(lo, l);
        const int size = __builtin_amdgcn_readlane(sz, l);
        if (k > cap_clusters) return;   // (k ascends through this wavefront's chunks: nothing further of the call is listed)
        if (lane == 0) cl_off[k] = (int32_t)(o < 0x7fffffffLL ? o : 0x7fffffffLL);
        if (k >= cap_clusters || o + size > cap_members) continue;
        const float4 cen = S.cw[b + c * 64 + l];
        int run = 0;
        for (int w = W - 1; w >= 0; --w) {   // descending: the reference's push_front
          const int i = w * 64 + 63 - lane;
          bool in = false;
          if (i < n) {
            const float* q3 = xyz + 3 * (size_t)(b + i);
            in = wms_sqdist(cen.x, cen.y, cen.z, q3[0], q3[1], q3[2]) < sq_radius;
          }
          const unsigned long long mb = __ballot(in);
          if (in) members[o + run + __popcll(mb & ((1ull << lane) - 1ull))] = i;
          run += __popcll(mb);
        }
      }
    }
  }
}

__global__ __launch_bounds__(WMS_THREADS) void wms_batch_kernel(const float* __restrict__ xyz, const float* __restrict__ fill,
                                                                const int32_t* __restrict__ off, int n_problems, float radius,
                                                                float merge, int min_pts, int max_iter, float hwd, WmsState S,
                                                                long long* out_tot, int32_t* cl_off, int cap_clusters,
                                                                int32_t* members, int cap_members, unsigned int* ticket) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  WmsLds& L = *reinterpret_cast<WmsLds*>(smem);
  __shared__ long long scan_s[2 * WMS_WAVES];
  const int p = blockIdx.x;
  const int b = off[p];
  const int n = off[p + 1] - b;
  if (n <= 0 || n > MS_CAP) {   // (the host checks the capacity before launching)
    if (threadIdx.x == 0) {
      S.ncl[p] = 0;
      S.nmem[p] = 0;
      S.iters[p] = 0;
    }
  } else {
    wms_body(
        L, [=](int i) { return make_float4(xyz[3 * (size_t)(b + i)], xyz[3 * (size_t)(b + i) + 1], xyz[3 * (size_t)(b + i) + 2], fill[b + i]); },
        b, n, p, radius, merge, min_pts, max_iter, hwd, S, WmsOwn());
  }
  if (!last_workgroup(ticket)) return;
  wms_emit(xyz, off, n_problems, radius, S, out_tot, cl_off, cap_clusters, members, cap_members, scan_s);
}

// Frame form: one workgroup per model over the frame's match lists.  Points = m_depth's camera-frame points (depth4:
// x, y, z, weight per match), fill distances from the frame's fill map at ((int) u, (int) v), clamped as DEPTHMAP_PROP's
// device form clamps (depth.hip), -1 without a map (DEPTHMAP_PROP_CPU.hpp:107-111).  Model m's clusters go to
// members[factor * model_off[m] ..): at most factor x its match count; the first cluster that would pass that is dropped
// whole with the model's later ones and ERR_CLUSTER_CAP is set.  The last workgroup lays the frame's cluster table out.
__global__ __launch_bounds__(WMS_THREADS) void wms_models_kernel(
    const mh_corr* __restrict__ corr, const float4* __restrict__ depth4, const int32_t* __restrict__ model_off, int n_models,
    const float* __restrict__ fillmap, int fw, int fh, float radius, float merge, int min_pts, int max_iter, float hwd, WmsState S,
    int32_t* members, int factor, int32_t* cl_start, int32_t* ncl, int max_clusters, int32_t* __restrict__ cl_model,
    int32_t* __restrict__ cl_begin, int32_t* __restrict__ cl_count, int32_t* __restrict__ n_clusters_out, int32_t* __restrict__ snap,
    FrameCounts* counts, unsigned int* ticket) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  WmsLds& L = *reinterpret_cast<WmsLds*>(smem);
  __shared__ int lay_s[WMS_WAVES];
  __shared__ int over_s;
  const int m = blockIdx.x;
  if (m < n_models) {
    if (threadIdx.x == 0) over_s = 0;
    const int b = model_off[m];
    int n = model_off[m + 1] - b;
    if (n > MS_CAP) {
      if (threadIdx.x == 0) atomicOr(&counts->error, ERR_MS_CAP);
      n = MS_CAP;
    }
    if (n <= 0 || n <= min_pts) {   // no canopy can hold more than MinPts points (:154)
      if (threadIdx.x == 0) {
        ncl[m] = 0;
        cl_start[b + m] = 0;
      }
    } else {
      WmsOwn own;
      own.members = members + (size_t)factor * b;
      own.member_cap = factor * n;
      own.member_base = b;
      own.cl_start = cl_start + b + m;
      own.over = &over_s;
      S.ncl = ncl;   // (the frame's per-model cluster counts are the state's)
      wms_body(
          L,
          [=](int i) {
            const float4 d = depth4[b + i];
            float f = -1.f;
            if (fillmap) {
              int ix = (int)corr[b + i].u, iy = (int)corr[b + i].v;
              ix = ix < 0 ? 0 : (ix >= fw ? fw - 1 : ix);
              iy = iy < 0 ? 0 : (iy >= fh ? fh - 1 : iy);
              f = fillmap[(size_t)iy * fw + ix];
            }
            return make_float4(d.x, d.y, d.z, f);
          },
          b, n, m, radius, merge, min_pts, max_iter, hwd, S, own);
      __syncthreads();
      if (threadIdx.x == 0 && over_s) atomicOr(&counts->error, ERR_CLUSTER_CAP);
    }
  }
  if (!last_workgroup(ticket)) return;
  const int k0 = layout_cluster_table(n_models, model_off, ncl, cl_start, 1, max_clusters, cl_model, cl_begin, cl_count, lay_s,
                                      [min_pts](int nn) { return nn > 0 && nn > min_pts; }, factor);
  if (threadIdx.x == 0) {
    if (k0 > max_clusters) atomicOr(&counts->error, ERR_CLUSTER_CAP);
    const int k = k0 < max_clusters ? k0 : max_clusters;
    counts->n_clusters = k;
    *n_clusters_out = k;
    if (snap) {
      snap[0] = counts->n_matches;
      snap[1] = k;
    }
  }
}

}  // namespace

size_t wms_state_bytes(size_t n_problems, size_t total) {
  return total * (sizeof(float4) + 4 * sizeof(int32_t)) + n_problems * (3 * sizeof(int32_t) + 2 * sizeof(long long)) + 64;
}

void launch_wms_batch(const float* xyz, const float* fill, const int32_t* off, int n_problems, int total, const WmsParams& prm,
                      void* state, float4** cw_out, int32_t** active_out, int32_t** ncl_out, int32_t** nmem_out,
                      int32_t** iters_out, long long* out_tot, int32_t* cl_off, int cap_clusters, int32_t* members,
                      int cap_members, unsigned int* ticket, hipStream_t s) {
  // state: cw | base_k | base_o | active | size | lk | lo | ncl | nmem | iters   (16- and 8-byte items first)
  WmsState S;
  unsigned char* q = static_cast<unsigned char*>(state);
  S.cw = reinterpret_cast<float4*>(q);
  q += (size_t)total * sizeof(float4);
  S.base_k = reinterpret_cast<long long*>(q);
  q += (size_t)n_problems * sizeof(long long);
  S.base_o = reinterpret_cast<long long*>(q);
  q += (size_t)n_problems * sizeof(long long);
  int32_t* w = reinterpret_cast<int32_t*>(q);
  S.active = w;
  S.size = w + total;
  S.lk = w + 2 * (size_t)total;
  S.lo = w + 3 * (size_t)total;
  S.ncl = w + 4 * (size_t)total;
  S.nmem = S.ncl + n_problems;
  S.iters = S.nmem + n_problems;
  if (cw_out) *cw_out = S.cw;
  if (active_out) *active_out = S.active;
  if (ncl_out) *ncl_out = S.ncl;
  if (nmem_out) *nmem_out = S.nmem;
  if (iters_out) *iters_out = S.iters;
  if (n_problems <= 0) return;
  static DynLds attr;
  attr.ensure(wms_batch_kernel, WMS_LDS_BYTES);
  hipLaunchKernelGGL(wms_batch_kernel, dim3(n_problems), dim3(WMS_THREADS), WMS_LDS_BYTES, s, xyz, fill, off, n_problems,
                     prm.radius, prm.merge, prm.min_pts, prm.max_iter, prm.half_weight_distance, S, out_tot, cl_off,
                     cap_clusters, members, cap_members, ticket);
}

void launch_wms_models(const mh_corr* corr, const float* depth4, const int32_t* model_off, int n_models, int max_m,
                       const DepthImage& dimg, const WmsParams& prm, void* state, int32_t* members, int factor, int32_t* cl_start,
                       int32_t* ncl, int max_clusters, int32_t* cl_model, int32_t* cl_begin, int32_t* cl_count,
                       int32_t* n_clusters_out, int32_t* snap, FrameCounts* counts, unsigned int* ticket, hipStream_t s) {
  // state as launch_wms_batch lays it out, for max_m points and n_models problems
  WmsState S;
  unsigned char* q = static_cast<unsigned char*>(state);
  const size_t np = (size_t)std::max(n_models, 1);
  S.cw = reinterpret_cast<float4*>(q);
  q += (size_t)max_m * sizeof(float4);
  S.base_k = reinterpret_cast<long long*>(q);
  q += np * sizeof(long long);
  S.base_o = reinterpret_cast<long long*>(q);
  q += np * sizeof(long long);
  int32_t* w = reinterpret_cast<int32_t*>(q);
  S.active = w;
  S.size = w + max_m;
  S.lk = w + 2 * (size_t)max_m;
  S.lo = w + 3 * (size_t)max_m;
  S.ncl = w + 4 * (size_t)max_m;
  S.nmem = S.ncl + np;
  S.iters = S.nmem + np;
  static DynLds attr;
  attr.ensure(wms_models_kernel, WMS_LDS_BYTES);
  // an empty database still gets one workgroup: it publishes "0 clusters"
  hipLaunchKernelGGL(wms_models_kernel, dim3(std::max(n_models, 1)), dim3(WMS_THREADS), WMS_LDS_BYTES, s, corr,
                     reinterpret_cast<const float4*>(depth4), model_off, n_models, dimg.fill, dimg.w, dimg.h, prm.radius, prm.merge,
                     prm.min_pts, prm.max_iter, prm.half_weight_distance, S, members, factor, cl_start, ncl, max_clusters, cl_model,
                     cl_begin, cl_count, n_clusters_out, snap, counts, ticket);
}

}  // namespace mh
