// CLUSTER_LINKAGE in MH_LINKAGE_ROWMAX mode (mh_linkage_set_mode): the clusterer of linkage.hip with another schedule
// and the same bytes, for lists of up to LK_MAX = 4096 matches.
//
// MATRIX STAGE on the whole grid, a pass boundary = a launch boundary (there is no grid-wide barrier):
//   plan   : the problems of the launch with their scratch bases, tile and row-block ranges (one small workgroup)
//   nn     : nearest-neighbour distances, a thread per row, the columns staged through LDS (skipped with given sigmas)
//   prep   : the fill weights; the sigma sums by ONE thread in index order (the order is the result)
//   pass 1..3 over 32 x 32 tiles of the upper triangle, the points of a tile's rows and columns staged in LDS; every
//            element by linkage_pair.h's expressions, as linkage.hip computes it.  The maxima of passes 1 and 2 are
//            integer atomic maxima over the floats' bit patterns: the values are >= 0, NaN is left out, "nothing
//            seen" stays -1 -- order-independent, and equal to the workgroup reduction of linkage.hip.
// AGGLOMERATION, one 1024-thread workgroup per problem: hierarchicalCluster (CLUSTER_LINKAGE_CPU.hpp:416-540, quirks as
// in oracle/linkage_oracle.cpp) with the first maximum of every listed row a over its listed columns b > a kept in LDS:
// cache[a] = (value, column), strict `>` from -1, ties to the smaller column, NaN never wins.  A scan is the first
// maximum of the row caches in ascending a -- O(n) where linkage.hip rescans all live pairs.  What keeps the caches
// the scan's truth:
//   - the scan after a merge (first, second): removeValue = second is still listed as a column; rows removeValue and
//     `skip` (the next listed index after it, if it was still listed) are left out of the reduction only;
//   - when that scan ends removeValue is delisted: listed rows a < removeValue whose cached column it was are dirty;
//   - the merge rewrites row and column `first` with nv[]: row `first` is dirty; a listed row a < first keeps a cached
//     column `first` with the new value if nv[a] >= the cached value, else (smaller or NaN) it is dirty; with another
//     cached column it takes (nv[a], first) when nv[a] is larger, or equal with first the smaller column;
//   - dirty rows are rescanned, a wavefront each, before the next scan.
// A stale winner (a, removeValue) is a merge with S2 = 0, as in linkage.hip.
#include <algorithm>

#include "linkage_pair.h"

namespace mh {

namespace {

constexpr int RM_THREADS = 1024;
constexpr int RM_DLDS = 160;      // up to this many rows the similarity matrix stays in LDS (as linkage.hip)
constexpr int RM_TILE = LK_RM_TILE;   // passes 1..3: 32 x 32 elements per 256-thread workgroup
constexpr int RM_ROWS = LK_RM_ROWS;   // nn: rows per workgroup
static_assert(RM_TILE == 32 && RM_ROWS == 256, "the pass kernels' thread layout (tid & 31, tid >> 5) and the 256-thread launches");
constexpr int RM_NONE = 0xFFFF;   // a row cache without a column
constexpr int RM_PER = LK_MAX / RM_THREADS;

struct RmProblem {
  int32_t b, n;          // the problem's points: rows [b, b + n) of its frame's corr / depth4 (n = 0: refused, nothing to do)
  int32_t p;             // its place in the outputs (problem of a step call, model of a frame)
  int32_t tile0, rb0;    // tiles / row blocks of the problems before it
  int32_t frame;         // frame of a merged batch (0: a step call, a frame alone)
  unsigned long long base;   // floats before its matrix region A | Dm | member lists
};
struct RmHeader {
  float sigma2, sigma3;
  int max1, max2;        // bit patterns of the maxima of passes 1 and 2
};
struct RmPlan {
  int32_t n_problems, n_tiles, n_rowblocks, pad;
  int32_t fstart[MH_MAX_BATCH + 1];   // frame form: frame f's problems are [fstart[f], fstart[f + 1])
};
constexpr size_t RM_PLAN_BYTES = (sizeof(RmPlan) + 63) & ~(size_t)63;
// What the matrix kernels work from.  A step call: one frame, arena = pt_stride = 0.  Frames of a merged batch: frame
// f's match arrays lie f * arena bytes behind frame 0's (FrameBatch), its depth map is maps.img[f] (f > 0), its
// per-point arrays start at f * pt_stride.
struct RmArgs {
  const mh_corr* corr;
  const float4* depth4;
  unsigned long long arena;
  int pt_stride;
  DepthImage dimg;
  DepthMaps maps;
  LinkageParams P;
  const RmPlan* plan;
  const RmProblem* problems;
  RmHeader* hdr;
  float *nn2, *nn3, *w;   // per point: nearest-neighbour distances, fill weight
  float* scratch;
};
__device__ __forceinline__ const mh_corr* corr_of(const RmArgs& a, const RmProblem& q) {
  return frame_ptr(a.corr, (unsigned long long)q.frame * a.arena) + q.b;
}
__device__ __forceinline__ const float4* depth4_of(const RmArgs& a, const RmProblem& q) {
  return frame_ptr(a.depth4, (unsigned long long)q.frame * a.arena) + q.b;
}
__device__ __forceinline__ size_t point_of(const RmArgs& a, const RmProblem& q) {
  return (size_t)q.frame * a.pt_stride + q.b;
}
__device__ __forceinline__ DepthImage map_of(const RmArgs& a, const RmProblem& q) {
  DepthImage D = a.dimg;
  if (q.frame) {
    D.img = a.maps.img[q.frame];
    D.fill = a.maps.fill[q.frame];
  }
  return D;
}

__device__ __forceinline__ int tiles_of(int n) {
  const int nt = (n + RM_TILE - 1) / RM_TILE;
  return nt * (nt + 1) / 2;
}

// problems of a step call: [off[p], off[p + 1]) of the concatenated arrays; empty ones are left out
__global__ void rm_plan_batch_kernel(const int32_t* __restrict__ off, int n_problems, size_t scratch_floats, RmPlan* plan,
                                     RmProblem* __restrict__ problems, RmHeader* __restrict__ hdr, int32_t* __restrict__ ncl) {
  if (threadIdx.x || blockIdx.x) return;
  int k = 0, tiles = 0, rbs = 0;
  size_t base = 0;
  for (int p = 0; p < n_problems; ++p) {
    const int b = off[p], n = off[p + 1] - b;
    ncl[p] = 0;
    if (n <= 0 || n > LK_MAX || base + 3 * (size_t)n * n > scratch_floats) continue;   // the host checks both before launching
    RmProblem q;
    q.b = b;
    q.n = n;
    q.p = p;
    q.tile0 = tiles;
    q.rb0 = rbs;
    q.frame = 0;
    q.base = base;
    problems[k] = q;
    hdr[k].sigma2 = hdr[k].sigma3 = 0.f;
    hdr[k].max1 = hdr[k].max2 = __float_as_int(-1.f);
    ++k;
    tiles += tiles_of(n);
    rbs += (n + RM_ROWS - 1) / RM_ROWS;
    base += 3 * (size_t)n * n;
  }
  plan->n_problems = k;
  plan->n_tiles = tiles;
  plan->n_rowblocks = rbs;
}

// the problem whose units (tiles: field 0, row blocks: field 1) hold unit u
__device__ __forceinline__ int problem_of(const RmProblem* __restrict__ problems, int n_problems, int u, int field) {
  int lo = 0, hi = n_problems - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int start = field ? problems[mid].rb0 : problems[mid].tile0;
    if (start <= u) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---- nn: getAverageNNDistances' minima (:97-123), row by row ----
__global__ __launch_bounds__(RM_ROWS) void rm_nn_kernel(RmArgs a) {
  const RmProblem* __restrict__ problems = a.problems;
  __shared__ float c_uv[RM_ROWS][2], c_mx[RM_ROWS][3];
  const int tid = threadIdx.x;
  const int n_units = a.plan->n_rowblocks, n_problems = a.plan->n_problems;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const RmProblem q = problems[problem_of(problems, n_problems, u, 1)];
    const int N = q.n, i = (u - q.rb0) * RM_ROWS + tid;
    const mh_corr* __restrict__ corr = corr_of(a, q);
    float uv_i[2] = {0.f, 0.f}, mx_i[3] = {0.f, 0.f, 0.f};
    if (i < N) {
      const mh_corr c = corr[i];
      uv_i[0] = c.u;
      uv_i[1] = c.v;
      mx_i[0] = c.x;
      mx_i[1] = c.y;
      mx_i[2] = c.z;
    }
    float m2 = __builtin_inff(), m3 = __builtin_inff();   // Float = DBL_MAX
    for (int j0 = 0; j0 < N; j0 += RM_ROWS) {
      __syncthreads();
      if (j0 + tid < N) {
        const mh_corr c = corr[j0 + tid];
        c_uv[tid][0] = c.u;
        c_uv[tid][1] = c.v;
        c_mx[tid][0] = c.x;
        c_mx[tid][1] = c.y;
        c_mx[tid][2] = c.z;
      }
      __syncthreads();
      const int cnt = min(RM_ROWS, N - j0);
      if (i < N)
        for (int jj = 0; jj < cnt; ++jj) {
          if (j0 + jj == i) continue;
          float d2, d3;
          lk_nn_pair(uv_i, c_uv[jj], mx_i, c_mx[jj], d2, d3);
          if (m2 > d2) m2 = d2;
          if (m3 > d3) m3 = d3;
        }
    }
    if (i < N) {
      a.nn2[point_of(a, q) + i] = m2;
      a.nn3[point_of(a, q) + i] = m3;
    }
  }
}

// ---- prep: fill weights; the sigmas (sums in index order by one thread) ----
__global__ __launch_bounds__(RM_ROWS) void rm_prep_kernel(RmArgs a) {
  const LinkageParams& P = a.P;
  __shared__ float s2[LK_MAX], s3[LK_MAX];
  const int tid = threadIdx.x;
  const int n_problems = a.plan->n_problems;
  const bool auto_sigma = P.sigma2d == -1.f || P.sigma3d == -1.f;
  for (int k = blockIdx.x; k < n_problems; k += gridDim.x) {
    const RmProblem q = a.problems[k];
    const int N = q.n;
    const mh_corr* __restrict__ corr = corr_of(a, q);
    const DepthImage D = map_of(a, q);
    const size_t pt = point_of(a, q);
    __syncthreads();
    for (int i = tid; i < N; i += RM_ROWS) {
      const mh_corr c = corr[i];
      const float uv[2] = {c.u, c.v};
      a.w[pt + i] = lk_fill_weight(D, uv);
      if (auto_sigma) {
        s2[i] = a.nn2[pt + i];
        s3[i] = a.nn3[pt + i];
      }
    }
    __syncthreads();
    if (tid == 0) {
      float k2DSigma = P.sigma2d, k3DSigma = P.sigma3d;
      if (auto_sigma) {
        float a2 = 0.f, a3 = 0.f;
        for (int i = 0; i < N; ++i) {
          a2 = __fadd_rn(a2, s2[i]);
          a3 = __fadd_rn(a3, s3[i]);
        }
        if (P.sigma2d == -1.f) k2DSigma = __fdiv_rn(a2, (float)N);
        if (P.sigma3d == -1.f) k3DSigma = __fdiv_rn(a3, (float)N);
      }
      a.hdr[k].sigma2 = k2DSigma;
      a.hdr[k].sigma3 = k3DSigma;
    }
  }
}

// ---- passes 1..3 over the tiles of the upper triangle ----
struct RmTilePts {
  float uv[RM_TILE][2], mx[RM_TILE][3], wx[RM_TILE][3], w[RM_TILE];
};

template <int PASS>
__global__ __launch_bounds__(256) void rm_pass_kernel(RmArgs a) {
  const LinkageParams& P = a.P;
  const RmProblem* __restrict__ problems = a.problems;
  RmHeader* hdr = a.hdr;
  __shared__ RmTilePts R, C;
  const int tid = threadIdx.x, tx = tid & (RM_TILE - 1), ty = tid >> 5;
  const int n_units = a.plan->n_tiles, n_problems = a.plan->n_problems;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int k = problem_of(problems, n_problems, u, 0);
    const RmProblem q = problems[k];
    const int N = q.n, nt = (N + RM_TILE - 1) / RM_TILE, t = u - q.tile0;
    const mh_corr* __restrict__ corr = corr_of(a, q);
    const float4* __restrict__ depth4 = depth4_of(a, q);
    const DepthImage D = map_of(a, q);
    const size_t pt = point_of(a, q);
    // tile t -> (ti, tj), ti <= tj, row-major over the upper triangle of tiles
    int ti;
    {
      auto row_start = [&](int r) { return r * nt - r * (r - 1) / 2; };
      int r = (int)(((double)(2 * nt + 1) - sqrt((double)(2 * nt + 1) * (2 * nt + 1) - 8.0 * (double)t)) * 0.5);
      r = r < 0 ? 0 : (r > nt - 1 ? nt - 1 : r);
      while (r + 1 < nt && row_start(r + 1) <= t) ++r;
      while (r > 0 && row_start(r) > t) --r;
      ti = r;
    }
    const int tj = ti + (t - (ti * nt - ti * (ti - 1) / 2));
    __syncthreads();   // the tile before is done with
    if (tid < 2 * RM_TILE) {
      RmTilePts& T = tid < RM_TILE ? R : C;
      const int l = tid & (RM_TILE - 1), i = (tid < RM_TILE ? ti : tj) * RM_TILE + l;
      if (i < N) {
        const mh_corr c = corr[i];
        const float4 d = depth4[i];
        T.uv[l][0] = c.u;
        T.uv[l][1] = c.v;
        T.mx[l][0] = c.x;
        T.mx[l][1] = c.y;
        T.mx[l][2] = c.z;
        T.wx[l][0] = d.x;
        T.wx[l][1] = d.y;
        T.wx[l][2] = d.z;
        T.w[l] = PASS == 3 ? a.w[pt + i] : 0.f;
      }
    }
    __syncthreads();
    float* A = a.scratch + q.base;
    float* Dm = A + (size_t)N * N;
    const RmHeader h = hdr[k];
    const float max1 = __int_as_float(h.max1);
    const float max2 = P.use3d_filter ? __int_as_float(h.max2) : max1;
    const float two2 = lk_two_sigma_sq(h.sigma2), two3 = lk_two_sigma_sq(h.sigma3);
    float mx = -1.f;
    const int j = tj * RM_TILE + tx;
    for (int r = ty; r < RM_TILE; r += 256 / RM_TILE) {
      const int i = ti * RM_TILE + r;
      if (i >= N || j >= N || j < i) continue;
      const size_t e = (size_t)i * N + j;
      if (PASS == 1) {
        float v2;
        const float s = lk_pass1(D, R.uv[r], C.uv[tx], R.wx[r], C.wx[tx], two2, two3, v2);
        Dm[e] = v2;
        A[e] = s;
        if (s > mx) mx = s;
      } else if (PASS == 2) {
        const float s = lk_pass2(P.use3d_filter, i == j, R.mx[r], C.mx[tx], R.wx[r], C.wx[tx], A[e], max1);
        A[e] = s;
        if (s > mx) mx = s;
      } else {
        const float val = lk_pass3(Dm[e], A[e], max2, R.w[r], C.w[tx]);
        Dm[e] = val;
        Dm[(size_t)j * N + i] = val;
      }
    }
    if (PASS != 3) {
      for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
      }
      // (>= 0: the bit patterns order as the values do; -1 = nothing but NaN seen, and the word stays as it is)
      if ((tid & 63) == 0 && mx >= 0.f) atomicMax(PASS == 1 ? &hdr[k].max1 : &hdr[k].max2, __float_as_int(mx));
    }
  }
}

// ---- agglomeration ----
struct RmLds {
  float cache_v[LK_MAX];
  unsigned short cache_c[LK_MAX];
  unsigned short clsize[LK_MAX];
  unsigned short dirty_list[LK_MAX];
  unsigned char inlist[LK_MAX];
  float red_v[2][RM_THREADS / 64];   // the scan's per-wavefront candidates, by iteration parity
  int red_a[2][RM_THREADS / 64];
  int n_dirty, skip_next;
  float dmat[RM_DLDS * RM_DLDS];
};

// cache[a] = first maximum of row a over its listed columns b > a, by one wavefront: every lane sees its candidates in
// ascending b, so its running first maximum is exact; across lanes: larger value, then smaller column
__device__ __forceinline__ void rm_rescan_row(RmLds& L, const float* Dm, int N, int a) {
  const int lane = threadIdx.x & 63;
  const float* row = Dm + (size_t)a * N;
  float bv = -1.f;
  int bb = RM_NONE;
  for (int b = a + 1 + lane; b < N; b += 64) {
    if (!L.inlist[b]) continue;
    const float v = row[b];
    if (v > bv) {
      bv = v;
      bb = b;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int ob = __shfl_xor(bb, off);
    if (ov > bv || (ov == bv && ob < bb)) {
      bv = ov;
      bb = ob;
    }
  }
  if (lane == 0) {
    L.cache_v[a] = bv;
    L.cache_c[a] = (unsigned short)bb;
  }
}

__device__ void rm_agglomerate(RmLds& L, int N, const LinkageParams& P, float* Dm, int32_t* __restrict__ mem,
                               int32_t* __restrict__ members_out, int32_t member_base, int32_t* __restrict__ cl_start_out,
                               int32_t* __restrict__ ncl_out, int32_t* __restrict__ label_out,
                               unsigned long long* __restrict__ stats) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < N; i += RM_THREADS) {
    L.clsize[i] = 1;
    L.inlist[i] = 1;
    mem[(size_t)i * N] = i;
  }
  if (N <= RM_DLDS) {   // the rescans re-read rows of the matrix: keep it in LDS when it fits
    for (int e = tid; e < N * N; e += RM_THREADS) L.dmat[e] = Dm[e];
    Dm = L.dmat;
  }
  __syncthreads();
  for (int a = wave; a < N; a += RM_THREADS / 64) rm_rescan_row(L, Dm, N, a);
  __syncthreads();
  // ---- hierarchicalCluster (:416-540) ----
  int removeValue = -1, skip = -1;
  unsigned long long merges = 0, rescans = 0;   // (thread 0's are the ones reported)
  for (int iter = 0; iter < 2 * N + 2; ++iter) {
    const bool rv_listed = removeValue >= 0 && L.inlist[removeValue];
    // the scan: first maximum of the listed rows' caches in ascending a; rows removeValue and skip (:446-450) left out
    float bv = -1.f;
    int ba = 0x7fffffff;
    for (int a = tid; a < N; a += RM_THREADS) {
      if (!L.inlist[a] || a == removeValue || (rv_listed && a == skip)) continue;
      if (L.cache_c[a] == RM_NONE) continue;
      const float v = L.cache_v[a];
      if (v > bv) {
        bv = v;
        ba = a;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oa = __shfl_xor(ba, off);
      if (ov > bv || (ov == bv && oa < ba)) {
        bv = ov;
        ba = oa;
      }
    }
    const int par = iter & 1;
    if (lane == 0) {
      L.red_v[par][wave] = bv;
      L.red_a[par][wave] = ba;
    }
    __syncthreads();
    bv = -1.f;
    ba = 0x7fffffff;
    for (int k = 0; k < RM_THREADS / 64; ++k) {
      const float ov = L.red_v[par][k];
      const int oa = L.red_a[par][k];
      if (ov > bv || (ov == bv && oa < ba)) {
        bv = ov;
        ba = oa;
      }
    }
    if (tid == 0) {
      if (rv_listed) L.inlist[removeValue] = 0;   // erased during this scan (read again only behind the barrier below)
      L.n_dirty = 0;
      L.skip_next = 0x7fffffff;
    }
    if (bv < P.cutoff || ba == 0x7fffffff) break;
    const int first = ba, second = L.cache_c[first];
    const int S1 = L.clsize[first], S2 = L.clsize[second];
    // merge: the absorbed cluster's members are appended back to front (:493-496)
    for (int k = tid; k < S2; k += RM_THREADS) mem[(size_t)first * N + S1 + k] = mem[(size_t)second * N + (S2 - 1 - k)];
    // the linkage row update (:506-526), all reads before any write
    float nv[RM_PER];
#pragma unroll
    for (int u = 0; u < RM_PER; ++u) {
      const int i = tid + u * RM_THREADS;
      nv[u] = 0.f;
      if (i < N) {
        const float da = Dm[(size_t)first * N + i], db = Dm[(size_t)second * N + i];
        nv[u] = lk_merged_value(P.linkage_type, da, db, S1, S2, L.clsize[i] == 0 || i == second);
      }
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
      L.clsize[first] = (unsigned short)(S1 + S2);
      L.clsize[second] = 0;
    }
#pragma unroll
    for (int u = 0; u < RM_PER; ++u) {
      const int a = tid + u * RM_THREADS;
      if (a >= N) continue;
      Dm[(size_t)first * N + a] = nv[u];
      Dm[(size_t)a * N + first] = nv[u];
      if (!L.inlist[a]) continue;
      // row a's cache (its own thread's): what the delisting and the new column `first` do to it
      const int c = L.cache_c[a];
      bool dirty = a == first || (rv_listed && c == removeValue);   // (c == removeValue implies a < removeValue)
      if (a < first && !dirty) {
        const float cv = L.cache_v[a], x = nv[u];
        if (c == first) {
          if (x >= cv) L.cache_v[a] = x;
          else dirty = true;   // smaller or NaN
        } else if (x > cv || (x == cv && c != RM_NONE && first < c)) {
          L.cache_v[a] = x;
          L.cache_c[a] = (unsigned short)first;
        }
      }
      if (dirty) L.dirty_list[atomicAdd(&L.n_dirty, 1)] = (unsigned short)a;
      if (a > second) atomicMin(&L.skip_next, a);   // the next listed index after the new removeValue
    }
    __threadfence_block();
    __syncthreads();
    const int n_dirty = L.n_dirty;
    for (int k = wave; k < n_dirty; k += RM_THREADS / 64) rm_rescan_row(L, Dm, N, L.dirty_list[k]);
    removeValue = second;
    skip = L.skip_next == 0x7fffffff ? -1 : L.skip_next;
    ++merges;
    rescans += (unsigned long long)n_dirty;
    __syncthreads();
  }
  // ---- clusters with MORE than MinPts members, in index order (:530-538) ----
  __syncthreads();
  if (label_out)
    for (int i = tid; i < N; i += RM_THREADS) label_out[i] = -1;
  __syncthreads();
  if (tid == 0) {
    int ncl = 0, w = 0;
    for (int c = 0; c < N; ++c) {
      const int sz = L.clsize[c];
      if (sz <= P.min_pts) continue;
      if (cl_start_out) cl_start_out[ncl] = w;
      for (int k = 0; k < sz; ++k) {
        const int m = mem[(size_t)c * N + k];
        if (members_out) members_out[w] = member_base + m;
        if (label_out) label_out[m] = ncl;
        ++w;
      }
      ++ncl;
    }
    if (cl_start_out) cl_start_out[ncl] = w;
    *ncl_out = ncl;
    if (stats) {
      atomicAdd(&stats[0], 1ull);
      atomicAdd(&stats[1], merges);
      atomicAdd(&stats[2], rescans);
      atomicMax(&stats[3], (unsigned long long)N);
    }
  }
}

// Per-step form: the problems of the plan, one workgroup each (looped over when there are more).
__global__ __launch_bounds__(RM_THREADS) void rm_agglomerate_batch_kernel(
    const RmPlan* __restrict__ plan, const RmProblem* __restrict__ problems, LinkageParams P, float* scratch,
    int32_t* __restrict__ members, int32_t* __restrict__ cl_start, int32_t* __restrict__ ncl, int32_t* __restrict__ label,
    unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  RmLds& L = *reinterpret_cast<RmLds*>(smem);
  const int n_problems = plan->n_problems;
  for (int k = blockIdx.x; k < n_problems; k += gridDim.x) {
    const RmProblem q = problems[k];
    const size_t nn = (size_t)q.n * q.n;
    float* Dm = scratch + q.base + nn;
    int32_t* mem = reinterpret_cast<int32_t*>(Dm + nn);
    __syncthreads();   // the previous problem's LDS is done with
    rm_agglomerate(L, q.n, P, Dm, mem, members + q.b, 0, cl_start + q.b + q.p, ncl + q.p, label + q.b, stats);
  }
}

// ---- frame form ----
// The busy models (more than MinPts matches) of every frame of the launch, in (frame, model) order, from the device's
// own counts: scratch bases by linkage_models_kernel's formula with the cap of this mode (3 k^2 floats per model before,
// k = min(matches, LK_MAX)), tile and row-block ranges, the frames' ranges of the list.  A list beyond LK_MAX is cut to
// its first LK_MAX matches, one whose region does not fit is listed with n = 0 and gets no clusters; both raise the
// frame's ERR_MS_CAP.  One wavefront per frame, lanes along the models.
template <typename T>
__device__ __forceinline__ T wave_exclusive(T v, T& total) {
  const int lane = threadIdx.x & 63;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  total = __shfl(incl, 63);
  return incl - v;
}

template <bool WRITE>
__device__ void rm_plan_frame(int f, const int32_t* __restrict__ model_off, int n_models, int min_pts, size_t scratch_floats,
                              int k0, int tiles0, int rbs0, RmProblem* __restrict__ problems, RmHeader* __restrict__ hdr,
                              int32_t* __restrict__ ncl, FrameCounts* counts, int& n_busy, int& n_tiles, int& n_rbs) {
  const int lane = threadIdx.x & 63;
  int run_busy = 0, run_tiles = 0, run_rbs = 0;
  unsigned long long run_base = 0;
  for (int c0 = 0; c0 < n_models; c0 += 64) {
    const int m = c0 + lane;
    const int b = m < n_models ? model_off[m] : 0;
    const int n = m < n_models ? model_off[m + 1] - b : 0;
    const int kc = n > LK_MAX ? LK_MAX : (n < 0 ? 0 : n);
    const bool busy = m < n_models && n > min_pts;   // a cluster is only emitted with MORE than MinPts members (:537)
    unsigned long long t_base;
    const unsigned long long base = run_base + wave_exclusive<unsigned long long>(3ull * kc * kc, t_base);
    const bool fits = base + 3ull * kc * kc <= scratch_floats;
    const int eff = busy && fits ? kc : 0;
    int t_busy, t_tiles, t_rbs;
    const int e_busy = wave_exclusive<int>(busy ? 1 : 0, t_busy);
    const int e_tiles = wave_exclusive<int>(tiles_of(eff), t_tiles);
    const int e_rbs = wave_exclusive<int>((eff + RM_ROWS - 1) / RM_ROWS, t_rbs);
    if (WRITE && busy) {
      const int k = k0 + run_busy + e_busy;
      RmProblem q;
      q.b = b;
      q.n = eff;
      q.p = m;
      q.tile0 = tiles0 + run_tiles + e_tiles;
      q.rb0 = rbs0 + run_rbs + e_rbs;
      q.frame = f;
      q.base = (unsigned long long)f * scratch_floats + base;
      problems[k] = q;
      hdr[k].sigma2 = hdr[k].sigma3 = 0.f;
      hdr[k].max1 = hdr[k].max2 = __float_as_int(-1.f);
      if (n > LK_MAX || !fits) atomicOr(&counts->error, ERR_MS_CAP);
      if (eff == 0) ncl[m] = 0;
    }
    run_base += t_base;
    run_busy += t_busy;
    run_tiles += t_tiles;
    run_rbs += t_rbs;
  }
  n_busy = run_busy;
  n_tiles = run_tiles;
  n_rbs = run_rbs;
}

__global__ __launch_bounds__(RM_THREADS) void rm_plan_models_kernel(const int32_t* __restrict__ model_off0, int n_models,
                                                                    int min_pts, size_t scratch_floats, int32_t* ncl0,
                                                                    FrameCounts* counts0, FrameBatch fbx, RmPlan* plan,
                                                                    RmProblem* __restrict__ problems,
                                                                    RmHeader* __restrict__ hdr) {
  __shared__ int s_busy[MH_MAX_BATCH + 1], s_tiles[MH_MAX_BATCH + 1], s_rbs[MH_MAX_BATCH + 1];
  const int n_frames = fbx.n > 1 ? fbx.n : 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int f = wave; f < n_frames; f += RM_THREADS / 64) {
    const unsigned long long a = (unsigned long long)f * fbx.arena;
    int nb, nt, nr;
    rm_plan_frame<false>(f, frame_ptr(model_off0, a), n_models, min_pts, scratch_floats, 0, 0, 0, nullptr, nullptr, nullptr,
                         nullptr, nb, nt, nr);
    if (lane == 0) {
      s_busy[f] = nb;
      s_tiles[f] = nt;
      s_rbs[f] = nr;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // counts -> starts
    int kb = 0, kt = 0, kr = 0;
    for (int f = 0; f < n_frames; ++f) {
      const int nb = s_busy[f], nt = s_tiles[f], nr = s_rbs[f];
      s_busy[f] = kb;
      s_tiles[f] = kt;
      s_rbs[f] = kr;
      plan->fstart[f] = kb;
      kb += nb;
      kt += nt;
      kr += nr;
    }
    plan->fstart[n_frames] = kb;
    plan->n_problems = kb;
    plan->n_tiles = kt;
    plan->n_rowblocks = kr;
  }
  __syncthreads();
  for (int f = wave; f < n_frames; f += RM_THREADS / 64) {
    const unsigned long long a = (unsigned long long)f * fbx.arena;
    int nb, nt, nr;
    rm_plan_frame<true>(f, frame_ptr(model_off0, a), n_models, min_pts, scratch_floats, s_busy[f], s_tiles[f], s_rbs[f],
                        problems, hdr, frame_ptr(ncl0, a), frame_ptr(counts0, a), nb, nt, nr);
  }
}

// The agglomeration of a frame's (a batch's frames') problems and the close of the frames' CLUSTER step, as
// linkage_models_kernel does both: ONE row of workgroups, problem k of the plan's list is workgroup k modulo the grid's;
// the workgroup that finishes a frame's last problem lays the frame's cluster table out.
__global__ __launch_bounds__(RM_THREADS) void rm_agglomerate_models_kernel(
    const RmPlan* __restrict__ plan, const RmProblem* __restrict__ problems, const int32_t* __restrict__ model_off0,
    int n_models, LinkageParams P, float* scratch, int32_t* members0, int32_t* cl_start0, int32_t* ncl0, int max_clusters,
    int32_t* __restrict__ cl_model0, int32_t* __restrict__ cl_begin0, int32_t* __restrict__ cl_count0,
    int32_t* __restrict__ n_clusters_out0, int32_t* __restrict__ snap0, FrameCounts* counts0, unsigned int* ticket0,
    FrameBatch fbx, int32_t* __restrict__ feedback, unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  RmLds& L = *reinterpret_cast<RmLds*>(smem);
  __shared__ int lay_s[RM_THREADS / 64];
  const int G = (int)gridDim.x;
  const int n_frames = fbx.n > 1 ? fbx.n : 1;
  for (int f = 0; f < n_frames; ++f) {
    const unsigned long long a = (unsigned long long)f * fbx.arena;
    const int32_t* model_off = frame_ptr(model_off0, a);
    int32_t* members = frame_ptr(members0, a);
    int32_t* cl_start = frame_ptr(cl_start0, a);
    int32_t* ncl = frame_ptr(ncl0, a);
    FrameCounts* counts = frame_ptr(counts0, a);
    unsigned int* ticket = frame_ptr(ticket0, a);
    const int k_lo = plan->fstart[f], k_hi = plan->fstart[f + 1];
    const int n_busy = k_hi - k_lo;
    int mine = 0;
    for (int k = k_lo + (((int)blockIdx.x - k_lo) % G + G) % G; k < k_hi; k += G) {
      ++mine;
      const RmProblem q = problems[k];
      __syncthreads();   // the previous problem's LDS is done with
      if (q.n <= 0) continue;   // (refused by the plan: its cluster count is zero already)
      const size_t nn = (size_t)q.n * q.n;
      float* Dm = scratch + q.base + nn;
      int32_t* mem = reinterpret_cast<int32_t*>(Dm + nn);
      rm_agglomerate(L, q.n, P, Dm, mem, members + q.b, q.b, cl_start + q.b + q.p, ncl + q.p, nullptr, stats);
    }
    bool last = false;
    if (mine > 0) last = frame_work_done(ticket, (unsigned)mine, (unsigned)n_busy);
    else if (n_busy == 0) last = (int)blockIdx.x == f % G;
    if (!last) continue;   // (`last` is the same in every thread of the workgroup)
    if (threadIdx.x == 0 && feedback) feedback[f] = n_busy;   // what the next launches size their grids by
    const int min_pts = P.min_pts;
    const int k0 = layout_cluster_table(n_models, model_off, ncl, cl_start, 1, max_clusters, frame_ptr(cl_model0, a),
                                        frame_ptr(cl_begin0, a), frame_ptr(cl_count0, a), lay_s,
                                        [min_pts](int nn) { return nn > min_pts; });   // (a model without work was never clustered)
    if (threadIdx.x == 0) {
      if (k0 > max_clusters) atomicOr(&counts->error, ERR_CLUSTER_CAP);
      const int k = k0 < max_clusters ? k0 : max_clusters;
      counts->n_clusters = k;
      *frame_ptr(n_clusters_out0, a) = k;
      if (snap0) {
        snap0[4 * f] = counts->n_matches;
        snap0[4 * f + 1] = k;
      }
    }
  }
}

// aux: plan | problems | headers | nn2 | nn3 | fill weights
struct RmAux {
  RmPlan* plan;
  RmProblem* problems;
  RmHeader* hdr;
  float *nn2, *nn3, *w;
};
RmAux carve_aux(unsigned char* aux, size_t n_problems, size_t points) {
  RmAux x;
  x.plan = reinterpret_cast<RmPlan*>(aux);
  x.problems = reinterpret_cast<RmProblem*>(aux + RM_PLAN_BYTES);
  x.hdr = reinterpret_cast<RmHeader*>(x.problems + n_problems);
  x.nn2 = reinterpret_cast<float*>(x.hdr + n_problems);
  x.nn3 = x.nn2 + points;
  x.w = x.nn3 + points;
  return x;
}

// the matrix stage's launches; grids: what the host knows of the work, looped over (the kernels stride and leave early)
void launch_matrix_stage(const RmArgs& a, int g_rows, int g_prep, int g_tiles, hipStream_t s) {
  const LinkageParams& prm = a.P;
  if (prm.sigma2d == -1.f || prm.sigma3d == -1.f) hipLaunchKernelGGL(rm_nn_kernel, dim3(g_rows), dim3(RM_ROWS), 0, s, a);
  hipLaunchKernelGGL(rm_prep_kernel, dim3(g_prep), dim3(RM_ROWS), 0, s, a);
  hipLaunchKernelGGL(rm_pass_kernel<1>, dim3(g_tiles), dim3(256), 0, s, a);
  if (prm.use3d_filter) hipLaunchKernelGGL(rm_pass_kernel<2>, dim3(g_tiles), dim3(256), 0, s, a);
  hipLaunchKernelGGL(rm_pass_kernel<3>, dim3(g_tiles), dim3(256), 0, s, a);
}

template <typename K>
void set_lds(K kernel) {
  static DynLds attr;   // one per kernel (template instantiation)
  attr.ensure(kernel, sizeof(RmLds));
}

}  // namespace

size_t linkage_rowmax_aux_bytes(size_t n_problems, size_t points) {
  return RM_PLAN_BYTES + n_problems * (sizeof(RmProblem) + sizeof(RmHeader)) + 3 * points * sizeof(float) + 64;
}

void launch_linkage_rowmax_batch(const mh_corr* corr, const float* depth4, const int32_t* off, int n_problems, int total,
                                 int n_tiles, int n_rowblocks, const DepthImage& dimg, const LinkageParams& prm,
                                 float* scratch, size_t scratch_floats, int32_t* members, int32_t* cl_start, int32_t* ncl,
                                 int32_t* label, unsigned char* aux, unsigned long long* stats, hipStream_t s) {
  if (n_problems <= 0) return;
  const RmAux x = carve_aux(aux, (size_t)n_problems, (size_t)total);
  hipLaunchKernelGGL(rm_plan_batch_kernel, dim3(1), dim3(64), 0, s, off, n_problems, scratch_floats, x.plan, x.problems, x.hdr,
                     ncl);
  if (!prm.given_matrix) {
    const RmArgs a = {corr, reinterpret_cast<const float4*>(depth4), 0ull, 0, dimg, DepthMaps(), prm, x.plan, x.problems,
                      x.hdr, x.nn2, x.nn3, x.w, scratch};
    launch_matrix_stage(a, std::max(1, std::min(n_rowblocks, 4096)), std::min(n_problems, 1024),
                        std::max(1, std::min(n_tiles, 8192)), s);
  }
  set_lds(rm_agglomerate_batch_kernel);
  hipLaunchKernelGGL(rm_agglomerate_batch_kernel, dim3(std::min(n_problems, 1024)), dim3(RM_THREADS), sizeof(RmLds), s, x.plan,
                     x.problems, prm, scratch, members, cl_start, ncl, label, stats);
}

void launch_linkage_rowmax_models(const mh_corr* corr, const float* depth4, const int32_t* model_off, int n_models, int max_m,
                                  const DepthImage& dimg, const LinkageParams& prm, float* scratch, size_t scratch_floats,
                                  int32_t* members, int32_t* cl_start, int32_t* ncl, int max_clusters, int32_t* cl_model,
                                  int32_t* cl_begin, int32_t* cl_count, int32_t* n_clusters_out, int32_t* snap,
                                  FrameCounts* counts, unsigned int* ticket, hipStream_t s, int grid, const FrameBatch* batch,
                                  const DepthMaps* maps, int32_t* feedback, unsigned char* aux, unsigned long long* stats) {
  const long n_frames = batch && batch->n > 1 ? batch->n : 1;
  const FrameBatch fbx = batch ? *batch : FrameBatch();
  const RmAux x = carve_aux(aux, (size_t)n_models * n_frames, (size_t)max_m * n_frames);
  hipLaunchKernelGGL(rm_plan_models_kernel, dim3(1), dim3(RM_THREADS), 0, s, model_off, n_models, prm.min_pts, scratch_floats,
                     ncl, counts, fbx, x.plan, x.problems, x.hdr);
  const RmArgs a = {corr, reinterpret_cast<const float4*>(depth4), n_frames > 1 ? fbx.arena : 0ull, max_m, dimg,
                    (maps && n_frames > 1) ? *maps : DepthMaps(), prm, x.plan, x.problems, x.hdr, x.nn2, x.nn3, x.w, scratch};
  // the counts live on the device: fixed grids that stride over the plan's lists
  launch_matrix_stage(a, 256, 64, 1024, s);
  const long all = std::max(1L, (long)n_models * n_frames);
  const int wgs = (int)std::max(1L, grid > 0 ? std::min((long)grid, all) : std::min(all, 256L));
  set_lds(rm_agglomerate_models_kernel);
  hipLaunchKernelGGL(rm_agglomerate_models_kernel, dim3(wgs), dim3(RM_THREADS), sizeof(RmLds), s, x.plan, x.problems, model_off,
                     n_models, prm, scratch, members, cl_start, ncl, max_clusters, cl_model, cl_begin, cl_count, n_clusters_out,
                     snap, counts, ticket, fbx, feedback, stats);
}
}  // namespace mh
