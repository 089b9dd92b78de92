// Object hulls: Object::getObjectHull + getConvexHull (moped2/libmoped/include/moped.hpp:266-327,
// moped3d/libmoped/include/moped.hpp:346-422) for every object of a list, one workgroup per object, and the projected
// corners of Model::boundingBox (src/moped.cpp:107-125, src/GLOBAL_DISPLAY.hpp:197-207) beside them.
//
//   1  project the model's rows (geom.h, the form mh_project_test pins to project()); rows with camera-frame z < 0.001
//      are counted (n_behind) and left out.  The same pass reduces min / max of the rows' xyz and the projected cloud's
//      extremes in eight directions (+-x, +-y, +-(x+y), +-(x-y)).
//   2  project again and keep what is not strictly inside the octagon of those eight extreme points (form 0; form 1
//      keeps everything).  Survivors go to LDS, or -- more than HULL_CAP of them -- to global scratch.
//   3  bitonic sort by (x, y), Pt<2>::operator< (moped.hpp:102).
//   4  one lane runs the reference's chain on the sorted survivors: forward to the last point, back to the first, pops
//      while det <= 0, the determinant as the reference writes it (every operation rounded on its own).
//   5  the vertices in the reference's order: the backward half (newest first, without the first point), then the
//      forward half (newest first, without the last point).
//
// Why the prefilter keeps the hull: a point that lies strictly to the left of every edge of a closed chain of data
// points is wound around by that chain, so it lies in the interior of the cloud's hull and is no vertex of it, nor on
// its boundary.  In exact arithmetic the chain over the survivors equals the chain over everything; in float that is
// observed (tests/test_hull_cpu.py, tests/test_gpu_object_hulls.py), not proved -- DESIGN.md section 6.
#include "context.h"
#include "geom.h"
#include "hull.h"

namespace mh {

namespace {

constexpr int HULL_THREADS = 1024;
constexpr int HULL_WAVES = HULL_THREADS / 64;
constexpr int HULL_CAP = MH_HULL_LDS_POINTS;   // points the LDS path sorts: two float2 arrays of this many = 128 KB
constexpr size_t HULL_LDS_BYTES = 2 * (size_t)HULL_CAP * sizeof(float2);

// project() (moped.hpp:330-354); false: z < 0.001, where the reference returns (FLT_MAX, FLT_MAX)
__device__ __forceinline__ bool hull_project(const TM& T, const DevCam& cam, float X, float Y, float Z, float& u, float& v) {
  float wx, wy, wz, cx, cy, cz;
  tm_apply(T.r, T.t, X, Y, Z, wx, wy, wz);
  tm_apply_inv(cam.Rc, cam.tc, wx, wy, wz, cx, cy, cz);
  if ((double)cz < 0.001) return false;
  u = __fadd_rn(__fmul_rn(__fdiv_rn(cx, cz), cam.K[0]), cam.K[2]);
  v = __fadd_rn(__fmul_rn(__fdiv_rn(cy, cz), cam.K[1]), cam.K[3]);
  return true;
}

// Pt<2>::operator< (moped.hpp:102)
__device__ __forceinline__ bool pt_less(float2 a, float2 b) { return a.x != b.x ? a.x < b.x : a.y < b.y; }

// getConvexHull's determinant (moped.hpp:309): p2 the newest point, p1 below it, p0 below that
__device__ __forceinline__ float hull_det(float2 p0, float2 p1, float2 p2) {
  return __fsub_rn(__fmul_rn(__fsub_rn(p0.x, p1.x), __fsub_rn(p2.y, p1.y)),
                   __fmul_rn(__fsub_rn(p2.x, p1.x), __fsub_rn(p0.y, p1.y)));
}

// the eight directions in counter-clockwise order: the key a point has in direction d
__device__ __forceinline__ float dir_key(int d, float x, float y) {
  switch (d) {
    case 0: return x;
    case 1: return x + y;
    case 2: return y;
    case 3: return y - x;
    case 4: return -x;
    case 5: return -(x + y);
    case 6: return -y;
    default: return x - y;
  }
}

// bitonic sort of pts[0, P), P a power of two, ascending by pt_less; every thread of the workgroup
template <typename Ptr>
__device__ __forceinline__ void hull_sort(Ptr pts, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += HULL_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const float2 a = pts[i], b = pts[l];
          const bool swap = (i & k) == 0 ? pt_less(b, a) : pt_less(a, b);
          if (swap) {
            pts[i] = b;
            pts[l] = a;
          }
        }
      }
      __syncthreads();
    }
}

// The chain (moped.hpp:297-324), one lane.  pts[0, n) sorted; the forward stack goes to stk[0, fs), the backward stack
// in place to pts[n - 1], pts[n - 2] ... (before point p is pushed the stack holds at most n - 1 - p entries, so the
// push lands at an index >= p, and p itself is in a register by then).  The two entries on top stay in registers.
template <typename Ptr>
__device__ __forceinline__ void hull_chain(Ptr pts, Ptr stk, int n, int& fs_out, int& bs_out) {
  if (n <= 0) {
    fs_out = bs_out = 0;
    return;
  }
  float2 top = pts[0], below = top;
  stk[0] = top;
  int sz = 1;
  for (int p = 1; p < n; ++p) {
    const float2 q = pts[p];
    while (sz >= 2 && hull_det(below, top, q) <= 0.f) {   // (halfHull.size() > 2 with q pushed)
      --sz;
      top = below;
      if (sz >= 2) below = stk[sz - 2];
    }
    stk[sz] = q;
    below = top;
    top = q;
    ++sz;
  }
  fs_out = sz;
  if (n == 1) {   // (the loop of :300 never runs: the one point is popped at :323)
    bs_out = 1;
    return;
  }
  top = pts[n - 1];
  below = top;
  sz = 1;
  for (int p = n - 2; p >= 0; --p) {
    const float2 q = pts[p];
    while (sz >= 2 && hull_det(below, top, q) <= 0.f) {
      --sz;
      top = below;
      if (sz >= 2) below = pts[n - 1 - (sz - 2)];
    }
    pts[n - 1 - sz] = q;
    below = top;
    top = q;
    ++sz;
  }
  bs_out = sz;
}

// One object: model m at `pose`, every thread of the workgroup.  Outputs: out_nv[0] = the true vertex count (-1: the
// scratch was too small), out_nb[0] = n_behind, out_bb[16], out_xy[min(count, max_vertices)][2].
__device__ void hull_object(const HullCore& a, int m, const float* pose, int32_t* out_nv, int32_t* out_nb, float* out_bb,
                            float* out_xy, float2* scratch) {
  extern __shared__ float2 hull_lds[];   // pts [HULL_CAP] | stk [HULL_CAP]
  __shared__ float s_key[HULL_WAVES][8], s_px[HULL_WAVES][8], s_py[HULL_WAVES][8];
  __shared__ float s_box[HULL_WAVES][6];
  __shared__ int s_behind[HULL_WAVES];
  __shared__ float s_ex[8], s_ey[8], s_bb[6];
  __shared__ int s_nb, s_count, s_fs, s_bs;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();   // (a workgroup that walks several objects: the one before is through with the shared words)
  if (m < 0 || m >= a.n_models) {   // (the host checks what it knows; a frame's slot cannot hold such a model)
    if (tid == 0) {
      out_nv[0] = 0;
      out_nb[0] = 0;
    }
    if (tid < 16) out_bb[tid] = 3.402823466e+38f;
    return;
  }
  const int r0 = a.model_begin[m];
  const int rows = a.model_begin[m + 1] - r0;
  const float* const xyz = a.xyz + 3 * (size_t)r0;
  TM T;
  tm_from_pose(T, pose, pose + 4);
  const float inf = __builtin_inff();

  // ---- 1: extremes, bounding box, n_behind ----
  float key[8], px[8], py[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    key[d] = -inf;
    px[d] = py[d] = 0.f;
  }
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  int behind = 0;
  for (int i = tid; i < rows; i += HULL_THREADS) {
    const float X = xyz[3 * (size_t)i], Y = xyz[3 * (size_t)i + 1], Z = xyz[3 * (size_t)i + 2];
    lo[0] = fminf(lo[0], X), lo[1] = fminf(lo[1], Y), lo[2] = fminf(lo[2], Z);
    hi[0] = fmaxf(hi[0], X), hi[1] = fmaxf(hi[1], Y), hi[2] = fmaxf(hi[2], Z);
    float u, v;
    if (!hull_project(T, a.cam, X, Y, Z, u, v)) {
      ++behind;
      continue;
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const float k = dir_key(d, u, v);
      if (k > key[d]) key[d] = k, px[d] = u, py[d] = v;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const float k = __shfl_xor(key[d], off), x = __shfl_xor(px[d], off), y = __shfl_xor(py[d], off);
      if (k > key[d]) key[d] = k, px[d] = x, py[d] = y;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], off));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off));
    }
    behind += __shfl_xor(behind, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) s_key[wave][d] = key[d], s_px[wave][d] = px[d], s_py[wave][d] = py[d];
#pragma unroll
    for (int c = 0; c < 3; ++c) s_box[wave][c] = lo[c], s_box[wave][3 + c] = hi[c];
    s_behind[wave] = behind;
  }
  if (tid == 0) s_count = 0;
  __syncthreads();
  if (tid < 8) {
    float k = s_key[0][tid], x = s_px[0][tid], y = s_py[0][tid];
    for (int w = 1; w < HULL_WAVES; ++w)
      if (s_key[w][tid] > k) k = s_key[w][tid], x = s_px[w][tid], y = s_py[w][tid];
    s_ex[tid] = x;
    s_ey[tid] = y;
  } else if (tid < 14) {
    const int c = tid - 8;
    float v = s_box[0][c];
    for (int w = 1; w < HULL_WAVES; ++w) v = c < 3 ? fminf(v, s_box[w][c]) : fmaxf(v, s_box[w][c]);
    s_bb[c] = v;
  } else if (tid == 14) {
    int nb = 0;
    for (int w = 0; w < HULL_WAVES; ++w) nb += s_behind[w];
    s_nb = nb;
  }
  __syncthreads();
  const int n_behind = s_nb;
  const int n_front = rows - n_behind;

  // the bounding box's corners in the order [x][y][z] of GLOBAL_DISPLAY.hpp:198-203 (a model without rows keeps the
  // reference's initial box, moped.cpp:107-108)
  if (tid < 8) {
    const int bx = tid >> 2, by = (tid >> 1) & 1, bz = tid & 1;
    const float X = rows > 0 ? s_bb[3 * bx] : (bx ? -10E10f : 10E10f);
    const float Y = rows > 0 ? s_bb[3 * by + 1] : (by ? -10E10f : 10E10f);
    const float Z = rows > 0 ? s_bb[3 * bz + 2] : (bz ? -10E10f : 10E10f);
    float u = 3.402823466e+38f, v = 3.402823466e+38f;
    hull_project(T, a.cam, X, Y, Z, u, v);
    out_bb[2 * tid] = u;
    out_bb[2 * tid + 1] = v;
  }
  if (tid == 0) out_nb[0] = n_behind;

  // ---- 2: the octagon's edges, the survivors ----
  // edge e: from extreme e to extreme e + 1; a point is dropped when it is left of every edge that has a length, by
  // more than the margin (no such edge: every point is the same point, and all are kept)
  float ex[8], ey[8], dx[8], dy[8];
  bool live[8];
  int n_live = 0;
  float span = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ex[e] = s_ex[e], ey[e] = s_ey[e];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    dx[e] = ex[(e + 1) & 7] - ex[e];
    dy[e] = ey[(e + 1) & 7] - ey[e];
    live[e] = dx[e] != 0.f || dy[e] != 0.f;
    n_live += live[e] ? 1 : 0;
  }
  span = fmaxf(ex[0] - ex[4], ey[2] - ey[6]);
  const float margin = 1e-4f * span * span;
  const bool filter = a.form == 0 && n_front > 0 && n_live > 0 && margin < inf && margin == margin;

  float2* const lds_pts = hull_lds;
  float2* const lds_stk = hull_lds + HULL_CAP;
  // pass: 0 = into LDS while there is room (and count), 1 = into global scratch (only when the count exceeded the room)
  bool global_path = false;
  float2* g_pts = nullptr;
  float2* g_stk = nullptr;
  int P = 1;
  for (int pass = 0; pass < 2; ++pass) {
    for (int base = 0; base < rows; base += HULL_THREADS) {   // (uniform trip count: the ballots below need every lane)
      const int i = base + tid;
      bool keep = false;
      float u = 0.f, v = 0.f;
      if (i < rows) {
        keep = hull_project(T, a.cam, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], u, v);
        if (keep && filter) {
          bool inside = true;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float cr = dx[e] * (v - ey[e]) - dy[e] * (u - ex[e]);
            if (live[e] && !(cr > margin)) inside = false;
          }
          keep = !inside;
        }
      }
      const unsigned long long mask = __ballot(keep);
      int wbase = 0;
      if (lane == 0 && mask) wbase = atomicAdd(&s_count, __popcll(mask));
      wbase = __shfl(wbase, 0);
      if (keep) {
        const int pos = wbase + __popcll(mask & ((1ull << lane) - 1ull));
        if (pass == 0) {
          if (pos < HULL_CAP) lds_pts[pos] = make_float2(u, v);
        } else if (pos < rows)
          g_pts[pos] = make_float2(u, v);
      }
    }
    __syncthreads();
    const int n = s_count;
    if (pass == 1 || n <= HULL_CAP) break;
    size_t need = 1;   // hull_scratch_points(rows): the host sizes the scratch from the models' rows
    while (need < (size_t)rows) need <<= 1;
    need += (size_t)rows;
    if (!scratch || need > a.scratch_stride) {
      if (tid == 0) out_nv[0] = -1;
      return;
    }
    global_path = true;
    g_pts = scratch;
    __syncthreads();
    if (tid == 0) s_count = 0;
    __syncthreads();
  }
  const int n = s_count;
  while (P < n) P <<= 1;
  if (global_path) g_stk = g_pts + P;

  // ---- 3: sort (padding: +inf pairs, which sort behind every point and are never read) ----
  if (global_path) {
    for (int i = n + tid; i < P; i += HULL_THREADS) g_pts[i] = make_float2(inf, inf);
    __syncthreads();
    hull_sort(g_pts, P);
  } else {
    for (int i = n + tid; i < P; i += HULL_THREADS) lds_pts[i] = make_float2(inf, inf);
    __syncthreads();
    hull_sort(lds_pts, P);
  }

  // ---- 4: the chain ----
  if (tid == 0) {
    int fs = 0, bs = 0;
    if (global_path) hull_chain(g_pts, g_stk, n, fs, bs);
    else hull_chain(lds_pts, lds_stk, n, fs, bs);
    s_fs = fs;
    s_bs = bs;
  }
  __syncthreads();

  // ---- 5: the vertices ----
  const int fs = s_fs, bs = s_bs;
  const int nb_v = max(bs - 1, 0), nf_v = max(fs - 1, 0);
  const int nv = nb_v + nf_v;
  if (tid == 0) out_nv[0] = nv;
  const int n_out = min(nv, a.max_vertices);
  for (int i = tid; i < n_out; i += HULL_THREADS) {
    float2 p;
    if (i < nb_v) {
      const int k = bs - 2 - i;   // backward stack entry k lies at pts[n - 1 - k]
      p = global_path ? g_pts[n - 1 - k] : lds_pts[n - 1 - k];
    } else {
      const int k = fs - 2 - (i - nb_v);
      p = global_path ? g_stk[k] : lds_stk[k];
    }
    out_xy[2 * (size_t)i] = p.x;
    out_xy[2 * (size_t)i + 1] = p.y;
  }
}

// mh_object_hulls: workgroup o = object o of the list
__global__ __launch_bounds__(HULL_THREADS) void hull_kernel(HullArgs a) {
  const int o = blockIdx.x;
  int n_obj = a.n_obj;
  if (a.n_obj_dev) n_obj = min(max(*a.n_obj_dev, 0), a.n_obj);
  if (o >= n_obj) return;
  hull_object(a.core, a.obj_model[o], a.obj_pose + 7 * (size_t)o, a.n_vertices + o, a.n_behind + o, a.bbox_uv + 16 * (size_t)o,
              a.hull_xy + 2 * (size_t)o * a.core.max_vertices, a.core.scratch ? a.core.scratch + (size_t)o * a.core.scratch_stride : nullptr);
}

// Frames: workgroup (x, f) walks the objects x, x + gridDim.x ... of result slot first_slot + f and writes their records
// {n_vertices, n_behind, corners [8][2], vertices [max_vertices][2]} into the slot of the hull block
__global__ __launch_bounds__(HULL_THREADS) void hull_frame_kernel(HullFrameArgs a) {
  const int slot = a.first_slot + blockIdx.y;
  const unsigned char* const result = a.result + (size_t)slot * a.result_bytes;
  const int n = min(max(*reinterpret_cast<const int32_t*>(result), 0), a.max_objects);
  const mh_object* const obj = reinterpret_cast<const mh_object*>(result + 16);
  HullCore core = a.core;
  if (a.cams) core.cam = a.cams[a.image];
  const size_t rec = hull_record_words(core.max_vertices);
  float2* const scratch = core.scratch ? core.scratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * core.scratch_stride : nullptr;
  for (int o = blockIdx.x; o < n; o += gridDim.x) {
    int32_t* const r = reinterpret_cast<int32_t*>(a.block + (size_t)slot * a.slot_bytes) + (size_t)o * rec;
    hull_object(core, obj[o].model, obj[o].pose, r, r + 1, reinterpret_cast<float*>(r + 2), reinterpret_cast<float*>(r + 18), scratch);
  }
}

DynLds hull_lds_attr, hull_frame_lds_attr;

}  // namespace

size_t hull_scratch_points(int rows) {
  if (rows <= HULL_CAP) return 0;
  size_t P = 1;
  while (P < (size_t)rows) P <<= 1;
  return P + (size_t)rows;
}

void launch_object_hulls(const HullArgs& a, hipStream_t s) {
  if (a.n_obj <= 0) return;
  hull_lds_attr.ensure(hull_kernel, HULL_LDS_BYTES);
  hipLaunchKernelGGL(hull_kernel, dim3(a.n_obj), dim3(HULL_THREADS), HULL_LDS_BYTES, s, a);
}

void launch_frame_hulls(const HullFrameArgs& a, int n_frames, hipStream_t s) {
  hull_frame_lds_attr.ensure(hull_frame_kernel, HULL_LDS_BYTES);
  hipLaunchKernelGGL(hull_frame_kernel, dim3(HULL_FRAME_GRID, n_frames), dim3(HULL_THREADS), HULL_LDS_BYTES, s, a);
}

}  // namespace mh
