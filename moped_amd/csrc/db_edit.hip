// Edits of the resident model database: add, replace, remove one model (moped.cpp:139-159) without starting over.
//
// All three are one splice of the row array, new = old[0, b) ++ rows ++ old[e, N), with the model ids behind the splice
// point shifted by +1, 0 or -1.  An edit never works in place -- other contexts (frames in flight) read the live arrays --
// it fills a second buffer set and the editing context flips to it; the contexts that share the old set keep it until
// they adopt the new one (mh_db_adopt), stream ordered, with no host wait.  What an edit leaves is, byte for byte, what
// mh_db_upload_raw makes of the same rows: the new rows' norm terms come from the upload's own launches, moved rows keep
// theirs, the f16 image is the same conversion of the same floats, and the aggregates (dmax, spread, the zero query's
// answer, usable) are recomputed over all rows by the upload's kernels, never patched -- removing a model can lower any
// of them.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "context.h"
#include "steps.h"
#include "view_check.h"

using namespace mh;

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
constexpr int DB_DD = 192;   // floats per 128-row tile of the -dd/2 array (SC_DD of screen_int.h; checked in alloc_set)

struct SpliceArgs {
  const float* old_desc;   // the live set
  const float* old_norm;
  const float* old_xyz;
  const int32_t* old_model;
  const float* new_desc;   // the staged rows
  const float* new_norm;
  const float* new_xyz;
  float* desc;             // the set being filled
  float* norm;
  float* xyz;
  int32_t* model;
  _Float16* dbh;           // nullptr: the result has no f16 image
  float* dneg;
  unsigned int* stats;
  int N;                   // rows of the result
  int b, n_rows;           // the staged rows become rows [b, b + n_rows)
  int shift;               // rows behind them come from old row r - shift
  int model_id, model_delta;   // model of the staged rows; what the models behind them move by
  size_t n_chunks;         // 8-float chunks of the result's padded extent
};

// One pass over the destination, shaped like db_to_half_kernel (screen_db.hip): one 8-float chunk per thread step,
// grid-strided; the f32 chunk is read once and written twice (f32, f16), chunk 0 of a row carries the row's scalars.
__global__ __launch_bounds__(256) void db_splice_kernel(const SpliceArgs a) {
  __shared__ unsigned int red[3];
  if (threadIdx.x < 3) red[threadIdx.x] = 0;
  __syncthreads();
  float x_max = 0.f, dd_max = 0.f;
  unsigned int bad = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_chunks; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i >> 4);
    const int c = (int)(i & 15);
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    const bool real = row < a.N;
    const bool staged = real && row >= a.b && row < a.b + a.n_rows;
    const int src = staged ? row - a.b : (row < a.b ? row : row - a.shift);
    if (real) {
      const float4* p = reinterpret_cast<const float4*>((staged ? a.new_desc : a.old_desc) + (size_t)src * DIM) + 2 * c;
      lo = p[0];
      hi = p[1];
    }
    reinterpret_cast<float4*>(a.desc)[2 * i] = lo;
    reinterpret_cast<float4*>(a.desc)[2 * i + 1] = hi;
    if (a.dbh) {
      half8 h;
      h[0] = (_Float16)lo.x; h[1] = (_Float16)lo.y; h[2] = (_Float16)lo.z; h[3] = (_Float16)lo.w;
      h[4] = (_Float16)hi.x; h[5] = (_Float16)hi.y; h[6] = (_Float16)hi.z; h[7] = (_Float16)hi.w;
      reinterpret_cast<half8*>(a.dbh)[i] = h;
    }
    if (c == 0) {
      // padding rows: +inf norm term, -inf -dd/2 (a reused set holds an older generation's rows there)
      const float dd = real ? (staged ? a.new_norm : a.old_norm)[src] : __builtin_inff();
      a.norm[row] = dd;
      if (a.dbh) a.dneg[(size_t)(row >> 7) * DB_DD + (row & 127)] = -0.5f * dd;
      if (real) {
        const float* x = (staged ? a.new_xyz : a.old_xyz) + (size_t)src * 3;
        a.xyz[(size_t)row * 3] = x[0];
        a.xyz[(size_t)row * 3 + 1] = x[1];
        a.xyz[(size_t)row * 3 + 2] = x[2];
        a.model[row] = staged ? a.model_id : a.old_model[src] + (row < a.b ? 0 : a.model_delta);
        if (!(dd >= 0.f) || dd == __builtin_inff()) bad = 1;
        else dd_max = fmaxf(dd_max, dd);
      }
    }
    if (real)   // (fmaxf drops NaNs: a NaN coordinate shows in the row's norm term)
      x_max = fmaxf(x_max, fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(lo.w))),
                                 fmaxf(fmaxf(fabsf(hi.x), fabsf(hi.y)), fmaxf(fabsf(hi.z), fabsf(hi.w)))));
  }
  if (!a.dbh) return;   // (uniform: no image, no statistics)
  // non-negative floats order like their bit patterns
  atomicMax(&red[0], __float_as_uint(dd_max));
  atomicMax(&red[1], __float_as_uint(x_max));
  if (bad) atomicOr(&red[2], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMax(&a.stats[0], red[0]);
    atomicMax(&a.stats[1], red[1]);
    if (red[2]) atomicOr(&a.stats[2], 1u);
  }
}

// the copy route's model ids: rows [first, N) move by delta
__global__ void db_model_shift_kernel(int32_t* __restrict__ model, int first, int N, int delta, int fill_first, int fill_n,
                                      int model_id) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  if (r >= fill_first && r < fill_first + fill_n) model[r] = model_id;
  else if (r >= first) model[r] += delta;
}

const char* why_not_editable(const DbStore* st) {
  if (!st) return nullptr;   // no store = an empty one
  if (!st->grouped) return "the rows of the store are not grouped by model in ascending order";
  if (st->n_blocks > 1) return "the store was uploaded in blocks (a sharded store is not editable)";
  if (st->index_base != 0) return "the store's index_base is not 0 (a sharded store is not editable)";
  return nullptr;
}

int refuse(mh_ctx* ctx, const char* who, const char* why) {
  ctx->err = std::string(who) + ": " + why;
  return MH_ERR_ARG;
}

// a buffer set for cap_rows rows (a multiple of 128), with the f16 image's arrays when a store of that many rows can have one
int alloc_set(mh_ctx* ctx, size_t cap_rows, std::shared_ptr<DbStore>& out) {
  if (screen_dneg_elems(128) != (size_t)DB_DD) {
    ctx->err = "db_edit: the -dd/2 array's tile pitch has changed";
    return MH_ERR_HIP;
  }
  std::shared_ptr<DbStore> st = make_store(ctx->device);
  cap_rows = std::max<size_t>(cap_rows, 128);
  hipStream_t s = ctx->stream;   // (a fresh set: nothing to wait for)
  MH_HIP(ctx, st->desc.ensure(cap_rows * DIM, s));
  MH_HIP(ctx, st->norm.ensure(cap_rows, s));
  MH_HIP(ctx, st->xyz.ensure(cap_rows * 3, s));
  MH_HIP(ctx, st->model.ensure(cap_rows, s));
  st->cap = cap_rows;
  if (screen_wanted(1 << 30, (int)cap_rows)) {
    MH_HIP(ctx, st->desc_h.ensure(screen_db_half_elems((int)cap_rows), s));
    MH_HIP(ctx, st->neg_h.ensure(screen_dneg_elems((int)cap_rows), s));
    st->cap_h = screen_db_half_elems((int)cap_rows);
    MH_HIP(ctx, st->stats.ensure(8, s));
  }
  MH_HIP(ctx, hipEventCreateWithFlags(&st->ready, hipEventDisableTiming));
  st->pool = ctx->pool;
  out = std::move(st);
  return MH_OK;
}

bool set_fits(const DbStore* st, size_t n_pad, bool image) {
  return st->cap >= n_pad && (!image || (st->cap_h >= n_pad * DIM && st->stats)) && st->ready;
}

// the set the next edit fills: the pool's spare when it is large enough, else a fresh one (a spare that is too small is
// freed first -- that free stalls the device)
int take_set(mh_ctx* ctx, size_t n_pad, bool image, std::shared_ptr<DbStore>& out) {
  DbStore* spare = nullptr;
  size_t cap_rows = 0;
  {
    std::lock_guard<std::mutex> lock(ctx->pool->mu);
    spare = ctx->pool->spare;
    ctx->pool->spare = nullptr;
    cap_rows = ctx->pool->cap_rows;
  }
  if (spare && !spare->ready && hipEventCreateWithFlags(&spare->ready, hipEventDisableTiming) != hipSuccess) spare->ready = nullptr;
  if (spare && set_fits(spare, n_pad, image)) {
    spare->pool = ctx->pool;
    out = std::shared_ptr<DbStore>(spare, retire_store);
    return MH_OK;
  }
  delete spare;
  return alloc_set(ctx, std::max(n_pad, cap_rows), out);
}

// rows the staging block holds: descriptors, norm terms and coordinates lie at that pitch one after the other
size_t stage_rows(const mh_ctx* ctx) { return ctx->db_stage.cap / (DIM + 1 + 3); }

int ensure_stage(mh_ctx* ctx, size_t rows) {
  if (rows <= stage_rows(ctx)) return MH_OK;
  const size_t cap = std::max<size_t>(rows + rows / 4, 4096);
  MH_HIP(ctx, ctx->db_stage.ensure(cap * (DIM + 1 + 3), ctx->stream));
  return MH_OK;
}

// The pass over the rows of an edit + the aggregates + the flip.  b, e: the old rows [b, e) leave; the n_rows staged rows
// take their place as model `model_id`; the models of the rows behind them move by model_delta; `table` = the new
// per-model row ranges.
int run_splice(mh_ctx* ctx, int b, int e, int n_rows, int model_id, int model_delta, std::vector<int32_t> table) {
  const DbStore* old = ctx->store.get();
  const int N_old = old ? old->N : 0;
  const long long N_ll = (long long)N_old - (e - b) + n_rows;
  if (N_ll > 0x7FFFFF00ll) {
    ctx->err = "mh_db_splice: more than 2^31 - 256 rows";
    return MH_ERR_CAPACITY;
  }
  const int N = (int)N_ll;
  const size_t n_pad = ((size_t)N + 127) / 128 * 128;
  const bool image = N > 0 && screen_wanted(1 << 30, N);
  if (!ctx->pool) ctx->pool = std::make_shared<DbPool>();
  std::shared_ptr<DbStore> st;
  int rc = take_set(ctx, n_pad, image, st);
  if (rc) return rc;
  st->N = 0;
  st->screen = ScreenDb();
  st->n_blocks = 0;
  st->index_base = 0;
  const float* stage = ctx->db_stage;
  const float* stage_norm = stage ? stage + stage_rows(ctx) * DIM : nullptr;
  const float* stage_xyz = stage ? stage_norm + stage_rows(ctx) : nullptr;
  const bool timed = ctx->timing;
  if (timed)
    for (hipEvent_t& ev : ctx->db_ev)
      if (!ev) MH_HIP(ctx, hipEventCreate(&ev));
  ctx->db_ev_valid = false;
  if (N > 0) {
    if (image) MH_HIP(ctx, hipMemsetAsync(st->stats, 0, 8 * sizeof(unsigned int), ctx->stream));
    if (timed) MH_HIP(ctx, hipEventRecord(ctx->db_ev[0], ctx->stream));
    if (ctx->db_edit_route == 0) {
      SpliceArgs a;
      a.old_desc = old ? old->desc : nullptr;
      a.old_norm = old ? old->norm : nullptr;
      a.old_xyz = old ? old->xyz : nullptr;
      a.old_model = old ? old->model : nullptr;
      a.new_desc = stage;
      a.new_norm = stage_norm;
      a.new_xyz = stage_xyz;
      a.desc = st->desc;
      a.norm = st->norm;
      a.xyz = st->xyz;
      a.model = st->model;
      a.dbh = image ? st->desc_h : nullptr;
      a.dneg = image ? st->neg_h : nullptr;
      a.stats = st->stats;
      a.N = N;
      a.b = b;
      a.n_rows = n_rows;
      a.shift = n_rows - (e - b);
      a.model_id = model_id;
      a.model_delta = model_delta;
      a.n_chunks = n_pad * (DIM / 8);
      const unsigned blocks = (unsigned)std::min<size_t>((a.n_chunks + 255) / 256, 2048);
      hipLaunchKernelGGL(db_splice_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a);
    } else {
      // the route the fused pass is measured against: device copies of the three runs of every array, then the upload's
      // own preparation of the f16 image
      const size_t tail = (size_t)N_old - e;   // old rows [e, N_old) -> new rows [b + n_rows, N)
      auto runs = [&](void* dst, const void* src_old, const void* src_new, size_t row_bytes) -> hipError_t {
        hipError_t err = hipSuccess;
        if (b > 0) err = hipMemcpyAsync(dst, src_old, (size_t)b * row_bytes, hipMemcpyDeviceToDevice, ctx->stream);
        if (err == hipSuccess && n_rows > 0)
          err = hipMemcpyAsync((char*)dst + (size_t)b * row_bytes, src_new, (size_t)n_rows * row_bytes, hipMemcpyDeviceToDevice, ctx->stream);
        if (err == hipSuccess && tail > 0)
          err = hipMemcpyAsync((char*)dst + ((size_t)b + n_rows) * row_bytes, (const char*)src_old + (size_t)e * row_bytes,
                               tail * row_bytes, hipMemcpyDeviceToDevice, ctx->stream);
        return err;
      };
      MH_HIP(ctx, runs(st->desc, old ? old->desc : nullptr, stage, DIM * sizeof(float)));
      MH_HIP(ctx, runs(st->norm, old ? old->norm : nullptr, stage_norm, sizeof(float)));
      MH_HIP(ctx, runs(st->xyz, old ? old->xyz : nullptr, stage_xyz, 3 * sizeof(float)));
      if (b > 0) MH_HIP(ctx, hipMemcpyAsync(st->model, old->model, (size_t)b * 4, hipMemcpyDeviceToDevice, ctx->stream));
      if (tail > 0)
        MH_HIP(ctx, hipMemcpyAsync(st->model + b + n_rows, old->model + e, tail * 4, hipMemcpyDeviceToDevice, ctx->stream));
      hipLaunchKernelGGL(db_model_shift_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, st->model, b + n_rows, N,
                         model_delta, b, n_rows, model_id);
      if (n_pad > (size_t)N) {
        MH_HIP(ctx, hipMemsetAsync(st->desc + (size_t)N * DIM, 0, (n_pad - N) * DIM * sizeof(float), ctx->stream));
        MH_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)(st->norm + N), 0x7F800000, n_pad - N, ctx->stream));
      }
      if (image) launch_db_to_half(st->desc, st->norm, N, st->desc_h, st->neg_h, st->stats, ctx->stream);
    }
    if (timed) MH_HIP(ctx, hipEventRecord(ctx->db_ev[1], ctx->stream));
    if (image && ctx->db_edit_route == 0) launch_db_aggregates(st->norm, N, st->neg_h, st->stats, ctx->stream);
    MH_HIP(ctx, hipGetLastError());
  }
  // the new per-model row ranges on the device (hull.hip), sized for the reserved model count so that a spare set keeps its block
  MH_HIP(ctx, st->model_begin_dev.ensure(std::max(table.size(), (size_t)ctx->pool->max_models + 1), ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(st->model_begin_dev, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(ctx, hipEventRecord(st->ready, ctx->stream));
  // the only host wait: the statistics words (the upload path waits for the same read-back).  It also means that this
  // context's frames on the old set have finished, so the old set may become the spare when its other holders let go.
  unsigned int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (image) MH_HIP(ctx, hipMemcpyAsync(h, st->stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (image) screen_from_stats(st.get(), h);
  ctx->db_ev_valid = timed && N > 0;
  st->N = N;
  st->n_models = (int)table.size() - 1;
  st->grouped = true;
  st->model_begin = std::move(table);
  st->generation = (old ? old->generation : 0) + 1;
  // flip: contexts that share the old set keep it; it parks in the pool when the last of them lets go
  std::shared_ptr<DbStore> prev = std::move(ctx->store);
  if (prev && !prev->pool) prev->pool = ctx->pool;
  ctx->store = std::move(st);
  bind_store(ctx);
  return MH_OK;
}

}  // namespace

namespace mh {

void db_poll_held(mh_ctx* ctx, bool wait) {
  size_t keep = 0;
  for (size_t i = 0; i < ctx->held.size(); ++i) {
    mh_ctx::HeldStore& h = ctx->held[i];
    bool done = true;
    if (h.done) {
      if (wait) hipEventSynchronize(h.done);
      else if (hipEventQuery(h.done) == hipErrorNotReady) {
        (void)hipGetLastError();   // (not an error: the runtime remembers it as one)
        done = false;
      }
    }
    if (done) {
      if (h.done) ctx->held_events.push_back(h.done);
      h.store.reset();
    } else {
      if (keep != i) ctx->held[keep] = std::move(h);
      ++keep;
    }
  }
  ctx->held.resize(keep);
}

}  // namespace mh

extern "C" {

int mh_db_model_rows(const mh_ctx* ctx, int model, int32_t* row_begin, int32_t* n_rows) {
  if (!ctx) return MH_ERR_ARG;
  mh_ctx* c = const_cast<mh_ctx*>(ctx);
  const DbStore* st = ctx->store.get();
  if (!st || !st->grouped) return refuse(c, "mh_db_model_rows", "the rows of the store are not grouped by model in ascending order");
  if (model < 0 || model >= st->n_models) return refuse(c, "mh_db_model_rows", "model index out of range");
  if (row_begin) *row_begin = st->model_begin[model];
  if (n_rows) *n_rows = st->model_begin[model + 1] - st->model_begin[model];
  return MH_OK;
}

int mh_db_generation(const mh_ctx* ctx, uint64_t* generation) {
  if (!ctx || !generation) return MH_ERR_ARG;
  *generation = ctx->store ? ctx->store->generation : 0;
  return MH_OK;
}

// what every edit checks before anything is launched: the operation, an editable store, the model index, room for one more
static int check_edit(mh_ctx* ctx, const char* who, int op, int model, int n_new = 1) {
  if (op < MH_DB_INSERT || op > MH_DB_REMOVE) return refuse(ctx, who, "unknown operation");
  const DbStore* old = ctx->store.get();
  if (const char* why = why_not_editable(old)) return refuse(ctx, who, why);
  const int nm = old ? old->n_models : 0;
  if (op == MH_DB_INSERT ? (model < 0 || model > nm) : (model < 0 || model >= nm))
    return refuse(ctx, who, nm == 0 && op != MH_DB_INSERT ? "model index out of range (the store is empty)"
                                                           : "model index out of range");
  if (op == MH_DB_INSERT && nm + n_new > MH_MAX_MODELS) {
    ctx->err = std::string(who) + ": more than MH_MAX_MODELS models";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

// the edit of a checked (op, model) whose n_rows new rows lie in the staging block with their norm terms
static int splice_staged(mh_ctx* ctx, int op, int model, int n_rows) {
  const DbStore* old = ctx->store.get();
  const int nm = old ? old->n_models : 0;
  // the rows that leave, [b, e), and the new per-model table
  static const std::vector<int32_t> none(1, 0);
  const std::vector<int32_t>& begin = old ? old->model_begin : none;   // [nm + 1]
  const int b = begin[model];
  const int e = op == MH_DB_INSERT ? b : begin[model + 1];
  const int shift = n_rows - (e - b);
  const int delta = op == MH_DB_INSERT ? 1 : op == MH_DB_REMOVE ? -1 : 0;
  std::vector<int32_t> table(begin.begin(), begin.begin() + model + 1);   // models up to `model` begin where they began
  if (op == MH_DB_INSERT) table.push_back(b + n_rows);                     // the model that was `model`, behind the new rows
  for (int m = model + (op == MH_DB_REMOVE ? 2 : 1); m <= nm; ++m) table.push_back(begin[m] + shift);
  return run_splice(ctx, b, e, n_rows, model, delta, std::move(table));
}

// the edit of a checked model whose n_rows new rows (staged) go behind its last row: old[0, e) ++ rows ++ old[e, N)
static int append_staged(mh_ctx* ctx, int model, int n_rows) {
  const DbStore* old = ctx->store.get();   // (checked: the model exists, so there is a store)
  const int e = old->model_begin[model + 1];
  std::vector<int32_t> table = append_table(old->model_begin, model, n_rows);
  return run_splice(ctx, e, e, n_rows, model, 0, std::move(table));
}

// the new rows of mh_db_splice / mh_db_append into the staging block: their norm terms by the upload's own launches, so
// that their bits are the upload's by construction
static int stage_given_rows(mh_ctx* ctx, const float* desc, const float* xyz, int n_rows, int normalize, int on_device) {
  if (n_rows <= 0) return MH_OK;
  int rc = ensure_stage(ctx, (size_t)n_rows);
  if (rc) return rc;
  float* sd = ctx->db_stage;
  float* sn = sd + stage_rows(ctx) * DIM;
  float* sx = sn + stage_rows(ctx);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  MH_HIP(ctx, hipMemcpyAsync(sd, desc, (size_t)n_rows * DIM * sizeof(float), kind, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(sx, xyz, (size_t)n_rows * 3 * sizeof(float), kind, ctx->stream));
  if (normalize) launch_normalize(sd, sn, n_rows, ctx->stream);
  else launch_row_norms(sd, sn, n_rows, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_db_splice(mh_ctx* ctx, int op, int model, const float* desc, const float* xyz, int n_rows, int normalize,
                 int on_device) {
  if (!ctx) return MH_ERR_ARG;
  if (op < MH_DB_INSERT || op > MH_DB_REMOVE) return refuse(ctx, "mh_db_splice", "unknown operation");
  if (op == MH_DB_REMOVE) n_rows = 0;
  if (n_rows < 0 || (n_rows > 0 && (!desc || !xyz))) return refuse(ctx, "mh_db_splice", "bad argument");
  if (int rc = check_edit(ctx, "mh_db_splice", op, model)) return rc;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  if (int rc = stage_given_rows(ctx, desc, xyz, n_rows, normalize, on_device)) return rc;
  return splice_staged(ctx, op, model, n_rows);
}

int mh_db_append(mh_ctx* ctx, int model, const float* desc, const float* xyz, int n_rows, int normalize, int on_device) {
  if (!ctx) return MH_ERR_ARG;
  if (n_rows < 0 || (n_rows > 0 && (!desc || !xyz))) return refuse(ctx, "mh_db_append", "bad argument");
  if (int rc = check_edit(ctx, "mh_db_append", MH_DB_REPLACE, model)) return rc;   // (REPLACE's check: an existing model)
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  if (int rc = stage_given_rows(ctx, desc, xyz, n_rows, normalize, on_device)) return rc;
  return append_staged(ctx, model, n_rows);
}

// ---- planar models from images: createPlanarModelsFromImages (moped.cpp:196-236) into the resident store ------------
namespace {

// the images, sizes and host row arrays of every call that teaches from images, checked before anything is launched
int check_images_call(mh_ctx* ctx, const char* who, const uint8_t* const* gray_dev, int n_images, int width, int height,
                      int max_keypoints, const float* rows_desc_host, const float* rows_xyz_host, int rows_cap) {
  if (!gray_dev || n_images <= 0 || n_images > MH_MAX_BATCH || width <= 0 || height <= 0 || max_keypoints <= 0 ||
      (rows_desc_host == nullptr) != (rows_xyz_host == nullptr) || (rows_desc_host && rows_cap <= 0))
    return refuse(ctx, who, "bad argument");
  for (int i = 0; i < n_images; ++i)
    if (!gray_dev[i]) return refuse(ctx, who, "bad argument (a null image)");
  return MH_OK;
}

// the arguments mh_db_splice_image[s] share
int check_planar_call(mh_ctx* ctx, const char* who, const uint8_t* const* gray_dev, int n_images, int width, int height,
                      int max_keypoints, const mh_planar_spec* spec, const float* rows_desc_host, const float* rows_xyz_host,
                      int rows_cap, int* all) {
  if (int rc = check_images_call(ctx, who, gray_dev, n_images, width, height, max_keypoints, rows_desc_host, rows_xyz_host, rows_cap))
    return rc;
  if (int rc = planar_spec_check(ctx, who, spec, all)) return rc;
  if (ctx->und_on && (spec->K[0] == 0.f || spec->K[1] == 0.f)) return refuse(ctx, who, "undistortion is on and fx or fy is 0");
  return MH_OK;
}

int ensure_planar(mh_ctx* ctx, int n_images, int cap, bool rows) {
  mh_ctx::Planar& p = ctx->planar;
  const size_t n = (size_t)n_images * cap;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, p.desc.ensure(n * DIM, s));
  MH_HIP(ctx, p.xy.ensure(n * 2, s));
  MH_HIP(ctx, p.words.ensure(6 * MH_MAX_BATCH, s));
  MH_HIP(ctx, p.box.ensure(6 * MH_MAX_BATCH, s));
  if (rows) {
    MH_HIP(ctx, p.rows_desc.ensure(n * DIM, s));
    MH_HIP(ctx, p.rows_xyz.ensure(n * 3, s));
  }
  return MH_OK;
}

// [UNDISTORTED_IMAGE] -> FEAT of n images into ctx->planar (counts in words[0 .. n)), FEAT's counter words behind the
// kept counts (words[2 B + 4 i ..])
int planar_feat(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int width, int height, int double_size, int cap,
                const float K[4]) {
  mh_ctx::Planar& p = ctx->planar;
  const uint8_t* staged[MH_MAX_BATCH];
  int rc;
  if (ctx->und_on) {
    if ((rc = undistort_frame(ctx, gray_dev, n, width, height, K, staged))) return rc;
    gray_dev = staged;
  }
  if (n == 1) {
    if ((rc = sift_into(ctx, gray_dev[0], width, height, double_size, cap, p.desc, p.xy, nullptr, p.words))) return rc;
  } else if ((rc = sift_into_batch(ctx, gray_dev, n, width, height, double_size, cap, p.desc, p.xy, p.words))) {
    return rc;
  }
  MH_HIP(ctx, hipMemcpyAsync(p.words + 2 * MH_MAX_BATCH, sift_counters_dev(ctx, 0), (size_t)n * 4 * sizeof(int32_t),
                             hipMemcpyDeviceToDevice, ctx->stream));
  return MH_OK;
}

// Behind the selection of a one-image edit, whose rows lie in the staging block and whose count, box and (with_stats)
// statistics in ctx->planar: the norm terms by the upload's own launch, over the count on the device, so that it is in
// flight while the count travels; the added host wait -- the kept count sizes the splice (the set it fills, the
// per-model table); the optional host rows; the edit (op of `model`, or append = rows behind its last);
// MH_ERR_CAPACITY when FEAT's list overflowed.
int staged_image_edit(mh_ctx* ctx, const char* who, bool append, int op, int model, int cap, int limit, bool with_stats,
                      int32_t* n_rows, float bbox[6], int32_t stats[8], float* rows_desc_host, float* rows_xyz_host,
                      int rows_cap) {
  mh_ctx::Planar& p = ctx->planar;
  float* sd = ctx->db_stage;
  float* sn = sd + stage_rows(ctx) * DIM;
  float* sx = sn + stage_rows(ctx);
  const int32_t* n_out = p.words + MH_MAX_BATCH;
  launch_normalize(sd, sn, limit, ctx->stream, n_out);
  MH_HIP(ctx, hipGetLastError());
  int32_t kept = 0, head[4] = {0, 0, 0, 0}, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float box[6];
  MH_HIP(ctx, hipMemcpyAsync(&kept, n_out, sizeof kept, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(head, p.words + 2 * MH_MAX_BATCH, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(box, p.box, sizeof box, hipMemcpyDeviceToHost, ctx->stream));
  if (with_stats) MH_HIP(ctx, hipMemcpyAsync(st, p.stats, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (kept < 0 || kept > limit) {
    ctx->err = std::string(who) + ": the selection reported a count outside its capacity";
    return MH_ERR_HIP;
  }
  if (rows_desc_host && kept > 0) {
    const size_t take = (size_t)std::min(kept, rows_cap);
    MH_HIP(ctx, hipMemcpyAsync(rows_desc_host, p.rows_desc, take * DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(rows_xyz_host, sx, take * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  // (either ends with a wait for the stream: the host rows are there)
  if (int rc = append ? append_staged(ctx, model, kept) : splice_staged(ctx, op, model, kept)) return rc;
  if (n_rows) *n_rows = kept;
  if (bbox) std::memcpy(bbox, box, sizeof box);
  if (stats) std::memcpy(stats, st, sizeof st);
  if (head[2] || head[1] > cap) {
    ctx->err = std::string(who) + ": more keypoints than max_keypoints (" + std::to_string(head[1]) + " found); the model has the first of the list";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

}  // namespace

int mh_db_splice_image(mh_ctx* ctx, int op, int model, const uint8_t* gray_dev, int width, int height, int double_size,
                       int max_keypoints, const mh_planar_spec* spec, int32_t* n_rows, float bbox[6],
                       float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_db_splice_image";
  if (n_rows) *n_rows = 0;
  if (op != MH_DB_INSERT && op != MH_DB_REPLACE) return refuse(ctx, who, "the operation is MH_DB_INSERT or MH_DB_REPLACE");
  int all = 0, rc;
  if ((rc = check_planar_call(ctx, who, &gray_dev, 1, width, height, max_keypoints, spec, rows_desc_host, rows_xyz_host,
                              rows_cap, &all)))
    return rc;
  if ((rc = check_edit(ctx, who, op, model))) return rc;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int cap = max_keypoints;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  if ((rc = ensure_planar(ctx, 1, cap, rows_desc_host != nullptr))) return rc;
  if ((rc = ensure_stage(ctx, (size_t)limit))) return rc;
  if ((rc = planar_feat(ctx, &gray_dev, 1, width, height, double_size, cap, spec->K))) return rc;
  mh_ctx::Planar& p = ctx->planar;
  // the selection writes the edit's staging block itself
  float* sd = ctx->db_stage;
  float* sx = sd + stage_rows(ctx) * (DIM + 1);
  PlanarArgs a = {};
  a.desc = p.desc;
  a.xy = p.xy;
  a.n = p.words;
  a.cap = cap;
  a.spec = *spec;
  a.all = all;
  a.desc_out = sd;
  a.desc_copy = rows_desc_host ? (float*)p.rows_desc : nullptr;   // (normalisation is in place: the host gets FEAT's bits)
  a.xyz_out = sx;
  a.out_pitch = 0;
  a.out_cap = limit;
  a.n_out = p.words + MH_MAX_BATCH;
  a.bbox = p.box;
  launch_planar_rows(a, 1, ctx->stream);
  return staged_image_edit(ctx, who, false, op, model, cap, limit, false, n_rows, bbox, nullptr, rows_desc_host, rows_xyz_host, rows_cap);
}

int mh_db_splice_images(mh_ctx* ctx, int model_first, const uint8_t* const* gray_dev, int n_images, int width, int height,
                        int double_size, int max_keypoints, const mh_planar_spec* spec, int32_t* n_rows, float (*bbox)[6],
                        float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_db_splice_images";
  int all = 0, rc;
  if ((rc = check_planar_call(ctx, who, gray_dev, n_images, width, height, max_keypoints, spec, rows_desc_host,
                              rows_xyz_host, rows_cap, &all)))
    return rc;
  if ((rc = check_edit(ctx, who, MH_DB_INSERT, model_first, n_images))) return rc;
  for (int i = 0; n_rows && i < n_images; ++i) n_rows[i] = 0;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int cap = max_keypoints;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  if ((rc = ensure_planar(ctx, n_images, cap, true))) return rc;
  if ((rc = ensure_stage(ctx, (size_t)limit))) return rc;
  if ((rc = planar_feat(ctx, gray_dev, n_images, width, height, double_size, cap, spec->K))) return rc;
  mh_ctx::Planar& p = ctx->planar;
  PlanarArgs a = {};
  a.desc = p.desc;
  a.xy = p.xy;
  a.n = p.words;
  a.cap = cap;
  a.spec = *spec;
  a.all = all;
  a.desc_out = p.rows_desc;
  a.desc_copy = nullptr;
  a.xyz_out = p.rows_xyz;
  a.out_pitch = (size_t)cap;
  a.out_cap = limit;
  a.n_out = p.words + MH_MAX_BATCH;
  a.bbox = p.box;
  launch_planar_rows(a, n_images, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  // one read-back for the whole batch
  int32_t kept[MH_MAX_BATCH], head[MH_MAX_BATCH][4];
  float box[MH_MAX_BATCH][6];
  MH_HIP(ctx, hipMemcpyAsync(kept, a.n_out, (size_t)n_images * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(head, p.words + 2 * MH_MAX_BATCH, (size_t)n_images * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(box, p.box, (size_t)n_images * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  bool over = false;
  for (int i = 0; i < n_images; ++i) {
    if (kept[i] < 0 || kept[i] > limit) {
      ctx->err = "mh_db_splice_images: the selection reported a count outside its capacity";
      return MH_ERR_HIP;
    }
    const float* rd = p.rows_desc + (size_t)i * cap * DIM;
    const float* rx = p.rows_xyz + (size_t)i * cap * 3;
    if (rows_desc_host && kept[i] > 0) {
      const size_t take = (size_t)std::min(kept[i], rows_cap);
      MH_HIP(ctx, hipMemcpyAsync(rows_desc_host + (size_t)i * rows_cap * DIM, rd, take * DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipMemcpyAsync(rows_xyz_host + (size_t)i * rows_cap * 3, rx, take * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    // the existing single-model pass, once per image (a multi-model pass is a later change)
    if ((rc = mh_db_splice(ctx, MH_DB_INSERT, model_first + i, rd, rx, kept[i], 1, 1))) return rc;
    if (n_rows) n_rows[i] = kept[i];
    if (bbox) std::memcpy(bbox[i], box[i], sizeof box[i]);
    over = over || head[i][2] || head[i][1] > cap;
  }
  if (over) {
    ctx->err = "mh_db_splice_images: an image has more keypoints than max_keypoints; its model has the first of the list";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

// ---- 3-D models from Kinect views (view_rows.hip) into the resident store --------------------------------------------
namespace {

// the arguments mh_db_splice_view[s] / mh_db_append_view share, checked before anything is launched; fills a's view part
int check_view_call(mh_ctx* ctx, const char* who, const uint8_t* const* gray_dev, const mh_view* views, int n, int width,
                    int height, int max_keypoints, const mh_view_spec* spec, const float* rows_desc_host,
                    const float* rows_xyz_host, int rows_cap, ViewArgs* a) {
  if (int rc = check_images_call(ctx, who, gray_dev, n, width, height, max_keypoints, rows_desc_host, rows_xyz_host, rows_cap)) return rc;
  if (int rc = view_args_check(ctx, who, views, n, width, height, spec, a)) return rc;
  if (ctx->und_on)
    if (const char* why = view_undistort_why(views, n)) return refuse(ctx, who, why);
  return MH_OK;
}

int ensure_view(mh_ctx* ctx, int cap, bool match) {
  mh_ctx::Planar& p = ctx->planar;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, p.stats.ensure(8 * MH_MAX_BATCH, s));
  if (match) {
    MH_HIP(ctx, p.qn.ensure((size_t)cap * DIM, s));
    MH_HIP(ctx, p.qnorm.ensure(cap, s));
    MH_HIP(ctx, p.m_idx.ensure(cap, s));
    MH_HIP(ctx, p.m_d1.ensure(cap, s));
    MH_HIP(ctx, p.m_d2.ensure(cap, s));
  }
  return MH_OK;
}

// What mh_db_splice_view, mh_db_append_view and mh_db_merge_view share behind their checks: the buffers, [UNDISTORTED_IMAGE]
// -> FEAT into ctx->planar, the model's rows so far (append: the box covers them, the duplicate test reads them) and, with
// the duplicate test on, MATCH of a normalised copy as a frame's.  Fills a's lists and dup part.
int view_front(mh_ctx* ctx, bool append, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
               int double_size, int cap, size_t stage, const mh_view_spec* spec, bool host_rows, ViewArgs& a) {
  int rc;
  const bool match = append && spec->merge_ratio > 0.f && spec->merge_dist >= 0.f && ctx->N > 0;
  if ((rc = ensure_planar(ctx, 1, cap, host_rows))) return rc;
  if ((rc = ensure_view(ctx, cap, match))) return rc;
  if ((rc = ensure_stage(ctx, stage))) return rc;
  if ((rc = planar_feat(ctx, &gray_dev, 1, width, height, double_size, cap, view->K))) return rc;
  mh_ctx::Planar& p = ctx->planar;
  if (append && ctx->N > 0) {   // the model's rows so far: the box covers them; the duplicate test reads them
    a.dup.model_of_dev = ctx->db_model;
    a.dup.xyz_dev = ctx->db_xyz;
    a.dup.n_db_rows = ctx->N;
    a.dup.model = model;
    a.dup.row_begin = ctx->store->model_begin[model];
    a.dup.row_end = ctx->store->model_begin[model + 1];
  }
  if (match) {
    // MATCH as a frame's: a normalised copy (the model's rows keep FEAT's bits), the count on the device
    MH_HIP(ctx, hipMemcpyAsync(p.qn, p.desc, (size_t)cap * DIM * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    launch_normalize(p.qn, p.qnorm, cap, ctx->stream, p.words);
    if ((rc = ctx_match(ctx, p.qn, p.qnorm, cap, p.m_idx, p.m_d1, p.m_d2, p.words, 0))) return rc;
    a.dup.idx_dev = p.m_idx;
    a.dup.d1_dev = p.m_d1;
    a.dup.d2_dev = p.m_d2;
    a.dup_on = 1;
  }
  a.desc = p.desc;
  a.xy = p.xy;
  a.n = p.words;
  a.cap = cap;
  a.desc_copy = host_rows ? (float*)p.rows_desc : nullptr;   // (normalisation is in place: the host gets FEAT's bits)
  a.out_pitch = 0;
  a.n_out = p.words + MH_MAX_BATCH;
  a.bbox = p.box;
  a.stats = p.stats;
  return MH_OK;
}

// mh_db_splice_view (append = false: op, model) and mh_db_append_view (append = true: model)
int view_edit(mh_ctx* ctx, const char* who, bool append, int op, int model, const uint8_t* gray_dev, const mh_view* view,
              int width, int height, int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows,
              float bbox[6], int32_t stats[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (n_rows) *n_rows = 0;
  if (!append && op != MH_DB_INSERT && op != MH_DB_REPLACE) return refuse(ctx, who, "the operation is MH_DB_INSERT or MH_DB_REPLACE");
  ViewArgs a = {};
  int rc;
  if ((rc = check_view_call(ctx, who, &gray_dev, view, 1, width, height, max_keypoints, spec, rows_desc_host, rows_xyz_host,
                            rows_cap, &a)))
    return rc;
  if ((rc = check_edit(ctx, who, append ? (int)MH_DB_REPLACE : op, model))) return rc;   // (append: an existing model)
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int cap = max_keypoints;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  if ((rc = view_front(ctx, append, model, gray_dev, view, width, height, double_size, cap, (size_t)limit, spec,
                       rows_desc_host != nullptr, a)))
    return rc;
  // the selection writes the edit's staging block itself, as mh_db_splice_image's does
  float* sd = ctx->db_stage;
  a.desc_out = sd;
  a.xyz_out = sd + stage_rows(ctx) * (DIM + 1);
  a.out_cap = limit;
  launch_view_rows(a, 1, ctx->stream);
  return staged_image_edit(ctx, who, append, op, model, cap, limit, true, n_rows, bbox, stats, rows_desc_host, rows_xyz_host, rows_cap);
}

// mh_db_merge_view with the duplicate test on: the model's rows, the merged ones among them overwritten, and the new rows
// behind them make up the staging block; one REPLACE splice.  Untouched rows are copied with their norm terms, so they
// keep their bits; only merged and new rows are normalised.
int merge_view_edit(mh_ctx* ctx, const char* who, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                    int double_size, int cap, const mh_view_spec* spec, ViewArgs& a, const int32_t* views_in_host,
                    int32_t* n_added, int32_t* n_merged, float bbox[6], int32_t stats[8], float* rows_desc_host,
                    float* rows_xyz_host, int rows_cap, int32_t* merged_idx_host, float* merged_desc_host,
                    float* merged_xyz_host, int merged_cap, int32_t* views_out_host) {
  int rc;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  const int b = ctx->store->model_begin[model], e = ctx->store->model_begin[model + 1], rows = e - b;
  const int mcap = std::max(std::min(rows, cap), 1);   // a merged row has an observation of its own
  if ((rc = view_front(ctx, true, model, gray_dev, view, width, height, double_size, cap, (size_t)rows + limit, spec,
                       rows_desc_host != nullptr, a)))
    return rc;
  if ((rc = ensure_view_merge(ctx, cap, rows))) return rc;
  mh_ctx::Planar& p = ctx->planar;
  hipStream_t s = ctx->stream;
  const size_t rows1 = (size_t)std::max(rows, 1);
  MH_HIP(ctx, p.mg_idx.ensure((size_t)mcap, s));
  MH_HIP(ctx, p.mg_views_in.ensure(rows1, s));
  MH_HIP(ctx, p.mg_views_out.ensure(rows1, s));
  MH_HIP(ctx, p.mg_n.ensure(1, s));
  MH_HIP(ctx, p.mg_desc.ensure((size_t)mcap * DIM, s));
  MH_HIP(ctx, p.mg_desc_n.ensure((size_t)mcap * DIM, s));
  MH_HIP(ctx, p.mg_norm.ensure((size_t)mcap, s));
  MH_HIP(ctx, p.mg_xyz.ensure((size_t)mcap * 3, s));
  MH_HIP(ctx, p.mg_box.ensure(6, s));
  float* sd = ctx->db_stage;
  float* sn = sd + stage_rows(ctx) * DIM;
  float* sx = sn + stage_rows(ctx);
  const DbStore* st = ctx->store.get();
  if (rows > 0) {
    MH_HIP(ctx, hipMemcpyAsync(sd, st->desc + (size_t)b * DIM, (size_t)rows * DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
    MH_HIP(ctx, hipMemcpyAsync(sn, st->norm + b, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    MH_HIP(ctx, hipMemcpyAsync(sx, st->xyz + (size_t)b * 3, (size_t)rows * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (views_in_host)
      MH_HIP(ctx, hipMemcpyAsync(p.mg_views_in, views_in_host, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  // the selection: the new rows behind the model's
  a.desc_out = sd + (size_t)rows * DIM;
  a.xyz_out = sx + (size_t)rows * 3;
  a.out_cap = limit;
  launch_view_rows(a, 1, s);
  // the merge: s into mg_desc (the host's) and mg_desc_n, which the upload's own launch normalises; then over the staged rows
  MergeArgs m = {};
  m.v = a;
  m.qn = p.qn;
  m.old_desc = st->desc;
  m.views_in = views_in_host ? (const int32_t*)p.mg_views_in : nullptr;
  m.obs_row = p.mg_obs_row;
  m.obs_xyz = p.mg_obs_xyz;
  m.touched = p.mg_touched;
  m.merged_idx = p.mg_idx;
  m.merged_desc = p.mg_desc;
  m.merged_desc_copy = p.mg_desc_n;
  m.merged_xyz = p.mg_xyz;
  m.merged_cap = rows > 0 ? mcap : 0;
  m.n_merged = p.mg_n;
  m.views_out = p.mg_views_out;
  if ((rc = launch_view_merge(ctx, m))) return rc;
  if (rows > 0) {
    launch_normalize(p.mg_desc_n, p.mg_norm, mcap, s, p.mg_n);
    launch_view_merge_scatter(p.mg_idx, p.mg_n, mcap, p.mg_desc_n, p.mg_norm, p.mg_xyz, sd, sn, sx, s);
  }
  launch_normalize(sd + (size_t)rows * DIM, sn + rows, limit, s, a.n_out);
  launch_view_box(sx, rows, a.n_out, p.mg_box, s);
  MH_HIP(ctx, hipGetLastError());
  // the one host wait before the splice: the counts size it
  int32_t kept = 0, nm = 0, head[4] = {0, 0, 0, 0}, stv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float box[6];
  MH_HIP(ctx, hipMemcpyAsync(&kept, a.n_out, sizeof kept, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(&nm, p.mg_n, sizeof nm, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(head, p.words + 2 * MH_MAX_BATCH, sizeof head, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(box, p.mg_box, sizeof box, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(stv, p.stats, sizeof stv, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  if (kept < 0 || kept > limit || nm < 0 || nm > (rows > 0 ? mcap : 0)) {
    ctx->err = std::string(who) + ": the selection or the merge reported a count outside its capacity";
    return MH_ERR_HIP;
  }
  if (rows_desc_host && kept > 0) {
    const size_t take = (size_t)std::min(kept, rows_cap);
    MH_HIP(ctx, hipMemcpyAsync(rows_desc_host, p.rows_desc, take * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipMemcpyAsync(rows_xyz_host, sx + (size_t)rows * 3, take * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  if (merged_idx_host && nm > 0) {
    const size_t take = (size_t)std::min(nm, merged_cap);
    MH_HIP(ctx, hipMemcpyAsync(merged_idx_host, p.mg_idx, take * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipMemcpyAsync(merged_desc_host, p.mg_desc, take * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipMemcpyAsync(merged_xyz_host, p.mg_xyz, take * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  if (views_out_host && rows > 0)
    MH_HIP(ctx, hipMemcpyAsync(views_out_host, p.mg_views_out, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  // (ends with a wait for the stream: the host arrays are there)
  if ((rc = splice_staged(ctx, MH_DB_REPLACE, model, rows + kept))) return rc;
  if (views_out_host) std::fill(views_out_host + rows, views_out_host + rows + kept, 1);
  if (n_added) *n_added = kept;
  if (n_merged) *n_merged = nm;
  if (bbox) std::memcpy(bbox, box, sizeof box);
  if (stats) std::memcpy(stats, stv, sizeof stv);
  if (head[2] || head[1] > cap) {
    ctx->err = std::string(who) + ": more keypoints than max_keypoints (" + std::to_string(head[1]) + " found); the model has the first of the list";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

}  // namespace

int mh_db_splice_view(mh_ctx* ctx, int op, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                      int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows, float bbox[6],
                      int32_t stats[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (!ctx) return MH_ERR_ARG;
  return view_edit(ctx, "mh_db_splice_view", false, op, model, gray_dev, view, width, height, double_size, max_keypoints, spec,
                   n_rows, bbox, stats, rows_desc_host, rows_xyz_host, rows_cap);
}

int mh_db_append_view(mh_ctx* ctx, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                      int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows, float bbox[6],
                      int32_t stats[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (!ctx) return MH_ERR_ARG;
  return view_edit(ctx, "mh_db_append_view", true, MH_DB_REPLACE, model, gray_dev, view, width, height, double_size,
                   max_keypoints, spec, n_rows, bbox, stats, rows_desc_host, rows_xyz_host, rows_cap);
}

int mh_db_merge_view(mh_ctx* ctx, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                     int double_size, int max_keypoints, const mh_view_spec* spec, const int32_t* views_in_host, int n_views_in,
                     int32_t* n_added, int32_t* n_merged, float bbox[6], int32_t stats[8], float* rows_desc_host,
                     float* rows_xyz_host, int rows_cap, int32_t* merged_idx_host, float* merged_desc_host,
                     float* merged_xyz_host, int merged_cap, int32_t* views_out_host, int views_out_cap) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_db_merge_view";
  if (n_added) *n_added = 0;
  if (n_merged) *n_merged = 0;
  ViewArgs a = {};
  int rc;
  if ((rc = check_view_call(ctx, who, &gray_dev, view, 1, width, height, max_keypoints, spec, rows_desc_host, rows_xyz_host,
                            rows_cap, &a)))
    return rc;
  if ((rc = check_edit(ctx, who, MH_DB_REPLACE, model))) return rc;   // an existing model
  const int rows = ctx->store->model_begin[model + 1] - ctx->store->model_begin[model];
  if (const char* why = view_counts_why(views_in_host, n_views_in, rows)) return refuse(ctx, who, why);
  if ((merged_idx_host == nullptr) != (merged_desc_host == nullptr) || (merged_idx_host == nullptr) != (merged_xyz_host == nullptr) ||
      merged_cap < 0)
    return refuse(ctx, who, "bad argument (the merged rows' host arrays come together; merged_cap >= 0)");
  const int cap = max_keypoints;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  // (the rows after the edit are known only behind the selection: the bound is what it can add at most)
  if (views_out_host && (long long)views_out_cap < (long long)rows + limit)
    return refuse(ctx, who, "views_out_cap is below the model's rows + the rows the view may add (max_rows, or max_keypoints)");
  if (!(spec->merge_ratio > 0.f && spec->merge_dist >= 0.f && ctx->N > 0)) {
    // the test off, or nothing to compare with: mh_db_append_view, the old counts followed by ones
    int32_t kept = 0;
    rc = view_edit(ctx, who, true, MH_DB_REPLACE, model, gray_dev, view, width, height, double_size, max_keypoints, spec, &kept,
                   bbox, stats, rows_desc_host, rows_xyz_host, rows_cap);
    if (rc != MH_OK && rc != MH_ERR_CAPACITY) return rc;
    if (n_added) *n_added = kept;
    if (views_out_host) {
      if (views_in_host) std::copy(views_in_host, views_in_host + rows, views_out_host);
      else std::fill(views_out_host, views_out_host + rows, 1);
      std::fill(views_out_host + rows, views_out_host + rows + kept, 1);
    }
    return rc;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  return merge_view_edit(ctx, who, model, gray_dev, view, width, height, double_size, cap, spec, a, views_in_host, n_added,
                         n_merged, bbox, stats, rows_desc_host, rows_xyz_host, rows_cap, merged_idx_host, merged_desc_host,
                         merged_xyz_host, merged_cap, views_out_host);
}

int mh_db_keep_rows(mh_ctx* ctx, int model, const uint8_t* keep_host, int n_flags, int32_t* n_rows, float bbox[6]) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_db_keep_rows";
  if (int rc = check_edit(ctx, who, MH_DB_REPLACE, model)) return rc;
  const DbStore* st = ctx->store.get();
  const int b = st->model_begin[model], rows = st->model_begin[model + 1] - b;
  if (n_flags != rows || (rows > 0 && !keep_host)) return refuse(ctx, who, "n_flags is not the model's row count, or no flags");
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  mh_ctx::Planar& p = ctx->planar;
  MH_HIP(ctx, p.keep.ensure((size_t)std::max(rows, 1), ctx->stream));
  MH_HIP(ctx, p.mg_box.ensure(6, ctx->stream));
  if (int rc = ensure_stage(ctx, (size_t)std::max(rows, 1))) return rc;
  int kept = 0;
  for (int r = 0; r < rows; ++r) kept += keep_host[r] != 0;
  float* sd = ctx->db_stage;
  float* sn = sd + stage_rows(ctx) * DIM;
  float* sx = sn + stage_rows(ctx);
  if (rows > 0) MH_HIP(ctx, hipMemcpyAsync(p.keep, keep_host, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
  // the store's own rows, packed in order with their norm terms: nothing is normalised again
  launch_view_keep(p.keep, b, rows, st->desc, st->norm, st->xyz, sd, sn, sx, p.mg_box, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  float box[6];
  MH_HIP(ctx, hipMemcpyAsync(box, p.mg_box, sizeof box, hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = splice_staged(ctx, MH_DB_REPLACE, model, kept)) return rc;   // (ends with a wait for the stream)
  if (n_rows) *n_rows = kept;
  if (bbox) std::memcpy(bbox, box, sizeof box);
  return MH_OK;
}

int mh_db_splice_views(mh_ctx* ctx, int model_first, const uint8_t* const* gray_dev, const mh_view* views, int n_views,
                       int width, int height, int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows,
                       float (*bbox)[6], int32_t (*stats)[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap) {
  if (!ctx) return MH_ERR_ARG;
  const char* who = "mh_db_splice_views";
  ViewArgs a = {};
  int rc;
  if ((rc = check_view_call(ctx, who, gray_dev, views, n_views, width, height, max_keypoints, spec, rows_desc_host,
                            rows_xyz_host, rows_cap, &a)))
    return rc;
  if ((rc = check_edit(ctx, who, MH_DB_INSERT, model_first, n_views))) return rc;
  for (int i = 0; n_rows && i < n_views; ++i) n_rows[i] = 0;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int cap = max_keypoints;
  const int limit = spec->max_rows > 0 ? std::min(cap, spec->max_rows) : cap;
  if ((rc = ensure_planar(ctx, n_views, cap, true))) return rc;
  if ((rc = ensure_view(ctx, cap, false))) return rc;
  if ((rc = ensure_stage(ctx, (size_t)limit))) return rc;
  if ((rc = planar_feat(ctx, gray_dev, n_views, width, height, double_size, cap, views[0].K))) return rc;
  mh_ctx::Planar& p = ctx->planar;
  a.desc = p.desc;
  a.xy = p.xy;
  a.n = p.words;
  a.cap = cap;
  a.desc_out = p.rows_desc;
  a.desc_copy = nullptr;
  a.xyz_out = p.rows_xyz;
  a.out_pitch = (size_t)cap;
  a.out_cap = limit;
  a.n_out = p.words + MH_MAX_BATCH;
  a.bbox = p.box;
  a.stats = p.stats;
  launch_view_rows(a, n_views, ctx->stream);
  MH_HIP(ctx, hipGetLastError());
  // one read-back for the whole batch
  int32_t kept[MH_MAX_BATCH], head[MH_MAX_BATCH][4], st[MH_MAX_BATCH][8];
  float box[MH_MAX_BATCH][6];
  MH_HIP(ctx, hipMemcpyAsync(kept, a.n_out, (size_t)n_views * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(head, p.words + 2 * MH_MAX_BATCH, (size_t)n_views * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(box, p.box, (size_t)n_views * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipMemcpyAsync(st, p.stats, (size_t)n_views * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  bool over = false;
  for (int i = 0; i < n_views; ++i) {
    if (kept[i] < 0 || kept[i] > limit) {
      ctx->err = "mh_db_splice_views: the selection reported a count outside its capacity";
      return MH_ERR_HIP;
    }
    const float* rd = p.rows_desc + (size_t)i * cap * DIM;
    const float* rx = p.rows_xyz + (size_t)i * cap * 3;
    if (rows_desc_host && kept[i] > 0) {
      const size_t take = (size_t)std::min(kept[i], rows_cap);
      MH_HIP(ctx, hipMemcpyAsync(rows_desc_host + (size_t)i * rows_cap * DIM, rd, take * DIM * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipMemcpyAsync(rows_xyz_host + (size_t)i * rows_cap * 3, rx, take * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    // the single-model pass, once per view
    if ((rc = mh_db_splice(ctx, MH_DB_INSERT, model_first + i, rd, rx, kept[i], 1, 1))) return rc;
    if (n_rows) n_rows[i] = kept[i];
    if (bbox) std::memcpy(bbox[i], box[i], sizeof box[i]);
    if (stats) std::memcpy(stats[i], st[i], sizeof st[i]);
    over = over || head[i][2] || head[i][1] > cap;
  }
  if (over) {
    ctx->err = "mh_db_splice_views: a view has more keypoints than max_keypoints; its model has the first of the list";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_db_reserve(mh_ctx* ctx, int64_t max_rows, int max_models) {
  if (!ctx || max_rows < 0 || max_rows > 0x7FFFFF00ll || max_models < 0 || max_models > MH_MAX_MODELS)
    return ctx ? refuse(ctx, "mh_db_reserve", "bad argument") : MH_ERR_ARG;
  if (const char* why = why_not_editable(ctx->store.get())) return refuse(ctx, "mh_db_reserve", why);
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  if (!ctx->pool) ctx->pool = std::make_shared<DbPool>();
  const size_t cap_rows = std::max<size_t>(((size_t)max_rows + 127) / 128 * 128, 128);
  DbStore* stale = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->pool->mu);
    ctx->pool->cap_rows = std::max(ctx->pool->cap_rows, cap_rows);
    ctx->pool->max_models = std::max(ctx->pool->max_models, max_models);
    if (ctx->pool->spare && ctx->pool->spare->cap < ctx->pool->cap_rows) std::swap(stale, ctx->pool->spare);
  }
  delete stale;
  ctx->db_models_reserved = ctx->pool->max_models;
  int rc = ensure_stage(ctx, (size_t)std::min<int64_t>(std::max<int64_t>(max_rows, 1), 65536));
  if (rc) return rc;
  // the live set at capacity: the identity splice into a fresh set (an empty store if the context has none) ...
  const DbStore* old = ctx->store.get();
  if (!old || !set_fits(old, ctx->pool->cap_rows, screen_wanted(1 << 30, (int)ctx->pool->cap_rows))) {
    std::vector<int32_t> table = old ? old->model_begin : std::vector<int32_t>(1, 0);
    const uint64_t gen = old ? old->generation : 0;
    rc = run_splice(ctx, 0, 0, 0, 0, 0, std::move(table));
    if (rc) return rc;
    ctx->store->generation = gen;   // (the same rows: not an edit)
  } else if (!ctx->store->pool) {
    ctx->store->pool = ctx->pool;
  }
  // ... and the spare
  bool have_spare;
  {
    std::lock_guard<std::mutex> lock(ctx->pool->mu);
    have_spare = ctx->pool->spare != nullptr;
  }
  if (!have_spare) {
    std::shared_ptr<DbStore> spare;
    if ((rc = alloc_set(ctx, ctx->pool->cap_rows, spare))) return rc;
    spare.reset();   // parks in the pool
  }
  return MH_OK;
}

int mh_db_adopt(mh_ctx* dst, mh_ctx* src) {
  if (!dst || !src || !src->store) {
    if (dst) dst->err = "mh_db_adopt: the source context holds no database";
    return MH_ERR_ARG;
  }
  if (dst == src || dst->store == src->store) return MH_OK;
  if (dst->device != src->device) return refuse(dst, "mh_db_adopt", "contexts on different devices");
  MH_HIP(dst, hipSetDevice(dst->device));
  if (int rc_stream = mh::use_stream(dst)) return rc_stream;
  db_poll_held(dst, false);
  // frames enqueued on dst from here on run behind the edit that filled the store ...
  if (src->store->ready) MH_HIP(dst, hipStreamWaitEvent(dst->stream, src->store->ready, 0));
  else if (src->stream) MH_HIP(dst, hipStreamSynchronize(src->stream));   // (an uploaded store: the upload was synchronous)
  // ... and dst's frames in flight finish on the store it had: it is held until an event behind them has completed
  if (dst->store) {
    mh_ctx::HeldStore h;
    if (!dst->held_events.empty()) {
      h.done = dst->held_events.back();
      dst->held_events.pop_back();
    } else {
      MH_HIP(dst, hipEventCreateWithFlags(&h.done, hipEventDisableTiming));
    }
    MH_HIP(dst, hipEventRecord(h.done, dst->stream));
    h.store = std::move(dst->store);
    if (!h.store->pool) h.store->pool = src->pool;
    dst->held.push_back(std::move(h));
  }
  dst->store = src->store;
  dst->pool = src->pool;
  dst->db_models_reserved = src->db_models_reserved;
  bind_store(dst);
  return MH_OK;
}

int mh_db_splice_models(mh_ctx* ctx, int op, int model, const mh_model_set* s, int set_index) {
  if (!ctx) return MH_ERR_ARG;
  if (op == MH_DB_REMOVE) return mh_db_splice(ctx, op, model, nullptr, nullptr, 0, 0, 0);
  int64_t row_begin = 0, n_rows = 0;
  if (!s || mh_models_range(s, set_index, &row_begin, &n_rows, nullptr) != MH_OK || n_rows > 0x7FFFFF00ll)
    return refuse(ctx, "mh_db_splice_models", "no such model in the set");
  return mh_db_splice(ctx, op, model, mh_models_desc(s) + row_begin * DIM, mh_models_xyz(s) + row_begin * 3, (int)n_rows, 1, 0);
}

int mh_db_debug_route(mh_ctx* ctx, int route) {
  if (!ctx || route < 0 || route > 1) return MH_ERR_ARG;
  ctx->db_edit_route = route;
  return MH_OK;
}

int mh_db_edit_ms(mh_ctx* ctx, float* ms) {
  if (!ctx || !ms) return MH_ERR_ARG;
  if (!ctx->db_ev_valid) return refuse(ctx, "mh_db_edit_ms", "no timed edit (mh_enable_timing before the edit)");
  MH_HIP(ctx, hipEventElapsedTime(ms, ctx->db_ev[0], ctx->db_ev[1]));
  return MH_OK;
}

int mh_db_debug_fetch(mh_ctx* ctx, int which, void* out_host, size_t bytes) {
  if (!ctx || which < 0 || which > 5 || (bytes > 0 && !out_host)) return MH_ERR_ARG;
  const DbStore* st = ctx->store.get();
  const size_t N = st ? (size_t)st->N : 0, n_pad = (N + 127) / 128 * 128;
  const bool image = st && st->screen.dbh;
  const void* src = nullptr;
  size_t extent = 0;
  switch (which) {
    case 0: src = st ? st->desc : nullptr; extent = n_pad * DIM * sizeof(float); break;
    case 1: src = st ? st->norm : nullptr; extent = n_pad * sizeof(float); break;
    case 2: src = st ? st->xyz : nullptr; extent = N * 3 * sizeof(float); break;
    case 3: src = st ? st->model : nullptr; extent = N * sizeof(int32_t); break;
    case 4: src = image ? st->desc_h : nullptr; extent = image ? n_pad * DIM * sizeof(_Float16) : 0; break;
    default: src = image ? st->neg_h : nullptr; extent = image ? n_pad / 128 * DB_DD * sizeof(float) : 0; break;
  }
  if (bytes > extent) return refuse(ctx, "mh_db_debug_fetch", "more bytes than the store defines for that array");
  if (bytes == 0) return MH_OK;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MH_HIP(ctx, hipMemcpy(out_host, src, bytes, hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_db_debug_screen(mh_ctx* ctx, uint32_t out[8]) {
  if (!ctx || !out) return MH_ERR_ARG;
  const ScreenDb& s = ctx->sdb;
  std::memcpy(&out[0], &s.dmax, 4);
  std::memcpy(&out[1], &s.spread, 4);
  out[2] = (uint32_t)s.zero_idx;
  std::memcpy(&out[3], &s.zero_d1, 4);
  std::memcpy(&out[4], &s.zero_d2, 4);
  out[5] = s.usable ? 1u : 0u;
  out[6] = s.dbh ? 1u : 0u;
  out[7] = (uint32_t)ctx->N;
  return MH_OK;
}

}  // extern "C"
