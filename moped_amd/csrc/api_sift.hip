// C ABI: SIFT extraction (FEAT_SIFT_CPU's job).
#include <algorithm>
#include <string>
#include <vector>

#include "context.h"
#include "sift.h"

using namespace mh;

struct SiftState {
  int width = 0, height = 0, double_size = -1, cap = 0, images = 1;
  SiftPlan plan;
  SiftBuffers B = {};            // what the launches take: views of the next six
  DevBuf<float> pyramid, tmp;
  DevBuf<unsigned int> owner;
  DevBuf<SiftCandidate> cand;
  DevBuf<SiftKey> keys;
  DevBuf<int32_t> counters;
  DevBuf<uint8_t> gray;          // staging for host-pointer calls
  DevBuf<float> desc, xy, scale_ori;
  DevBuf<int32_t> n_dev;
  unsigned int own_epoch = 0;    // B.own_epoch points here
  int last_n = 0;                // image slots the last launch filled (mh_sift_debug_*); 0 = none yet
};

namespace {

// images > 1: room for a batch's images side by side (mh_frame_enqueue_image_batch: one launch per stage for all of them)
int ensure_sift(mh_ctx* ctx, int width, int height, int double_size, int cap, int images = 1) {
  SiftState* st = ctx->sift;
  // internal keypoint room is never below 8192, so that a small output capacity still selects
  // the FIRST keypoints of the reference's list (which are the last ones generated)
  cap = std::max(cap, 8192);
  if (st && st->width == width && st->height == height && st->double_size == double_size && st->cap >= cap &&
      st->images >= images)
    return MH_OK;
  if (st) {
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    cap = std::max(cap, st->cap);
    images = std::max(images, st->images);
    delete st;
    ctx->sift = nullptr;
  }
  st = new SiftState;
  ctx->sift = st;
  st->width = width;
  st->height = height;
  st->double_size = double_size;
  st->cap = cap;
  st->images = images;
  if (sift_plan(width, height, double_size, &st->plan) == 0) {
    ctx->err = "mh_sift: image too small (both sides must exceed 12 pixels after scaling)";
    delete st;   // no half-built state: the next call with this geometry fails the same way
    ctx->sift = nullptr;
    return MH_ERR_ARG;
  }
  size_t owner = 0;
  for (int o = 0; o < st->plan.n_octaves; ++o) owner += (size_t)st->plan.rows[o] * st->plan.cols[o];
  const size_t ni = (size_t)images;
  hipStream_t s = ctx->stream;
  st->B.owner_elems = owner;
  st->B.own_epoch = &st->own_epoch;
  st->B.cand_cap = 4 * cap;
  st->B.key_cap = cap;
  st->B.images = images;
  hipError_t e = st->pyramid.ensure(st->plan.floats * ni, s);
  if (e == hipSuccess) e = st->tmp.ensure((size_t)st->plan.rows0 * st->plan.cols0 * ni, s);
  if (e == hipSuccess) e = st->owner.ensure(owner * ni, s);
  if (e == hipSuccess) e = st->cand.ensure((size_t)st->B.cand_cap * ni, s);
  if (e == hipSuccess) e = st->keys.ensure((size_t)cap * ni, s);
  if (e == hipSuccess) e = st->counters.ensure(4 * ni, s);
  if (e == hipSuccess) e = st->gray.ensure((size_t)width * height, s);
  if (e == hipSuccess) e = st->desc.ensure((size_t)cap * 128, s);
  if (e == hipSuccess) e = st->xy.ensure((size_t)cap * 2, s);
  if (e == hipSuccess) e = st->scale_ori.ensure((size_t)cap * 2, s);
  if (e == hipSuccess) e = st->n_dev.ensure(1, s);
  if (e != hipSuccess) {
    delete st;
    ctx->sift = nullptr;
    ctx->err = std::string("mh_sift: ") + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  st->B.pyramid = st->pyramid;
  st->B.tmp = st->tmp;
  st->B.owner = st->owner;
  st->B.cand = st->cand;
  st->B.keys = st->keys;
  st->B.counters = st->counters;
  return MH_OK;
}

}  // namespace

namespace mh {

// SIFT of a device image into caller-chosen device buffers, on the context's stream;
// *n_dev_out = the context's device word holding the keypoint count afterwards.
int sift_into(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size, int cap,
              float* desc_dev, float* xy_dev, int32_t** n_dev_out, int32_t* count_word) {
  int rc = ensure_sift(ctx, width, height, double_size ? 1 : 0, cap);
  if (rc) return rc;
  SiftState* st = ctx->sift;
  int32_t* const n_dev = count_word ? count_word : st->n_dev;   // (a batch of images keeps every image's count)
  launch_sift(gray_dev, width, height, double_size ? 1 : 0, st->plan, st->B, cap, desc_dev, xy_dev, nullptr,
              n_dev, ctx->stream);
  st->last_n = 1;
  MH_HIP(ctx, hipGetLastError());
  if (n_dev_out) *n_dev_out = n_dev;
  return MH_OK;
}

// n images of one size into the rows of a batch: image i's keypoints at desc_dev + i cap 128 / xy_dev + i cap 2, its count
// in count_words[i]; one launch per stage for all of them.
int sift_into_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int width, int height, int double_size, int cap,
                    float* desc_dev, float* xy_dev, int32_t* count_words) {
  int rc = ensure_sift(ctx, width, height, double_size ? 1 : 0, cap, n);
  if (rc) return rc;
  SiftState* st = ctx->sift;
  launch_sift_batch(gray_dev, n, width, height, double_size ? 1 : 0, st->plan, st->B, cap, cap, desc_dev, xy_dev, nullptr,
                    count_words, 1, ctx->stream);
  st->last_n = n;   // (n = 1 goes image by image into slot 0)
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

const int32_t* sift_counters_dev(mh_ctx* ctx, int slot) { return ctx->sift ? ctx->sift->B.counters + 4 * slot : nullptr; }

}  // namespace mh

extern "C" {

void mh_free_sift_state(mh_ctx* ctx) {
  delete ctx->sift;
  ctx->sift = nullptr;
}

int mh_sift_extract_dev(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size,
                        float* desc_dev, float* xy_dev, float* scale_ori_dev, int cap, int32_t* n_dev) {
  if (!ctx || !gray_dev || width <= 0 || height <= 0 || !desc_dev || !xy_dev || cap <= 0 || !n_dev) {
    if (ctx) ctx->err = "mh_sift_extract_dev: bad argument";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ensure_sift(ctx, width, height, double_size ? 1 : 0, cap);
  if (rc) return rc;
  SiftState* st = ctx->sift;
  launch_sift(gray_dev, width, height, double_size ? 1 : 0, st->plan, st->B, cap, desc_dev, xy_dev, scale_ori_dev,
              n_dev, ctx->stream);
  st->last_n = 1;
  MH_HIP(ctx, hipGetLastError());
  return MH_OK;
}

int mh_sift_extract(mh_ctx* ctx, const uint8_t* gray_host, int width, int height, int double_size, float* xy_host,
                    float* scale_ori_host, float* desc_host, int cap, int32_t* n_keypoints) {
  if (!ctx || !gray_host || width <= 0 || height <= 0 || !xy_host || !desc_host || cap <= 0 || !n_keypoints) {
    if (ctx) ctx->err = "mh_sift_extract: bad argument";
    return MH_ERR_ARG;
  }
  *n_keypoints = 0;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  int rc = ensure_sift(ctx, width, height, double_size ? 1 : 0, cap);
  if (rc) return rc;
  SiftState* st = ctx->sift;
  hipStream_t s = ctx->stream;
  MH_HIP(ctx, hipMemcpyAsync(st->gray, gray_host, (size_t)width * height, hipMemcpyHostToDevice, s));
  launch_sift(st->gray, width, height, double_size ? 1 : 0, st->plan, st->B, st->cap, st->desc, st->xy, st->scale_ori,
              st->n_dev, s);
  st->last_n = 1;
  MH_HIP(ctx, hipGetLastError());
  int32_t head[4] = {0, 0, 0, 0};
  int32_t n = 0;
  MH_HIP(ctx, hipMemcpyAsync(&n, st->n_dev, sizeof n, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipMemcpyAsync(head, st->B.counters, sizeof head, hipMemcpyDeviceToHost, s));
  MH_HIP(ctx, hipStreamSynchronize(s));
  const int take = std::min(n, cap);
  if (take > 0) {
    MH_HIP(ctx, hipMemcpyAsync(desc_host, st->desc, (size_t)take * 128 * sizeof(float), hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipMemcpyAsync(xy_host, st->xy, (size_t)take * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (scale_ori_host)
      MH_HIP(ctx, hipMemcpyAsync(scale_ori_host, st->scale_ori, (size_t)take * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    MH_HIP(ctx, hipStreamSynchronize(s));
  }
  *n_keypoints = take;
  if (head[2] || n > cap) {
    ctx->err = "mh_sift_extract: more keypoints than the capacity given (" + std::to_string(head[1]) + " found)";
    return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

int mh_sift_extract_batch_dev(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_images, int width, int height,
                              int double_size, float* desc_dev, float* xy_dev, int cap, int32_t* counts_dev) {
  if (!ctx || !gray_dev || n_images <= 0 || n_images > MH_MAX_BATCH || width <= 0 || height <= 0 || !desc_dev || !xy_dev ||
      cap <= 0 || !counts_dev) {
    if (ctx) ctx->err = "mh_sift_extract_batch_dev: bad argument";
    return MH_ERR_ARG;
  }
  for (int i = 0; i < n_images; ++i)
    if (!gray_dev[i]) {
      ctx->err = "mh_sift_extract_batch_dev: bad argument";
      return MH_ERR_ARG;
    }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  return mh::sift_into_batch(ctx, gray_dev, n_images, width, height, double_size, cap, desc_dev, xy_dev, counts_dev);
}

// ---- for verification: the stages of the last extraction (include/moped_hip.h) ------------------------------------
static_assert(sizeof(mh_sift_candidate) == sizeof(SiftCandidate) && sizeof(mh_sift_key) == sizeof(SiftKey) &&
                  MH_SIFT_MAX_OCTAVES == SIFT_MAX_OCTAVES,
              "the header's records are the kernels' records");

namespace {

// the state of the last extraction, stream idle; null (and ctx->err) when there is none or `slot` was not filled
SiftState* last_sift(mh_ctx* ctx, int slot, const char* who) {
  if (!ctx) return nullptr;
  SiftState* st = ctx->sift;
  if (!st || st->last_n <= 0 || slot < 0 || slot >= st->last_n) {
    ctx->err = std::string(who) + ": no extraction yet, or no such image slot";
    return nullptr;
  }
  return st;
}

}  // namespace

int mh_sift_debug_plan(mh_ctx* ctx, int32_t* n_images, int32_t* n_octaves, int32_t* rows, int32_t* cols) {
  SiftState* st = last_sift(ctx, 0, "mh_sift_debug_plan");
  if (!st || !n_octaves || !rows || !cols) return MH_ERR_ARG;
  if (n_images) *n_images = st->last_n;
  *n_octaves = st->plan.n_octaves;
  for (int o = 0; o < st->plan.n_octaves; ++o) {
    rows[o] = st->plan.rows[o];
    cols[o] = st->plan.cols[o];
  }
  return MH_OK;
}

int mh_sift_debug_level(mh_ctx* ctx, int slot, int octave, int kind, int level, float* out_host) {
  SiftState* st = last_sift(ctx, slot, "mh_sift_debug_level");
  if (!st) return MH_ERR_ARG;
  if (octave < 0 || octave >= st->plan.n_octaves || kind < 0 || kind > 1 || level < 0 || level > 4 || !out_host) {
    ctx->err = "mh_sift_debug_level: no such image (Gaussian levels 0..4 and DoG levels 0..4 are kept)";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  // the layout launch_sift_images gives the pyramid: per octave 6 Gaussian + 5 DoG images
  size_t at = 0;
  for (int o = 0; o < octave; ++o) at += (size_t)st->plan.rows[o] * st->plan.cols[o] * SIFT_IMAGES_PER_OCTAVE;
  const size_t px = (size_t)st->plan.rows[octave] * st->plan.cols[octave];
  at += px * (kind == 0 ? level : 6 + level);
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MH_HIP(ctx, hipMemcpy(out_host, st->B.pyramid + (size_t)slot * st->plan.floats + at, px * sizeof(float),
                        hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_sift_debug_candidates(mh_ctx* ctx, int slot, mh_sift_candidate* out_host, uint8_t* won_host, int cap, int32_t* n) {
  SiftState* st = last_sift(ctx, slot, "mh_sift_debug_candidates");
  if (!st || !out_host || !won_host || cap < 0 || !n) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int32_t head[4];
  MH_HIP(ctx, hipMemcpy(head, st->B.counters + 4 * slot, sizeof head, hipMemcpyDeviceToHost));
  *n = std::min(head[0], st->B.cand_cap);
  const int take = std::min(*n, cap);
  if (take <= 0) return MH_OK;
  MH_HIP(ctx, hipMemcpy(out_host, st->B.cand + (size_t)slot * st->B.cand_cap, (size_t)take * sizeof(SiftCandidate),
                        hipMemcpyDeviceToHost));
  std::vector<unsigned int> own(st->B.owner_elems);
  MH_HIP(ctx, hipMemcpy(own.data(), st->B.owner + (size_t)slot * st->B.owner_elems, own.size() * sizeof(unsigned int),
                        hipMemcpyDeviceToHost));
  const unsigned prefix = sift_own_prefix(st->plan, st->own_epoch);
  std::vector<size_t> first(st->plan.n_octaves, 0);
  for (int o = 1; o < st->plan.n_octaves; ++o) first[o] = first[o - 1] + (size_t)st->plan.rows[o - 1] * st->plan.cols[o - 1];
  for (int i = 0; i < take; ++i) {
    const mh_sift_candidate& q = out_host[i];
    won_host[i] = 0;
    if (q.octave < 0 || q.octave >= st->plan.n_octaves || q.r < 0 || q.r >= st->plan.rows[q.octave] || q.c < 0 ||
        q.c >= st->plan.cols[q.octave])
      continue;
    won_host[i] = own[first[q.octave] + (size_t)q.r * st->plan.cols[q.octave] + q.c] == (prefix | q.key) ? 1 : 0;
  }
  return MH_OK;
}

int mh_sift_debug_keys(mh_ctx* ctx, int slot, mh_sift_key* out_host, int cap, int32_t* n) {
  SiftState* st = last_sift(ctx, slot, "mh_sift_debug_keys");
  if (!st || !out_host || cap < 0 || !n) return MH_ERR_ARG;
  MH_HIP(ctx, hipSetDevice(ctx->device));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int32_t head[4];
  MH_HIP(ctx, hipMemcpy(head, st->B.counters + 4 * slot, sizeof head, hipMemcpyDeviceToHost));
  *n = std::min(head[1], st->B.key_cap);
  const int take = std::min(*n, cap);
  if (take > 0)
    MH_HIP(ctx, hipMemcpy(out_host, st->B.keys + (size_t)slot * st->B.key_cap, (size_t)take * sizeof(SiftKey),
                          hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_sift_debug_describe(mh_ctx* ctx, int slot, const mh_sift_key* keys_host, int n, int workgroups, float* desc_host,
                           float* xy_host, float* scale_ori_host) {
  const char* const who = "mh_sift_debug_describe";
  SiftState* st = last_sift(ctx, slot, who);
  if (!st) return MH_ERR_ARG;
  if (!keys_host || n < 1 || workgroups < 0 || workgroups > 65536 || !desc_host || !xy_host) {
    ctx->err = std::string(who) + ": bad argument";
    return MH_ERR_ARG;
  }
  // what the kernel takes on trust from the key stage: a level that exists, a window that can be counted, orders that
  // rank the keys
  std::vector<unsigned long long> orders(n);
  for (int i = 0; i < n; ++i) {
    const mh_sift_key& k = keys_host[i];
    const bool level = k.octave >= 0 && k.octave < st->plan.n_octaves && k.index >= 1 && k.index <= 3;
    const bool window = k.fsize > 0.f && k.fsize <= 64.f && fabsf(k.frow) <= 1e6f && fabsf(k.fcol) <= 1e6f && fabsf(k.ori) <= 8.f;
    if (!level || !window) {   // (a NaN fails the comparisons)
      ctx->err = std::string(who) + ": key " + std::to_string(i) +
                 (level ? ": fsize in (0, 64], |frow|, |fcol| <= 1e6 and |ori| <= 8 are taken"
                        : ": octave / index outside the plan (keys come from Gaussian levels 1..3)");
      return MH_ERR_ARG;
    }
    orders[i] = k.order;
  }
  std::sort(orders.begin(), orders.end());
  if (std::adjacent_find(orders.begin(), orders.end()) != orders.end()) {
    ctx->err = std::string(who) + ": the keys' order values are not distinct";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  hipStream_t s = ctx->stream;
  const size_t un = (size_t)n;
  // everything temporary: the context's key buffer, counters and outputs stay as the extraction left them
  DevBuf<SiftKey> keys;
  DevBuf<int32_t> count, n_out;
  DevBuf<float> desc, xy, scale_ori;
  hipError_t e = keys.ensure(un, s);
  if (e == hipSuccess) e = count.ensure(1, s);
  if (e == hipSuccess) e = n_out.ensure(1, s);
  if (e == hipSuccess) e = desc.ensure(un * 128, s);
  if (e == hipSuccess) e = xy.ensure(un * 2, s);
  if (e == hipSuccess) e = scale_ori.ensure(un * 2, s);
  const int32_t n32 = n;
  if (e == hipSuccess) e = hipMemcpyAsync(keys, keys_host, un * sizeof(SiftKey), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(count, &n32, sizeof n32, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    launch_sift_describe(st->plan, st->B.pyramid + (size_t)slot * st->plan.floats, keys, count, n,
                         workgroups ? workgroups : SIFT_KEY_WORKGROUPS, desc, xy, scale_ori, n_out, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(desc_host, desc, un * 128 * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(xy_host, xy, un * 2 * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && scale_ori_host)
    e = hipMemcpyAsync(scale_ori_host, scale_ori, un * 2 * sizeof(float), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);   // (before the buffers go)
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    ctx->err = std::string(who) + ": " + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  return MH_OK;
}

int mh_sift_debug_blur(mh_ctx* ctx, int variant, const float* src_host, int src_rows, int src_cols, float sigma, int half,
                       float* dst_host, float* dog_host, float* half_host) {
  if (!ctx || !src_host || !dst_host || src_rows <= 0 || src_cols <= 0 || src_rows > 32767 || src_cols > 32767) {
    if (ctx) ctx->err = "mh_sift_debug_blur: bad argument";
    return MH_ERR_ARG;
  }
  MH_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc_stream = mh::use_stream(ctx)) return rc_stream;
  const int rows = half ? src_rows >> 1 : src_rows, cols = half ? src_cols >> 1 : src_cols;
  const size_t spx = (size_t)src_rows * src_cols, px = (size_t)std::max(rows, 0) * std::max(cols, 0);
  // one allocation: source | dst | dog | half | scratch (8 images)
  DevBuf<float> buf;
  MH_HIP(ctx, buf.ensure(spx + 11 * std::max<size_t>(px, 1), ctx->stream));
  float *src = buf, *dst = buf + spx, *dog = dst + px, *hdst = dog + px, *scratch = hdst + px;
  int rc = MH_OK;
  hipError_t e = hipMemcpyAsync(src, src_host, spx * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (launch_sift_blur_variant(variant, src, src_rows, src_cols, sigma, half ? 1 : 0, dst, dog_host ? dog : nullptr,
                                 half_host ? hdst : nullptr, scratch, ctx->stream)) {
      ctx->err = "mh_sift_debug_blur: this variant does not take these arguments";
      rc = MH_ERR_ARG;
    } else {
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(dst_host, dst, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && dog_host) e = hipMemcpyAsync(dog_host, dog, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && half_host) e = hipMemcpyAsync(half_host, hdst, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
    }
  }
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);   // (before buf goes)
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    ctx->err = std::string("mh_sift_debug_blur: ") + hipGetErrorString(e);
    return MH_ERR_HIP;
  }
  return rc;
}

}  // extern "C"
