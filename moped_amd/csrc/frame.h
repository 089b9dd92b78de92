// The device-resident frame: FrameState (its buffers on the device), FrameCall (what one run of the rest chain works
// from) and the functions of frame_rest.hip that the entry points (api_frame.hip, api_stage.hip, api_step.hip) share.
#pragma once
#include "context.h"
#include "steps.h"

// Device buffers of one frame.  Match records are kept sorted by (model, query):
// matches[model] of the reference is the slice [model_off[m], model_off[m+1]).
constexpr int FETCH_PIN_OBJECTS = 32;   // objects that come with a frame's head in mh_frame_fetch's first copy

struct FrameState {
  int max_m = 0, max_clusters = 0, max_objects = 0, n_models_cap = 0;
  // The working arrays below (counts .. tickets) are carved out of ONE allocation of MH_MAX_BATCH equal arenas: the
  // pointers name frame 0's copy, frame f of a batch that goes through the stages in one launch (FrameBatch, steps.h)
  // has its own at + f * arena_bytes.  Results and count snapshots are slot-indexed arrays outside the arenas.
  mh::DevBuf<unsigned char> arena;
  size_t arena_bytes = 0;
  int n_arenas = 1;   // copies allocated: 1 until the first merged batch of B frames asks for B
  mh::FrameCounts* counts = nullptr;
  int32_t* n_slots = nullptr;      // object slots in use (device scalar)
  int32_t* n_clusters = nullptr;   // rows of the current cluster table (device scalar)
  // ... and of the table FILTER rewrites for POSE2: a word of its own -- a POSE launch's workgroups read every frame's
  // cluster count as they walk the batch, and the frame's closing workgroup (fused FILTER) may have rewritten the table
  // by the time a workgroup without a task in that frame comes by
  int32_t* n_clusters2 = nullptr;
  // group
  int32_t *acc_q = nullptr, *acc_model = nullptr, *m_q = nullptr, *m_model = nullptr, *m_rep = nullptr;
  mh_corr* m_corr = nullptr;
  // several images: image of every match; the matches again in (model, image, query) order for CLUSTER / POSE
  int32_t *m_img = nullptr, *mi_img = nullptr, *off2 = nullptr;
  mh_corr* mi_corr = nullptr;
  mh_depth* m_depth = nullptr;     // per match, when the frame carries depth attributes
  int32_t* model_off = nullptr;
  // cluster
  int32_t *ms_members = nullptr, *ms_cl_start = nullptr, *ms_ncl = nullptr;
  bool list_wms = false;   // the last frame's CLUSTER was the weighted mean shift: members in ctx->wms_members, MH_WMS_MEMBER_FACTOR x model_off apart
  int32_t *cl_model = nullptr, *cl_begin = nullptr, *cl_count = nullptr;
  // objects
  int32_t *obj_model = nullptr, *obj_ninl = nullptr, *obj_cluster = nullptr, *obj_valid = nullptr,
          *obj_npts = nullptr, *obj_clsize = nullptr;
  float *obj_pose = nullptr, *obj_err = nullptr, *obj_score = nullptr, *obj_score_raw = nullptr;
  // filter
  unsigned long long* best = nullptr;
  int32_t* new_members = nullptr;
  // POSE as two launches (PoseSplit, steps.h): the tasks' winning hypotheses, scratch for clusters past the refine's LDS cache
  mh::PoseHyp* hyp = nullptr;
  float* rf_pts = nullptr;
  int32_t* rf_list = nullptr;
  // packed result {int32 n; int32 pad[3]; mh_object[max_objects]}
  mh::DevBuf<unsigned char> result;
  size_t result_bytes = 0;
  mh::DevBuf<int32_t> snap;  // [4] counts snapshot: matches, clusters, objects after POSE, after FILTER
  int task_grid = 32;   // workgroups for the POSE/FILTER launches: follows the task count of the last fetched frame
  int ms_grid = 8;      // ... and of the CLUSTER launch: its cluster count + head room
  // result slots whose match lists are still in the arenas: [list_first, list_first + list_n) (frame_rest, from its call's slot)
  int list_first = 0, list_n = 1;
  // ... and what CLUSTER's per-"model" lists of those frames are lists of: 1 = models (model_off), n_images > 1 = (model,
  // image) pairs in (model, image) order (off2 over mi_corr) -- the debug reads of api_frame.hip follow it
  int list_pairs = 1;
  // What the last launches found, written by the kernels' tails into host-visible (pinned, mapped) words and read -- without
  // any synchronisation: a guess is all it is -- when the next launches are sized: [0][f] (cluster, replica) tasks of POSE
  // in frame f of the batch, [1][f] of POSE2, [2][f] models that CLUSTER had to cluster.
  mh::PinBuf<int32_t> fb;
  // mh_frame_fetch[_slot]: where the frame's head, counters and first objects land -- pinned, so that the copies are
  // enqueued together and one synchronisation ends them (into pageable memory every one of them blocks: four round
  // trips, ~40 us of one synchronous frame's 550)
  struct FetchPin {
    int32_t head[4];
    mh_object objects[FETCH_PIN_OBJECTS];
    int32_t snap[4];
    mh::FrameCounts fc;
    int32_t n_feat;
    int32_t img_n[MH_MAX_IMAGES];   // mh_frame_enqueue_images: the images' clamped counts lie right behind the frame's total (one copy)
  };
  mh::PinBuf<FetchPin> fetch_pin;
  // one frame alone: the closing workgroup of FILTER2 writes the frame's head, counters and objects HERE itself
  // (page-locked, device-writable): mh_frame_fetch then synchronises and reads -- no copy at all
  mh::PinBuf<mh::FrameHostBlock> host_block;
  bool host_armed = false;   // the frame enqueued last writes host_block (a batch, a frame without FILTER2: no)
  uint32_t host_seq_expect = 0;   // armed enqueues so far = what host_block->seq reads once the last of them is through
  // the fused FILTER / FILTER2 steps' arguments on the device + what the host last stored there (FilterFuse, steps.h)
  mh::DevBuf<mh::FilterFuseArgs> fuse_dev;   // [2]
  mh::FilterFuseArgs fuse_shadow[2];
  bool fuse_valid[2] = {false, false};
  unsigned int* tickets = nullptr;  // [8] last_workgroup() words: 0 CLUSTER, 1 POSE, 2 FILTER, 3 POSE2, 4 FILTER2
};

// Everything ONE call of frame_rest works from; the context holds only what outlives a call (the DB, the buffers, the
// depth map / rules / linkage / image indices as their setters left them, exchange_tags).
struct FrameCall {
  const float* q_uv;   // the frame's keypoints (batch_n > 1: frame 0's, the others behind them)
  int Q;
  const mh_cam* cam;
  const mh_frame_params* prm;
  uint64_t seed;
  const uint64_t* seeds = nullptr;   // batch_n > 1: the frames' seeds
  int batch_n = 1;                   // > 1: that many frames in one launch per stage (FrameBatch, steps.h), slots 0 ..
  // exchange-1 blocks ([n_shards][3][Q]) to merge first, or nullptr: the context's top-2 arrays hold the frame's MATCH
  const int32_t* gathered = nullptr;
  int n_shards = 0;
  int shard_stride = 0;   // words between the shards' blocks (0 = packed: 3 Q)
  int plane_stride = 0;   // words between the idx / d1 / d2 planes of one block (0 = packed: Q)
  int slot = 0;    // result / snap slot the frame writes
  int q0 = 0;      // the frame's first entry in nn_idx / nn_d1 / nn_d2 and q_depth (a batch matched in one launch; 0 with `gathered`)
  int frame = 0;   // the frame's slice of q_img (per-query image indices lie frame after frame)
  int stage_lo = 0, stage_hi = 5;   // the stages to launch (mh_step_*): 0 MATCH's tail .. 5 FILTER2
  // the frame's own depth map where a batch has one per frame (mh_frame_set_depth_image_batch); nullptr: the context's
  const float4* img = nullptr;
  const float* fill = nullptr;
  // the frame's keypoint count on the device where FEAT made the keypoints (batch_n > 1: one word per frame), nullptr: Q
  const int32_t* q_count = nullptr;
};

namespace mh {

// what an entry point that enqueues work begins with: the context's device current, its stream valid
inline int enter(mh_ctx* ctx) {
  MH_HIP(ctx, hipSetDevice(ctx->device));
  return use_stream(ctx);
}

// frame_rest.hip
int ensure_fs(mh_ctx* ctx, int max_m, int max_clusters, int max_objects, int n_models, int n_arenas = 1);
int prepare_frame(mh_ctx* ctx, int Q, int q_frame = 0, int frames = 1);
int frame_rest(mh_ctx* ctx, const FrameCall& c);
int ensure_wms_buffers(mh_ctx* ctx);   // ctx->wms_members / wms_state for what ctx->fs holds
bool merged_batch_ok(const mh_ctx* ctx, const mh_frame_params* prm, bool attrs_ok = false, int maps_for = 0);
int ensure_batch_arenas(mh_ctx* ctx, int B);
int ensure_linkage_scratch(mh_ctx* ctx, size_t floats);
FilterBuffers make_fb(const FrameState* fs, int n_models);
// filter_depth_kernel's arguments from the context's test points, a depth map and the class's parameters (the per-object
// outputs stay off)
FilterDepthArgs make_filter_depth_args(const mh_ctx* ctx, const DepthImage& dimg, const mh_filter_depth_params& prm,
                                       const mh_cam& depth_cam);
void stamp(mh_ctx* ctx, int i);

// api_frame.hip.  The frame's cameras into the context's device table.
int upload_cams(mh_ctx* ctx, const mh_cam* cams, int n_images);
// A frame from features on the device: normalise, MATCH, then the stages [stage_lo, stage_hi] of the rest chain.
// write_back: ctx->wb_ev is recorded behind the normalisation (mh_frame_run_host copies the descriptors back from there).
struct FeatureOptions {
  int stage_lo = 0, stage_hi = 5;
  bool write_back = false;
};
int enqueue_features(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q, const mh_cam* cam,
                     const mh_frame_params* prm, uint64_t seed, const FeatureOptions& opt);
// ... and from features in host memory (mh_frame_run_host_begin; mh_step_match, with a stage range)
int host_frame_begin(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                     const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, const FeatureOptions& opt);

}  // namespace mh
