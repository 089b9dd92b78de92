// mh_ctx: device state kept across frames (the analogue of the kd-tree
// MATCH_ANN_CPU keeps between frames, MATCH_ANN_CPU.hpp:70) plus the per-frame
// device buffers.  Everything lives in HBM; host pointers only at the C ABI.
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "devbuf.h"
#include "screen.h"
#include "steps.h"

// The model database in HBM.  Contexts (= frames in flight) of one device may share one store
// (mh_db_share): one upload and one copy per GPU instead of one per frame slot, and one set of lines in
// the Infinity Cache for all frames in flight.  A store that is shared is never resized or rewritten:
// an upload into a context whose store has other users gives that context a fresh store.  An edit (db_edit.hip) never
// writes the live store either: it fills a second buffer set and the editing context flips to it.
struct DbStore;

// The buffer sets of one edited database: the reserved capacity and one idle set (the spare) that the next edit writes.
// Shared by the contexts that share the store; a set parks here when its last holder lets go of it (retire_store).
struct DbPool {
  std::mutex mu;
  size_t cap_rows = 0;       // mh_db_reserve: rows every new set is allocated for (0: as many as the edit needs)
  int max_models = 0;        // mh_db_reserve: models the contexts' per-model tables are sized for
  DbStore* spare = nullptr;  // idle set, owned
  ~DbPool();
};

struct DbStore {
  int device = 0;
  int N = 0, n_models = 0;
  int32_t index_base = 0;
  int n_blocks = 0;            // > 1: the rows are n_blocks runs of global rows (mh_db_upload_blocks; RowMap, common.h)
  mh::DevBuf<int32_t> blk_glo;   // device [n_blocks]: first global row of each block
  mh::DevBuf<int32_t> blk_llo;   // device [n_blocks + 1]: first local row of each block, N at the end
  mh::DevBuf<float> desc;        // [rows padded to 128][128], zero padding rows
  mh::DevBuf<float> norm;        // [padded] dot(d,d), +inf on padding rows
  mh::DevBuf<float> xyz;         // [padded][3]
  mh::DevBuf<int32_t> model;     // [padded]
  size_t cap = 0;                // rows every one of the four holds (written after the last of them has its size)
  mh::DevBuf<_Float16> desc_h;   // f16 image for the screen (match_screen.hip)
  mh::DevBuf<float> neg_h;       // [tiles][192] -norm/2 per row + row-block extrema (screen.h)
  size_t cap_h = 0;              // elements of desc_h, once neg_h has its size too
  mh::DevBuf<unsigned int> stats;
  mh::ScreenDb screen;
  // what an edit needs to know (host side): the rows are grouped by model in ascending order, and then model m's rows
  // are [model_begin[m], model_begin[m + 1]) (empty models allowed)
  bool grouped = false;
  std::vector<int32_t> model_begin;   // [n_models + 1] when grouped
  mh::DevBuf<int32_t> model_begin_dev;   // ... and its device copy (hull.hip), written with it by the upload and by every edit
  uint64_t generation = 0;            // edits since the upload (mh_db_generation)
  hipEvent_t ready = nullptr;         // recorded behind the edit that filled this set (mh_db_adopt waits on it)
  std::shared_ptr<DbPool> pool;       // where the set parks when its last holder lets go (none: it is freed)
  ~DbStore() {   // (the arrays free themselves afterwards: hipFree finds a block's device by itself)
    if (!ready) return;
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    hipSetDevice(device);
    hipEventDestroy(ready);
    if (have) hipSetDevice(cur);
  }
};

inline DbPool::~DbPool() { delete spare; }

// Deleter of every store: a set whose pool has no spare becomes the spare (its holders are done with it: the editing
// context waited for its stream, an adopting one for the event behind its last frame on the old set); any other set is
// freed -- and hipFree stalls the device.
inline void retire_store(DbStore* st) {
  if (!st) return;
  std::shared_ptr<DbPool> pool = std::move(st->pool);
  st->pool.reset();
  if (pool) {
    std::lock_guard<std::mutex> lock(pool->mu);
    if (!pool->spare && st->n_blocks <= 1 && st->cap >= pool->cap_rows) {
      pool->spare = st;
      return;
    }
  }
  delete st;
}
inline std::shared_ptr<DbStore> make_store(int device) {
  std::shared_ptr<DbStore> st(new DbStore, retire_store);
  st->device = device;
  return st;
}

// ScreenDb's scalars from the eight statistics words (launch_db_to_half / db_splice_kernel + the aggregate kernels)
inline void screen_from_stats(DbStore* st, const unsigned int h[8]) {
  float dd_max, x_max;
  std::memcpy(&dd_max, &h[0], 4);
  std::memcpy(&x_max, &h[1], 4);
  st->screen.dbh = st->desc_h;
  st->screen.dneg = st->neg_h;
  st->screen.dmax = std::sqrt(dd_max);
  std::memcpy(&st->screen.spread, &h[3], 4);   // (0 for a DB of fewer than 32 rows: no whole block, never used)
  st->screen.zero_idx = (int32_t)h[4];
  std::memcpy(&st->screen.zero_d1, &h[5], 4);
  std::memcpy(&st->screen.zero_d2, &h[6], 4);
  st->screen.usable = h[2] == 0 && x_max < 60000.f;   // (a NaN coordinate reads as a huge bit pattern: not < 60000)
}

// A lane: a few streams for the kernels whose workgroups take whole compute units (passes A and B of the two-stage
// MATCH), either confined to a CU mask that leaves `reserve` units of every XCD to everything else, or of lower priority
// than the contexts' own streams.  Shared by the contexts (= frames in flight) of a device (mh_lane_create).
struct mh_lane {
  int device = 0;
  std::vector<hipStream_t> streams;
  unsigned next = 0;   // round-robin hand-out to contexts
  int reserve = 0, low_priority = 0;
};

struct mh_ctx {
  int device = 0;
  int n_cus = 0;   // compute units of the device (mh_create)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;

  // ---- model database (resident; the arrays belong to `store`, these are its pointers) ----
  std::shared_ptr<DbStore> store;
  int N = 0, n_models = 0;
  int32_t index_base = 0;
  mh::RowMap rmap;               // local row <-> global row of the store (one block at index_base unless uploaded in blocks)
  float* db_desc = nullptr;      // [N][128]
  float* db_norm = nullptr;      // [N]
  float* db_xyz = nullptr;       // [N][3]
  int32_t* db_model = nullptr;   // [N]
  mh::ScreenDb sdb;
  mh::ScreenBufs sbuf;           // the screen's per-frame scratch as the launches take it: views of `screen_own`
  struct ScreenOwn {             // ... which ensure_match_scratch sizes together (sbuf.q_pad says for how many queries)
    mh::DevBuf<_Float16> qh;
    mh::DevBuf<uint8_t> qbad;
    mh::DevBuf<unsigned char> part;
    mh::DevBuf<float> tau;
    mh::DevBuf<uint2> recs, ovf;
    mh::DevBuf<int32_t> ovf_cnt;   // per query: overflow records, or (16x16x32 launches) the records of its counted list
    mh::DevBuf<unsigned int> stats, inc;
  } screen_own;
  int match_mode = -1;           // mh_match_set_mode
  // mh_match_set_accept: 0 = resident frames hand MATCH their ratio (frame_accept_ratio), mh_match* never; > 0 = mh_match /
  // mh_normalize_match hand it this ratio as well; < 0 = nobody does
  float match_accept = 0.f;
  int pose_split = 1;            // mh_pose_set_split: POSE as two launches (hypotheses, one-wavefront refines) in the frame paths
  // ---- edits of the resident DB (db_edit.hip) ----
  std::shared_ptr<DbPool> pool;      // buffer sets of the store this context edits or adopted
  int db_models_reserved = 0;        // mh_db_reserve's max_models: mh_reserve / mh_reserve_batch size the per-model tables for it
  struct HeldStore {                 // mh_db_adopt: the previous store, kept until `done` (recorded on this context's stream at adoption) has completed
    std::shared_ptr<DbStore> store;
    hipEvent_t done = nullptr;
  };
  std::vector<HeldStore> held;
  std::vector<hipEvent_t> held_events;   // idle events of released entries
  mh::DevBuf<float> db_stage;        // an edit's new rows: [rows][128] descriptors, [rows] norm terms, [rows][3] coordinates
  struct Planar {                    // mh_db_splice_image[s]: FEAT's lists of the images being taught, the selection's results
    mh::DevBuf<float> desc, xy;      // device [images][cap][128], [images][cap][2]
    mh::DevBuf<float> rows_desc, rows_xyz;   // device [images][cap] selected rows (batch; the host copy of a single edit)
    mh::DevBuf<int32_t> words;       // device [6][MH_MAX_BATCH]: FEAT's counts | kept counts | FEAT's 4 counter words per image
    mh::DevBuf<float> box;           // device [MH_MAX_BATCH][6]
    // mh_db_*_view[s]: the selection's statistics; mh_db_append_view's duplicate test: FEAT's descriptors normalised,
    // their norm terms, MATCH's answer
    mh::DevBuf<int32_t> stats;       // device [MH_MAX_BATCH][8]
    mh::DevBuf<float> qn, qnorm, m_d1, m_d2;   // device [cap][128], [cap], [cap], [cap]
    mh::DevBuf<int32_t> m_idx;       // device [cap]
    // the merge of re-seen points (view_merge.hip): per keypoint the row it re-observes and its X_model, the marks of
    // the touched rows; mh_db_merge_view's results: s as handed to the host, its normalised copy with the norm terms
    mh::DevBuf<int32_t> mg_obs_row, mg_touched;   // device [cap], [rows]
    mh::DevBuf<float> mg_obs_xyz;                 // device [cap][3]
    mh::DevBuf<int32_t> mg_idx, mg_views_in, mg_views_out, mg_n;   // device [rows] x 3, [1]
    mh::DevBuf<float> mg_desc, mg_desc_n, mg_norm, mg_xyz, mg_box;   // device [rows][128] x 2, [rows], [rows][3], [6]
    mh::DevBuf<uint8_t> keep;                     // mh_db_keep_rows' flags, device [rows]
  } planar;
  int db_edit_route = 0;             // 0: the fused pass (db_splice_kernel); 1: device copies + the upload's preparation (mh_db_debug_route)
  hipEvent_t db_ev[2] = {nullptr, nullptr};   // around an edit's pass over the rows when timing is on (mh_db_edit_ms)
  bool db_ev_valid = false;
  uint32_t match_launches[3] = {0, 0, 0};   // MATCH launch sequences by kernel: VALU, f32 matrix pipe, two-stage (mh_match_launches)
  struct mh_lane* lane = nullptr;   // mh_set_lane: where the chip-filling MATCH passes run (not owned)
  hipStream_t lane_stream = nullptr;
  hipEvent_t lane_in = nullptr, lane_out = nullptr;

  // ---- per-frame buffers ----
  int max_q = 0, max_clusters = 0, max_objects = 0;
  mh::DevBuf<float> q_desc;      // [max_q][128] staging for host-pointer entry points
  mh::DevBuf<float> q_norm;      // [max_q]
  mh::DevBuf<float> q_uv;        // [max_q][2]
  mh::DevBuf<int32_t> nn_idx;    // [max_q]
  mh::DevBuf<float> nn_d1;       // [max_q]
  mh::DevBuf<float> nn_d2;       // [max_q]
  mh::DevBuf<mh::Top2> match_scratch;
  mh::DevBuf<float> match_pack;  // queries re-laid out for scalar loads (match.hip)

  // generic byte scratch for host-pointer entry points
  mh::DevBuf<unsigned char> scratch;
  mh::PinBuf<unsigned char> pinned;
  // mh_frame_run_host's write-back of the normalised descriptors: a stream of its own behind an event recorded right
  // after normalize_kernel, so that the 1.5 MB copy runs beside MATCH .. FILTER2 instead of after them
  hipStream_t wb_stream = nullptr;
  hipEvent_t wb_ev = nullptr;
  bool wb_pending = false;   // a write-back is in flight on wb_stream (mh_frame_wait_descriptors)

  // mh_step_*: the frame's six slots one call each (api_step.hip).  step: where the resident frame stands and what the
  // host needs to know to read its results back.
  struct StepState {
    int done = -1;          // last stage run on the resident frame (-1: none / invalidated)
    int Q = 0, M = 0;       // queries, accepted matches
    int n_clusters = 0;     // clusters POSE / POSE2 will work on (CLUSTER's, then FILTER's)
    int n_slots = 0;        // object slots in use
    mh_cam cam;
    std::vector<int32_t> model_off;   // host copy of the per-model offsets into the match list
    std::vector<int32_t> valid;       // slots that hold an object, ascending = the host's list order
    std::vector<int32_t> valid_model; // ... and the model of each
  } step;

  // frame state (group / cluster / pose / filter): frame.h, allocated by frame_rest.hip
  struct FrameState* fs = nullptr;
  struct SiftState* sift = nullptr;   // pyramid + keypoint buffers of the SIFT extractor (api_sift.hip)
  struct UndistortState* und = nullptr;   // undistortion maps + staging (undistort.hip); made on first use
  bool und_on = false;                // mh_frame_set_undistort: the image paths remap before FEAT
  float und_dist[4] = {0, 0, 0, 0};   // ... with these k1, k2, p1, p2 and the frame camera's K
  int32_t* feat_count_dev = nullptr;  // frame enqueued from an image: device word with its keypoint count
  mh::DevBuf<int32_t> img_counts;     // mh_frame_enqueue_image_batch: [MH_MAX_BATCH] keypoint counts of the batch's images (device)
  int feat_expected = 0;              // keypoints of the last fetched image frame (sizes the next MATCH launch)
  int feat_last = -1;
  const float4* batch_img[MH_MAX_BATCH] = {};   // depth maps of the frames of a batch (mh_frame_set_depth_image_batch)
  const float* batch_fill[MH_MAX_BATCH] = {};
  int batch_imgs = 0;                 // how many of them are set (0: one depth map, one frame)
  const int32_t* exchange_tags = nullptr;   // comm.hip: shard 0's tag words in the gathered buffer (checked by the frame's first launch)

  // N > 1 (comm.hip): the send / receive blocks of the frame exchange, the flush buffer of the last frames
  struct Exchange {
    mh::DevBuf<int32_t> local;      // [3][B Q] top-2 words + B result heads
    mh::DevBuf<int32_t> gathered;   // world of those
    size_t stride = 0;              // words
    int world = 0, batch = 0, bq = 0;
    mh::DevBuf<unsigned char> flush;
    std::vector<int32_t> host;
  } ex;

  // frames with several images (mh_frame_set_images): image of every query + the cameras; n_images == 1 = off
  const int32_t* q_img = nullptr;     // device, [Q]
  mh::DevBuf<int32_t> hf_img;         // mh_frame_run_host's copy of the per-query image indices
  mh::DevBuf<mh::DevCam> cams_dev;    // device, [MH_MAX_IMAGES]: the table mh_frame_set_images fills
  const mh::DevCam* cams_view = nullptr;   // the table the kernels read (not owned): cams_dev, or imf.cams while mh_frame_enqueue_images runs
  int n_images = 1;

  // frames with several cameras from device images (mh_frame_enqueue_images[_batch]): FEAT writes every image's list at a
  // stride of `cap` rows here, images_pack_kernel hands them over to the frames' packed lists (images_pack.hip)
  struct ImagesFrame {
    mh::DevBuf<float> desc;        // device [rows][128]
    mh::DevBuf<float> xy;          // device [rows][2]
    mh::DevBuf<int32_t> words;     // device [3][MH_MAX_BATCH]: FEAT's count per image | the clamped count per image | the total per frame
    mh::DevBuf<int32_t> q_img;     // device: image index of every row of the packed lists
    mh::DevBuf<mh::DevCam> cams;   // device [MH_MAX_IMAGES]: the rig of the call in flight (the table of mh_frame_set_images stays the caller's)
    int n_live = 0;                // images of the frame whose total feat_count_dev names (0: not such a frame)
    int last_n = 0;                // mh_frame_image_counts: images of the frame last fetched, their clamped counts
    int32_t last[MH_MAX_IMAGES] = {};
    int und_n = 0;                 // mh_frame_set_undistort_images: cameras with coefficients of their own (0 = off)
    float und_dist[MH_MAX_IMAGES][4] = {};
  } imf;

  // optional depth attributes of the current queries (moped3d residuals)
  const mh_depth* q_depth = nullptr;
  int depth_kind = 0;
  float depth_alpha = 0.5f;
  mh::DepthImage depth_img;      // or: the depth map itself, looked up per match on the device (DEPTHMAP_PROP)

  // moped3d depth rules (mh_frame_set_depth_rules): DEPTHFILTER / DEPTHFILTER2 / adaptive ratio
  struct DepthRuleState {
    bool on = false;
    int patch = 64;
    float feature_filter = -1.f, match_filter = -1.f;   // Density * 100 * 100; < 0 = off
    float K[4] = {0, 0, 0, 0};
    float max_depth = 4.f, default_depth = 1.f, cauchy_scale = 0.1f;
    mh::DevBuf<float> ratio_table;  // device [n_models][4]
    int table_models = 0;           // models of the table in use (0: none)
    mh::DevBuf<double> inv_size;    // device [patches]
    mh::DevBuf<int32_t> cnt;        // device [n_models][patches], zero between frames
    mh::DevBuf<uint8_t> keep1;      // device [max_q]
    // what the last frame's front end left in these buffers (mh_depth_rules_debug_fetch): patches and queries per
    // frame, the result slots [first, first + frames) whose maps lie frame after frame, which arrays were written
    struct Last {
      int patches = 0, q = 0, first = 0, frames = 0;
      bool inv = false, keep = false, depth = false;
    } last;
  } rules;

  // moped3d CLUSTER_LINKAGE instead of mean shift (mh_frame_set_cluster_linkage)
  bool linkage_on = false;
  // moped3d CLUSTER_WEIGHTED_MEAN_SHIFT instead (mh_frame_set_cluster_wms; whichever of the two was set last is on)
  bool wms_on = false;
  mh::WmsParams wms;
  mh::DevBuf<int32_t> wms_members;        // MH_WMS_MEMBER_FACTOR x max_m: the frame's clusters' members (they may overlap)
  mh::DevBuf<unsigned char> wms_state;    // the kernel's per-point / per-model state (wms_state_bytes)
  mh::LinkageParams linkage;
  mh::DevBuf<float> own_depth;    // device copies of a host depth / distance map (ensure_own_depth)
  mh::DevBuf<float> own_fill;
  mh::DevBuf<uint8_t> own_gray;   // device copy of a host gray image (mh_frame_run_kinect_host)
  mh::DevBuf<unsigned char> own_raw;   // device copy of a host's raw sensor depth (mh_depth_map_from_raw_host)
  // the frames' images as the camera delivers them (mh_frame_set_image_format; image_gray.hip)
  bool img_fmt_on = false;
  mh_raw_image img_fmt = {};
  mh::DevBuf<uint8_t> img_stage;       // the converted gray images of the call in flight (not undistortion's staging)
  mh::DevBuf<unsigned char> img_raw;   // device copy of a host's raw image (mh_image_gray_host)
  mh::DevBuf<float> lk_scratch;
  mh::DevBuf<unsigned char> df_buf;   // mh_depth_fill[_batch]: [status words | per frame: downscaled depths, downscaled distances]
  int df_mode = 0;                    // mh_depth_fill_set_mode (MH_DEPTH_FILL_REPLAY); LEVELS: [status words | stats | per frame: depthfill.hip]
  int df_lv_frames = 0;               // frames of the last fill if it was a LEVELS one (mh_depth_fill_stats), else 0
  size_t lk_scratch_limit = (size_t)4 << 30;   // bytes; mh_set_linkage_scratch_limit
  int lk_mode = 0;                                // mh_linkage_set_mode (MH_LINKAGE_SCAN)
  mh::DevBuf<unsigned long long> lk_stats;        // MH_LINKAGE_ROWMAX: problems, merges, rows rescanned, largest n (mh_linkage_stats)

  // moped3d FILTER_PROJECTION_DEPTH instead of FILTER_PROJECTION (mh_filter_depth_set_points, mh_frame_set_filter_depth)
  struct FilterDepthState {
    mh::DevBuf<float> pts;        // device [total][3]: the models' test points, model after model
    mh::DevBuf<int32_t> off;      // device [n_models + 1]
    int n_models = 0;             // 0: no points set
    int db_models = 0;            // the context's database when they were set: its model count (mh_db_size) ...
    uint64_t db_generation = 0;   // ... and its generation (mh_db_generation)
    bool on[2] = {false, false};  // the frames' FILTER / FILTER2 are the depth class
    mh_filter_depth_params prm[2] = {};
    mh_cam cam = {};              // the depth map's K and pose
    int debug_form = 0;           // mh_filter_depth_debug_form: 0 the workgroup form, 1 filter_depth_score_wave
  } fdepth;
  int depth_verify_debug_form = 0;  // mh_depth_verify_debug_form: 0 a workgroup per object, 1 a wavefront per object (depth_verify.hip)
  // DEPTH_VERIFY behind the frames (mh_frame_set_depth_verify): one launch of depth_verify_frame_kernel behind FILTER2
  struct VerifyState {
    bool on = false;
    mh_depth_verify_params prm = {};
    mh_cam cam = {};                  // the depth map's K and pose
    // device [MH_MAX_BATCH] slots of {int32 n_before; int32 pad[3]; mh_verify_record[max_objects]}, and the slots' tickets
    mh::DevBuf<unsigned char> block;
    mh::DevBuf<unsigned int> tickets;
    size_t slot_bytes = 0;
    bool slot_on[MH_MAX_BATCH] = {};  // per result slot: the frame enqueued last into it ran with the verification
  } verify;
  int hull_debug_form = 0;          // mh_hull_debug_form: 0 the octagon prefilter, 1 sort and chain every point (hull.hip)
  // object hulls behind the frames (mh_frame_set_hulls): one launch of hull_frame_kernel behind FILTER2 (or POSE)
  struct HullState {
    int max_vertices = 0;             // 0 = off
    int image = 0;                    // the camera of a several-camera frame whose hulls are wanted
    mh::DevBuf<unsigned char> block;  // device [MH_MAX_BATCH] slots of max_objects records (hull_record_words, hull.h)
    size_t slot_bytes = 0;            // ... bytes of a slot: the frame state's max_objects records
    int block_vertices = 0;           // ... whose records hold that many vertices
    mh::DevBuf<float2> scratch;       // sort scratch of the launch's workgroups (models of more than MH_HULL_LDS_POINTS rows)
    const DbStore* scratch_store = nullptr;   // ... sized for the largest model of this store
    uint64_t scratch_generation = 0;          // ... at this generation
    // per result slot: the max_vertices the frame enqueued last into it ran with (0: hulls were off, or no frame yet)
    int slot_vertices[MH_MAX_BATCH] = {};
    hipEvent_t done = nullptr;        // mh_frame_fetch_batch_hulls_async: recorded behind the copy (mh_frame_fetch_wait)
    bool pending = false;
  } hulls;
  // the last frame or batch enqueued: frames, 1 = they shared their launches, 1 = FILTER in the POSE tails, depth class
  // bits (mh_frame_route; written by frame_rest on the host)
  int32_t frame_route[4] = {0, 0, 0, 0};

  // mh_frame_fetch_batch_async / mh_frame_fetch_previous_async: delivery of a batch's objects into the caller's pinned block
  struct Delivery {
    hipEvent_t done = nullptr;          // recorded behind the delivery on the context's stream
    bool pending = false;
    mh::DevBuf<unsigned char> stage;    // device staging for blocks the device cannot write directly
    unsigned char* host_block = nullptr;   // the pending delivery's destination, as the caller knows it
    int B = 0, max_objects = 0;
    uint32_t tag = 0;
  } dlv;

  bool timing = false;
  hipEvent_t ev[10] = {};
  static constexpr int MEV_SETS = 32;
  hipEvent_t mev[MEV_SETS][6] = {};   // around the kernels of the two-stage MATCH, one set per launch sequence (mh_match_timing)
  int mev_next = 0, mev_used = 0;     // ring position, sets recorded since the last mh_match_timing
  bool ev_made = false;
};

namespace mh {

#define MH_HIP(ctx, call)                                                         \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);             \
      return MH_ERR_HIP;                                                          \
    }                                                                             \
  } while (0)

int use_stream(mh_ctx* ctx);  // make sure ctx->stream is valid (creates the own stream lazily)
void bind_store(mh_ctx* ctx);   // the context's view of its store (api.hip)
void db_poll_held(mh_ctx* ctx, bool wait);   // db_edit.hip: let go of adopted-away stores whose event has completed (wait: all of them)
// The depth FILTER (mh_frame_set_filter_depth).  filter_depth_points_ok: the test points are set, for n_models models, and
// the context's database is the one they were set for -- else MH_ERR_ARG with `who` in the message.
// filter_depth_frame_ok: what an entry point asks before it enqueues anything of a frame that has the depth FILTER in
// a slot (no such frame: MH_OK) -- a depth map, one camera, no shards' blocks (`sharded`), the points.
int filter_depth_points_ok(mh_ctx* ctx, const char* who, int n_models);
int filter_depth_frame_ok(mh_ctx* ctx, const char* who, const mh_frame_params* prm, int n_cameras = 1, bool sharded = false);
// ... and, asked by the same entry points at the same place, while hulls are on (mh_frame_set_hulls; off: MH_OK): no shards'
// blocks, the wanted camera among the frame's, a store with whole models in ascending order
int hulls_frame_ok(mh_ctx* ctx, const char* who, int n_cameras, bool sharded);
// ... and while DEPTH_VERIFY is on (mh_frame_set_depth_verify; off, or a frame without FILTER2: MH_OK): a depth map, one
// camera, no shards, a store of whole models
int depth_verify_frame_ok(mh_ctx* ctx, const char* who, const mh_frame_params* prm, int n_cameras, bool sharded);
int ensure_frame_buffers(mh_ctx* ctx, int Q);
int ensure_scratch(mh_ctx* ctx, size_t bytes);
int ensure_pinned(mh_ctx* ctx, size_t bytes);
int ensure_own_depth(mh_ctx* ctx, size_t px);   // own_depth [px][4] and own_fill [px]
int ensure_match_scratch(mh_ctx* ctx, int Q);
// depthmap.hip: a host's raw sensor depth uploaded into own_raw and its xyzn map built into own_depth, on the context's
// stream, after every check of mh_depth_map_from_raw_host (`who` in the message); no wait
int depth_map_from_raw_own(mh_ctx* ctx, const char* who, const void* raw_host, const mh_raw_depth* raw, const float K[4],
                           int width, int height);
// MATCH of Q normalised queries against the context's DB on its stream: exact (idx1, d1, d2) per query, by the
// two-stage screen when it pays and the DB allows it, else by the exact kernels (bit-identical results either way).
// accept_ratio > 0: the caller applies `d1 / d2 < accept_ratio` (match_accepted) to every result and reads nothing else of
// a query that fails it; the screen may then answer such a query with (-1, inf, inf) (ScreenBufs::accept_ratio).
int ctx_match(mh_ctx* ctx, const float* qn, const float* qnorm, int Q, int32_t* idx1, float* d1, float* d2,
              const int32_t* q_count = nullptr, int q_expected = 0, float accept_ratio = 0.f);
// what a resident single-GPU frame hands ctx_match: its ratio, unless the context adjusts the ratio by depth
// (rules.ratio_table: group_kernel's ratio is then another for every match) or mh_match_set_accept(-1) switched it off
inline float frame_accept_ratio(const mh_ctx* ctx, const mh_frame_params* prm) {
  return ctx->match_accept >= 0.f && !ctx->rules.ratio_table && prm && prm->ratio > 0.f ? prm->ratio : 0.f;
}
// Delivery of a batch's heads into a caller's host block (api_frame.hip): delivery_begin -> where the delivering kernel
// writes (the block itself when the device can address it, else the context's staging buffer); delivery_end -> the copy
// out of the staging buffer if one is needed, and the event behind it all.
int delivery_begin(mh_ctx* ctx, void* host_block, size_t bytes, unsigned char** dst_dev);
int delivery_end(mh_ctx* ctx, void* host_block, size_t bytes, unsigned char* dst_dev, int B, int max_objects, uint32_t tag);
int sift_into(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size, int cap,
              float* desc_dev, float* xy_dev, int32_t** n_dev_out, int32_t* count_word = nullptr);
// undistort.hip: n device images remapped with the map of (width, height, K, ctx->und_dist) into the context's staging
// buffer, one launch on the context's stream; staged[f] = image f's undistorted copy
int undistort_frame(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int width, int height, const float K[4],
                    const uint8_t** staged);
int sift_into_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int width, int height, int double_size, int cap,
                    float* desc_dev, float* xy_dev, int32_t* count_words);
// image_gray.hip, while mh_frame_set_image_format is on (off: both MH_OK, nothing done).  image_format_frame_ok: the
// frame's size is the format's, else MH_ERR_ARG with `who` -- asked before anything of the context changes.
// image_format_stage: the n raw device images of a call converted by one launch on the context's stream into its staging
// buffer; staged[f] = image f's gray copy (staged may be raw_dev itself).  image_format_bytes: what a host image spans.
int image_format_frame_ok(mh_ctx* ctx, const char* who, int width, int height);
int image_format_stage(mh_ctx* ctx, const uint8_t* const* raw_dev, int n, const uint8_t** staged);
size_t image_format_bytes(const mh_ctx* ctx, int width, int height);
// undistort.hip: the same for a rig -- image f is camera f % n_cams' and gets the map of (cams[..].K, dist[..])
int undistort_frame_images(mh_ctx* ctx, const uint8_t* const* gray_dev, int n, int n_cams, int width, int height,
                           const mh_cam* cams, const float (*dist)[4], const uint8_t** staged);

// images_pack.hip: the hand-over from FEAT's strided per-image lists to the packed lists of n_frames frames of n_images
// cameras each, one launch.  Image j = f n_images + i has sdesc + j cap 128, sxy + j cap 2 and its count in scount[j]
// (clamped to cap here); frame f's list starts at row f n_images cap of desc / uv / q_img, image after image, its length
// goes to totals[f], the clamped counts to counts[j], the rig to cams_dev.
struct ImagesPackArgs {
  const float* sdesc;
  const float* sxy;
  const int32_t* scount;
  float* desc;
  float* uv;
  int32_t* q_img;
  int32_t* totals;
  int32_t* counts;
  DevCam* cams_dev;
  int cap, n_images;
  DevCam cams[MH_MAX_IMAGES];
};
void launch_images_pack(const ImagesPackArgs& a, int n_frames, hipStream_t s);

// planar.hip: FEAT's lists -> model rows (createPlanarModelsFromImages, moped.cpp:196-236), one launch, workgroup i =
// image i.  Image i reads desc + i cap 128, xy + i cap 2 and n[i]; it writes its kept rows at desc_out / xyz_out + i
// out_pitch rows (desc_copy: a second copy of the descriptors, or null), at most out_cap of them, their count to
// n_out[i] and their bounding box to bbox + 6 i.
struct PlanarArgs {
  const float* desc;
  const float* xy;
  const int32_t* n;
  int cap;
  mh_planar_spec spec;
  int all;   // the region of interest is "every keypoint"
  float* desc_out;
  float* desc_copy;
  float* xyz_out;
  size_t out_pitch;
  int out_cap;
  int32_t* n_out;
  float* bbox;
};
void launch_planar_rows(const PlanarArgs& a, int n_images, hipStream_t s);
// MH_ERR_ARG (and ctx->err) for a spec mh_db_splice_image refuses; *all = its roi means every keypoint
int planar_spec_check(mh_ctx* ctx, const char* who, const mh_planar_spec* spec, int* all);
// view_rows.hip: FEAT's lists + a Kinect view each (depth map, pose) -> model rows at the measured 3-D points, one
// launch, workgroup i = view i; lists and outputs laid out as PlanarArgs', stats + 8 i.  dup_on: the duplicate test
// against dup's MATCH result (view i's at + i cap); dup.row_begin .. row_end: old rows folded into the box.
struct ViewArgs {
  const float* desc;
  const float* xy;
  const int32_t* n;
  int cap;
  int w, h;
  mh_view_spec spec;
  int roi_all, box_all, dup_on;
  mh_view_dup dup;
  float* desc_out;
  float* desc_copy;
  float* xyz_out;
  size_t out_pitch;
  int out_cap;
  int32_t* n_out;
  float* bbox;
  int32_t* stats;
  struct View {
    const float4* map;
    const float* fill;
    float pose[7];
  } v[MH_MAX_BATCH];
};
void launch_view_rows(const ViewArgs& a, int n_views, hipStream_t s);
// MH_ERR_ARG (and ctx->err) for a spec, views or map size mh_db_splice_view refuses; fills a's spec, flags and views
int view_args_check(mh_ctx* ctx, const char* who, const mh_view* views, int n_views, int width, int height,
                    const mh_view_spec* spec, ViewArgs* a);
// view_merge.hip: the keypoints of view 0 of `v` that rule 7 drops (v.dup, v.dup_on; the selection's outputs in v are not
// used), folded into the rows [v.dup.row_begin, v.dup.row_end) they re-observe -- the arithmetic above mh_view_merge_dev.
struct MergeArgs {
  ViewArgs v;
  const float* qn;            // the list's descriptors as MATCH saw them, [cap][128]
  const float* old_desc;      // the store's descriptors, [v.dup.n_db_rows][128]
  const int32_t* views_in;    // [rows], or null: every count is 1
  int32_t* obs_row;           // scratch [cap]
  float* obs_xyz;             // scratch [cap][3]
  int32_t* touched;           // scratch [rows]
  int32_t* merged_idx;        // [merged_cap], relative to row_begin, ascending
  float* merged_desc;         // [merged_cap][128]: s, not normalised
  float* merged_desc_copy;    // a second copy, or null
  float* merged_xyz;          // [merged_cap][3]
  int merged_cap;
  int32_t* n_merged;          // the full count
  int32_t* views_out;         // [rows]
};
int launch_view_merge(mh_ctx* ctx, const MergeArgs& m);
int ensure_view_merge(mh_ctx* ctx, int cap, int rows);   // the scratch arrays of ctx->planar
void launch_view_merge_scatter(const int32_t* idx, const int32_t* n_merged, int cap, const float* desc, const float* norm,
                               const float* xyz, float* stage_desc, float* stage_norm, float* stage_xyz, hipStream_t s);
// bbox[6] = Model::boundingBox of xyz[0, n_fixed + *n_more) (n_more may be null)
void launch_view_box(const float* xyz, int n_fixed, const int32_t* n_more, float* bbox, hipStream_t s);
// rows [b, b + rows) of (desc, norm, xyz) whose flag is set, packed in order into the stage arrays; their box
void launch_view_keep(const uint8_t* keep, int b, int rows, const float* desc, const float* norm, const float* xyz,
                      float* stage_desc, float* stage_norm, float* stage_xyz, float* bbox, hipStream_t s);
// api_sift.hip: the four counter words of image `slot` of the context's last extraction (device): [1] keys found, [2] != 0:
// a list overflowed
const int32_t* sift_counters_dev(mh_ctx* ctx, int slot);

}  // namespace mh
