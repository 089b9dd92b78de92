/* include/moped_hip.h -- C ABI of libmoped_hip.so
 *
 * MI355X (gfx950) implementation of libmoped's per-frame hot path
 *   MATCH (brute-force 2-NN + ratio) -> CLUSTER (mean shift) -> POSE (RANSAC + LM)
 *   [-> FILTER -> POSE2 -> FILTER2]
 * behind plain C entry points: opaque context, plain pointers and sizes, int
 * status (0 = ok, < 0 = error, text via mh_last_error), never aborts, never
 * throws.  One context per pipeline; calls on one context are serialised by the
 * caller (libmoped calls its steps from one thread, src/moped.cpp:184-191).
 *
 * What each entry point replaces (paths relative to moped2/libmoped/):
 *   mh_db_upload        MATCH_ANN_CPU::Update            src/match/MATCH_ANN_CPU.hpp:72-109
 *   mh_db_splice        Moped::addModel / removeModel    src/moped.cpp:139-159 (+ the Update() they trigger)
 *   mh_db_splice_image[s]  Moped::createPlanarModelsFromImages  src/moped.cpp:196-236 (image -> model of the store)
 *   mh_planar_rows_dev  ... its loop over detectedFeatures  src/moped.cpp:220-232
 *   mh_db_splice_view / mh_db_append_view / mh_db_append   (no counterpart: a model from Kinect views, grown view by view)
 *   mh_db_merge_view / mh_db_keep_rows   moped-modeling-py src/MopedModeling.py:863-894, :915 (one descriptor per point from all
 *                       its observations, nviews; here the plain mean, on the device, view by view)
 *   mh_models_write_xml the file samples/createModels/createModels.cpp:121-126 writes (sXML::print, include/sXML.hpp:146-170)
 *   mh_normalize        MATCH_ANN_CPU::norm              src/match/MATCH_ANN_CPU.hpp:54-57
 *   mh_match            MATCH_ANN_CPU::process search    src/match/MATCH_ANN_CPU.hpp:155-165
 *                       (= MATCH_FLANN_CPU::process      src/match/MATCH_FLANN_CPU.hpp:133-191)
 *   mh_match_local /    the same search on one model shard + the cross-shard
 *   mh_match_merge      top-2 merge (new: the reference has one kd-tree over all
 *                       models, MATCH_ANN_CPU.hpp:76-107)
 *   mh_meanshift        CLUSTER_MEAN_SHIFT_CPU::MeanShift src/cluster/CLUSTER_MEAN_SHIFT_CPU.hpp:80-158
 *   mh_pose_ransac      POSE_RANSAC_LM_DIFF_REPROJECTION_CPU::RANSAC/process
 *                                                        src/pose/POSE_RANSAC_LM_DIFF_REPROJECTION_CPU.hpp:76-211,264-307
 *   mh_pose_ransac_depth  POSE_RANSAC_LM_DIFF_BACKPROJECTION_DEPTH_CPU / ..._REPROJECTION_DEPTH_CPU
 *                       moped3d/libmoped/src/pose/POSE_RANSAC_LM_DIFF_BACKPROJECTION_DEPTH_CPU.hpp:108-325,
 *                       moped3d/libmoped/src/pose/POSE_RANSAC_LM_DIFF_REPROJECTION_DEPTH_CPU.hpp:106-216
 *   mh_project_test     testAllPoints / project()        …REPROJECTION_CPU.hpp:166-180, include/moped.hpp:330-354
 *   mh_filter           FILTER_PROJECTION_CPU::process   src/filter/FILTER_PROJECTION_CPU.hpp:80-162
 *   mh_filter_depth     FILTER_PROJECTION_DEPTH_CPU::process   moped3d .../filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329
 *   mh_depth_verify     DEPTH_VERIFY_CPU::process        moped3d .../depthVerify/DEPTH_VERIFY_CPU.hpp:86-208
 *   mh_frame_*          the per-frame loop over those steps, MopedPimpl::processImages
 *                                                        src/moped.cpp:166-194 (device-resident form)
 *
 * Pointer arguments named *_host are host memory; *_dev are device (HBM)
 * pointers on the context's device.  Poses are (qx,qy,qz,qw,tx,ty,tz) as in
 * MopedNS::Pose (include/moped.hpp:136-164); intrinsics K = (fx,fy,cx,cy) as in
 * Image::intrinsicLinearCalibration (include/moped.hpp:233).
 */
#ifndef MOPED_HIP_H
#define MOPED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_DESC_DIM 128
#define MH_MAX_BATCH 32  /* frames one context can carry through one MATCH launch (mh_frame_enqueue_batch / _sharded_batch) */
#define MH_MAX_IMAGES 8    /* images (cameras) of one frame (mh_frame_set_images, mh_*_images) */
#define MH_MAX_MODELS 8192   /* models a context's frames can address (sharded: the global count); more -> MH_ERR_CAPACITY */
#define MH_OK 0
#define MH_ERR_ARG (-1)
#define MH_ERR_HIP (-2)
#define MH_ERR_CAPACITY (-3)
#define MH_ERR_NODEVICE (-4)

typedef struct mh_ctx mh_ctx;

/* ---- context ------------------------------------------------------------ */

/* Selects `device`, checks it is a gfx950 part, creates the context's stream.
 * Failure is the signal for a STEP plugin to set capable = false
 * (src/util.hpp:151-159). */
int mh_create(int device, mh_ctx** out);
void mh_destroy(mh_ctx* ctx);
const char* mh_last_error(const mh_ctx* ctx);
/* Run subsequent work on a caller-owned hipStream_t (e.g. the stream a
 * framework uses); NULL restores the context's own stream. */
int mh_set_stream(mh_ctx* ctx, void* hip_stream);
int mh_synchronize(mh_ctx* ctx);
/* Capacities of the per-frame device buffers (defaults: 16384 queries, 16384
 * matches, 1024 clusters, 4096 objects). Call before the first frame. */
int mh_reserve(mh_ctx* ctx, int max_queries, int max_clusters, int max_objects);
/* The same for a context that will carry BATCHES: `frames` <= MH_MAX_BATCH frames of up to `queries_per_frame` queries
 * each per mh_frame_enqueue_batch / _sharded_batch / _rest_frames call.  The MATCH buffers are sized for all
 * frames x queries_per_frame queries of a launch, the working arrays of CLUSTER..FILTER2 once per frame for
 * queries_per_frame matches each (mh_reserve would size every one of them for the whole launch), so that no enqueue
 * ever has to stop the stream and reallocate. */
int mh_reserve_batch(mh_ctx* ctx, int queries_per_frame, int frames, int max_clusters, int max_objects);

/* ---- model database (A2) -------------------------------------------------- */

/* desc_host: N x 128 row-major, ALREADY L2-normalised by the caller (the
 * reference normalises model descriptors in place in Update(), :94);
 * model_of_host[N]: model index of each row, 0..n_models-1 (a shard passes global model
 * ids and the global n_models); a value outside that range -> MH_ERR_ARG;
 * xyz_host: N x 3 model coordinates.  index_base: value added to row numbers in
 * every index this context reports (global row id of row 0 when the DB is a
 * shard).  Re-upload after modelsUpdated(). */
int mh_db_upload(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host,
                 const float* xyz_host, int N, int n_models, int32_t index_base);
/* The same for a shard whose rows are SEVERAL runs of global rows -- a rank that owns models m, m + W, m + 2 W, ...
 * of the flattened database (round-robin assignment: SURVEY 8(e) "interleave model -> GPU to balance POSE"; the
 * one-tree order it must preserve is MATCH_ANN_CPU::Update's, src/match/MATCH_ANN_CPU.hpp:76-107).  The N rows are
 * the blocks one after the other; block b holds global rows [block_global_row[b], + block_rows[b]); blocks in
 * ascending global order, so a tie between two rows breaks the same way as in the unsharded database.  Every index
 * the context reports is a global row.  normalize != 0: L2-normalise on the device (A1). */
int mh_db_upload_blocks(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host, const float* xyz_host, int N,
                        int n_models, const int32_t* block_global_row, const int32_t* block_rows, int n_blocks,
                        int normalize);
int mh_db_size(const mh_ctx* ctx, int* N, int* n_models);
/* Let `dst` use the database `src` holds: same device, no copy -- one upload and one HBM copy per GPU
 * however many contexts (frames in flight) work against it.  The analogue of the ONE kd-tree every
 * frame of the reference searches (MATCH_ANN_CPU.hpp:70,106).  The store lives as long as its last
 * user; a later mh_db_upload into either context gives that context a new store of its own and leaves
 * the other one's untouched.  Frames already enqueued on `dst` finish on its old database first. */
int mh_db_share(mh_ctx* dst, mh_ctx* src);

/* ---- edits of the resident database: addModel / removeModel (src/moped.cpp:139-159) ------------------------------
 * The reference serves a change of the model set by rebuilding its kd-tree over all models (modelsUpdated() ->
 * MATCH_ANN_CPU::Update, src/match/MATCH_ANN_CPU.hpp:72-109).  Here one model is added, replaced or removed ON THE
 * DEVICE, while the other contexts' frames keep flowing.  All three are one splice of the row array,
 *   new = old[0, b) ++ rows ++ old[e, N),
 * and what an edit leaves equals, byte for byte, what mh_db_upload_raw makes of the same rows.
 *
 * Editable: a store whose rows are grouped by model in ascending order (empty models allowed), uploaded in one block
 * with index_base 0 -- or no store at all (an empty one).  Every entry point below returns MH_ERR_ARG on anything
 * else, and on a model index out of range, before anything is launched; the store is then as it was.  Sharded stores
 * (index_base != 0, mh_db_upload_blocks) are not editable: every rank's global rows would have to move together. */
enum { MH_DB_INSERT = 0, MH_DB_REPLACE = 1, MH_DB_REMOVE = 2 };
/* Rows of model `model` of the context's store: [*row_begin, *row_begin + *n_rows). */
int mh_db_model_rows(const mh_ctx* ctx, int model, int32_t* row_begin, int32_t* n_rows);
/* INSERT: the n_rows rows become model `model` (0 .. n_models; n_models = append, what addModel does for a new name,
 *   moped.cpp:146); later models move up by one.
 * REPLACE: model `model` gets these rows and keeps its index (addModel with a known name, moped.cpp:141-144).
 * REMOVE: model `model` leaves, later models move down by one (removeModel, moped.cpp:152-159); desc / xyz unused.
 * desc [n_rows][128], xyz [n_rows][3]: host pointers, or device pointers with on_device != 0 (e.g. the rows
 * mh_frame_features_dev hands out).  normalize != 0: the rows are raw and are L2-normalised on the device
 * (MATCH_ANN_CPU.hpp:94), else they are normalised already, as for mh_db_upload.
 *
 * Ordered on the context's stream: frames this context enqueued before the edit finish on the old arrays, frames
 * enqueued after it search the new ones.  The one host wait is the read-back of the statistics words, as in
 * mh_db_upload.  The edit fills a second buffer set and the context flips to it; contexts that share the old store
 * keep it, untouched, until they adopt the new one (mh_db_adopt).  The per-frame capacities of the context follow
 * the new model count at its next frame unless mh_db_reserve sized them. */
int mh_db_splice(mh_ctx* ctx, int op, int model, const float* desc, const float* xyz, int n_rows, int normalize,
                 int on_device);
/* Capacity for edits: the live buffer set and one spare for max_rows rows each, staging for the new rows of an edit
 * (up to 65536; larger models grow it), and -- through mh_reserve / mh_reserve_batch called AFTER this -- per-model
 * tables for max_models models.  Inside that capacity an edit allocates and frees nothing: it fills the spare, and
 * the set it retires becomes the spare once its last holder has let go.  If the spare is still held (contexts that
 * have not adopted the previous edit), the edit allocates a fresh set; a retired set beyond the one spare is freed,
 * and THAT FREE STALLS THE DEVICE (hipFree waits for all of it).  Callable with or without a store. */
int mh_db_reserve(mh_ctx* ctx, int64_t max_rows, int max_models);
/* Stream-ordered mh_db_share: `dst` takes the store `src` holds now without blocking the host.  dst's stream waits
 * for the event the edit recorded; dst's frames in flight finish on the store it had, which dst holds until an event
 * recorded on its own stream here has completed (polled at dst's later calls, waited for in mh_destroy). */
int mh_db_adopt(mh_ctx* dst, mh_ctx* src);
/* Edits since the upload of the store the context holds: a host sees which contexts have yet to adopt. */
int mh_db_generation(const mh_ctx* ctx, uint64_t* generation);
/* For tests and measurements, in the style of mh_sift_debug_*.  which: 0 desc [rows padded to 128][128] f32, 1 norm
 * [padded], 2 xyz [N][3], 3 model [N], 4 desc_h [padded][128] f16, 5 neg_h [padded / 128][192] f32 (4, 5: nothing when
 * the store has no f16 image).  bytes beyond what the store defines -> MH_ERR_ARG.  Synchronises the context. */
int mh_db_debug_fetch(mh_ctx* ctx, int which, void* out_host, size_t bytes);
/* {bits of dmax, bits of spread, zero_idx, bits of zero_d1, bits of zero_d2, usable, has an f16 image, N} */
int mh_db_debug_screen(mh_ctx* ctx, uint32_t out[8]);
/* 0: edits run the fused pass (default); 1: device copies + the upload's preparation (the route it is measured against) */
int mh_db_debug_route(mh_ctx* ctx, int route);
/* Device time of the last edit's pass over the rows (after mh_enable_timing), without staging and aggregates. */
int mh_db_edit_ms(mh_ctx* ctx, float* ms);

/* ---- MATCH ---------------------------------------------------------------- */

/* A1: in-place L2 normalisation of n descriptors on the device, bit-identical
 * to MATCH_ANN_CPU::norm.  Host round trip. */
int mh_normalize(mh_ctx* ctx, float* desc_host, int n);

/* A3: exact 2-NN of Q normalised queries against the uploaded DB, squared L2.
 * nn_idx[i] = row (index_base applied) of the nearest descriptor if
 * d1/d2 < ratio, else -1; nn_raw (optional) = the nearest row regardless of the
 * ratio test; d1/d2 (optional) = best / second-best squared distance. */
int mh_match(mh_ctx* ctx, const float* q_host, int Q, float ratio,
             int32_t* nn_idx, int32_t* nn_raw, float* d1, float* d2);
/* mh_normalize + mh_match in one call, as MATCH_ANN_CPU::process does both to a frame's descriptors
 * (moped2/libmoped/src/match/MATCH_ANN_CPU.hpp:155-165: norm() in place, then the search): q_host [Q][128] goes up
 * raw, is normalised on the device and comes back normalised; results as mh_match.  One upload and one
 * synchronisation instead of two of each (what MATCH_BRUTE_HIP calls). */
int mh_normalize_match(mh_ctx* ctx, float* q_host, int Q, float ratio, int32_t* nn_idx, int32_t* nn_raw, float* d1,
                       float* d2);

/* How MATCH ran on this context since the last reset: stats[0] = candidate rows the exact stage evaluated,
 * stats[1] = queries searched by brute force inside it (candidate list overflow, or a query the f16
 * screen cannot represent), stats[2] = queries through the two-stage path, stats[3] = 1 if a MATCH of
 * `Q` queries against the current DB takes the two-stage path (f16 screen + exact rescoring), 0 if it
 * takes the exact kernels.  Synchronises the context's stream. */
int mh_match_stats(mh_ctx* ctx, int Q, uint32_t stats[4], int reset);
/* Which kernels search: -1 (default) = the two-stage path when the work is large enough (Q x N >= 8e6,
 * N >= 4096) and every DB row is finite and inside f16's range, 0 = always the exact f32 kernels (the
 * VALU kernel below 1536 queries, the f32 matrix-pipe kernel from there), 1 = the two-stage path whenever
 * the DB allows, 2 = the exact VALU kernel (match_kernel) whatever the query count, 3 = the exact f32
 * matrix-pipe kernel (match_mfma_kernel) whatever the query count.  The results are the same bits in every
 * mode (tests/test_gpu_match_kernels.py compares them). */
int mh_match_set_mode(mh_ctx* ctx, int mode);
/* POSE / POSE2 of the device-resident frame paths as two launches (1, the default: the hypotheses of every (cluster,
 * replica) task, then the refines on one wavefront each) or as one (0: the workgroup that found a task's winner refines it
 * on one of its four wavefronts).  The objects are the same bits either way (tests/test_gpu_frame.py); the per-step entry
 * points (mh_pose_ransac*) and frames with stage timing always run the one-launch form. */
int mh_pose_set_split(mh_ctx* ctx, int on);
/* MATCH launch sequences this context has issued, by the kernel that searched: out[0] = match_kernel (VALU),
 * out[1] = match_mfma_kernel (f32 matrix pipe), out[2] = the two-stage path.  Host counters, no synchronisation;
 * for tests that must know which kernel produced a result. */
int mh_match_launches(mh_ctx* ctx, uint32_t out[3]);
/* The two-stage path's error model (host arithmetic, no device needed): a row can be one of a query's
 * two nearest only if its f16 screen value exceeds T - mh_screen_margin(dot(q,q), max row norm), T =
 * any lower bound of the second largest screen value.  Exposed so that tests can check the bound. */
float mh_screen_margin(float qq, float dmax);
/* More of the same, for tests (none of these is on a frame's path):
 *   mh_screen_values        the screen value of every (query, row) pair for Q queries (a multiple of 32; host, [Q][128],
 *                           as the caller normalised them) against the first n_rows rows (a multiple of 32) of the
 *                           uploaded DB, computed on the device by pass A's arithmetic -- f16 operands, accumulator
 *                           seeded with -dot(d,d)/2, the block's f16 MFMAs in ascending k (either shape) -- so that the error
 *                           model can be held against what the HARDWARE's matrix pipe accumulates, not an emulation of
 *                           it; *dmax / *spread (optional) = the DB statistics the thresholds use.  The DB needs an
 *                           f16 image (>= 4096 rows).
 *   mh_screen_record_value  the 16-bit value a candidate record of pass B carries for a block whose largest dot
 *                           product is `top` under the threshold `thr` = tau - the block's largest -dd/2
 *   mh_screen_record_bounds what pass C concludes from it: *hi >= the largest screen value among the record's rows,
 *                           *lo <= it (or -inf); it drops the record when hi < (second largest lo) - mh_screen_margin.
 *                           Host arithmetic, the same inline function the kernel runs. */
int mh_screen_values(mh_ctx* ctx, const float* q_host, int Q, int n_rows, float* out_host, float* dmax, float* spread,
                     int shape /* 0 = the MFMA shape the large launches use, 1 = 32x32x16, 2 = 16x16x32 */);
uint16_t mh_screen_record_value(float top, float thr);
void mh_screen_record_bounds(uint16_t value_bits, uint32_t row0, float tau, float spread, int N, float dmax, float* lo,
                             float* hi);
/* The one-sweep launches (pass A of the large launches keeps the identity of its best 8-row blocks, pass B leaves the
 * sampled tiles out); host arithmetic for tests, the same inline functions the kernels run:
 *   mh_screen_pack_value    a block's largest screen value with the block's number `id` in its low `bits` mantissa bits
 *   mh_screen_pack_pert     a bound of |packed - value| for every screen value of a query with dot(q,q) = qq
 *   mh_screen_sample_bounds what pass C concludes from the record of a sampled tile's block (value_bits = f16 of packed
 *                           value - tau): *lo <= the block's largest screen value <= *hi
 *   mh_screen_launch_plan   how a two-stage MATCH of Q queries (q_expected of them expected, 0 = Q) against N rows is
 *                           launched: out = {1 if one sweep, first sampled tile, sampling stride, sampled tiles, pass A
 *                           splits, identity bits, pass B splits, pass B tiles}; all zero when the launch does not run
 *                           on the 16x16x32 passes
 *   mh_screen_plan          the whole plan of that call, for either kernel family: out = {family (32 = the 32x32x16
 *                           passes with lane-private record lists, 16 = the 16x16x32 passes with counted lists), 32-query
 *                           blocks per wavefront; pass A: first tile, stride, tiles, splits, identity bits, 1 if one
 *                           sweep; pass B: tiles, splits, slots per sub-list (0 = counted lists), first skipped tile, skip
 *                           stride (0 = none skipped); record slots per query pass C scans (0 = by the list's count)}
 *   mh_screen_park_places   hits a wavefront of pass B of the 16x16x32 launches parks in LDS during its sweep before
 *                           further hits append to their queries' lists from the hit path (for tests that fill it)
 *   mh_match_incomplete     queries since the last reset for which a lane slot of pass A held more blocks above the
 *                           threshold than it keeps, so that pass C swept that slot's rows (bounded; never the brute-force
 *                           search mh_match_stats counts).  Synchronises the context's stream.
 *   mh_screen_sample_values the values pass C names the rows of a sampled tile's record by, from the code it runs: for
 *                           query q (host, [Q][128], normalised) and the two 8-row lane blocks row0[2 q], row0[2 q + 1]
 *                           (row0 = 128 tile + 32 row block + 4 quarter; bit b = row row0 + (b & 3) + 16 (b >> 2)),
 *                           out[q][8 block + b].  They are mh_screen_values(shape 2)'s, bit for bit. */
float mh_screen_pack_value(float v, uint32_t id, int bits);
float mh_screen_pack_pert(float qq, float dmax, int bits);
void mh_screen_sample_bounds(uint16_t value_bits, float tau, float pert, float dmax, float* lo, float* hi);
void mh_screen_launch_plan(int Q, int q_expected, int N, int32_t out[8]);
#define MH_SCREEN_PLAN_WORDS 14
void mh_screen_plan(int Q, int q_expected, int N, int32_t out[MH_SCREEN_PLAN_WORDS]);
int mh_screen_park_places(void);
int mh_match_incomplete(mh_ctx* ctx, uint32_t* count, int reset);
/* MATCH for a caller that applies the ratio test.  The frames' only reader of a query's (idx1, d1, d2) is the test
 * `d1 / d2 < ratio`; of a query that fails it nothing else is read.  Pass C of the two-stage MATCH holds, after its first
 * round trip, bounds of the query's two best screen values, and answers a query they prove to fail with (-1, inf, inf)
 * -- "no neighbour", which the test rejects as well -- without the search.
 *   mh_screen_reject_proved  the proof, in host arithmetic (the inline function the kernel runs): qq = dot(q,q), dmax =
 *                            the largest row norm, h1 = the largest upper bound and l2 = the second largest lower bound
 *                            (over distinct records) of a record's largest screen value, tau = the query's threshold.
 *                            1 = no exact arithmetic can give d1 / d2 < ratio; 0 for ratio <= 0, a non-finite input,
 *                            l2 = -inf or a d2 whose upper bound is not positive.
 *   mh_match_set_accept      ratio = 0 (the default): resident single-GPU frames hand MATCH their mh_frame_params::ratio
 *                            unless the context has a depth-adaptive ratio table; every mh_match* entry point, the
 *                            sharded frames, the steps and the DB edits get the exact triple of every query.
 *                            ratio > 0: mh_match / mh_normalize_match hand MATCH this ratio as well (nn_raw, d1, d2 of a
 *                            query it rejects may then read -1, inf, inf).  ratio < 0: nobody does, frames included.
 *   mh_match_prerejected     queries answered that way since the last reset.  Synchronises the context's stream. */
int mh_screen_reject_proved(float qq, float dmax, float h1, float l2, float tau, float ratio);
int mh_match_set_accept(mh_ctx* ctx, float ratio);
int mh_match_prerejected(mh_ctx* ctx, uint32_t* count, int reset);
int mh_screen_sample_values(mh_ctx* ctx, const float* q_host, int Q, const int32_t* row0_host, float* out_host);
/* mh_match_stats' candidate rows -- rows that ran the canonical chain in pass C -- per query since the last reset:
 * out[q] for the first Q queries of the context's two-stage launches.  Synchronises the context's stream. */
int mh_match_query_candidates(mh_ctx* ctx, int Q, uint32_t* out);

/* Device-pointer forms for a model-sharded DB: local top-2 of this shard
 * (idx carries index_base; -1 when the shard is empty), then the merge of S
 * shards' results laid out [S][Q] (e.g. the output of an all-gather). All
 * pointers are device memory; work is enqueued on the context's stream. */
int mh_match_local_dev(mh_ctx* ctx, const float* qn_dev, const float* qnorm_dev, int Q,
                       int32_t* idx1_dev, float* d1_dev, float* d2_dev);
/* mh_match_local_dev for Q rows of capacity of which the first min(Q, *q_count_dev) are queries, the count read on the
 * device (as the image frames have it behind FEAT): the rows behind the count get idx -1, d1 = d2 = inf without being
 * searched.  q_expected: the host's estimate of the count (sizes the launches), 0 = Q. */
int mh_match_local_counted_dev(mh_ctx* ctx, const float* qn_dev, const float* qnorm_dev, int Q,
                               const int32_t* q_count_dev, int q_expected, int32_t* idx1_dev, float* d1_dev,
                               float* d2_dev);
int mh_match_merge_dev(mh_ctx* ctx, const int32_t* idx1_s_dev, const float* d1_s_dev,
                       const float* d2_s_dev, int n_shards, int Q,
                       int32_t* idx1_dev, float* d1_dev, float* d2_dev);
/* Normalise on device: q_dev [Q x 128] in place, qnorm_dev[Q] = dot(q,q) of the
 * normalised rows (the norm term of the distance). */
int mh_normalize_dev(mh_ctx* ctx, float* q_dev, float* qnorm_dev, int Q);

/* ---- CLUSTER (A6) ----------------------------------------------------------- */

/* Mean shift of n points (dim 2 or 3) exactly as MeanShift<T,N>: label[i] =
 * cluster number in the reference's emission order, -1 for points whose canopy
 * ended below min_pts; order[] (optional, n entries) = point indices grouped by
 * cluster, in the reference's within-cluster (splice) order; n_clusters out. */
int mh_meanshift(mh_ctx* ctx, const float* pts_host, int n, int dim, float radius,
                 float merge, int min_pts, int max_iter, int32_t* label,
                 int32_t* order, int32_t* n_clusters);
/* The same for n_problems independent point sets in one call -- the per-model loop of
 * CLUSTER_MEAN_SHIFT_CPU::process (src/cluster/CLUSTER_MEAN_SHIFT_CPU.hpp:182-199): one
 * upload, one launch (a workgroup per problem), one download.  pts_host = the problems'
 * points concatenated, off[n_problems+1] = first point of each problem (off[0] = 0);
 * label / order (optional) are laid out like pts and hold problem-local indices;
 * n_clusters[n_problems]. */
int mh_meanshift_batch(mh_ctx* ctx, const float* pts_host, const int32_t* off, int n_problems,
                       int dim, float radius, float merge, int min_pts, int max_iter,
                       int32_t* label, int32_t* order, int32_t* n_clusters);

/* ---- POSE (A8-A13) ---------------------------------------------------------- */

typedef struct {
  float u, v;    /* image coordinates of the matched keypoint */
  float x, y, z; /* model coordinates of the matched point */
} mh_corr;

typedef struct {
  float K[4];    /* fx, fy, cx, cy */
  float cam[7];  /* camera pose (qx,qy,qz,qw,tx,ty,tz) */
} mh_cam;

typedef struct {
  int n_hypotheses;        /* P3P hypotheses per (cluster, replica); 0 -> 1024 */
  int max_objects_per_cluster; /* replicas per cluster (reference: 4) */
  int n_pts_align;         /* distinct 2-D points a cluster needs (5 POSE / 6 POSE2) */
  int min_n_pts_object;    /* a hypothesis needs MORE inliers than this (6 / 8) */
  float error_threshold;   /* squared pixel error of an inlier (10 / 5) */
  int lm_iters_l2;         /* LM iterations on plain residuals (default 2: a warm start; with depth residuals,
                              depth_kind 1 / 2, values 1..9 are raised to 10; 0 = no plain phase) */
  int lm_iters_l4;         /* then on the reference's squared residuals */
} mh_pose_params;

typedef struct {
  float pose[7];
  int32_t cluster;     /* input cluster this object came from */
  int32_t n_inliers;   /* inliers of the winning hypothesis */
  float err;           /* final sum of squared residuals of the refine */
} mh_pose_out;

/* RANSAC on n_clusters clusters: corr_host[cluster_off[c] .. cluster_off[c+1]).
 * out_host has capacity n_clusters * max_objects_per_cluster; *n_out = objects
 * found (cluster-major, replica order).  Deterministic for a given seed. */
int mh_pose_ransac(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* cluster_off,
                   int n_clusters, const mh_cam* cam, const mh_pose_params* prm,
                   uint64_t seed, mh_pose_out* out_host, int32_t* n_out);
/* The same with every correspondence in its own image (LmData::image, …REPROJECTION_CPU.hpp:213-237; POSE2's
 * clusters, rewritten by FILTER, mix images): image_of_host[i] in [0, n_images), cams[n_images].  A minimal
 * sample is drawn inside one image; inliers and the refinement use every point's own camera; two
 * correspondences with the same (image, coord2D) are never sampled together (:76-98). */
int mh_pose_ransac_images(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* image_of_host,
                          const int32_t* cluster_off, int n_clusters, const mh_cam* cams, int n_images,
                          const mh_pose_params* prm, uint64_t seed, mh_pose_out* out_host, int32_t* n_out);

/* moped3d (Kinect) variants: every correspondence also carries the camera-frame point
 * read from the depth map and its Cauchy weight (Match.depthData.coord3D and
 * getCauchyWeight(fillDistance), moped3d/libmoped/src/util.hpp:73-84,
 * ...BACKPROJECTION_DEPTH_CPU.hpp:194-197). */
typedef struct {
  float wx, wy, wz; /* world3D: camera-frame xyz of the keypoint from the depth map */
  float w;          /* cauchyWeight */
} mh_depth;

#define MH_DEPTH_NONE 0          /* moped2 residuals (u,v only) */
#define MH_DEPTH_BACKPROJECTION 1 /* POSE_RANSAC_LM_DIFF_BACKPROJECTION_DEPTH_CPU (moped3d default) */
#define MH_DEPTH_REPROJECTION 2   /* POSE_RANSAC_LM_DIFF_REPROJECTION_DEPTH_CPU */

/* As mh_pose_ransac, with depth_host[i] beside corr_host[i]; kind = MH_DEPTH_*, alpha =
 * the class's Alpha (0.5 in moped3d/libmoped/src/config.hpp:46,48).  Hypotheses and the
 * inlier test are the 2-D ones (the reference's testAllPoints is unchanged); the refine
 * minimises the depth-aware residuals of the chosen class. */
int mh_pose_ransac_depth(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host,
                         const int32_t* cluster_off, int n_clusters, const mh_cam* cam,
                         const mh_pose_params* prm, int kind, float alpha, uint64_t seed,
                         mh_pose_out* out_host, int32_t* n_out);

/* testAllPoints: inlier_host[i] = squared reprojection error < thr; err2_host
 * (optional) the squared error (FLT_MAX-based for z < 0.001 like project()). */
int mh_project_test(mh_ctx* ctx, const float pose[7], const mh_corr* corr_host, int n,
                    const mh_cam* cam, float thr, uint8_t* inlier_host, float* err2_host,
                    int32_t* n_inliers);

/* For verification only (tests/test_gpu_pose_rows.py), in the style of mh_sift_debug_* / mh_wms_debug_state: the device
 * functions of POSE's LM refine on one wavefront, everything they compute written out.  Host pointers, temporary device
 * buffers, one launch, synchronised; nothing of the context's frame state changes.
 *
 * mh_pose_debug_rows: kind = the points' layout, res = the residual model, one of the pairs the refine runs: (0,0)
 * (1,1) (2,2) (3,3) (1,0) (2,0).  0 reprojection, 1 back-projection + depth, 2 reprojection + depth, 3 reprojection with
 * every point in its own image.  phase 0: plain errors, 1: the reference's squared errors.  Pose R [9] row major, t [3]
 * (world frame); cams [n_images] (kinds 0..2 use cams[0]).  pts [n_pts][stride] in the kernel's own layout: u, v, x, y,
 * z, then for kind 3 the image number as an int in word 5 (stride 6), for kinds 1 and 2 wx, wy, wz, cauchyWeight (stride
 * 9); kind 0: stride 5.  list [n]: indices into pts.
 * Out, per list entry i: nrows [n], r [n][4], J [n][4][6] (rows >= nrows[i]: the word MH_POSE_DEBUG_FILL); of the whole
 * list: cost (the sum of squared rows), H [21] (upper triangle of J^T J, row by row, scaled as the refine scales it) and
 * g [6] (J^T r), each summed over the wavefront exactly as the refine sums them; devcams [n_images][16]: K [4], Rc [9],
 * tc [3] of every camera as the kernel got them.
 * MH_ERR_ARG, a message that begins with the call's name and nothing written: a null pointer; n_pts or n outside
 * 1 .. MH_POSE_MAX_PTS; a list entry outside [0, n_pts); a kind-3 image word outside [0, n_images); n_images outside
 * 1 .. MH_MAX_IMAGES; another (kind, res) pair; a phase other than 0, 1. */
#define MH_POSE_MAX_PTS 2048
#define MH_POSE_DEBUG_FILL 0xFFC0DE00u
int mh_pose_debug_rows(mh_ctx* ctx, int kind, int res, int phase, float alpha, const float R[9], const float t[3],
                       const mh_cam* cams, int n_images, const float* pts, int n_pts, const int32_t* list, int n,
                       int32_t* nrows, float* r, float* J, float* cost, float* H, float* g, float* devcams);
/* One LM step's linear algebra, the same work in all 64 lanes: *solved = whether (H + mu I) dx = -g had a Cholesky
 * factor (H [21] packed as above); dx [6], Rn [9] = exp([dx[0..2]]x) R, tn [3] = t + dx[3..5] (without a solution: every
 * word MH_POSE_DEBUG_FILL); *lanes_agree = the 64 lanes held the same words.  MH_ERR_ARG on a null pointer. */
int mh_pose_debug_step(mh_ctx* ctx, const float H[21], const float g[6], float mu, const float R[9], const float t[3],
                       int32_t* solved, float dx[6], float Rn[9], float tn[3], int32_t* lanes_agree);

/* ---- FILTER (N1) ------------------------------------------------------------- */

/* FILTER_PROJECTION_CPU::process for one image.  corr_host: all matches in
 * (model, query) order, model_off[n_models+1]; objects (model, pose) in list
 * order.  score[n_obj], keep[n_obj]; the rewritten clusters of kept objects in
 * (model, list) order: out_order[kept] object indices, cl_off[kept+1] /
 * cl_members (match index inside its model). */
/* The same for a frame whose matches come from n_images images (FILTER_PROJECTION_CPU.hpp:100-141: every match
 * is projected through *images[match.imageIdx], the ownership map is keyed by (coord2D, image)):
 * image_of_host[i] = image of match i (same order as corr_host), cams[n_images].  n_images == 1: mh_filter. */
int mh_filter_images(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* image_of_host, const int32_t* model_off,
                     int n_models, const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cams,
                     int n_images, int min_points, float feature_distance, float min_score, float* score,
                     uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off, int32_t* n_kept);
int mh_filter(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
              const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
              int min_points, float feature_distance, float min_score,
              float* score, uint8_t* keep, int32_t* out_order, int32_t* cl_members,
              int32_t* cl_off, int32_t* n_kept);

/* ---- FILTER, depth class (moped3d) ---------------------------------------------- */

/* FILTER_PROJECTION_DEPTH_CPU (moped3d/libmoped/src/filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329):
 * FILTER_PROJECTION_CPU plus a test of every object's pose against the frame's depth map.  A sample of the model's
 * own 3-D points is transformed by the pose and projected into the depth camera; where the sensor MEASURED a depth (not
 * a filled pixel) that lies behind the point, the object pays a Cauchy penalty, the "incorrect score" IS (:207-267);
 * object->score = score - IS (:270) and MinScore is applied to that (:309).  Keypoint ownership still goes by the
 * projection score (:277). */
typedef struct {
  float plausible_sq_distance;  /* PlausibleSqDistance: matches with err2 below it are the clusterSize IS is scaled to (:202-204, :266) */
  float depth_fraction;         /* DepthFraction: cauchyScale = DepthFraction * kinectDepth (:248) */
  float min_keypoint_fraction;  /* MinKeypointFraction: used <= (int)(fraction * n_test) -> IS = 0 (:260) */
} mh_filter_depth_params;

/* TestPoints (:94-116) of the context: a CSR of 3-D model points, model m's slice is xyz_host[off_host[m] ..
 * off_host[m + 1]) in the order the reference would walk TestPoints[m].  The library does not sample: which points to
 * take is the caller's choice, as the reference makes it with rand() (:78-92, :107-113).  Copied into the context.
 * n_models == 0 clears them.  The call records the context's database (model count, mh_db_generation): after an edit or
 * a new upload the points must be set again -- frames and mh_filter_depth fail with MH_ERR_ARG until then, and launch
 * nothing. */
int mh_filter_depth_set_points(mh_ctx* ctx, const float* xyz_host, const int32_t* off_host, int n_models);

/* FILTER_PROJECTION_DEPTH_CPU::process (:140-329) for one image: mh_filter's arguments and results, plus the depth map's
 * camera (:162 K = intrinsicLinearCalibration, :221 TM = its pose), the class's own parameters and, optionally, per
 * object in list order: the IS that was subtracted (:260-267), usedKeypointCount (:237) and clusterSize (:202-204).
 * The map is the one the context holds (mh_frame_set_depth_image[_host]; fill_distance NULL = every pixel measured);
 * without one, without test points for n_models models or with stale ones: MH_ERR_ARG.  A projected coordinate that is
 * NaN, infinite or outside int's range -- where the reference's (int) is undefined -- counts as off the image. */
int mh_filter_depth(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
                    const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                    int min_points, float feature_distance, float min_score, const mh_cam* depth_cam,
                    const mh_filter_depth_params* prm, float* score, uint8_t* keep, int32_t* out_order,
                    int32_t* cl_members, int32_t* cl_off, int32_t* n_kept, float* incorrect_score, int32_t* used,
                    int32_t* plausible);

/* FILTER (f1) and / or FILTER2 (f2) of the frames enqueued from now on are FILTER_PROJECTION_DEPTH_CPU (:140-329) with
 * the frame's depth map (mh_frame_set_depth_image[_batch | _host]) seen through depth_cam, MinPoints / FeatureDistance /
 * MinScore from mh_frame_params as before.  NULL: that slot stays FILTER_PROJECTION_CPU; both NULL: off.  Such a frame
 * runs its FILTER steps where a plain one does, in the tails of the POSE launches (POSE always as its two launches:
 * hypotheses, then refines), and the frames of a batch that brings a map per frame (mh_frame_set_depth_image_batch with
 * as many maps as frames) share one launch per stage, every object scored against its own frame's map; mh_frame_route
 * says which way the last one went.  The FILTER steps are launches of their own -- the same objects, bit for bit -- with
 * stage timing on (mh_enable_timing), with MH_FUSE_FILTER=0, with mh_pose_set_split(ctx, 0) / MH_POSE_SPLIT=0 and with
 * more than four objects per cluster (the one-launch POSE kernel does not carry the depth class); then, and with
 * MH_MERGE_BATCH=0 or a number of maps other than the number of frames, the frames of a batch run one after the other.
 * Frames that run one after the other with different maps and fused FILTERs cost two one-wavefront launches each: the
 * maps' addresses are stored on the device whenever they change.
 * Refused with MH_ERR_ARG before anything is enqueued: no depth map, several cameras, the sharded entry points
 * (mh_frame_enqueue_sharded*, mh_frame_enqueue_rest*), test points not set or stale.  mh_step_filter stays the plain
 * class. */
int mh_frame_set_filter_depth(mh_ctx* ctx, const mh_filter_depth_params* f1, const mh_filter_depth_params* f2,
                              const mh_cam* depth_cam);

/* How the last frame or batch enqueued on the context went through CLUSTER .. FILTER2: out[0] the frames it carried,
 * out[1] 1 if they shared one launch per stage (a merged batch), out[2] 1 if the FILTER steps ran in the tails of the
 * POSE launches (0: as launches of their own), out[3] bit 0 set if FILTER was the depth class, bit 1 if FILTER2 was.
 * Host bookkeeping of the enqueue: no device work, no synchronisation.  All zero before the first frame. */
int mh_frame_route(mh_ctx* ctx, int32_t out[4]);

/* Debug entry, like mh_sift_debug_*: the device form mh_filter_depth scores F1 with.  0 (default): a workgroup walks the
 * object slots, lane 0 adds the terms out of LDS -- the stand-alone FILTER launch of a frame.  1: one wavefront per
 * object slot and no LDS -- the form the POSE tails of a fused frame run.  The results are the same bit for bit; frames
 * ignore the setting. */
int mh_filter_depth_debug_form(mh_ctx* ctx, int form);

/* ---- DEPTH_VERIFY (moped3d) ---------------------------------------------------- */

#define MH_DEPTH_VERIFY_CHUNK 192   /* terms of one round of the workgroup form (mh_depth_verify_debug_form 0) */

/* DEPTH_VERIFY_CPU (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp): the check of every object that left
 * FILTER2 against the Kinect map.  The constructor's arguments (:64-66): */
typedef struct {
  float feature_distance;  /* FeatureDistance: a match with projectionError below it is plausible (:132) */
  float max_multiplier;    /* MaxMultiplier: the cap of keypointCount / usedKeypointCount (:194-196) */
  float max_distance;      /* MaxDistance: a keypoint on a pixel with a fill distance above it is skipped (:168) */
  float depth_fraction;    /* DepthFraction: cauchyScale = DepthFraction * kinectDepth (:182) */
} mh_depth_verify_params;

/* What the class computes for one object, and prints (:192-202) */
typedef struct {
  float qs_raw, is_raw;    /* QS and IS as :192 prints them: the two ordered chains (:135, :188) */
  float multiplier;        /* (Float)keypointCount / usedKeypointCount (:191) AFTER the cap (:194-196) */
  float qs, is;            /* QS / plausibleMatchCount, IS * multiplier / keypointCount (:197-200) */
  int32_t plausible;       /* plausibleMatchCount (:133) */
  int32_t used;            /* usedKeypointCount (:171) */
  int32_t keypoints;       /* keypointCount (:156): the rows the store holds for the model */
  int32_t keep;            /* 0: IS > QS, the reference erases the object (:204-206) */
} mh_verify_record;

/* DEPTH_VERIFY_CPU::process (:86-208) for n_obj objects, a synchronous round trip like mh_filter_depth.
 *   corr_host / model_off[n_models + 1]: the frame's matches, matches[m] = corr_host[model_off[m] .. model_off[m + 1])
 *   (:128); obj_model[n_obj] (modelNum, :121-127: indices, not names), obj_pose[n_obj][7]; cam: the image the matches
 *   were found in (project(), :129); depth_cam: the depth map's K and pose (:105, :162).
 *   The map and its distance map are the ones the context holds (mh_frame_set_depth_image[_host]; :98-116); without a
 *   distance map -- the reference would dereference null -- there is no distance test (:168) and every pixel is used.
 *   The keypoints (:142-150) are the rows the resident store holds for the model, in row order: one descriptor type.
 *   records[n_obj]: every object's numbers in list order; nothing is erased, `keep` is the verdict (:204).
 * Both scores are the reference's ordered Float += double chains, word for word.  A keypoint that projects off the map
 * (the reference reads outside the buffer there, :167 / :173), or to a coordinate that is NaN, infinite or outside int,
 * is counted in keypointCount and not used.
 * MH_ERR_ARG before any launch, records untouched: a null pointer, no depth map, no database, a store whose rows are not
 * grouped by model in ascending order or that was uploaded in blocks (mh_object_hulls' conditions), n_models other than
 * the store's, a model index outside the database, offsets that decrease.  n_obj = 0: MH_OK, nothing is done. */
int mh_depth_verify(mh_ctx* ctx, const mh_corr* corr_host, const int32_t* model_off, int n_models,
                    const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                    const mh_cam* depth_cam, const mh_depth_verify_params* prm, mh_verify_record* records);

/* Debug entry, like mh_filter_depth_debug_form: the device form mh_depth_verify runs.  0 (default): a workgroup per
 * object, three wavefronts produce MH_DEPTH_VERIFY_CHUNK terms a round into LDS and one chains them.  1: one wavefront
 * per object and no LDS.  The records are the same bit for bit. */
int mh_depth_verify_debug_form(mh_ctx* ctx, int form);

/* DEPTH_VERIFY behind the frames: prm != NULL switches the step on for the frames and batches enqueued afterwards (NULL,
 * the default: off), depth_cam is the depth map's K and pose (:105, :162).  Such a frame runs ONE more launch behind
 * FILTER2 and in front of the hull launch (mh_frame_set_hulls) -- a merged batch one launch for all its slots, and it
 * stays merged -- stream-ordered, without a host wait, the object counts read on the device.  Every object of every
 * result slot is scored against its own frame's map (mh_frame_set_depth_image[_batch | _host]) and its own frame's match
 * lists; a record per object is written in the order BEFORE the erase; then the objects with IS > QS (:204-206) are
 * removed from the result slot, stably, and its object count is lowered: every fetch path, every delivery and the hulls
 * see the reference's list.  counts[] stay as they are (counts[3] = objects after FILTER2's erase).  The frame's objects
 * come to the host by a copy from the result slot (FILTER2's direct write into the host's block is off for such a frame).
 * Frames that stop after POSE (run_stage2 = 0) and stepped frames (mh_step_*) ignore the setting.
 * While it is on, refused with MH_ERR_ARG before anything is enqueued: no depth map, several cameras, the sharded entry
 * points (mh_frame_enqueue_sharded*, mh_frame_enqueue_rest*), a store mh_depth_verify refuses. */
int mh_frame_set_depth_verify(mh_ctx* ctx, const mh_depth_verify_params* prm, const mh_cam* depth_cam);
/* The records of the frame in result slot `slot` (mh_frame_fetch_verify: slot 0), one per object that left FILTER2, in
 * that order: *n_records = their number, the first min(*n_records, max_records) are written.  The objects
 * mh_frame_fetch[_slot] returns are those with keep = 1, in the same order.  Synchronises the context's stream.
 * MH_ERR_ARG: the frame enqueued last into that slot ran without the verification. */
int mh_frame_fetch_verify_slot(mh_ctx* ctx, int slot, int max_records, mh_verify_record* records, int32_t* n_records);
int mh_frame_fetch_verify(mh_ctx* ctx, int max_records, mh_verify_record* records, int32_t* n_records);

/* ---- object hulls ------------------------------------------------------------ */

#define MH_HULL_LDS_POINTS 8192   /* points of one object the hull kernel sorts in LDS; more go through global scratch */

/* Object::getObjectHull (include/moped.hpp:266-287; moped3d/libmoped/include/moped.hpp:402-422) with its getConvexHull
 * (:293-327 / :346-380) for n_obj objects of the resident database, one workgroup per object, and beside it the
 * footprint GLOBAL_DISPLAY draws (src/GLOBAL_DISPLAY.hpp:197-207): the eight projected corners of Model::boundingBox
 * (min / max of the model's points, src/moped.cpp:107-125).  A synchronous round trip like mh_filter.
 *   obj_model[n_obj], obj_pose[n_obj][7]: the objects; cam: the image (project(), include/moped.hpp:330-354).
 *   hull_xy_host[n_obj][max_vertices][2]: the first min(n_vertices[o], max_vertices) vertices of object o in the
 *   reference's order (the backward half of the chain, newest point first, then the forward half); rows beyond them are
 *   not written.  n_vertices[n_obj]: the true count.  Collinear and duplicate points are dropped as the reference drops
 *   them (det <= 0); one projected point gives an empty hull, two give both, none (the reference: undefined) an empty one.
 *   n_behind[n_obj] (optional): model points with camera-frame z < 0.001.  They are LEFT OUT of the hull -- the
 *   reference gives them (FLT_MAX, FLT_MAX) and feeds those to the chain, whose determinants then are inf - inf.
 *   bbox_uv_host[n_obj][8][2] (optional): the corners in the order [x][y][z] of GLOBAL_DISPLAY.hpp:198-203, index 0 =
 *   min, 1 = max; a corner with z < 0.001 is (FLT_MAX, FLT_MAX) as project() returns it.
 * The hull is over the rows the store holds for the model: one descriptor type (the reference walks every type's points).
 * The vertices are bit for bit the reference's for the same projected points.
 * MH_ERR_ARG before any launch: a null pointer, max_vertices < 1, a model index outside the database, a non-finite pose
 * or camera element (the reference's sort order of NaN is undefined), no database, a store whose rows are not grouped by
 * model in ascending order or that was uploaded in blocks (mh_db_upload_blocks).  n_obj = 0: MH_OK, nothing is done. */
int mh_object_hulls(mh_ctx* ctx, const int32_t* obj_model, const float* obj_pose, int n_obj, const mh_cam* cam,
                    int max_vertices, float* hull_xy_host, int32_t* n_vertices, int32_t* n_behind, float* bbox_uv_host);

/* Debug entry, like mh_filter_depth_debug_form: the device form mh_object_hulls runs.  0 (default): points strictly
 * inside the octagon of the cloud's eight extreme points are discarded before the sort.  1: every point is sorted and
 * chained.  The results are the same on every input the tests hold (DESIGN.md section 6 on why that is observed and
 * not proved). */
int mh_hull_debug_form(mh_ctx* ctx, int form);

/* Hulls of every object of a frame, computed behind the frame on the device: what MopedBench's outputObjectCH writes for
 * every object of every frame (moped3d/libmoped/src/MopedBench.cpp:153-174) and the display steps draw.
 * mh_frame_set_hulls: max_vertices > 0 switches them on for the frames and batches enqueued afterwards, 0 (the default)
 * off; image: the camera of a several-camera frame whose hulls are wanted (0 otherwise).  Such a frame runs ONE more
 * launch behind FILTER2 (run_stage2 = 0: behind POSE) over the objects of its result slots -- a merged batch one launch for
 * all its slots -- stream-ordered, without a host wait, the object counts read on the device; the prefilter form always
 * (mh_hull_debug_form is not consulted).  Objects, counts and everything else of the frame are what they are without
 * hulls.  The device block: MH_MAX_BATCH slots of the reserved max_objects (mh_reserve*) records.
 * While hulls are on, refused with MH_ERR_ARG before anything is enqueued: the sharded entry points
 * (mh_frame_enqueue_sharded*, mh_frame_enqueue_rest*: model indices are shard-local, exchange 2 carries no hulls), an
 * `image` that is not among the frame's cameras, a store mh_object_hulls refuses. */
int mh_frame_set_hulls(mh_ctx* ctx, int max_vertices, int image);
/* The hulls of the frame in result slot `slot` (mh_frame_fetch_hulls: slot 0, as mh_frame_fetch), in the order of the
 * objects mh_frame_fetch[_slot] returns: *n_objects = their number, and for the first min(*n_objects, max_objects) of
 * them n_vertices / n_behind / bbox_uv_host / hull_xy_host[max_objects][max_vertices][2] as mh_object_hulls gives them
 * (vertices beyond the frame's max_vertices or the array's were not kept).  Synchronises the context's stream.
 * MH_ERR_ARG: the frame enqueued last into that slot ran with hulls off. */
int mh_frame_fetch_hulls_slot(mh_ctx* ctx, int slot, int max_objects, int max_vertices, float* hull_xy_host,
                              int32_t* n_vertices, int32_t* n_behind, float* bbox_uv_host, int32_t* n_objects);
int mh_frame_fetch_hulls(mh_ctx* ctx, int max_objects, int max_vertices, float* hull_xy_host, int32_t* n_vertices,
                         int32_t* n_behind, float* bbox_uv_host, int32_t* n_objects);
/* A whole batch's hulls into the caller's (page-locked) block in one stream-ordered copy, beside
 * mh_frame_fetch_batch_async's objects: frame f's records lie at f * mh_frame_hull_block_stride(max_objects,
 * max_vertices) -- max_vertices the value given to mh_frame_set_hulls -- record o = object o of the frame:
 * {int32 n_vertices; int32 n_behind; float bbox_uv[8][2]; float hull_xy[max_vertices][2]}.  Records at and beyond the
 * frame's object count (mh_frame_head::n_objects of the objects' block) are not meaningful.  mh_frame_fetch_wait waits
 * for it too; one delivery in flight.  mh_frame_block_stride and mh_frame_head are unchanged. */
size_t mh_frame_hull_block_stride(int max_objects, int max_vertices);
int mh_frame_fetch_batch_hulls_async(mh_ctx* ctx, int B, int max_objects, void* host_block);

/* ---- whole frame, device resident --------------------------------------------- */

typedef struct {
  float ratio;               /* 0.8  (config.hpp:83) */
  float ms_radius, ms_merge; /* 200, 20 (config.hpp:101) */
  int ms_min_pts, ms_max_iter; /* 7, 100 */
  mh_pose_params pose1;      /* (.., 4, 5, 6, 10)  config.hpp:110 */
  int f1_min_points; float f1_feature_distance, f1_min_score; /* 5, 4096, 2  config.hpp:115 */
  mh_pose_params pose2;      /* (.., 4, 6, 8, 5)   config.hpp:118 */
  int f2_min_points; float f2_feature_distance, f2_min_score; /* 7, 4096, 3  config.hpp:120 */
  int run_stage2;            /* 0: stop after POSE (objects unscored) */
} mh_frame_params;

void mh_frame_default_params(mh_frame_params* p);

typedef struct {
  int32_t model;   /* model index (local to the context) */
  float pose[7];
  float score;
  int32_t n_points; /* size of the object's final cluster */
} mh_object;

/* One frame from device-resident inputs: q_desc_dev [Q x 128] raw descriptors
 * (normalised in place, as the reference mutates detectedFeatures), q_uv_dev
 * [Q x 2].  Everything is enqueued on the context's stream; no host
 * synchronisation.  Results stay on the device until mh_frame_fetch. */
int mh_frame_enqueue(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q,
                     const mh_cam* cam, const mh_frame_params* prm, uint64_t seed);
/* B <= MH_MAX_BATCH frames at once: their descriptors / keypoints one after the other ([B Q][128], [B Q][2]); ONE
 * MATCH launch sequence over all B Q queries (the DB passes the chip once per batch), then CLUSTER .. FILTER2 frame
 * by frame on the context's stream; frame f leaves its objects in result slot f (mh_frame_fetch_slot), the same
 * objects, bit for bit, as mh_frame_enqueue(…, seeds[f]) gives it alone.  Per-query depth attributes
 * (mh_frame_set_depth) are then [B Q] like the queries, and so is the per-query image index of frames with several
 * images (mh_frame_set_images: q_image_dev [B Q]; one camera table for the batch); depth maps (and the depth rules that
 * read them) come one per frame through mh_frame_set_depth_image_batch. */
/* The same frame from HOST memory, objects back on return: the body of the frame loop of
 * MopedPimpl::processImages (src/moped.cpp:183-191 -- MATCH_SIFT, CLUSTER, POSE, FILTER, POSE2, FILTER2 on one
 * FrameData) as one call.  q_desc_host [Q][128] raw descriptors (written back L2-normalised if write_back, as
 * MATCH_ANN_CPU.hpp:157 leaves them), q_uv_host [Q][2], q_image_host [Q] or NULL (FrameData::DetectedFeature::imageIdx,
 * renumbered into cams[]; needed when n_images > 1), cams[n_images] (1 <= n_images <= MH_MAX_IMAGES).  Results as
 * mh_frame_fetch.  What the STEP plugins move over PCIe between the steps (matches, clusters, objects, twice) stays on
 * the device; FRAME_RESIDENT_HIP (moped_amd/host) is the MopedAlg that calls this. */
int mh_frame_run_host(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                      const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, int write_back,
                      mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts);
/* The same in two halves, for a host that has work of its own to do while the frame runs (FRAME_RESIDENT_HIP copies the
 * normalised descriptors back into FrameData::detectedFeatures meanwhile): mh_frame_run_host_begin uploads and enqueues
 * the frame and returns; mh_frame_wait_descriptors returns when q_desc_host holds the normalised descriptors (write_back
 * was set; they are through right after the frame's first kernel); mh_frame_fetch ends the frame as usual.  The host
 * buffers must stay untouched by the caller until mh_frame_wait_descriptors (q_desc_host) / mh_frame_fetch (the others). */
int mh_frame_run_host_begin(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, const int32_t* q_image_host, int Q,
                            const mh_cam* cams, int n_images, const mh_frame_params* prm, uint64_t seed, int write_back);
int mh_frame_wait_descriptors(mh_ctx* ctx);
/* Page-locked host memory for the buffers a host hands to mh_frame_run_host (and to the other host-pointer entry points):
 * from pageable memory the frame's 1.5 MB of descriptors cross PCIe through the driver's staging copies (~0.1 ms each
 * way), from here at the link's rate and asynchronously.  FRAME_RESIDENT_HIP packs FrameData::detectedFeatures
 * (src/util.hpp:70-79) straight into such a block.  mh_host_free(NULL) is a no-op. */
int mh_host_alloc(mh_ctx* ctx, size_t bytes, void** out);
int mh_host_free(mh_ctx* ctx, void* p);

/* ---- the six slots one call each, the frame resident between them (the per-step plugins' hand-over) ----------------
 * The reference runs its steps strictly one after the other on one FrameData (src/moped.cpp:183-191, the step list of
 * src/config.hpp:83-120); every step's contract is what it leaves in FrameData for the next (src/util.hpp:68-110).  These
 * entry points keep that contract -- each returns what its slot writes into FrameData -- but the step that follows does
 * not upload it again: the frame's match lists, clusters and objects stay in the context's working arrays and each
 * call launches only its own slot's kernels behind the previous call's.  Order: mh_step_match, mh_step_match_fetch,
 * mh_step_cluster, mh_step_pose(1), mh_step_filter(1), mh_step_pose(2), mh_step_filter(2).  A call out of that order, or
 * after any other call that uses the context's frame arrays (mh_frame_*, mh_filter*, mh_pose_ransac*), is refused with
 * MH_ERR_ARG -- the plugin then takes the upload path of its slot (mh_normalize_match / mh_meanshift_batch /
 * mh_pose_ransac_images / mh_filter_images), which is always valid.  One camera per frame.  Objects are bit for bit
 * those of mh_frame_run_host with the same constants and seeds (POSE: seed, POSE2: seed ^ 0x5DEECE66D there).
 *
 * mh_step_match: MATCH_ANN_CPU::process (src/match/MATCH_ANN_CPU.hpp:136-178) -- uploads the frame's features
 * (q_desc_host [Q][128] raw, q_uv_host [Q][2]; page-locked memory from mh_host_alloc crosses PCIe asynchronously),
 * normalises (:157), searches, applies the ratio test and leaves matches[model] (:165-176) on the device; returns
 * without waiting.  write_back: the normalised descriptors come back into q_desc_host on a stream of their own
 * (mh_frame_wait_descriptors).  mh_step_match_fetch waits and returns the lists: model_off_host[n_models + 1],
 * match (model_off[m] + k) = k-th element of matches[m] = {query index, {u, v, x, y, z}}; cap >= Q always suffices. */
int mh_step_match(mh_ctx* ctx, float* q_desc_host, const float* q_uv_host, int Q, const mh_cam* cam, float ratio,
                  int write_back);
int mh_step_match_fetch(mh_ctx* ctx, int32_t* model_off_host, int32_t* match_query, mh_corr* match_pts, int cap,
                        int32_t* n_matches);
/* CLUSTER_MEAN_SHIFT_CPU::process (src/cluster/CLUSTER_MEAN_SHIFT_CPU.hpp:182-199) on the resident lists: cluster c
 * belongs to model cl_model_host[c] and holds members_host[cl_off_host[c] .. cl_off_host[c + 1]) = indices into
 * matches[model], in the reference's emission and member order; clusters in (model, emission) order. */
int mh_step_cluster(mh_ctx* ctx, float radius, float merge, int min_pts, int max_iter, int32_t* cl_model_host,
                    int32_t* cl_off_host /* cap_clusters + 1 */, int32_t* members_host, int cap_clusters, int cap_members,
                    int32_t* n_clusters);
/* POSE_RANSAC_LM_DIFF_REPROJECTION_CPU::process (src/pose/...REPROJECTION_CPU.hpp:264-307) on the resident clusters
 * (which = 1: CLUSTER's; 2: the clusters FILTER rewrote): the objects this step APPENDS to FrameData::objects (:299), in
 * task order. */
typedef struct {
  int32_t model;
  float pose[7];   /* qx qy qz qw tx ty tz */
} mh_step_object;
int mh_step_pose(mh_ctx* ctx, int which, const mh_pose_params* prm, uint64_t seed, mh_step_object* out, int cap,
                 int32_t* n_out);
/* FILTER_PROJECTION_CPU::process (src/filter/FILTER_PROJECTION_CPU.hpp:80-162) on the resident objects (which = 1:
 * FILTER, 2: FILTER2).  n_objects = length of the host's object list (checked against the device's).  Outputs as
 * mh_filter_images, indexed by LIST position: score[i], keep[i]; kept object k was list element out_order[k] and now
 * owns cl_members[cl_off[k] .. cl_off[k + 1]) = indices into its model's match list. */
int mh_step_filter(mh_ctx* ctx, int which, int min_points, float feature_distance, float min_score, int n_objects,
                   float* score, uint8_t* keep, int32_t* out_order, int32_t* cl_members, int32_t* cl_off /* n_objects + 1 */,
                   int cap_members, int32_t* n_kept);
int mh_frame_enqueue_batch(mh_ctx* ctx, float* q_desc_dev, const float* q_uv_dev, int Q, int B, const mh_cam* cam,
                           const mh_frame_params* prm, const uint64_t* seeds);
/* Frames with several images (FrameData::images; every DetectedFeature carries its imageIdx, src/util.hpp:70-79):
 * q_image_dev[Q] = image of every query of the frames enqueued from now on (device memory, read when a frame
 * runs), cams[n_images] their cameras.  CLUSTER then runs per (model, image) in image order
 * (CLUSTER_MEAN_SHIFT_CPU.hpp:189-195), POSE / FILTER project every correspondence through its own image; the
 * `cam` argument of mh_frame_enqueue* is ignored.  n_images <= 1 or NULL: back to one image.  With batches
 * (mh_frame_enqueue_batch, mh_frame_enqueue_sharded_batch) q_image_dev holds [B Q] entries, frame after frame like the
 * queries.  Not together with the moped3d depth steps: those are single-camera in the reference itself (DEPTHMAP_PROP
 * looks every match up in the ONE depth map of the frame whatever its image,
 * moped3d/libmoped/src/depthprop/DEPTHMAP_PROP_CPU.hpp:86-112). */
int mh_frame_set_images(mh_ctx* ctx, const int32_t* q_image_dev, const mh_cam* cams, int n_images);

/* Per-query depth attributes for the next frames (device pointer, [Q] mh_depth, in query
 * order; NULL switches back to the 2-D residuals).  POSE and POSE2 of the frame then use
 * the MH_DEPTH_* residuals `kind` with `alpha`. */
int mh_frame_set_depth(mh_ctx* ctx, const mh_depth* q_depth_dev, int kind, float alpha);
/* The same from the depth map itself, as moped3d holds it (moped3d/moped3d.cpp:279-333):
 * depth_xyzn_dev [height][width][4] floats (camera-frame x, y, z, norm or negative = invalid),
 * fill_distance_dev [height][width] or NULL (DEPTH_FILL's ".distance" map; NULL = -1 everywhere).
 * Each accepted match looks its pixel up on the device -- DEPTHMAP_PROP_CPU::process
 * (moped3d/libmoped/src/depthprop/DEPTHMAP_PROP_CPU.hpp:101-134): truncated coordinates, no
 * interpolation -- and gets weight getCauchyWeight(fillDistance) with `cauchy_scale` (0.1 in
 * POSE_..._BACKPROJECTION_DEPTH_CPU.hpp:66, 25 in ..._REPROJECTION_DEPTH_CPU.hpp:66).
 * NULL image switches depth off. */
int mh_frame_set_depth_image(mh_ctx* ctx, const float* depth_xyzn_dev, const float* fill_distance_dev,
                             int width, int height, int kind, float alpha, float cauchy_scale);
/* One depth map (and distance map) per frame of the batches enqueued from now on (mh_frame_enqueue_batch with
 * B = n_frames): pointer arrays of n_frames <= MH_MAX_BATCH device images of the same size.  The batch's frames share
 * their launches (round 4): every frame's map must stay valid until the batch's results are fetched. */
int mh_frame_set_depth_image_batch(mh_ctx* ctx, const float* const* depth_xyzn_dev, const float* const* fill_distance_dev,
                                   int n_frames, int width, int height, int kind, float alpha, float cauchy_scale);
/* The same for hosts that hold the maps in host memory (the STEP plugins): copies them into
 * context-owned device buffers (4.9 MB + 1.2 MB for 640x480) and sets them. */
int mh_frame_set_depth_image_host(mh_ctx* ctx, const float* depth_xyzn_host, const float* fill_distance_host,
                                  int width, int height, int kind, float alpha, float cauchy_scale);

/* moped3d's DEPTHFILL step: DEPTH_FILL_EXACT_CPU::process / fillInScaled
 * (moped3d/libmoped/src/depthfill/DEPTH_FILL_EXACT_CPU.hpp:268-349, 416-428; config.hpp:39 ships
 * DEPTH_FILL_EXACT_CPU(8, false)).  depth_xyzn_dev [height][width][4] floats (x, y, z, norm; z < 0 = hole) is filled
 * IN PLACE on the context's stream: every hole takes the depth the reference's FIFO wavefront over the map downscaled
 * by scale_factor gives it (nearest-neighbour upsampling with the reference's late row advance, or bilinear != 0:
 * its bilinear one), then x, y and norm of the filled pixels are recomputed from K = the depth map's
 * intrinsicLinearCalibration (:249-273).  fill_distance_dev [height][width] receives the distance map the step
 * appends to the frame ("<name>.distance": 0 on valid pixels), the one mh_frame_set_depth_image takes.
 * scale_factor = -1 chooses the factor from the share of holes as the reference does (:283-296; one small
 * reduction and a 4-byte read back); with a factor of 1 the reference never hands the filled depths back
 * (:336-338) and neither does this: only the distance map is written.  *scale_used (optional) = the factor.
 * Bit-identical to the reference's arithmetic (tests/test_gpu_depthfill.py against the oracle's restatement).
 * Limits (the default mode; mh_depth_fill_set_mode below lifts them): the downscaled map holds at most 8192 pixels
 * (640 x 480 from factor 8 on) -> MH_ERR_CAPACITY.
 * Asynchronous; mh_depth_fill_status synchronises the stream and reports MH_ERR_CAPACITY if the fill's queue
 * outgrew its 16384-entry ring in a call since the last status (no map of a real sensor comes near it). */
int mh_depth_fill(mh_ctx* ctx, float* depth_xyzn_dev, int width, int height, int scale_factor, int bilinear,
                  const float K[4], float* fill_distance_dev, int* scale_used);
int mh_depth_fill_status(mh_ctx* ctx);
/* How the fill runs (opt-in, like mh_match_set_mode; the default is MH_DEPTH_FILL_REPLAY: everything above and below as
 * it is written, limits included).  MH_DEPTH_FILL_LEVELS runs the same FIFO queue generation by generation: the seeds
 * are generation 0, what a generation-k element pushes is generation k + 1, and within a generation the updates of
 * different pixels never interact -- all 1024 threads of the map's workgroup work on the generation, one target pixel
 * each, and lay out the next one in exactly the order the serial loop would have pushed it.  The results are byte for
 * byte those of the replay wherever the replay accepts the map (tests/test_gpu_depthfill_levels.py), and mh_depth_fill,
 * mh_depth_fill_batch, mh_depth_fill_host and everything that fills through them (mh_frame_run_kinect_host, the Kinect
 * batch path) take any map whose downscaled size is 1 x 1 to 2^21 pixels (more: MH_ERR_CAPACITY before any launch);
 * scale_factor = -1 in mh_depth_fill then works for every share of holes (in the batch call it stays MH_ERR_ARG).
 * State and generation lists live in the context's scratch, 128 bytes per downscaled pixel and frame: a fill of a
 * larger map or of more frames than any LEVELS fill before it on the context reallocates the scratch at the start of
 * the call, before its launches (that synchronises the context's stream; the sticky overflow word is carried over).
 * Capacity: a generation may hold up to 4 * dw * dh elements (no bound on a generation's size is known; sensor-like
 * maps stay under 1.0 * dw * dh) and a fill up to dw * dh generations; beyond either the fill stops, nothing is written
 * out of bounds, the sticky overflow word is set (mh_depth_fill_status -> MH_ERR_CAPACITY: the maps of that call are
 * incomplete) and the context stays usable.  One workgroup per map, in either mode.
 * mh_depth_fill_stats: of frame `frame` of the context's last fill, which must have been a LEVELS one (else
 * MH_ERR_ARG): {non-empty generations processed (seeds included), largest generation, elements over all generations
 * (saturating), overflowed}; synchronises the context. */
enum { MH_DEPTH_FILL_REPLAY = 0, MH_DEPTH_FILL_LEVELS = 1 };
int mh_depth_fill_set_mode(mh_ctx* ctx, int mode);
int mh_depth_fill_get_mode(mh_ctx* ctx, int* mode);   /* (a user of a shared context saves the mode, sets its own, puts it back) */
int mh_depth_fill_stats(mh_ctx* ctx, int frame, int32_t out[4]);
/* DEPTHFILL of n_frames <= MH_MAX_BATCH maps of one size, each in place with its own distance map, in ONE launch per
 * stage: what moped3d's pipeline (moped3d/libmoped/src/config.hpp:39, DEPTH_FILL_EXACT_CPU.hpp:268-349) does to every
 * frame's map, for the frames of a batch at once -- the FIFO wavefront of a map occupies ONE workgroup for as long as its
 * holes are deep (0.07-0.10 ms for speckle and shallow holes, about 2.4 ms for sensor-like blobs of up to 70 pixels radius
 * over half the map), the maps of a batch occupy one workgroup each side by side.  Every frame needs a depth map and a
 * distance map of its own: the frames are filled in place at the same time, the same buffer for two frames -> MH_ERR_ARG.  Every map's result is bit for bit what mh_depth_fill
 * gives that map alone (the same kernel bodies behind entry points of their own; mh_depth_fill's launches are unchanged).  Asynchronous on the context's stream;
 * the overflow word is shared and sticky (mh_depth_fill_status reports a ring overflow of any frame of any batch since
 * the last status).  The downscaled map's 8192-pixel limit -> MH_ERR_CAPACITY before anything is launched;
 * scale_factor = -1 would need a read-back per map -> MH_ERR_ARG (mh_depth_fill takes it, one map per call).  The
 * first call sizes the context's scratch for MH_MAX_BATCH frames (2 MiB), so no later batch waits for one in flight. */
int mh_depth_fill_batch(mh_ctx* ctx, float* const* depth_xyzn_dev, float* const* fill_distance_dev, int n_frames,
                        int width, int height, int scale_factor, int bilinear, const float K[4]);
/* The same on host maps (what the DEPTH_FILL_EXACT_HIP plugin calls): upload, fill, both maps back, status. */
int mh_depth_fill_host(mh_ctx* ctx, float* depth_xyzn_host, int width, int height, int scale_factor, int bilinear,
                       const float K[4], float* fill_distance_host, int* scale_used);

/* The depth map itself from what a Kinect delivers: the block of moped3d's ROS node in front of the pipeline
 * (moped3d/moped3d.cpp:279-333), one thread per pixel of the map.  A raw value is read at
 * raw + offset + y * row_stride + x * elem_stride (bytes):
 *   MH_RAW_DEPTH_F32_M    a float in metres, NaN = no reading -> -1e30f (:288-292)
 *   MH_RAW_DEPTH_U16_MM   OpenNI's uint16 millimetres, 0 = no reading -> -1e30f, else (float) mm * 0.001f
 * A plain image has elem_stride 4 or 2; an organised PointCloud2 buffer is read in place with elem_stride = point_step,
 * offset = the z field's offset, row_stride = row_step (:287: no host repacking).
 * (width, height) == the raw size: the pixel's depth is the raw value (:298-300).  Any other size: it comes from the raw
 * map resized to exactly (2 raw width, 2 raw height) (:303, cv::resize's bilinear path for float, restated from memory of
 * OpenCV 2.x and therefore unpinned: csrc/depthmap.hip has the arithmetic); pixels beyond the resized map are invalid
 * (:313-316), a smaller target crops it.  A missing reading at (x, y) invalidates [2x - 1, 2x + 2] x [2y - 1, 2y + 2].
 * Depth < 0: the pixel's four floats are -1 (:318-319; 0.0 and -0.0 are valid); else x = depth (u - K[2]) / K[0],
 * y = depth (v - K[3]) / K[1], z = depth, norm = sqrt(x x + y y + z z) (:325-330), every operation rounded on its own:
 * bit for bit tests/depthmap_ref.py (tests/test_gpu_depthmap.py).  K = the DEPTH camera's fx, fy, cx, cy (:306).
 * MH_ERR_ARG before any launch: a null pointer, a size <= 0, an unknown format, a stride or an offset that is not a
 * multiple of the element size (or negative), a stride smaller than the element, a raw pointer not aligned to the
 * element or a map not aligned to 16 bytes, n_frames outside 1 .. MH_MAX_BATCH, two frames writing the same map. */
enum { MH_RAW_DEPTH_F32_M = 0, MH_RAW_DEPTH_U16_MM = 1 };
typedef struct mh_raw_depth {
  int32_t format, width, height;             /* the sensor's size */
  int32_t elem_stride, row_stride, offset;   /* bytes */
} mh_raw_depth;
/* raw_dev -> depth_xyzn_dev [height][width][4], both on the device; asynchronous on the context's stream. */
int mh_depth_map_from_raw_dev(mh_ctx* ctx, const void* raw_dev, const mh_raw_depth* raw, const float K[4],
                              float* depth_xyzn_dev, int width, int height);
/* n_frames <= MH_MAX_BATCH raw buffers of one description -> a map each, ONE launch (the frame index is in the grid);
 * every map bit for bit what the single call gives it.  Pointer arrays on the host; asynchronous. */
int mh_depth_map_from_raw_batch_dev(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_depth* raw, const float K[4],
                                    float* const* depth_xyzn_dev, int n_frames, int width, int height);
/* The same for a host that holds the sensor's buffer: its offset + (raw height - 1) row_stride + (raw width - 1)
 * elem_stride + element size bytes are copied into a context-owned buffer (1.2 MB of float z, 0.6 MB of 16-bit for
 * 640 x 480, against the 4.9 MB of the finished map), the map is built into the buffers mh_frame_set_depth_image_host
 * fills and copied to depth_xyzn_host; with NULL it only stays there (what mh_frame_run_kinect_raw_host goes on from).
 * A frame's map that lived in those buffers is switched off: set it again.  Synchronous. */
int mh_depth_map_from_raw_host(mh_ctx* ctx, const void* raw_host, const mh_raw_depth* raw, const float K[4],
                               float* depth_xyzn_host, int width, int height);

/* The 8-bit gray image from what a camera delivers: the first line of moped3d's image callback,
 * cv_bridge::toCvCopy(iMsg, "mono8") (moped3d/moped3d.cpp:249), on the device.  A pixel is read at
 * raw + offset + y * row_stride + x * bytes-per-pixel; the output is a packed [height][width] gray image.  Neither pointer
 * needs any alignment, offsets and strides are arbitrary byte counts.  The formats carry the names of ROS's
 * sensor_msgs/image_encodings.h.  The arithmetic restates what OpenCV 2.x cvtColor does for 8-bit data, written WITHOUT
 * OpenCV at hand and therefore UNPINNED (like the resize of mh_depth_map_from_raw_*); the project's definition is
 * tests/image_gray_ref.py, integers only, and the kernel gives its bytes (tests/test_gpu_image_gray.py).  With R2Y = 4899,
 * G2Y = 9617, B2Y = 1868 (sum 2^14), unsigned 32-bit sums:
 *   MH_IMAGE_GRAY8                 the byte itself: the call only removes strides and offsets
 *   MH_IMAGE_BGR8 / RGB8 / BGRA8 / RGBA8
 *                                  (R2Y R + G2Y G + B2Y B + 8192) >> 14; alpha is ignored
 *   MH_IMAGE_BAYER_RGGB8 / BGGR8 / GBRG8 / GRBG8
 *                                  the four letters are the top-left 2 x 2 sites row by row.  Interior pixels (1 <= x <=
 *                                  w - 2, 1 <= y <= h - 2), p the site's byte, C() a colour's coefficient: at an R or B
 *                                  site of own colour o and opposite colour q
 *                                    (C(q) (4 diagonal neighbours) + G2Y (4 edge neighbours) + 4 C(o) p + 32768) >> 16,
 *                                  at a G site with ch the colour of (x + 1, y) and cv that of (x, y + 1)
 *                                    (C(ch) (left + right) + C(cv) (up + down) + 2 G2Y p + 16384) >> 15.
 *                                  Columns 0 and w - 1 copy columns 1 and w - 2, then rows 0 and h - 1 copy rows 1 and
 *                                  h - 2.  Bayer images are at least 3 x 3.
 * (moped2's node, moped2/moped.cpp:175-204, converts to BGR8 and copies `width` bytes of every three-channel row: a defect,
 * not reproduced.)
 * MH_ERR_ARG before any launch, the context unchanged, mh_last_error naming the argument: a null pointer, an unknown
 * format, a size <= 0, Bayer below 3 x 3, a negative offset, row_stride < width * bytes-per-pixel, an extent (offset +
 * (height - 1) row_stride + width * bytes-per-pixel) or width * height beyond INT_MAX, n outside 1 .. MH_MAX_BATCH, two
 * images of a batch writing the same (or overlapping) output, an output that overlaps its own raw extent or another
 * image's.  Nothing outside the extent is read, nothing outside the width * height output bytes is written. */
enum { MH_IMAGE_GRAY8 = 0, MH_IMAGE_BGR8, MH_IMAGE_RGB8, MH_IMAGE_BGRA8, MH_IMAGE_RGBA8,
       MH_IMAGE_BAYER_RGGB8, MH_IMAGE_BAYER_BGGR8, MH_IMAGE_BAYER_GBRG8, MH_IMAGE_BAYER_GRBG8 };
typedef struct mh_raw_image {
  int32_t format, width, height;
  int32_t row_stride, offset;   /* bytes */
} mh_raw_image;
/* raw_dev -> gray_dev [height][width], both on the device; asynchronous on the context's stream (:249). */
int mh_image_gray_dev(mh_ctx* ctx, const void* raw_dev, const mh_raw_image* fmt, uint8_t* gray_dev);
/* n <= MH_MAX_BATCH raw buffers of one description -> a gray image each, ONE launch (the image index is in the grid): a
 * 640 x 480 conversion is a stream of 1.2 MB and costs its launch, so a batch pays it once (:249 per frame of a batch).
 * Every output is byte for byte the single call's.  Pointer arrays on the host; asynchronous. */
int mh_image_gray_batch_dev(mh_ctx* ctx, const void* const* raw_dev, const mh_raw_image* fmt, uint8_t* const* gray_dev, int n);
/* The same for a host that holds the camera's buffer (:249 as one call): its extent goes into a context-owned buffer, the
 * gray image comes back into gray_host [height][width].  Synchronous. */
int mh_image_gray_host(mh_ctx* ctx, const void* raw_host, const mh_raw_image* fmt, uint8_t* gray_host);
/* The frames' images as the camera delivers them (:249 in front of processImages): while a format is set, the image
 * pointers of mh_frame_enqueue_image, mh_frame_enqueue_image_batch, mh_frame_enqueue_images and
 * mh_frame_enqueue_images_batch are raw buffers of that description (their width and height must be the format's, else
 * MH_ERR_ARG).  The images of a call are converted by ONE launch into a staging buffer of the context -- its own, not the
 * one undistortion writes --, then comes mh_frame_set_undistort[_images] if it is on, then FEAT: bit for bit
 * mh_image_gray_batch_dev followed by the same call with no format set.  mh_frame_run_kinect_host and
 * mh_frame_run_kinect_raw_host then read gray_host as such a raw buffer and upload its extent instead of width * height
 * bytes; with raw depth that is the node's whole callback (:240-338) in one call.  fmt NULL = packed 8-bit gray, the default;
 * the description is copied.  The teaching calls (mh_db_splice_image*, mh_db_splice_view*, mh_db_append_view) and
 * mh_sift_extract* keep taking gray whatever is set here: their callers run mh_image_gray_dev first. */
int mh_frame_set_image_format(mh_ctx* ctx, const mh_raw_image* fmt);

/* moped3d's rules on which features and matches reach CLUSTER, applied on the device inside the
 * frame (they need the depth map: mh_frame_set_depth_image):
 *  - DEPTHFILTER_CPU (moped3d/libmoped/src/depthfilter/DEPTHFILTER_CPU.hpp:117-254), ToFilter = 1
 *    on the detected features (`feature_density`, config.hpp: 0.05) and ToFilter = 2 on every
 *    model's matches (`match_density`, 0.01): density per square metre of scene surface over
 *    PatchSize x PatchSize pixel patches, dilated 3x3, must exceed Density.  K = the depth map's
 *    intrinsicLinearCalibration.  A negative density switches that filter off.
 *  - MATCH_ADAPTIVE_FLANN_CPU's ratio (.../match/MATCH_ADAPTIVE_FLANN_CPU.hpp:193-215,361-376,
 *    457-467): ratio_table[m] = (maxRatioDepth, minRatioDepth, ratioLow, ratioHigh) of model m as
 *    its Update() derives them (:144-177; the host plugin MATCH_ADAPTIVE_BRUTE_HIP does);
 *    features deeper than maximum_depth never match; NULL = mh_frame_params.ratio for all.
 * Coordinates outside the depth map are clamped to it (the reference reads out of bounds).
 * rules == NULL switches all of it off. */
typedef struct mh_depth_rules {
  int32_t patch_size;
  float feature_density;
  float match_density;
  const float* ratio_table; /* host, [n_models][4]; copied by the call */
  int32_t n_models;
  float maximum_depth;      /* 4.0  (MATCH_ADAPTIVE_FLANN_CPU.hpp:107) */
  float default_depth;      /* 1.0  (:108) */
  float cauchy_scale;       /* 0.1  (:109) */
} mh_depth_rules;
int mh_frame_set_depth_rules(mh_ctx* ctx, const mh_depth_rules* rules, const float K[4]);
/* moped3d's default clusterer instead of mean shift: CLUSTER_LINKAGE_CPU
 * (moped3d/libmoped/src/cluster/CLUSTER_LINKAGE_CPU.hpp:573-704) as config.hpp:45 constructs it --
 * per model a similarity matrix over its matches (Gaussian kernels on image / camera-frame
 * distances with sigma = average nearest-neighbour distance, depth-discontinuity kernel along the
 * image line between two matches, model/world distance-consistency kernel, fill-distance weighted
 * sum) and average-linkage agglomeration down to `cutoff`.  Needs the depth map
 * (mh_frame_set_depth_image); at most 1024 matches per model.  LinkageType 0, 1 (average, as shipped) or 2. */
typedef struct mh_linkage_params {
  float cutoff;         /* 0.1 */
  int32_t min_pts;      /* 7: clusters need MORE than this many members (:535) */
  int32_t use3d_filter; /* 2: multiply (1: add, 0: skip) the distance-consistency kernel */
  float sigma2d;        /* -1: average nearest-neighbour distance */
  float sigma3d;        /* -1 */
  int32_t linkage_type; /* 1: average linkage (config.hpp:45); 0 minimum, 2 maximum (CLUSTER_LINKAGE_CPU.hpp:506-526) */
} mh_linkage_params;
/* CLUSTER of the following frames: linkage with *prm, or mean shift again when prm == NULL. */
int mh_frame_set_cluster_linkage(mh_ctx* ctx, const mh_linkage_params* prm);
/* The clusterer's scratch is three n x n similarity matrices per (model, frame) problem (CLUSTER_LINKAGE_CPU.hpp:573-704
 * keeps the same three as vector<vector<Float>>): sized for the worst case of what the context has reserved -- 3 x 1024 x
 * max matches floats per frame of a batch, 37 MB at 3 000 (MH_LINKAGE_ROWMAX, below: 3 x min(4096, max matches) x max
 * matches, 108 MB at 3 000, and 48 bytes per model + 12 per match of plan and per-point arrays) -- and bounded: a frame or batch that would need more than
 * `bytes` (0 = the default, 4 GiB) fails with MH_ERR_CAPACITY before anything is allocated or launched. */
int mh_set_linkage_scratch_limit(mh_ctx* ctx, size_t bytes);
/* The step on its own, n_problems point sets (one per model) in one call: corr_host / depth_host
 * = the matches (image point + model point / camera-frame point from the depth map), problem p =
 * rows [off[p], off[p+1]).  label[i] = cluster of row i within its problem or -1; order (optional)
 * = rows of each problem's clusters in the reference's member order, problem-local, -1 padded;
 * n_clusters[p].  Uses the depth map set by mh_frame_set_depth_image. */
int mh_cluster_linkage(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, const int32_t* off,
                       int n_problems, const mh_linkage_params* prm, int32_t* label, int32_t* order,
                       int32_t* n_clusters);
/* For tests, in the style of mh_depth_rules_debug_fetch / mh_sift_debug_*: the clusterer's two halves on their own.
 * mh_linkage_debug_matrix: ONE problem of n matches (1 .. 1024; MH_LINKAGE_ROWMAX: 1 .. 4096, also below) as mh_cluster_linkage takes it (cutoff, min_pts and
 *   linkage_type of *prm are not used) -> two n x n float matrices: A_host = the 3-D side after pass 2 -- K3D +
 *   discontinuity kernel (CLUSTER_LINKAGE_CPU.hpp:133-149, 231-285, 681), normalised, + / x K3F (:151-173, 683-692),
 *   BEFORE the division by its maximum (use3d_filter 0: the first sum, before its only normalisation) -- and K_host = the
 *   final similarity (adaptiveWeightSum, :325-366) as hierarchicalCluster (:416) first sees it.  The same kernel, run with
 *   a cutoff above every similarity so that its loop ends in the first scan.  A is computed for j >= i only: the call
 *   mirrors it; K is handed out as the device holds it, both halves.
 * mh_linkage_debug_agglomerate: hierarchicalCluster (:416-540) alone, over a symmetric n x n host matrix K_host in place of
 *   the matrix stages (the kernel skips the sigmas and passes 1-3 and takes the matrix as uploaded; everything from there
 *   on is the shipped code).  label [n] / order [n] (optional) / *n_clusters as mh_cluster_linkage's for one problem.
 * n outside 1 .. 1024, a linkage_type outside 0 .. 2, no depth map (matrix) -> MH_ERR_ARG / MH_ERR_CAPACITY with a
 * message, nothing is launched. */
int mh_linkage_debug_matrix(mh_ctx* ctx, const mh_corr* corr_host, const mh_depth* depth_host, int n,
                            const mh_linkage_params* prm, float* A_host, float* K_host);
int mh_linkage_debug_agglomerate(mh_ctx* ctx, const float* K_host, int n, float cutoff, int min_pts, int linkage_type,
                                 int32_t* label, int32_t* order, int32_t* n_clusters);
/* How the linkage clusterer runs (opt-in, per context, like mh_depth_fill_set_mode; the default is MH_LINKAGE_SCAN:
 * everything above as it is written, the 1024-point limit and its error codes included).  MH_LINKAGE_ROWMAX computes the
 * same matrices and the same clusters with another schedule and takes 1 .. MH_LINKAGE_MAX_POINTS points per problem:
 *   - the matrix stage runs on the whole grid, a launch per pass (plan, nearest neighbours, sigmas and fill weights,
 *     passes 1-3 over 32 x 32 tiles of the upper triangle); every element by the same expressions as the default mode,
 *     the two maxima by integer atomic maxima over the floats' bit patterns (values >= 0, NaN left out, order-independent),
 *     so A and K are the default mode's bit for bit wherever both run;
 *   - the agglomeration (one 1024-thread workgroup per problem) keeps every listed row's first maximum over its listed
 *     later columns and rescans only the rows a merge invalidates -- about two per merge -- where the default mode
 *     rescans every live pair per merge; clusters, member order and labels are the reference's, quirks included.
 * In this mode mh_cluster_linkage, mh_linkage_debug_matrix, mh_linkage_debug_agglomerate and the frames of
 * mh_frame_set_cluster_linkage (single frames and merged batches with their own maps) accept up to 4096 points per
 * problem; 4097 -> MH_ERR_CAPACITY, nothing launched (in a frame: the first 4096 matches and the frame's capacity flag,
 * as the default mode does at 1024).  Scratch: 3 n^2 floats per problem as before, within mh_set_linkage_scratch_limit.
 * mh_linkage_set_mode: any other value -> MH_ERR_ARG, the mode stays.
 * mh_linkage_stats: counted on the device by the row-maxima kernels since the last reset -- out[0] problems clustered,
 * out[1] merges, out[2] rows rescanned (the first fill of the row maxima not counted), out[3] the largest n; reset != 0
 * zeroes them.  Synchronises the context.  All zero in the default mode. */
enum { MH_LINKAGE_SCAN = 0, MH_LINKAGE_ROWMAX = 1 };
#define MH_LINKAGE_MAX_POINTS 4096
int mh_linkage_set_mode(mh_ctx* ctx, int mode);
int mh_linkage_get_mode(mh_ctx* ctx, int* mode);   /* (a user of a shared context saves the mode, sets its own, puts it back) */
int mh_linkage_stats(mh_ctx* ctx, int64_t out[4], int reset);
/* moped3d's second depth-aware clusterer: CLUSTER_WEIGHTED_MEAN_SHIFT_CPU
 * (moped3d/libmoped/src/cluster/CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp:72-208), a true mean shift over the matches'
 * camera-frame points.  Every point starts as an active canopy; an iteration moves every active canopy to the mean --
 * weighted by a Cauchy function of the fill distance -- of the points within `radius` of its centre and then switches
 * off, in a greedy ordered scan, every later canopy within `merge` of an active one.  The clusters are the points
 * within `radius` of the surviving centres, kept when they have MORE than min_pts members: they MAY OVERLAP, a point
 * can be a member of several.  O(iterations x n^2), no matrix; at most 2048 points per problem.  fp32 in the
 * reference's operation order: clusters, member order, centres and iteration counts are its own, bit for bit. */
typedef struct mh_wms_params {
  float radius;               /* canopy radius, in the points' unit */
  float merge;                /* centres closer than this merge */
  int32_t min_pts;            /* clusters need MORE than this many members (:154) */
  int32_t max_iter;
  float half_weight_distance; /* the fill distance at which a point's weight is 1/2 (:184-186) */
} mh_wms_params;
/* The step on its own, n_problems point sets (one per (model, image)) in one call -- one upload, one launch, one
 * download: xyz_host [total][3] = the matches' camera-frame points, fill_host [total] = their fill distances, problem p =
 * rows [off[p], off[p+1]).  The clusters of all problems come back as one CSR in problem order, in the reference's
 * emission order within a problem: n_clusters[p] of them belong to problem p, cluster k's members are
 * members[cl_off[k] .. cl_off[k+1]) -- problem-local row indices, DESCENDING as the reference's push_front leaves them.
 * cl_off holds cap_clusters + 1 entries, members cap_members.  If more clusters or members exist than the caps hold:
 * MH_ERR_CAPACITY, needed[0..1] = the clusters / members that exist (also filled on success; may be NULL), and the
 * longest prefix of the cluster list that fits both caps is written -- whole clusters only, n_clusters[] counts those.
 * MH_ERR_ARG before any launch, mh_last_error naming the argument: a null pointer, an `off` that does not start at 0 or
 * decreases, a problem of more than 2048 points, a NaN or negative radius / merge / half_weight_distance, max_iter < 0,
 * a negative cap. */
int mh_cluster_wms(mh_ctx* ctx, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
                   const mh_wms_params* prm, int32_t* n_clusters, int32_t* cl_off, int cap_clusters, int32_t* members,
                   int cap_members, int64_t needed[2]);
/* For tests, in the style of mh_linkage_debug_*: the same kernel on the same arguments, its state instead of the
 * clusters -- per point the weight [total], the final centre [total][3] (a canopy that was switched off keeps the centre
 * it had then) and the active flag [total]; per problem the iteration count (the reference's nIter). */
int mh_wms_debug_state(mh_ctx* ctx, const float* xyz_host, const float* fill_host, const int32_t* off, int n_problems,
                       const mh_wms_params* prm, float* weight, float* centre, int32_t* active, int32_t* iterations);
/* CLUSTER of the following single-camera frames: this clusterer over the matches' camera-frame points from the depth map
 * (what DEPTHMAP_PROP leaves in depthData.coord3D), fill distances read from the frame's fill map at ((int) u, (int) v),
 * clamped to the map as mh_depth_prop clamps; -1 without a fill map (DEPTHMAP_PROP_CPU.hpp:107-111).  prm == NULL switches
 * it off.  It and mh_frame_set_cluster_linkage exclude each other: the one set last (with parameters) is on.
 * The clusters may overlap, so POSE reads their members from a buffer of the context, MH_WMS_MEMBER_FACTOR x the matches
 * the context has reserved (allocated when the mode is set, regrown when a frame reserves more).  Model m's clusters
 * may hold up to MH_WMS_MEMBER_FACTOR x its match count: the first cluster that would pass that is dropped whole, with
 * the model's later ones, and the frame's capacity flag is set (MH_ERR_CAPACITY from the fetch, the objects of the
 * clusters kept delivered).  A model's first 2048 matches are clustered (more: the capacity flag, as mean shift).
 * mh_frame_debug_fetch_clusters_slot and mh_frame_debug_fetch_cluster_table_slot follow the buffer (the last frame's).
 * Such frames do not share launches: a batch runs frame by frame.  Refused with MH_ERR_ARG by the frame calls: no depth
 * map, several cameras, the sharded entry points, the stepped calls (mh_step_*).  MH_ERR_ARG here, the context
 * unchanged: a NaN or negative radius / merge / half_weight_distance, max_iter < 0. */
#define MH_WMS_MEMBER_FACTOR 4
int mh_frame_set_cluster_wms(mh_ctx* ctx, const mh_wms_params* prm);
/* The two halves around exchange 1 when the DB is sharded over ranks.
 *   mh_frame_enqueue_match_local : normalise + this shard's top-2 -> top2_dev, a
 *       caller-owned device block of [3][Q] 32-bit words {idx1 (global row, int32),
 *       bits of d1, bits of d2}: the send buffer of the all-gather
 *   mh_frame_enqueue_rest        : gathered_dev = the all-gather's receive buffer,
 *       [n_shards][3][Q] words in rank order; merges the shards' top-2, keeps the
 *       matches of models this context owns, then CLUSTER..FILTER2 as above. */
int mh_frame_enqueue_match_local(mh_ctx* ctx, float* q_desc_dev, int Q, int32_t* top2_dev);
int mh_frame_enqueue_rest(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev,
                          int n_shards, const mh_cam* cam, const mh_frame_params* prm,
                          uint64_t seed);
/* The same with the shards' blocks `shard_stride_words` (>= 3 Q) 32-bit words apart in the
 * gathered buffer: whatever rides behind each [3][Q] block (e.g. the previous frame's result
 * block, so that exchange 2 needs no collective of its own) is ignored here. */
int mh_frame_enqueue_rest_strided(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev,
                                  int n_shards, int shard_stride_words, const mh_cam* cam,
                                  const mh_frame_params* prm, uint64_t seed);
/* Frames in batches (small shards: one MATCH launch and one exchange for B frames).  The B frames'
 * descriptors lie one after the other, so mh_frame_enqueue_match_local(ctx, q_desc, B * Q, top2) is
 * the batched MATCH as it is: top2 = [3][B Q] words.  After the exchange, frame f of the batch is
 *   mh_frame_enqueue_rest_batch(ctx, q_uv + 2 f Q, Q, gathered + f Q, W, shard_stride, B Q, f, ...)
 * -- `plane_stride_words` = the distance between the idx / d1 / d2 planes of a shard's block (B Q),
 * `slot` = f < MH_MAX_BATCH selects the result block the frame writes.  The frames of a batch run
 * one after the other on the context's stream.  mh_frame_fetch_slot / mh_frame_result_copy_slots_dev
 * are the per-slot forms of mh_frame_fetch / mh_frame_result_copy_dev (the latter packs the heads
 * of slots 0..n_slots-1 one after the other). */
int mh_frame_enqueue_rest_batch(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards,
                                int shard_stride_words, int plane_stride_words, int slot, const mh_cam* cam,
                                const mh_frame_params* prm, uint64_t seed);
/* All B frames of such a batch at once -- the B calls above for f = 0..B-1 (q_uv_dev / gathered_dev name frame 0's,
 * the others lie Q rows / Q words further on; results in slots 0..B-1), but with ONE launch per stage for the B frames
 * where the frames allow it (no per-frame depth state): same objects, a quarter to an eighth of the dependent launches. */
int mh_frame_enqueue_rest_frames(mh_ctx* ctx, const float* q_uv_dev, int Q, const int32_t* gathered_dev, int n_shards,
                                 int shard_stride_words, int plane_stride_words, int B, const mh_cam* cam,
                                 const mh_frame_params* prm, const uint64_t* seeds);
int mh_frame_fetch_slot(mh_ctx* ctx, int slot, mh_object* objects_host, int max_objects, int32_t* n_objects,
                        int32_t* counts);
int mh_frame_result_copy_slots_dev(mh_ctx* ctx, void* dst_dev, int n_slots, int max_objects);
/* Enqueues a device copy of the head of the context's result block {int32 n; int32 pad[3];
 * mh_object[max_objects]} -- the result of the last frame enqueued on this context, n = 0
 * before the first -- to dst_dev (16 + 40 max_objects bytes). */
int mh_frame_result_copy_dev(mh_ctx* ctx, void* dst_dev, int max_objects);
/* Synchronises the stream and copies the frame's objects out (capacity
 * max_objects); *n_objects = count.  counts (optional, 4 ints): accepted
 * matches, clusters, objects after POSE, objects after FILTER. */
int mh_frame_fetch(mh_ctx* ctx, mh_object* objects_host, int max_objects,
                   int32_t* n_objects, int32_t* counts);
/* ---- delivery: the objects of EVERY frame of a batch to the host, without stopping the stream -------------------
 *
 * The reference's frame loop hands each frame's list<SP_Object> to its caller (MopedPimpl::processImages,
 * src/moped.cpp:166-194; the test node prints them, moped2/moped_test.cpp:205-207).  For a host that keeps batches in
 * flight the per-frame fetches above cost a stream synchronisation each; these two move a whole batch in ONE
 * stream-ordered operation into a block of PINNED host memory the caller owns (hipHostMalloc / hipHostRegister /
 * torch's pin_memory), and a wait that touches only that delivery's event:
 *
 *   mh_frame_enqueue_batch(ctx, ..., B, ...);                      // batch k on this context
 *   mh_frame_fetch_batch_async(ctx, B, cap, block, tag);           // behind it, on the same stream: no host wait
 *   ... other contexts' batches ...
 *   mh_frame_fetch_wait(ctx, &flags);                              // before the context's next batch: usually done long ago
 *   for f < B: head f = (const mh_frame_head*)((char*)block + f * mh_frame_block_stride(cap)); objects follow it
 *
 * Block layout: B records of mh_frame_block_stride(max_objects) bytes, record f = mh_frame_head {n_objects, flags,
 * counts[4] (accepted matches, clusters, objects after POSE, after FILTER; -1 where unknown), tag, frame} followed
 * by mh_object[max_objects] of which the first min(n_objects, max_objects) are written (model ids as
 * mh_frame_fetch gives them).  `tag` is the caller's: a block that still holds an older delivery is recognisable.
 * A block the device can address (pinned) is written by the delivering kernel itself over PCIe; any other host
 * memory goes through a device staging buffer and one hipMemcpyAsync (pageable memory makes that copy synchronous).
 * The next batch on the context may be enqueued at once -- the delivery is ordered before it on the stream -- but the
 * BLOCK must not be handed to another delivery before mh_frame_fetch_wait returned.  One delivery per context in
 * flight: a second async call before the wait -> MH_ERR_ARG. */
typedef struct {
  int32_t n_objects;
  int32_t flags;       /* capacity / exchange flags of the frame; 0 = clean */
  int32_t counts[4];
  uint32_t tag;
  int32_t frame;       /* 0 .. B-1 */
} mh_frame_head;
size_t mh_frame_block_stride(int max_objects);   /* sizeof(mh_frame_head) + max_objects * sizeof(mh_object) */
int mh_frame_fetch_batch_async(mh_ctx* ctx, int B, int max_objects, void* host_block, uint32_t tag);
/* The same for a SHARDED context (mh_frame_enqueue_sharded[_batch]): the objects of ALL ranks, in rank order, of
 * the B frames this context ran BEFORE the current batch, as they arrived with the current batch's exchange
 * (mh_frame_previous_objects without its stream synchronisation).  counts[3] = n_objects, the others -1; flags = the
 * ranks' flags or-ed, bit 30 set when a rank had more than MH_EX2_OBJECTS objects (its surplus did not travel). */
int mh_frame_fetch_previous_async(mh_ctx* ctx, int max_objects, void* host_block, uint32_t tag);
/* Blocks until the context's pending delivery has landed (returns at once if there is none).  *flags_or (optional)
 * = the or of the B heads' flags; any set -> MH_ERR_CAPACITY with the text mh_frame_fetch_slot gives.
 * mh_frame_fetch_query: MH_OK when the delivery has landed (or none is pending), 1 while it is still in flight. */
int mh_frame_fetch_wait(mh_ctx* ctx, int32_t* flags_or);
int mh_frame_fetch_query(mh_ctx* ctx);

/* The frame's accepted matches after MATCH (+ the depth rules): query index and model of each,
 * sorted by (model, query) = the reference's `matches[model]` lists one after the other
 * (MATCH_ANN_CPU.hpp:165-176).  Synchronises the stream; *n_matches = their number. */
int mh_frame_fetch_matches(mh_ctx* ctx, int32_t* query_host, int32_t* model_host, int cap, int32_t* n_matches);
/* The same matches as correspondences {u, v, x, y, z} (FrameData::Match's coord2D and coord3D, src/util.hpp:81-88), in the
 * same order, of the last frame: what a host needs to fill `frameData.matches` the way MATCH_ANN_CPU::process does. */
int mh_frame_fetch_match_points(mh_ctx* ctx, mh_corr* corr_host, int cap, int32_t* n_matches);
/* The same for frame `slot` of the last batch (mh_frame_enqueue_batch / _rest_frames / _sharded_batch): the B frames of a
 * batch that shared their launches keep their lists side by side; of frames that went through the steps one after the
 * other (depth maps per frame, stage timing) only the last one's remain -> MH_ERR_ARG for the others. */
int mh_frame_fetch_matches_slot(mh_ctx* ctx, int slot, int32_t* query_host, int32_t* model_host, int cap,
                                int32_t* n_matches);
/* The representatives of frame `slot`'s list entries, in list order: rep[i] = the first entry j <= i with the same
 * image coordinate (u, v) as entry i (compared as floats: -0.0 == 0.0), and in frames with several images
 * (mh_frame_set_images) also the same image -- the key under which FILTER's bestPoints map files entry i
 * (FILTER_PROJECTION_CPU.hpp:89).  Read only; the same slots and errors as mh_frame_fetch_matches_slot, and slot -1 =
 * the last frame (the lists mh_frame_fetch_matches gives). */
int mh_frame_fetch_match_reps_slot(mh_ctx* ctx, int slot, int32_t* rep_host, int cap, int32_t* n_matches);
/* For tests, in the style of mh_db_debug_fetch: what the moped3d front end (mh_frame_set_depth_rules + a depth map)
 * left behind for frame `slot` of the last frame / batch, by host-side copies after the stream has drained.
 *   which 0: inv_size, double [pw ph] -- per patch 1.0 / sizeMap (DEPTHFILTER_CPU.hpp:168-178,193)
 *   which 1: keep1, uint8 [Q]         -- DEPTHFILTER's verdict on every feature (feature_density >= 0); a frame from an
 *                                        image: Q = the keypoint capacity, the flags behind the frame's keypoint count
 *                                        are not written (nothing reads them: those rows have no neighbour)
 *   which 2: m_depth, mh_depth [M]    -- DEPTHMAP_PROP's world point and Cauchy weight of every accepted match, in the
 *                                        order of mh_frame_fetch_matches_slot (any frame with depth attributes)
 * bytes must be exactly the array's size; a wrong size, a slot whose maps are gone or an array the last frame did not
 * write -> MH_ERR_ARG, nothing is read. */
int mh_depth_rules_debug_fetch(mh_ctx* ctx, int which, int slot, void* out_host, size_t bytes);
/* For tests, next to mh_frame_fetch_matches_slot: what CLUSTER left for frame `slot` of the last frame / batch, as
 * mh_step_cluster reports a stepped frame's -- cl_model_host[c] = the model of cluster c (clusters in (model, emission)
 * order, the order POSE walks them), members of cluster c = members_host[cl_off_host[c] .. cl_off_host[c + 1]), indices
 * INSIDE that model's match list in the clusterer's member order.  Read from the per-model lists the clusterer wrote (the
 * flat cluster table is FILTER's by the end of a frame).  A frame with several images (mh_frame_set_images) was
 * clustered per (model, image) pair: the lists read are the pairs' (off2 over the (model, image, query) copy of the
 * matches), clusters come in (model, image, emission) order, cl_model_host names the real model and the members are
 * indices inside the PAIR's list.  The same slots and errors as mh_frame_fetch_matches_slot;
 * cl_off_host holds cap_clusters + 1 entries; more clusters or members than the caps -> MH_ERR_CAPACITY with
 * *n_clusters = their number. */
int mh_frame_debug_fetch_clusters_slot(mh_ctx* ctx, int slot, int32_t* cl_model_host, int32_t* cl_off_host,
                                       int32_t* members_host, int cap_clusters, int cap_members, int32_t* n_clusters);
/* For tests: the FLAT cluster table of frame `slot` as the device holds it -- the arrays POSE walks.  Reads, at the
 * slot's arena offset, cl_model / cl_begin / cl_count (row k: cluster k's model, its first entry in ms_members as an
 * absolute position in the frame's match list -- the (model, image, query) copy for a frame with several images --
 * and its member count), FrameCounts::n_clusters into *n_clusters (the rows CLUSTER published, which no later stage
 * writes: that many rows are copied) and the device word fs->n_clusters into *n_clusters_now (optional; the row count
 * the NEXT stage would read: CLUSTER's until FILTER / FILTER2 rewrite table and word, so 0 after a whole frame whose
 * FILTER2 kept nothing).  The rows are CLUSTER's only while no FILTER has kept an object (it rewrites the first
 * `kept` rows).  The same slots and errors as mh_frame_fetch_matches_slot; more rows than cap_clusters ->
 * MH_ERR_CAPACITY with *n_clusters = their number and the first cap_clusters rows copied. */
int mh_frame_debug_fetch_cluster_table_slot(mh_ctx* ctx, int slot, int32_t* cl_model_host, int32_t* cl_begin_host,
                                            int32_t* cl_count_host, int cap_clusters, int32_t* n_clusters,
                                            int32_t* n_clusters_now);
/* Device address of the frame's packed result block {int32 n; mh_object[cap]}
 * for exchange 2 (gather of per-rank objects); *bytes = its size. */
int mh_frame_result_dev(mh_ctx* ctx, void** block_dev, int64_t* bytes);

/* ---- N > 1: the DB sharded over ranks, the frame's exchanges inside the library ----------------
 *
 * Rank r of W holds the models [r n/W, (r+1) n/W) (mh_db_upload with index_base = its first global row) and every
 * rank sees every frame.  A sharded frame = this shard's top-2 per query, ONE all-gather of [3][Q] words per rank
 * (exchange 1; behind them rides the result block of the context's previous frame = exchange 2, so a frame costs
 * one collective), merge, then CLUSTER .. FILTER2 for the models the rank owns -- all on the context's stream.
 * The objects of a sharded frame are bit-identical to the single-context frame's (tests/test_gpu_comm.py).
 * The loop this serves: MopedPimpl::processImages, moped2/libmoped/src/moped.cpp:166-194.
 *
 * Transport: RCCL (ncclAllGather over xGMI), resolved at run time -- the copy already in the process, else
 * librccl.so.1 from the loader path or /opt/rocm/lib, else $MH_RCCL_PATH -- or a host callback.
 *   mh_comm_create      one process per GPU: rank 0 makes the id (mh_comm_unique_id), the host's launcher hands
 *                       it to the others (MPI_Bcast, a file, torch.distributed ...), every rank calls this
 *   mh_comm_create_all  one process that owns W devices (ncclCommInitAll): comms[r] belongs to ctxs[r]
 *   mh_comm_create_host bring-your-own transport: fn(user, send, recv, bytes) must fill recv[W][bytes] with every
 *                       rank's send block in rank order; it is called on the host with the stream drained
 *                       (ranks that share a device, MPI-only hosts, test rigs)
 * A communicator may serve several contexts of its device (frames in flight); like any NCCL communicator it wants
 * its collectives issued in the same order on every rank. */
#define MH_COMM_ID_BYTES 128
#define MH_EX2_OBJECTS 62   /* objects per rank and frame that ride on the next frame's exchange */
typedef struct mh_comm mh_comm;
typedef int (*mh_allgather_fn)(void* user, const void* send_host, void* recv_host, size_t bytes_per_rank);
int mh_comm_unique_id(unsigned char id[MH_COMM_ID_BYTES]);
int mh_comm_create(mh_ctx* ctx, const unsigned char id[MH_COMM_ID_BYTES], int rank, int world, mh_comm** comm);
int mh_comm_create_all(mh_ctx* const* ctxs, int world, mh_comm** comms);
int mh_comm_create_host(mh_ctx* ctx, int rank, int world, mh_allgather_fn fn, void* user, mh_comm** comm);
int mh_comm_destroy(mh_comm* comm);
int mh_comm_info(const mh_comm* comm, int* rank, int* world, int* is_rccl);
/* One frame / a batch of B <= MH_MAX_BATCH frames (descriptors and keypoints of the B frames one after the other:
 * one MATCH launch and one exchange for all of them; frame f leaves its objects in result slot f). */
int mh_frame_enqueue_sharded(mh_ctx* ctx, mh_comm* comm, float* q_desc_dev, const float* q_uv_dev, int Q,
                             const mh_cam* cam, const mh_frame_params* prm, uint64_t seed);
int mh_frame_enqueue_sharded_batch(mh_ctx* ctx, mh_comm* comm, float* q_desc_dev, const float* q_uv_dev, int Q, int B,
                                   const mh_cam* cam, const mh_frame_params* prm, const uint64_t* seeds);
/* The single-process form: rank r's copy of the frame inputs on its device in q_desc_dev[r] / q_uv_dev[r]; the W
 * collectives go out as one group. */
int mh_frame_enqueue_sharded_all(mh_ctx* const* ctxs, mh_comm* const* comms, int world, float* const* q_desc_dev,
                                 const float* const* q_uv_dev, int Q, int B, const mh_cam* cam,
                                 const mh_frame_params* prm, const uint64_t* seeds);
/* Objects of ALL ranks (rank order = model order) for the frame(s) this context ran BEFORE the current one, as
 * they arrived with the current exchange: frame_in_batch < B.  Synchronises the stream.  *n_objects may exceed
 * cap (the first cap are written).  A rank with more than MH_EX2_OBJECTS objects -> MH_ERR_CAPACITY (use
 * mh_frame_gather_objects for that frame). */
int mh_frame_previous_objects(mh_ctx* ctx, int frame_in_batch, mh_object* objects_host, int cap, int32_t* n_objects);
/* Exchange 2 on its own for the frame in result slot `slot` (the last frame of a stream, or any frame whose
 * objects are wanted at once): all ranks call it; all ranks get all objects. */
int mh_frame_gather_objects(mh_ctx* ctx, mh_comm* comm, int slot, mh_object* objects_host, int cap,
                            int32_t* n_objects);

/* ---- FEAT: SIFT extraction ---------------------------------------- */

/* FEAT_SIFT_CPU::process for one image (src/feat/FEAT_SIFT_CPU.hpp:78-112 over libsiftfast 1.1's
 * GetKeypoints, libs.tgz -> libsiftfast-1.1-src/libsiftfast.cpp:301-361): gray = height x width
 * bytes; double_size = the ScaleOrigin "-1" setting (config.hpp:69).  Keypoints come out in the
 * reference's (single-thread) list order: xy = coord2D = (col, row), scale_ori (optional) =
 * (scale, orientation), desc = 128 floats, unit length.  `cap` = capacity of the outputs; more
 * keypoints than that -> MH_ERR_CAPACITY (the first `cap` are still written). */
int mh_sift_extract(mh_ctx* ctx, const uint8_t* gray_host, int width, int height, int double_size,
                    float* xy_host, float* scale_ori_host, float* desc_host, int cap,
                    int32_t* n_keypoints);
/* The same with everything on the device and no host synchronisation: desc_dev [cap][128] and
 * xy_dev [cap][2] can be handed to mh_frame_enqueue once *n_dev (device int32) has been read. */
int mh_sift_extract_dev(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size,
                        float* desc_dev, float* xy_dev, float* scale_ori_dev, int cap, int32_t* n_dev);

/* n_images <= MH_MAX_BATCH device images of one size through FEAT alone, ONE launch per stage for all of them (what
 * mh_frame_enqueue_image_batch runs ahead of MATCH): image i's keypoints at desc_dev + i cap 128 / xy_dev + i cap 2,
 * its count in counts_dev[i] (device int32).  Asynchronous.  Every image's output is bit for bit that of
 * mh_sift_extract_dev on it alone. */
int mh_sift_extract_batch_dev(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_images, int width, int height,
                              int double_size, float* desc_dev, float* xy_dev, int cap, int32_t* counts_dev);

/* FOR VERIFICATION (tests/test_gpu_sift_stages.py): what the context's LAST extraction left on the device, stage by
 * stage, for image `slot` of that launch (0 for a single image, 0 .. n_images - 1 after a batch).  Every call
 * synchronises the context's stream and copies to host memory; none launches a kernel or changes the state.
 * MH_ERR_ARG: no extraction yet, a slot / octave / level that does not exist. */
#define MH_SIFT_MAX_OCTAVES 8
typedef struct {             /* a refined extremum: InterpKeyPoint's result (libsiftfast.cpp:1164-1206) */
  int32_t octave, index;     /* scale index 1..3 */
  uint32_t key;              /* generation order within the octave: (index - 1) rows cols + start r * cols + start c */
  int32_t r, c;              /* final pixel */
  float x0, x1, x2;          /* offsets in scale, row, column */
} mh_sift_candidate;
typedef struct {             /* one (extremum, orientation peak) */
  int32_t octave, index;
  uint64_t order;            /* octave << 40 | key << 8 | histogram bin */
  float fsize, frow, fcol, ori;
} mh_sift_key;
/* The octave plan of the last extraction: rows[o], cols[o] for o < *n_octaves (arrays of MH_SIFT_MAX_OCTAVES), and the
 * number of image slots its launch filled. */
int mh_sift_debug_plan(mh_ctx* ctx, int32_t* n_images, int32_t* n_octaves, int32_t* rows, int32_t* cols);
/* kind 0: Gaussian level 0..4 (level 5 is never stored: only its DoG is kept), kind 1: DoG level 0..4 of `octave`;
 * out_host = rows x cols floats. */
int mh_sift_debug_level(mh_ctx* ctx, int slot, int octave, int kind, int level, float* out_host);
/* The candidates in the order the kernel appended them (any), won_host[i] = 1 where candidate i's claim is the owner
 * word of its final pixel (the first extremum in generation order to end there).  *n = their number; `cap` are written. */
int mh_sift_debug_candidates(mh_ctx* ctx, int slot, mh_sift_candidate* out_host, uint8_t* won_host, int cap, int32_t* n);
/* The key buffer, slots in the order the kernel filled them (any).  *n = their number; `cap` are written. */
int mh_sift_debug_keys(mh_ctx* ctx, int slot, mh_sift_key* out_host, int cap, int32_t* n);
/* The shipped descriptor kernel alone on n keys of the caller's, over the pyramid the last extraction left in `slot`,
 * launched on `workgroups` workgroups (0: as in production, 4 096; fewer workgroups than keys: a workgroup describes
 * several keys, as in batches of five or more images).  Keys and outputs live in temporary buffers: the context's key
 * buffer, counters and outputs stay untouched.  Output place i (desc_host [n][128], xy_host [n][2] = (col, row),
 * scale_ori_host [n][2], optional) = the key with i keys of larger `order`, as in production.  Synchronises.
 * MH_ERR_ARG: no extraction yet, no such slot, n < 1, a key whose octave is outside the plan or whose index is not 1..3,
 * `order` values that are not distinct, fsize outside (0, 64], |frow| or |fcol| above 1e6, |ori| above 8, a NaN. */
int mh_sift_debug_describe(mh_ctx* ctx, int slot, const mh_sift_key* keys_host, int n, int workgroups, float* desc_host,
                           float* xy_host, float* scale_ori_host);
/* ONE blur level of a host image through a named kernel of the blur chain, with GaussianBlur's kernel for `sigma`:
 *   0  row kernel + column kernel         any tap count below 64
 *   1  tile kernel, one level             half-width <= 16
 *   2  tile kernel, job list              half-width <= 16 (a kernel of its own for 11, 13, 17, 21, 25 taps); half = 1:
 *                                         the source is read at every second row and column (HalfImageSize fused into
 *                                         the level) and half_host gets those pixels
 *   3  HalfImageSize alone                half = 1, sigma unused, dst_host = every second row and column
 *   4  single-workgroup chain             at most 6 912 pixels, dog_host required
 * dst_host (and dog_host = source - blurred, optional for 0 .. 2) are rows x cols floats: src_rows x src_cols, or half
 * of each (rounded down) with half = 1.  A variant that cannot take the arguments returns MH_ERR_ARG and launches
 * nothing.  Synchronises. */
int mh_sift_debug_blur(mh_ctx* ctx, int variant, const float* src_host, int src_rows, int src_cols, float sigma, int half,
                       float* dst_host, float* dog_host, float* half_host);

/* FEAT + the whole frame, image in, objects out, nothing through the host: SIFT of the device image
 * (as mh_sift_extract_dev) straight into the frame's query buffers, then mh_frame_enqueue's launch
 * list.  The keypoint count stays on the device: every launch is sized for `max_keypoints` and the
 * kernels read the count (query blocks beyond it leave at once); more keypoints than that -> the
 * first max_keypoints in list order are used.  Results: mh_frame_fetch; mh_frame_keypoints = the
 * keypoint count of the frame last fetched; mh_frame_features_dev = the device buffers
 * (descriptors already L2-normalised like MATCH_ANN_CPU.hpp:157 leaves them).
 * With a depth map (mh_frame_set_depth_image), the depth rules (mh_frame_set_depth_rules) and the linkage clusterer this
 * is moped3d's pipeline (moped3d/libmoped/src/config.hpp:38-49) behind FEAT for one Kinect frame: DEPTHFILTER counts
 * the frame's keypoints from the device word, not the capacity (tests/test_gpu_kinect_image_batch.py). */
int mh_frame_enqueue_image(mh_ctx* ctx, const uint8_t* gray_dev, int width, int height, int double_size,
                           int max_keypoints, const mh_cam* cam, const mh_frame_params* prm, uint64_t seed);
/* B <= MH_MAX_BATCH images at once: FEAT image by image (every image's keypoints at a stride of max_keypoints rows,
 * its count in a device word of its own), then ONE MATCH launch sequence over all of them -- an image's ~600
 * keypoints alone leave the matrix pipes a sixth as busy per query as a batch does --, then CLUSTER..FILTER2 image
 * after image into result slots 0 .. B-1 (mh_frame_fetch_slot).  Every image's objects are bit for bit those of
 * mh_frame_enqueue_image(..., seeds[f]) on it alone.  One camera.
 * moped3d's front end (moped3d/libmoped/src/config.hpp:38-49: DEPTHFILTER x 2, the adaptive ratio, DEPTHMAP_PROP,
 * CLUSTER_LINKAGE or mean shift, either depth residual of POSE) travels with the batch when the context holds exactly
 * one depth map per image: mh_frame_set_depth_image_batch with n_images maps (n_images = 1: mh_frame_set_depth_image
 * counts too).  Frame f reads map f and counts its own keypoints (count word f): rows behind a frame's count, whatever
 * an earlier batch left there, reach no keep flag, patch counter, ratio or match.  The frames share one launch per
 * stage; with mh_enable_timing on they run one after the other, each with its own map and count.  Depth maps are not
 * undistorted (mh_frame_set_undistort remaps the gray images only).
 * Refused with MH_ERR_ARG, the context unchanged, the message naming the call to use instead: per-query depth attributes
 * (mh_frame_set_depth: nobody has attributes for keypoints the device makes), a per-query image index with more than
 * one image (mh_frame_set_images), a number of depth maps other than n_images, the depth rules without any depth map
 * (as before: they would be ignored). */
int mh_frame_enqueue_image_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_images, int width, int height,
                                 int double_size, int max_keypoints, const mh_cam* cam, const mh_frame_params* prm,
                                 const uint64_t* seeds);
int mh_frame_features_dev(mh_ctx* ctx, float** desc_dev, float** uv_dev, int32_t** n_dev);
int mh_frame_keypoints(mh_ctx* ctx, int32_t* n_keypoints);

/* ---- moped3d's depth steps on a step's own lists (the STEP plugins DEPTHFILTER_HIP / DEPTHMAP_PROP_HIP) -----------
 *
 * Inside the resident frame these rules run in group_kernel / feature_density_kernel (mh_frame_set_depth_rules); a
 * libmoped tree that keeps moped3d's DEPTHFILTER, DEPTHFILTER2 and DEPTHPROP slots (moped3d/libmoped/src/config.hpp:41,
 * 43,44) as steps of their own hands every step its own lists.  Both calls are synchronous host round trips like
 * mh_meanshift and mh_filter.  depth_xyzn_host [height][width][4] (x, y, z, norm; negative norm = invalid) is copied
 * into the context-owned buffers mh_frame_set_depth_image_host fills; NULL = the map the context holds already
 * (mh_frame_set_depth_image[_host], its width and height), so that a frame's map crosses PCIe once for all its steps.
 * A host map handed in here serves this call alone; a frame map that lived in those buffers
 * (mh_frame_set_depth_image_host, mh_frame_run_kinect_host) is overwritten by it and therefore switched off: set it again.
 *
 * mh_depth_filter: DEPTHFILTER_CPU::process (moped3d/libmoped/src/depthfilter/DEPTHFILTER_CPU.hpp:117-254) on n =
 * group_off_host[n_groups] points uv_host [n][2]: group g = points [group_off_host[g], group_off_host[g + 1]) is counted
 * by itself -- n_groups = 1 is ToFilter = 1 (:180-214, the detected features), n_groups = the models is ToFilter = 2
 * (:215-251, matches[model] one after the other).  keep_host[i] = 1 where the density of point i's group per square
 * metre of scene surface over patch_size x patch_size pixel patches, dilated 3x3 (:76-113), exceeds density * 100 * 100
 * (:130).  K = the depth map's intrinsicLinearCalibration.  The reference's arithmetic as written: `y1 = min(..,
 * width)` (:171), a NaN depth never wins the minimum (:162), coordinates outside the map are clamped to it (the
 * reference indexes out of bounds).  Bit for bit the verdicts of the frame path (mh_depth_rules_debug_fetch which 1;
 * the lists mh_frame_fetch_matches gives).  More than 4096 patches -> MH_ERR_CAPACITY. */
int mh_depth_filter(mh_ctx* ctx, const float* depth_xyzn_host, int width, int height, const float K[4], int patch_size,
                    float density, const float* uv_host, const int32_t* group_off_host, int n_groups, uint8_t* keep_host);
/* Match::depthInformation (moped3d/libmoped/src/util.hpp:73-84) */
typedef struct {
  int32_t depth_valid;   /* depthValid: the pixel's norm >= 0 */
  float coord3d[3];      /* coord3D: the pixel's x, y, z */
  float depth;           /* depth: its z */
  float fill_distance;   /* fillDistance: the ".distance" map's value, -1 without such a map */
} mh_depth_info;
/* mh_depth_prop: DEPTHMAP_PROP_CPU::process (moped3d/libmoped/src/depthprop/DEPTHMAP_PROP_CPU.hpp:52-134) for n points
 * uv_host [n][2]: out_host[i] = the record of pixel ((int) u, (int) v) -- truncated, no interpolation (:103,119-132),
 * clamped to the map.  With depth_xyzn_host, fill_distance_host [height][width] is that map's ".distance" map or NULL =
 * none (fillDistance -1, :107-111); with depth_xyzn_host NULL the context's distance map, if it holds one. */
int mh_depth_prop(mh_ctx* ctx, const float* depth_xyzn_host, const float* fill_distance_host, int width, int height,
                  const float* uv_host, int n, mh_depth_info* out_host);

/* ONE Kinect frame of moped3d's pipeline (moped3d/libmoped/src/config.hpp:38-49) in one synchronous call, host memory
 * in, objects out -- what FRAME_RESIDENT_HIP's mh_frame_run_host is to moped2 (the STEP plugin FRAME_RESIDENT_3D_HIP):
 * gray_host [height][width] and depth_xyzn_host [height][width][4] are copied into context-owned buffers; fill_scale > 0
 * (or -1: the reference's automatic factor): mh_depth_fill(fill_scale, bilinear, K = cam->K) fills the map on the
 * device, and the filled map and its distance map are copied back into depth_xyzn_host / fill_distance_host (both
 * required: DEPTH_FILL_EXACT_CPU::process leaves them in the frame's images); fill_scale = 0: the maps arrive filled,
 * fill_distance_host is read, or NULL = no distance map.  Then mh_frame_set_depth_image(kind, alpha, cauchy_scale),
 * mh_frame_enqueue_image(double_size, max_keypoints, cam, prm, seed) and mh_frame_fetch -- the calls a host composes
 * itself from device buffers, launch for launch (this call has no kernel of its own), so the objects are bit for bit
 * theirs.  The depth rules and the clusterer are what mh_frame_set_depth_rules / mh_frame_set_cluster_linkage left.
 * The frame's lists afterwards: mh_frame_fetch_matches / mh_frame_fetch_match_points; the context keeps the map
 * (mh_depth_filter / mh_depth_prop with NULL read it). */
int mh_frame_run_kinect_host(mh_ctx* ctx, const uint8_t* gray_host, float* depth_xyzn_host, float* fill_distance_host,
                             int width, int height, int double_size, int max_keypoints, const mh_cam* cam,
                             const mh_frame_params* prm, int fill_scale, int bilinear, int kind, float alpha,
                             float cauchy_scale, uint64_t seed, mh_object* objects_host, int max_objects,
                             int32_t* n_objects, int32_t* counts);
/* The same from what the sensor delivers (moped3d/moped3d.cpp:270-338: the node builds the map, then processImages):
 * raw_host / raw as mh_depth_map_from_raw_host takes them, the map of width x height (the gray image's size, :277-278)
 * is built on the device with K = cam->K (the cameras coincide, as for the fill of mh_frame_run_kinect_host), and from
 * there on the call is mh_frame_run_kinect_host launch for launch: the objects and counts are bit for bit those of that
 * call fed the same map.  depth_xyzn_host and fill_distance_host are optional OUTPUTS (NULL: nothing is copied back):
 * the map as the frame used it (filled when fill_scale != 0) and its distance map (fill_scale != 0 only; with
 * fill_scale = 0 there is no distance map and fill_distance_host is left alone). */
int mh_frame_run_kinect_raw_host(mh_ctx* ctx, const uint8_t* gray_host, const void* raw_host, const mh_raw_depth* raw,
                                 float* depth_xyzn_host, float* fill_distance_host, int width, int height,
                                 int double_size, int max_keypoints, const mh_cam* cam, const mh_frame_params* prm,
                                 int fill_scale, int bilinear, int kind, float alpha, float cauchy_scale, uint64_t seed,
                                 mh_object* objects_host, int max_objects, int32_t* n_objects, int32_t* counts);

/* ONE frame seen by n_images cameras, images resident on the device: FEAT of every image
 * (FEAT_SIFT_CPU.hpp:80-107: image 0's keypoints in libsiftfast's list order, then image 1's, ...,
 * imageIdx = i), then MATCH..FILTER2 of the frame with every keypoint in its own image
 * (what mh_frame_set_images + mh_frame_enqueue do for a host that knows the counts): CLUSTER per (model, image)
 * (CLUSTER_MEAN_SHIFT_CPU.hpp:189-195), POSE through cams[image], FILTER keyed by (coord2D, image).
 * gray_dev: HOST array of n_images device images, all width x height; cams[n_images].  The frame's list is packed:
 * image 0's first min(count, max_keypoints_per_image) keypoints, then image 1's, ...; one frame takes
 * n_images * max_keypoints_per_image rows (mh_reserve).  The counts never leave the device: one launch packs the
 * list, MATCH is launched for the capacity and reads the total.  mh_frame_fetch as for any frame; mh_frame_keypoints
 * = the total; mh_frame_features_dev = the packed, normalised list; mh_frame_image_counts = what each image gave.
 * n_images = 1 gives bit for bit what mh_frame_enqueue_image gives.  The call owns the context's image indices and
 * cameras (mh_frame_set_images) for its own duration only.  UNDISTORTED_IMAGE: mh_frame_set_undistort_images, or
 * mh_frame_set_undistort's one set of coefficients with every camera's K.
 * MH_ERR_CAPACITY: n_images > MH_MAX_IMAGES.  MH_ERR_ARG: a depth map, depth rules or per-query depth attributes are
 * set (several cameras: the linkage clusterer too).  Nothing of the context changes on a refusal. */
int mh_frame_enqueue_images(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_images, int width, int height,
                            int double_size, int max_keypoints_per_image, const mh_cam* cams,
                            const mh_frame_params* prm, uint64_t seed);
/* B = n_frames such frames of one rig (cams[n_images]): frame f's images are gray_dev[f * n_images .. f * n_images +
 * n_images - 1], its packed list starts at row f * n_images * max_keypoints_per_image, its total lies in a device word
 * of its own.  FEAT: one launch per stage for all n_frames * n_images <= MH_MAX_BATCH images (more: MH_ERR_CAPACITY);
 * one launch packs every frame's list; ONE MATCH launch sequence; CLUSTER..FILTER2 into result slots 0 .. B-1
 * (mh_frame_fetch_slot), merged where one camera allows it.  Every frame's objects and counts are bit for bit those of
 * mh_frame_enqueue_images(..., seeds[f]) on it alone.  Reserve with mh_reserve_batch(n_images *
 * max_keypoints_per_image, n_frames, ...). */
int mh_frame_enqueue_images_batch(mh_ctx* ctx, const uint8_t* const* gray_dev, int n_frames, int n_images, int width,
                                  int height, int double_size, int max_keypoints_per_image, const mh_cam* cams,
                                  const mh_frame_params* prm, const uint64_t* seeds);
/* Keypoints each image contributed to the frame last fetched with mh_frame_fetch (after clamping to the per-image
 * capacity): min(cap, *n_images) counts are written.  A frame of mh_frame_enqueue_image counts as one image.
 * MH_ERR_ARG: no such frame fetched yet. */
int mh_frame_image_counts(mh_ctx* ctx, int32_t* counts, int cap, int32_t* n_images);
/* The image index (device int32, one per row) beside the list mh_frame_features_dev hands out, for the frame
 * mh_frame_enqueue_images enqueued last (FEAT_SIFT_CPU.hpp:100: imageIdx).  MH_ERR_ARG: the last frame is no such frame. */
int mh_frame_features_image_dev(mh_ctx* ctx, int32_t** q_image_dev);

/* ---- UNDISTORT: lens undistortion (UTIL_UNDISTORT) ------------------------------------ */

/* UTIL_UNDISTORT (src/util/UTIL_UNDISTORT.hpp) on the device.  K = fx, fy, cx, cy (Image::intrinsicLinearCalibration,
 * :77-81); dist = k1, k2, p1, p2 (intrinsicNonlinearCalibration, :84-87; k3 = 0).  The maps are cvInitUndistortMap's
 * (:68-98: OpenCV 2.x initUndistortRectifyMap with R = I and the new camera = K, in double); the resampling is
 * cvRemap(CV_INTER_LINEAR + CV_WARP_FILL_OUTLIERS) (:127: 5-bit fixed-point bilinear, border 0).  A context keeps the
 * maps of its last MH_MAX_IMAGES cameras (the reference keeps all, keyed by size and calibration, :52-66); a new one is
 * built on the context's stream.  MH_ERR_ARG: a null pointer, a side <= 0 or > 32767, a non-finite K or dist, fx or
 * fy = 0. */
/* The float maps UTIL_UNDISTORT::init builds (:94): mapx, mapy [height][width] each.  Synchronises. */
int mh_undistort_map(mh_ctx* ctx, int width, int height, const float K[4], const float dist[4],
                     float* mapx_host, float* mapy_host);
/* UTIL_UNDISTORT::process for one image (:121-131): height x width bytes; out == in allowed.  Synchronises. */
int mh_undistort(mh_ctx* ctx, const uint8_t* gray_host, uint8_t* out_host, int width, int height,
                 const float K[4], const float dist[4]);
/* The same on device images, stream-ordered, no host synchronisation; out != in (MH_ERR_ARG). */
int mh_undistort_dev(mh_ctx* ctx, const uint8_t* gray_dev, uint8_t* out_dev, int width, int height,
                     const float K[4], const float dist[4]);
/* "UNDISTORTED_IMAGE" ahead of FEAT in the resident image path (config.hpp:59): mh_frame_enqueue_image and
 * mh_frame_enqueue_image_batch remap their image(s) with (width, height, cam->K, dist) into a staging buffer of the
 * context, one launch for a batch, and FEAT reads that.  dist = NULL: off (the default). */
int mh_frame_set_undistort(mh_ctx* ctx, const float dist[4]);
/* UNDISTORTED_IMAGE per camera for mh_frame_enqueue_images[_batch] (UTIL_UNDISTORT.hpp:52-66 keys its maps by
 * calibration): dist[i] goes with cams[i].K, every image is remapped with its camera's map -- the entries of the same
 * cache of MH_MAX_IMAGES maps, still one remap launch per call.  n_images must be the rig's (else the enqueue returns
 * MH_ERR_ARG).  NULL / 0 = off. */
int mh_frame_set_undistort_images(mh_ctx* ctx, const float (*dist)[4], int n_images);

/* ---- model files ------------------------------------------------ */

/* Host-side set of models: parsed from `.moped.xml` files the way Moped::addModel(sXML&)
 * reads them (src/moped.cpp:101-137 over include/sXML.hpp:53-118) or mapped from a packed
 * `.mopeddb` container.  Rows are flattened in model order like
 * MATCH_ANN_CPU::Update (src/match/MATCH_ANN_CPU.hpp:76-99).  Only points whose desc_type
 * equals the set's (default "SIFT") are kept; a point whose descriptor does not have 128
 * values is an error.  Adding a model whose name exists replaces it (moped.cpp:141-146). */
typedef struct mh_model_set mh_model_set;
int mh_models_create(mh_model_set** out, const char* desc_type /* NULL = "SIFT" */);
void mh_models_destroy(mh_model_set* s);
const char* mh_models_last_error(const mh_model_set* s);
int mh_models_add_xml(mh_model_set* s, const char* path);
int mh_models_add_xml_buffer(mh_model_set* s, const char* data, int64_t bytes);
int mh_models_count(const mh_model_set* s);
int64_t mh_models_rows(const mh_model_set* s);
const char* mh_models_name(const mh_model_set* s, int i);
/* rows [row_begin, row_begin + n_rows) of model i; bbox = min xyz, max xyz (moped.cpp:107-124) */
int mh_models_range(const mh_model_set* s, int i, int64_t* row_begin, int64_t* n_rows, float bbox[6]);
const float* mh_models_desc(const mh_model_set* s);   /* [rows][128], as parsed (not normalised) */
const float* mh_models_xyz(const mh_model_set* s);    /* [rows][3] */
/* Packed container: written once, then mapped read-only and uploaded as it lies. */
int mh_models_save(const mh_model_set* s, const char* path);
int mh_models_load(mh_model_set** out, const char* path);
/* Update() for models [first_model, first_model + n_models) of the set (a rank's shard):
 * uploads their rows, L2-normalises them on the device (A1) and sets index_base to the
 * first row, so row and model ids stay global. */
int mh_db_upload_models(mh_ctx* ctx, const mh_model_set* s, int first_model, int n_models);
/* mh_db_splice with the rows of model `set_index` of a parsed set, normalised on the device (s unused for REMOVE). */
int mh_db_splice_models(mh_ctx* ctx, int op, int model, const mh_model_set* s, int set_index);
/* mh_db_upload with the normalisation done on the device (normalize != 0). */
int mh_db_upload_raw(mh_ctx* ctx, const float* desc_host, const int32_t* model_of_host,
                     const float* xyz_host, int N, int n_models, int32_t index_base, int normalize);
/* A model from rows (e.g. the ones mh_db_splice_image hands back): `name` replaces a model of that name, else appends
 * (moped.cpp:141-146, as mh_models_add_xml).  desc [n_rows][128], xyz [n_rows][3] are kept as given, NOT normalised;
 * the bounding box is min / max of xyz (moped.cpp:107-125).  MH_ERR_ARG: n_rows < 0, a null name, null arrays with
 * n_rows > 0, a set that is a mapped .mopeddb. */
int mh_models_add_rows(mh_model_set* s, const char* name, const float* desc, const float* xyz, int64_t n_rows);
/* Model i of the set as the `.moped.xml` file samples/createModels/createModels.cpp:121-126 writes: the tree
 * Moped::createPlanarModelsFromImages builds (src/moped.cpp:211-233: <Model name=..> with one <Points> child, one <Point>
 * per row with p3d, desc_type, desc), printed as sXML::print prints it (include/sXML.hpp:146-170: one tab per level,
 * properties in std::map order = desc, desc_type, p3d), numbers as toString prints them (include/moped.hpp:359-360:
 * ostream << float = %g, 6 significant digits; a z of 0 prints as "0", the literal of moped.cpp:225).
 * WHICH DESCRIPTORS: the file holds the set's rows -- for a model taught by mh_db_splice_image FEAT's unit-length
 * descriptors.  The reference's file holds what MATCH left in detectedFeatures: the same rows renormalised once more in
 * place (src/match/MATCH_ANN_CPU.hpp:157), and only when its database had more than one point (:140, skipCalculation);
 * the rows mh_frame_features_dev hands out after a frame are exactly those.  The 6-digit text hides the difference on
 * almost every value; it is not pinned. */
int mh_models_write_xml(const mh_model_set* s, int i, const char* path);

/* ---- planar models from images: Moped::createPlanarModelsFromImages (src/moped.cpp:196-236) -----------------------
 * The reference runs the pipeline's front on each image and turns every detected feature into a model point at
 * (u scale, v scale, 0), in detectedFeatures order (:220-232); samples/createModels/createModels.cpp is its user.  Here:
 * image on the device in, a new model in the resident store out, while frames keep flowing.
 *
 * form 0 (the reference's, :225): x = u scale, y = v scale, z = 0.
 * form 1 (a plane at depth z in front of a camera K = fx, fy, cx, cy):  x = (u - cx) / fx * z, y = (v - cy) / fy * z, z.
 * One float32 rounding per operation in that order, no fused multiply-add, correctly rounded division.
 * roi = u0, v0, u1, v1: keypoint (u, v) is kept if u0 <= u < u1 && v0 <= v < v1 (a NaN coordinate is dropped); all zeros
 * = every keypoint.  max_rows > 0: only the first max_rows kept keypoints (list order).  Kept rows come out densely
 * packed in FEAT's list order; descriptors are copied unchanged. */
typedef struct {
  int32_t form;
  float scale;
  float K[4];
  float z;
  float roi[4];
  int32_t max_rows;
} mh_planar_spec;
/* The selection alone, on given device arrays (the rows of mh_sift_extract_dev or mh_frame_features_dev): desc_dev
 * [cap][128], xy_dev [cap][2], *n_dev keypoints (clamped to [0, cap]).  Writes the
 * kept rows to desc_out_dev [out_cap][128] / xyz_out_dev [out_cap][3] -- the first out_cap if more are kept -- their
 * count to *n_out_dev and Model::boundingBox (moped.cpp:107-125: min xyz, max xyz; +-10E10 when nothing is kept) to
 * bbox_dev[6].  Rows at and beyond *n_out_dev are not written.  Stream-ordered, no host wait.  MH_ERR_ARG: a spec
 * mh_db_splice_image refuses, descriptor arrays not 16-byte aligned. */
int mh_planar_rows_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int cap,
                       const mh_planar_spec* spec, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                       int32_t* n_out_dev, float* bbox_dev);
/* n_images <= MH_MAX_BATCH lists in ONE launch (the layout of mh_sift_extract_batch_dev: image i at desc_dev + i cap 128,
 * xy_dev + i cap 2, n_dev[i]); image i's rows go to desc_out_dev + i out_cap 128 / xyz_out_dev + i out_cap 3, n_out_dev[i],
 * bbox_dev + 6 i, bit for bit what mh_planar_rows_dev writes for it alone. */
int mh_planar_rows_batch_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int n_images,
                             int cap, const mh_planar_spec* spec, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                             int32_t* n_out_dev, float* bbox_dev);
/* createPlanarModelsFromImages for one image, into the resident store: [UNDISTORTED_IMAGE with spec->K if
 * mh_frame_set_undistort is on] -> FEAT (max_keypoints = the list's capacity) -> selection -> mh_db_splice(op, model)
 * of the kept rows with normalize = 1, as Update() normalises model descriptors (src/match/MATCH_ANN_CPU.hpp:94).
 * op = MH_DB_INSERT or MH_DB_REPLACE.  The selection writes straight into the edit's staging block; the rows never
 * leave the device.  Every guarantee of mh_db_splice holds: MH_ERR_ARG (a store that is not editable, a model index out
 * of range, MH_DB_REMOVE, a null image, a spec with form outside 0 / 1, a non-finite scale, z or K, fx or fy = 0 in
 * form 1 or with undistortion on, a NaN in roi, max_rows < 0) comes before anything is launched; the edit is ordered on
 * the context's stream like mh_db_splice; flip, mh_db_adopt and mh_db_generation work as there.  ONE host wait is added:
 * the read-back of the kept count that sizes the splice.  *n_rows, bbox[6] (either may be NULL): rows of the new model
 * and its bounding box.  rows_desc_host [rows_cap][128], rows_xyz_host [rows_cap][3] (both or neither): the first
 * min(*n_rows, rows_cap) selected rows, descriptors as FEAT made them (what mh_models_add_rows takes).  No kept row: the
 * edit mh_db_splice makes of n_rows = 0 (an empty model).  More keypoints in the image than max_keypoints: the edit
 * is made from the first max_keypoints of the list and the call returns MH_ERR_CAPACITY, as mh_sift_extract does. */
int mh_db_splice_image(mh_ctx* ctx, int op, int model, const uint8_t* gray_dev, int width, int height, int double_size,
                       int max_keypoints, const mh_planar_spec* spec, int32_t* n_rows, float bbox[6],
                       float* rows_desc_host, float* rows_xyz_host, int rows_cap);
/* n_images <= MH_MAX_BATCH device images of one size -> models model_first .. model_first + n_images - 1 (INSERT, one
 * after the other, so image i becomes model model_first + i): FEAT as ONE batch, ONE selection launch, one read-back of
 * all counts, then the single-model splice n_images times.  Every model, and the store afterwards, are byte for byte
 * those of mh_db_splice_image called per image.  n_rows [n_images], bbox [n_images][6] (may be NULL); image i's host
 * rows at rows_desc_host + i rows_cap 128 / rows_xyz_host + i rows_cap 3.  Nothing is launched on MH_ERR_ARG; an error of
 * a later splice leaves the earlier models in. */
int mh_db_splice_images(mh_ctx* ctx, int model_first, const uint8_t* const* gray_dev, int n_images, int width, int height,
                        int double_size, int max_keypoints, const mh_planar_spec* spec, int32_t* n_rows, float (*bbox)[6],
                        float* rows_desc_host, float* rows_xyz_host, int rows_cap);

/* ---- 3-D models from Kinect views ------------------------------------------------------------------------------------
 * A Kinect host has the measured 3-D point of every pixel on the device: the [h][w][4] map (x, y, z, valid) every depth
 * entry point takes (DEPTHMAP_PROP_CPU.hpp:103-131), the depth camera at the origin as moped3d's node sets it
 * (moped3d.cpp:259-260,275-276).  A view = image + map + the object's pose in that view, pose = (qx,qy,qz,qw,tx,ty,tz)
 * as MOPED reports poses, X_cam = R X_model + t, q normalised.  Every keypoint whose pixel holds a measured point
 * becomes a model row at X_model = inverseTransform(pose, point) (moped.hpp:189-194).  The first view makes the model
 * (mh_db_splice_view), further views grow it (mh_db_append_view) and leave out the keypoints the model already holds:
 * MOPED's models carry one descriptor per 3-D point, and a point held twice fails the 2-NN ratio test against itself
 * (MATCH_ANN_CPU.hpp:165).
 *
 * Per keypoint (u, v) of the list, in list order; the FIRST failing test decides its counter:
 *  1 pixel     u, v finite and -1 < u < w, -1 < v < h in float32; ix = (int)u, iy = (int)v (truncation,
 *              DEPTHMAP_PROP_CPU.hpp:103: u = -0.5 reads pixel 0).  No clamping, unlike mh_depth_prop: a model point
 *              must be measured.
 *  2 depth     the pixel's 4th word >= 0 (:131; NaN fails)
 *  3 fill      with a distance map and max_fill_distance >= 0: dropped if dist > max_fill_distance or NaN
 *              (DEPTH_VERIFY_CPU.hpp:167-170)
 *  4 roi       u0 <= u < u1 && v0 <= v < v1, all zeros = none: mh_planar_spec's rule
 *  5 X_model   = R^T (point - t): one float32 rounding per operation in the reference's order, no fused multiply-add
 *  6 box       min xyz, max xyz in the model frame, kept if min <= X_model <= max componentwise; all zeros = none; a
 *              NaN coordinate is dropped when a box is set
 *  7 duplicate only with mh_view_dup, merge_ratio > 0 and merge_dist >= 0: dropped if MATCH accepts the keypoint at
 *              merge_ratio (d1 / d2 < merge_ratio, the test of mh_normalize_match), its nearest row belongs to `model`,
 *              and dx dx + dy dy + dz dz <= merge_dist merge_dist against that row's xyz (float32, left to right)
 *  8 limit     only the first max_rows kept keypoints (0 = no limit), never more than the output holds
 * Kept rows come out densely packed in list order, descriptors unchanged, xyz = X_model.
 * stats[8]: [0] keypoints seen, [1..7] dropped by tests 1, 2, 3, 4, 6, 7, 8; kept + sum stats[1..7] == stats[0]. */
typedef struct {
  float roi[4];
  float box[6];
  float max_fill_distance;   /* < 0: no fill test */
  int32_t max_rows;
  float merge_ratio;         /* duplicate test (mh_db_append_view, mh_view_dup): on if merge_ratio > 0 && merge_dist >= 0 */
  float merge_dist;
} mh_view_spec;
typedef struct {
  const void* depth_xyzn_dev;       /* device [h][w][4] floats, 16-byte aligned */
  const float* fill_distance_dev;   /* device [h][w], or NULL */
  float pose[7];
  float K[4];   /* fx, fy, cx, cy of the gray image: read only while mh_frame_set_undistort is on (fx, fy != 0 then) */
} mh_view;
/* The duplicate test's inputs and the old rows of an append (all device): MATCH's result for the list against a store
 * (view i of a batch at + i cap), that store's model_of [n_db_rows] and xyz [n_db_rows][3] (local rows, index_base 0),
 * the model being grown and its rows [row_begin, row_end), whose xyz are folded into the bounding box so that it is
 * the box of the whole model after the edit.  Duplicates are judged against these rows, never against the call's own. */
typedef struct {
  const int32_t* idx_dev;
  const float* d1_dev;
  const float* d2_dev;
  const int32_t* model_of_dev;
  const float* xyz_dev;
  int32_t n_db_rows;
  int32_t model;
  int32_t row_begin, row_end;
} mh_view_dup;
/* The selection alone on given device arrays, like mh_planar_rows_dev: desc_dev [cap][128], xy_dev [cap][2], *n_dev
 * keypoints (clamped to [0, cap]); the view's map is w x h.  dup may be NULL (no duplicate test, no old rows).  Writes
 * desc_out_dev [out_cap][128], xyz_out_dev [out_cap][3], *n_out_dev, bbox_dev[6] (Model::boundingBox with the planar
 * kernel's `<` / `>` rule) and stats_dev[8].  Rows at and beyond *n_out_dev are not written.  Stream-ordered, no host
 * wait.  MH_ERR_ARG before anything is launched: a non-finite pose or box, NaN in roi, max_fill_distance, merge_ratio or
 * merge_dist, max_rows < 0, a null map or one not 16-byte aligned, w or h <= 0, descriptor arrays not 16-byte aligned, a
 * dup with a null array or rows outside [0, n_db_rows]. */
int mh_view_rows_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int cap,
                     const mh_view* view, int width, int height, const mh_view_spec* spec, const mh_view_dup* dup,
                     float* desc_out_dev, float* xyz_out_dev, int out_cap, int32_t* n_out_dev, float* bbox_dev,
                     int32_t* stats_dev);
/* n_views <= MH_MAX_BATCH lists in ONE launch, one map and pose each (lists and outputs laid out as in
 * mh_planar_rows_batch_dev; stats_dev + 8 i); every view's outputs are bit for bit those of the single call. */
int mh_view_rows_batch_dev(mh_ctx* ctx, const float* desc_dev, const float* xy_dev, const int32_t* n_dev, int n_views,
                           int cap, const mh_view* views, int width, int height, const mh_view_spec* spec,
                           const mh_view_dup* dup, float* desc_out_dev, float* xyz_out_dev, int out_cap,
                           int32_t* n_out_dev, float* bbox_dev, int32_t* stats_dev);
/* Rows added behind the last row of an existing model: the splice old[0, e) ++ rows ++ old[e, N) with e = the model's
 * end.  The model keeps its index, later models move up.  Arguments and every guarantee as mh_db_splice (which keeps
 * refusing an operation beyond MH_DB_REMOVE): afterwards the store equals, byte for byte, a fresh mh_db_upload_raw of
 * the same rows. */
int mh_db_append(mh_ctx* ctx, int model, const float* desc, const float* xyz, int n_rows, int normalize, int on_device);
/* A view becomes model `model` (op = MH_DB_INSERT or MH_DB_REPLACE): [UNDISTORTED_IMAGE of the gray image with view->K if
 * mh_frame_set_undistort is on; the map is read as it lies, as the Kinect frames do] -> FEAT -> selection into the
 * edit's staging block -> splice.  In every other respect the contract of mh_db_splice_image: one added host wait,
 * MH_ERR_CAPACITY with the edit made from the first max_keypoints, host rows with FEAT's bits.  stats[8] (may be NULL)
 * as above.  merge_ratio / merge_dist are not used (there is no model to compare with). */
int mh_db_splice_view(mh_ctx* ctx, int op, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                      int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows, float bbox[6],
                      int32_t stats[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap);
/* A further view of model `model`: its kept rows are appended (mh_db_append).  With the duplicate test on (merge_ratio > 0
 * && merge_dist >= 0, and a store that has rows) FEAT's descriptors are normalised into a scratch copy and matched
 * against the context's store with the count on the device, as a frame's are; the selection then drops the keypoints
 * the model already holds.  Still one host wait before the splice.  With the test off no MATCH is launched.  *n_rows:
 * rows added; bbox: the whole model's box after the edit. */
int mh_db_append_view(mh_ctx* ctx, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                      int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows, float bbox[6],
                      int32_t stats[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap);
/* ---- re-seen points: merged, counted, pruned ----
 * mh_db_append_view drops a keypoint the model already holds.  mh_db_merge_view folds it into the row it re-observes
 * instead, as MOPED's model builder gives every model point one descriptor from all its observations and writes their
 * number (moped-modeling-py MopedModeling.py:863-894, :915) -- with the plain mean where the builder runs a mean shift
 * over dozens of observations: a model taught on the device sees a handful of views.
 *
 * The model's rows before the call are [row_begin, row_end) of the store.  For an old row r: d_r its descriptor as the
 * store holds it (normalised), p_r its point, c_r >= 1 its view count (no array: 1).  The observations of r are the
 * keypoints rule 7 drops whose nearest row is r, in list order i_1 < .. < i_k; q_i the keypoint's descriptor as MATCH saw
 * it (the normalised scratch copy), X_i its X_model.  float32, one rounding per operation, no fused multiply-add:
 *   a = q_i1; a = a + q_ij (j = 2 .. k); if k > 1: a = a / (float)k;   s  = d_r * (float)c_r + a
 *   b = X_i1; b = b + X_ij (j = 2 .. k); if k > 1: b = b / (float)k;   p' = (p_r * (float)c_r + b) / (float)(c_r + 1)
 * The new row is A1's normalisation of s by the code every upload uses, its point p', its count c_r + 1: a count of
 * views, not of keypoints.  Rows without an observation keep their bits and their count.  Duplicates are judged against
 * the rows present before the call; the merge does not feed back into the call's verdicts.
 *
 * The merge alone on given device arrays, like mh_view_rows_dev (same lists, view, spec and dup -- which is required):
 * qn_desc_dev [cap][128] the normalised copy MATCH searched, old_desc_dev the store's [n_db_rows][128], views_in_dev
 * [row_end - row_begin] or NULL.  Writes merged_idx_dev (relative to row_begin, ascending), merged_desc_dev = s (NOT
 * normalised), merged_xyz_dev = p', at most merged_cap rows of each; *n_merged_dev = the full count even beyond
 * merged_cap; views_out_dev [row_end - row_begin].  With the duplicate test off nothing merges.  Stream-ordered, no host
 * wait.  No floating-point atomics: one wavefront sums a row's observations in list order, so the result depends neither
 * on the grid nor on the order workgroups run in.  MH_ERR_ARG before anything is launched: whatever mh_view_rows_dev
 * refuses, a null dup, old_desc_dev null or not 16-byte aligned, a null output, merged_cap < 0. */
int mh_view_merge_dev(mh_ctx* ctx, const float* desc_dev, const float* qn_desc_dev, const float* xy_dev, const int32_t* n_dev,
                      int cap, const mh_view* view, int width, int height, const mh_view_spec* spec, const mh_view_dup* dup,
                      const float* old_desc_dev, const int32_t* views_in_dev, int32_t* merged_idx_dev, float* merged_desc_dev,
                      float* merged_xyz_dev, int merged_cap, int32_t* n_merged_dev, int32_t* views_out_dev);
/* A further view of model `model`, merged: mh_db_append_view's path ([UNDISTORTED_IMAGE] -> FEAT -> normalised copy ->
 * MATCH -> selection) + the merge, into the edit's staging block, ONE host wait, one splice.  views_in_host [n_views_in]
 * = the model's counts (n_views_in = its row count), or NULL / 0 = all ones; a count < 1 is refused.  *n_added new rows
 * (byte for byte mh_db_append_view's, count 1), *n_merged rows merged; stats as mh_db_append_view; bbox over the model's
 * final points.  rows_*_host: the new rows with FEAT's bits; merged_*_host (all three or none, at most merged_cap rows):
 * the merged rows' index in the model, s and p'; views_out_host: the counts of the model's rows after the edit --
 * views_out_cap >= rows before + min(max_keypoints, max_rows if > 0), what the view can add at most, else MH_ERR_ARG
 * with nothing launched.
 * Guarantee: a caller who keeps a host mirror of raw rows, overwrites mirror rows merged_idx with merged_desc /
 * merged_xyz and appends the new rows holds a mirror whose fresh mh_db_upload_raw(normalize = 1) equals the store byte
 * for byte.  Untouched rows are not normalised again.  With the duplicate test off (merge_ratio <= 0 or merge_dist < 0)
 * or a store without rows the call is mh_db_append_view: n_merged = 0, the old counts followed by ones, no MATCH.
 * MH_ERR_CAPACITY as mh_db_append_view; a sharded store is refused, like every edit. */
int mh_db_merge_view(mh_ctx* ctx, int model, const uint8_t* gray_dev, const mh_view* view, int width, int height,
                     int double_size, int max_keypoints, const mh_view_spec* spec, const int32_t* views_in_host, int n_views_in,
                     int32_t* n_added, int32_t* n_merged, float bbox[6], int32_t stats[8], float* rows_desc_host,
                     float* rows_xyz_host, int rows_cap, int32_t* merged_idx_host, float* merged_desc_host,
                     float* merged_xyz_host, int merged_cap, int32_t* views_out_host, int views_out_cap);
/* Model `model` keeps the rows whose flag is set (n_flags = its row count), in order: a stable compaction of the store's
 * own rows (descriptor, norm term, point) on the device, then a REPLACE splice; nothing is normalised again, so the
 * store equals a fresh mh_db_upload_raw(normalize = 1) of the mirror's kept rows.  No flag set: the empty model that
 * mh_db_splice makes of n_rows = 0.  *n_rows: rows kept; bbox: their box. */
int mh_db_keep_rows(mh_ctx* ctx, int model, const uint8_t* keep_host, int n_flags, int32_t* n_rows, float bbox[6]);
/* n_views <= MH_MAX_BATCH views of one size -> models model_first .. model_first + n_views - 1 (INSERT): FEAT as ONE batch,
 * ONE selection launch, one read-back, then the single-model splice n_views times; byte for byte what mh_db_splice_view
 * gives per view.  n_rows [n_views], bbox [n_views][6], stats [n_views][8] (may be NULL); host rows as
 * mh_db_splice_images.  Duplicates among the views of one call are not looked for. */
int mh_db_splice_views(mh_ctx* ctx, int model_first, const uint8_t* const* gray_dev, const mh_view* views, int n_views,
                       int width, int height, int double_size, int max_keypoints, const mh_view_spec* spec, int32_t* n_rows,
                       float (*bbox)[6], int32_t (*stats)[8], float* rows_desc_host, float* rows_xyz_host, int rows_cap);

/* ---- timing --------------------------------------------------------------------- */

/* Device-side counters of the last frame that ran on the context (synchronises its stream):
 * out[0] accepted matches, [1] clusters, [2..4] reserved, [5] (cluster, replica) tasks of POSE + POSE2 that
 * evaluated hypotheses, [6] capacity flags, [7] P3P hypotheses those tasks evaluated -- POSE stops after the
 * first 256 of a task's n_hypotheses when the inlier ratio they reached makes a better all-inlier sample
 * unlikely; n_hypotheses < 0 in mh_pose_params means "-n_hypotheses, all of them". */
int mh_frame_counters(mh_ctx* ctx, int32_t out[8]);
/* Resource use of the RANSAC kernel behind mh_pose_ransac* and the frame's POSE / POSE2 launches, as the HIP runtime
 * reports it for this device (occupancy of the RANSAC kernel next to every GPU figure; the reference's
 * step is POSE_RANSAC_LM_DIFF_REPROJECTION_CPU::process, src/pose/POSE_RANSAC_LM_DIFF_REPROJECTION_CPU.hpp:264-307):
 * kind = MH_DEPTH_* (3 = frames with several images); out[0] VGPRs per lane, [1] LDS bytes per workgroup, [2] threads
 * per workgroup, [3] workgroups resident per compute unit, [4] scratch bytes per lane (spills), [5] wavefronts per
 * workgroup. */
int mh_pose_kernel_info(mh_ctx* ctx, int kind, int32_t out[8]);
/* GPU time of the kernels of the two-stage MATCH on this context, after mh_enable_timing(ctx, 1): the mean over
 * the launch sequences since the previous call (at most the last 32; synchronises the context's stream):
 * ms[0] query image (f16), [1] pass A (thresholds from a sample of the rows), [2] threshold merge,
 * [3] pass B (the f16 screen of every (query, row) pair: the dominant kernel), [4] pass C (canonical
 * f32 arithmetic on the candidates).  MH_ERR_ARG if no two-stage MATCH has run with timing on. */
int mh_match_timing(mh_ctx* ctx, float ms[5]);

typedef struct {
  float match_ms, group_ms, cluster_ms, pose1_ms, filter1_ms, pose2_ms, filter2_ms, total_ms;
} mh_times;
/* GPU time of each stage of the last frame (hipEvents on the context's stream;
 * collected only after mh_enable_timing(ctx, 1)). */
int mh_enable_timing(mh_ctx* ctx, int on);
int mh_timing(mh_ctx* ctx, mh_times* out);

#ifdef __cplusplus
}
#endif
#endif /* MOPED_HIP_H */
