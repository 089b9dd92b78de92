"""ctypes binding of libmoped_hip.so (include/moped_hip.h).

This is plumbing for tests/ and bench.py: it adds no computation of its own.
There is no CPU fallback -- if the HIP library is missing or no gfx950 device is
present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MH_LIB_PATH") or os.path.join(_HERE, "libmoped_hip.so")  # override: A/B kernel builds

MH_OK = 0
MH_ERR_ARG = -1
MH_ERR_CAPACITY = -3


class MhError(RuntimeError):
    pass


class mh_corr(C.Structure):
    _fields_ = [("u", C.c_float), ("v", C.c_float), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class mh_cam(C.Structure):
    _fields_ = [("K", C.c_float * 4), ("cam", C.c_float * 7)]


class mh_pose_params(C.Structure):
    _fields_ = [("n_hypotheses", C.c_int), ("max_objects_per_cluster", C.c_int),
                ("n_pts_align", C.c_int), ("min_n_pts_object", C.c_int),
                ("error_threshold", C.c_float), ("lm_iters_l2", C.c_int), ("lm_iters_l4", C.c_int)]


class mh_pose_out(C.Structure):
    _fields_ = [("pose", C.c_float * 7), ("cluster", C.c_int32), ("n_inliers", C.c_int32),
                ("err", C.c_float)]


class mh_frame_params(C.Structure):
    _fields_ = [("ratio", C.c_float), ("ms_radius", C.c_float), ("ms_merge", C.c_float),
                ("ms_min_pts", C.c_int), ("ms_max_iter", C.c_int), ("pose1", mh_pose_params),
                ("f1_min_points", C.c_int), ("f1_feature_distance", C.c_float),
                ("f1_min_score", C.c_float), ("pose2", mh_pose_params),
                ("f2_min_points", C.c_int), ("f2_feature_distance", C.c_float),
                ("f2_min_score", C.c_float), ("run_stage2", C.c_int)]


class mh_object(C.Structure):
    _fields_ = [("model", C.c_int32), ("pose", C.c_float * 7), ("score", C.c_float),
                ("n_points", C.c_int32)]


class mh_times(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("match_ms", "group_ms", "cluster_ms", "pose1_ms",
                                         "filter1_ms", "pose2_ms", "filter2_ms", "total_ms")]


CORR_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
OBJECT_DTYPE = np.dtype([("model", "<i4"), ("pose", "<f4", (7,)), ("score", "<f4"), ("n_points", "<i4")])
STEP_OBJECT_DTYPE = np.dtype([("model", "<i4"), ("pose", "<f4", (7,))])   # mh_step_object
DEPTH_DTYPE = np.dtype([("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4"), ("w", "<f4")])
DEPTH_BACKPROJECTION, DEPTH_REPROJECTION = 1, 2
DEPTH_FILL_REPLAY, DEPTH_FILL_LEVELS = 0, 1   # mh_depth_fill_set_mode
LINKAGE_SCAN, LINKAGE_ROWMAX = 0, 1   # mh_linkage_set_mode
LINKAGE_MAX_POINTS = 4096   # points per problem in LINKAGE_ROWMAX (LINKAGE_SCAN: 1024)
DEPTH_INFO_DTYPE = np.dtype([("depth_valid", "<i4"), ("coord3d", "<f4", (3,)), ("depth", "<f4"),
                             ("fill_distance", "<f4")])   # mh_depth_info
POSE_OUT_DTYPE = np.dtype([("pose", "<f4", (7,)), ("cluster", "<i4"), ("n_inliers", "<i4"), ("err", "<f4")])
SIFT_CANDIDATE_DTYPE = np.dtype([("octave", "<i4"), ("index", "<i4"), ("key", "<u4"), ("r", "<i4"), ("c", "<i4"),
                                 ("x0", "<f4"), ("x1", "<f4"), ("x2", "<f4")])                      # mh_sift_candidate
SIFT_KEY_DTYPE = np.dtype([("octave", "<i4"), ("index", "<i4"), ("order", "<u8"), ("fsize", "<f4"), ("frow", "<f4"),
                           ("fcol", "<f4"), ("ori", "<f4")])                                        # mh_sift_key
SIFT_MAX_OCTAVES = 8     # MH_SIFT_MAX_OCTAVES

# every symbol include/moped_hip.h declares
MAX_BATCH = 32   # MH_MAX_BATCH


class mh_linkage_params(C.Structure):
    _fields_ = [("cutoff", C.c_float), ("min_pts", C.c_int32), ("use3d_filter", C.c_int32), ("sigma2d", C.c_float),
                ("sigma3d", C.c_float), ("linkage_type", C.c_int32)]

    def __init__(self, cutoff=0.1, min_pts=7, use3d_filter=2, sigma2d=-1.0, sigma3d=-1.0, linkage_type=1):
        # (average linkage unless said otherwise: a positional call with the five older fields must not mean "minimum")
        super().__init__(cutoff, min_pts, use3d_filter, sigma2d, sigma3d, linkage_type)


def default_linkage_params():
    """CLUSTER_LINKAGE_CPU( 0.1, 7, 2, 1, 0.0, 1, -1, -1 ) (moped3d/libmoped/src/config.hpp:45)."""
    return mh_linkage_params(0.1, 7, 2, -1.0, -1.0, 1)


class mh_wms_params(C.Structure):
    """CLUSTER_WEIGHTED_MEAN_SHIFT_CPU's constructor arguments (Radius, Merge, MinPts, MaxIterations, halfWeightDistance)."""
    _fields_ = [("radius", C.c_float), ("merge", C.c_float), ("min_pts", C.c_int32), ("max_iter", C.c_int32),
                ("half_weight_distance", C.c_float)]

    def __init__(self, radius=0.1, merge=0.02, min_pts=7, max_iter=100, half_weight_distance=10.0):
        super().__init__(radius, merge, min_pts, max_iter, half_weight_distance)


WMS_MAX_POINTS = 2048   # points per weighted mean-shift problem
WMS_MEMBER_FACTOR = 4   # MH_WMS_MEMBER_FACTOR: a model's clusters in a frame hold up to this many times its matches


class mh_depth_rules(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("feature_density", C.c_float), ("match_density", C.c_float),
                ("ratio_table", C.c_void_p), ("n_models", C.c_int32), ("maximum_depth", C.c_float),
                ("default_depth", C.c_float), ("cauchy_scale", C.c_float)]


class mh_filter_depth_params(C.Structure):
    """FILTER_PROJECTION_DEPTH_CPU's own constructor arguments (PlausibleSqDistance, DepthFraction, MinKeypointFraction)."""
    _fields_ = [("plausible_sq_distance", C.c_float), ("depth_fraction", C.c_float), ("min_keypoint_fraction", C.c_float)]


class mh_depth_verify_params(C.Structure):
    """DEPTH_VERIFY_CPU's constructor arguments (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction)."""
    _fields_ = [("feature_distance", C.c_float), ("max_multiplier", C.c_float), ("max_distance", C.c_float),
                ("depth_fraction", C.c_float)]


# mh_verify_record: one object's numbers as DEPTH_VERIFY_CPU prints them, and the verdict
VERIFY_DTYPE = np.dtype([("qs_raw", "<f4"), ("is_raw", "<f4"), ("multiplier", "<f4"), ("qs", "<f4"), ("is", "<f4"),
                         ("plausible", "<i4"), ("used", "<i4"), ("keypoints", "<i4"), ("keep", "<i4")])
DEPTH_VERIFY_CHUNK = 192   # MH_DEPTH_VERIFY_CHUNK


class mh_planar_spec(C.Structure):
    _fields_ = [("form", C.c_int32), ("scale", C.c_float), ("K", C.c_float * 4), ("z", C.c_float), ("roi", C.c_float * 4),
                ("max_rows", C.c_int32)]


def make_planar_spec(scale=None, z=None, K=None, roi=None, max_rows=0) -> mh_planar_spec:
    """Exactly one of `scale` (form 0: x = u scale, y = v scale, z = 0 -- moped.cpp:225) and `z` (form 1: the plane at
    depth z in front of the camera K = fx, fy, cx, cy).  roi = (u0, v0, u1, v1), half-open; None = every keypoint."""
    if (scale is None) == (z is None):
        raise ValueError("exactly one of scale and z")
    sp = mh_planar_spec()
    sp.form = 0 if z is None else 1
    sp.scale = 1.0 if scale is None else float(scale)
    sp.z = 0.0 if z is None else float(z)
    sp.K[:] = [float(v) for v in (K if K is not None else (1.0, 1.0, 0.0, 0.0))]
    sp.roi[:] = [float(v) for v in (roi if roi is not None else (0.0, 0.0, 0.0, 0.0))]
    sp.max_rows = int(max_rows)
    return sp


class mh_view_spec(C.Structure):
    _fields_ = [("roi", C.c_float * 4), ("box", C.c_float * 6), ("max_fill_distance", C.c_float), ("max_rows", C.c_int32),
                ("merge_ratio", C.c_float), ("merge_dist", C.c_float)]


class mh_view(C.Structure):
    _fields_ = [("depth_xyzn_dev", C.c_void_p), ("fill_distance_dev", C.c_void_p), ("pose", C.c_float * 7), ("K", C.c_float * 4)]


class mh_view_dup(C.Structure):
    _fields_ = [("idx_dev", C.c_void_p), ("d1_dev", C.c_void_p), ("d2_dev", C.c_void_p), ("model_of_dev", C.c_void_p),
                ("xyz_dev", C.c_void_p), ("n_db_rows", C.c_int32), ("model", C.c_int32), ("row_begin", C.c_int32),
                ("row_end", C.c_int32)]


POSE_IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def make_view_spec(roi=None, box=None, max_fill_distance=-1.0, max_rows=0, merge_ratio=0.0, merge_dist=-1.0) -> mh_view_spec:
    """The rules of a Kinect view's selection (mh_view_spec): roi = (u0, v0, u1, v1), half-open, None = every keypoint;
    box = (min xyz, max xyz) in the model frame, None = none; max_fill_distance < 0 = no fill test; the duplicate test of
    an appended view is on when merge_ratio > 0 and merge_dist >= 0."""
    sp = mh_view_spec()
    sp.roi[:] = [float(v) for v in (roi if roi is not None else (0.0,) * 4)]
    sp.box[:] = [float(v) for v in (box if box is not None else (0.0,) * 6)]
    sp.max_fill_distance = float(max_fill_distance)
    sp.max_rows = int(max_rows)
    sp.merge_ratio = float(merge_ratio)
    sp.merge_dist = float(merge_dist)
    return sp


def make_view(depth_ptr, fill_ptr=None, pose=None, K=None) -> mh_view:
    """A view: the device depth map [h][w][4], optionally its distance map [h][w], the object's pose in the view
    (qx, qy, qz, qw, tx, ty, tz: X_cam = R X_model + t; None = identity), K of the gray image (read only while
    undistortion is on)."""
    v = mh_view()
    v.depth_xyzn_dev = depth_ptr
    v.fill_distance_dev = fill_ptr
    v.pose[:] = [float(x) for x in (pose if pose is not None else POSE_IDENTITY)]
    v.K[:] = [float(x) for x in (K if K is not None else (1.0, 1.0, 0.0, 0.0))]
    return v


RAW_DEPTH_F32_M, RAW_DEPTH_U16_MM = 0, 1   # MH_RAW_DEPTH_*


class mh_raw_depth(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("elem_stride", C.c_int32),
                ("row_stride", C.c_int32), ("offset", C.c_int32)]


def make_raw_depth(fmt, width, height, elem_stride=None, row_stride=None, offset=0) -> mh_raw_depth:
    """What a sensor's depth buffer looks like: RAW_DEPTH_F32_M (float metres, NaN = no reading) or RAW_DEPTH_U16_MM
    (uint16 millimetres, 0 = no reading), width x height readings at offset + y row_stride + x elem_stride bytes.
    Defaults: a plain image.  A PointCloud2: elem_stride = point_step, row_stride = row_step, offset = z's offset."""
    es = 4 if fmt == RAW_DEPTH_F32_M else 2
    elem_stride = es if elem_stride is None else elem_stride
    row_stride = width * elem_stride if row_stride is None else row_stride
    return mh_raw_depth(int(fmt), int(width), int(height), int(elem_stride), int(row_stride), int(offset))


# MH_IMAGE_*: what a camera delivers, under the names of ROS's sensor_msgs/image_encodings.h
(IMAGE_GRAY8, IMAGE_BGR8, IMAGE_RGB8, IMAGE_BGRA8, IMAGE_RGBA8, IMAGE_BAYER_RGGB8, IMAGE_BAYER_BGGR8, IMAGE_BAYER_GBRG8,
 IMAGE_BAYER_GRBG8) = range(9)
IMAGE_BPP = {IMAGE_GRAY8: 1, IMAGE_BGR8: 3, IMAGE_RGB8: 3, IMAGE_BGRA8: 4, IMAGE_RGBA8: 4, IMAGE_BAYER_RGGB8: 1,
             IMAGE_BAYER_BGGR8: 1, IMAGE_BAYER_GBRG8: 1, IMAGE_BAYER_GRBG8: 1}


class mh_raw_image(C.Structure):
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("row_stride", C.c_int32),
                ("offset", C.c_int32)]


def make_raw_image(format, w, h, row_stride=None, offset=0) -> mh_raw_image:
    """What a camera's image buffer looks like: an IMAGE_* format, w x h pixels at offset + y row_stride + x
    bytes-per-pixel.  Default: packed rows.  (An unknown format keeps whatever row_stride it is given: the library
    refuses it.)"""
    if row_stride is None:
        row_stride = w * IMAGE_BPP.get(format, 1)
    return mh_raw_image(int(format), int(w), int(h), int(row_stride), int(offset))


def raw_image_bytes(fmt: mh_raw_image) -> int:
    """The bytes of the buffer a description speaks of: offset + (height - 1) row_stride + width bytes-per-pixel."""
    return fmt.offset + (fmt.height - 1) * fmt.row_stride + fmt.width * IMAGE_BPP.get(fmt.format, 1)


def make_filter_depth_params(p):
    """None, an mh_filter_depth_params or (plausible_sq_distance, depth_fraction, min_keypoint_fraction)."""
    if p is None or isinstance(p, mh_filter_depth_params):
        return p
    a, b, c = p
    return mh_filter_depth_params(float(a), float(b), float(c))


def make_depth_verify_params(p):
    """None, an mh_depth_verify_params or (feature_distance, max_multiplier, max_distance, depth_fraction)."""
    if p is None or isinstance(p, mh_depth_verify_params):
        return p
    a, b, c, d = p
    return mh_depth_verify_params(float(a), float(b), float(c), float(d))


EXPORTS = [
    "mh_create", "mh_destroy", "mh_last_error", "mh_set_stream", "mh_synchronize", "mh_reserve",
    "mh_db_upload", "mh_db_size", "mh_normalize", "mh_match", "mh_normalize_match", "mh_match_local_dev", "mh_match_local_counted_dev",
    "mh_match_merge_dev", "mh_normalize_dev", "mh_meanshift", "mh_meanshift_batch", "mh_pose_ransac", "mh_pose_ransac_depth",
    "mh_frame_set_depth", "mh_project_test",
    "mh_filter", "mh_frame_default_params", "mh_frame_enqueue", "mh_frame_set_depth_image", "mh_frame_enqueue_match_local",
    "mh_frame_enqueue_rest", "mh_frame_fetch", "mh_frame_result_dev", "mh_enable_timing", "mh_timing",
    "mh_frame_set_cluster_linkage", "mh_cluster_linkage", "mh_frame_set_depth_image_host",
    "mh_depth_fill", "mh_depth_fill_status", "mh_depth_fill_host", "mh_depth_fill_batch", "mh_depth_fill_set_mode", "mh_depth_fill_get_mode", "mh_depth_fill_stats",
    "mh_frame_enqueue_rest_batch", "mh_frame_enqueue_rest_frames", "mh_frame_fetch_slot", "mh_frame_result_copy_slots_dev",
    "mh_frame_set_depth_rules", "mh_frame_fetch_matches", "mh_frame_enqueue_rest_strided", "mh_frame_result_copy_dev",
    "mh_sift_extract", "mh_sift_extract_dev", "mh_frame_enqueue_image", "mh_frame_enqueue_image_batch", "mh_frame_features_dev", "mh_frame_keypoints",
    "mh_models_create", "mh_models_destroy", "mh_models_last_error", "mh_models_add_xml",
    "mh_models_add_xml_buffer", "mh_models_count", "mh_models_rows", "mh_models_name", "mh_models_range",
    "mh_models_desc", "mh_models_xyz", "mh_models_save", "mh_models_load", "mh_db_upload_models",
    "mh_db_splice", "mh_db_reserve", "mh_db_adopt", "mh_db_generation", "mh_db_model_rows", "mh_db_splice_models",
    "mh_db_debug_fetch", "mh_depth_rules_debug_fetch", "mh_db_debug_screen", "mh_db_debug_route", "mh_db_edit_ms",
    "mh_db_upload_raw", "mh_db_share", "mh_match_stats", "mh_match_set_mode", "mh_match_launches", "mh_pose_set_split", "mh_frame_fetch_match_points", "mh_screen_margin", "mh_frame_counters", "mh_match_timing", "mh_frame_set_images", "mh_filter_images",
    "mh_pose_ransac_images",
    "mh_comm_unique_id", "mh_comm_create", "mh_comm_create_all", "mh_comm_create_host", "mh_comm_destroy", "mh_comm_info",
    "mh_frame_enqueue_sharded", "mh_frame_enqueue_sharded_batch", "mh_frame_enqueue_sharded_all",
    "mh_frame_previous_objects", "mh_frame_gather_objects", "mh_frame_enqueue_batch", "mh_frame_set_depth_image_batch",
    "mh_pose_kernel_info", "mh_db_upload_blocks", "mh_frame_fetch_matches_slot", "mh_frame_fetch_match_reps_slot",
    "mh_screen_values", "mh_screen_record_value", "mh_screen_record_bounds", "mh_reserve_batch", "mh_frame_run_host",
    "mh_frame_block_stride", "mh_frame_fetch_batch_async", "mh_frame_fetch_previous_async", "mh_frame_fetch_wait",
    "mh_frame_fetch_query", "mh_host_alloc", "mh_host_free", "mh_frame_run_host_begin", "mh_frame_wait_descriptors",
    "mh_step_match", "mh_step_match_fetch", "mh_step_cluster", "mh_step_pose", "mh_step_filter",
    "mh_set_linkage_scratch_limit",
    "mh_undistort_map", "mh_undistort", "mh_undistort_dev", "mh_frame_set_undistort",
    "mh_sift_extract_batch_dev", "mh_sift_debug_plan", "mh_sift_debug_level", "mh_sift_debug_candidates",
    "mh_sift_debug_keys", "mh_sift_debug_describe", "mh_sift_debug_blur",
    "mh_screen_pack_value", "mh_screen_pack_pert", "mh_screen_sample_bounds", "mh_screen_launch_plan", "mh_screen_plan", "mh_match_incomplete",
    "mh_screen_sample_values", "mh_match_query_candidates", "mh_screen_park_places",
    "mh_frame_enqueue_images", "mh_frame_enqueue_images_batch", "mh_frame_set_undistort_images", "mh_frame_image_counts",
    "mh_frame_features_image_dev",
    "mh_filter_depth_set_points", "mh_filter_depth", "mh_frame_set_filter_depth",
    "mh_frame_route", "mh_filter_depth_debug_form",
    "mh_depth_filter", "mh_depth_prop", "mh_frame_run_kinect_host",
    "mh_linkage_debug_matrix", "mh_linkage_debug_agglomerate", "mh_linkage_set_mode", "mh_linkage_get_mode", "mh_linkage_stats", "mh_frame_debug_fetch_clusters_slot",
    "mh_planar_rows_dev", "mh_planar_rows_batch_dev", "mh_db_splice_image", "mh_db_splice_images",
    "mh_models_add_rows", "mh_models_write_xml",
    "mh_view_rows_dev", "mh_view_rows_batch_dev", "mh_db_append", "mh_db_splice_view", "mh_db_append_view", "mh_db_splice_views",
    "mh_view_merge_dev", "mh_db_merge_view", "mh_db_keep_rows",
    "mh_depth_map_from_raw_dev", "mh_depth_map_from_raw_batch_dev", "mh_depth_map_from_raw_host",
    "mh_frame_run_kinect_raw_host",
    "mh_frame_debug_fetch_cluster_table_slot",
    "mh_object_hulls", "mh_hull_debug_form",
    "mh_frame_set_hulls", "mh_frame_fetch_hulls_slot", "mh_frame_fetch_hulls", "mh_frame_hull_block_stride",
    "mh_frame_fetch_batch_hulls_async",
    "mh_screen_reject_proved", "mh_match_set_accept", "mh_match_prerejected",
    "mh_image_gray_dev", "mh_image_gray_batch_dev", "mh_image_gray_host", "mh_frame_set_image_format",
    "mh_cluster_wms", "mh_wms_debug_state", "mh_frame_set_cluster_wms",
    "mh_pose_debug_rows", "mh_pose_debug_step",
    "mh_depth_verify", "mh_depth_verify_debug_form",
    "mh_frame_set_depth_verify", "mh_frame_fetch_verify_slot", "mh_frame_fetch_verify",
]
POSE_DEBUG_FILL = 0xFFC0DE00   # MH_POSE_DEBUG_FILL
POSE_MAX_PTS = 2048            # MH_POSE_MAX_PTS
POSE_POINT_STRIDE = {0: 5, 1: 9, 2: 9, 3: 6}   # words of one point in mh_pose_debug_rows' pts, by kind
COMM_ID_BYTES = 128      # MH_COMM_ID_BYTES
EX2_OBJECTS = 62         # MH_EX2_OBJECTS
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)   # mh_allgather_fn

DIM = 128   # MH_DESC_DIM
HULL_LDS_POINTS = 8192   # MH_HULL_LDS_POINTS
DB_INSERT, DB_REPLACE, DB_REMOVE = 0, 1, 2   # MH_DB_*
_lib = None


def load():
    """dlopen the HIP library and declare prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # When PyTorch-ROCm shares the process (bench.py, multi-GPU tests) its bundled
    # HIP/HSA runtime must be the one in the process: two HSA runtimes cannot both
    # own the GPU.  Importing torch first makes libmoped_hip.so bind to that copy
    # (same SONAME libamdhip64.so.7); without torch the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch absent: plain ROCm runtime
        pass
    if not os.path.exists(LIB_PATH):
        raise MhError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.mh_create.argtypes = [i32, C.POINTER(vp)]
    L.mh_destroy.argtypes = [vp]
    L.mh_destroy.restype = None
    L.mh_last_error.argtypes = [vp]
    L.mh_last_error.restype = C.c_char_p
    L.mh_set_stream.argtypes = [vp, vp]
    L.mh_synchronize.argtypes = [vp]
    L.mh_reserve.argtypes = [vp, i32, i32, i32]
    L.mh_reserve_batch.argtypes = [vp, i32, i32, i32, i32]
    if hasattr(L, "mh_lane_create"):   # experiment builds only (csrc/api.hip)
        L.mh_lane_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.mh_lane_destroy.argtypes = [vp]
        L.mh_set_lane.argtypes = [vp, vp]
    L.mh_db_upload.argtypes = [vp, vp, vp, vp, i32, i32, C.c_int32]
    L.mh_db_size.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.mh_normalize.argtypes = [vp, vp, i32]
    L.mh_match.argtypes = [vp, vp, i32, f32, vp, vp, vp, vp]
    L.mh_normalize_match.argtypes = [vp, vp, i32, f32, vp, vp, vp, vp]
    L.mh_match_local_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    if hasattr(L, "mh_match_local_counted_dev"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_match_local_counted_dev.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp]
    L.mh_match_merge_dev.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.mh_normalize_dev.argtypes = [vp, vp, vp, i32]
    L.mh_meanshift.argtypes = [vp, vp, i32, i32, f32, f32, i32, i32, vp, vp, C.POINTER(C.c_int32)]
    L.mh_meanshift_batch.argtypes = [vp, vp, vp, i32, i32, f32, f32, i32, i32, vp, vp, vp]
    L.mh_pose_ransac.argtypes = [vp, vp, vp, i32, C.POINTER(mh_cam), C.POINTER(mh_pose_params),
                                 C.c_uint64, vp, C.POINTER(C.c_int32)]
    L.mh_pose_ransac_depth.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_cam), C.POINTER(mh_pose_params), i32, f32,
                                       C.c_uint64, vp, C.POINTER(C.c_int32)]
    L.mh_frame_set_depth.argtypes = [vp, vp, i32, f32]
    L.mh_project_test.argtypes = [vp, vp, vp, i32, C.POINTER(mh_cam), f32, vp, vp, C.POINTER(C.c_int32)]
    L.mh_filter.argtypes = [vp, vp, vp, i32, vp, vp, i32, C.POINTER(mh_cam), i32, f32, f32,
                            vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
    L.mh_frame_default_params.argtypes = [C.POINTER(mh_frame_params)]
    L.mh_frame_default_params.restype = None
    L.mh_frame_enqueue.argtypes = [vp, vp, vp, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params), C.c_uint64]
    L.mh_frame_run_host.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_cam), i32, C.POINTER(mh_frame_params), C.c_uint64, i32,
                                    vp, i32, C.POINTER(C.c_int32), vp]
    L.mh_frame_run_host_begin.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_cam), i32, C.POINTER(mh_frame_params), C.c_uint64, i32]
    L.mh_sift_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_sift_extract_dev.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, vp]
    L.mh_sift_extract_batch_dev.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    L.mh_sift_debug_plan.argtypes = [vp, vp, vp, vp, vp]
    L.mh_sift_debug_level.argtypes = [vp, i32, i32, i32, i32, vp]
    L.mh_sift_debug_candidates.argtypes = [vp, i32, vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_sift_debug_keys.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_int32)]
    L.mh_sift_debug_describe.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp]
    L.mh_sift_debug_blur.argtypes = [vp, i32, vp, i32, i32, f32, i32, vp, vp, vp]
    L.mh_frame_enqueue_image.argtypes = [vp, vp, i32, i32, i32, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params),
                                         C.c_uint64]
    L.mh_frame_enqueue_image_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params), vp]
    L.mh_frame_set_depth_image_host.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32]
    L.mh_depth_fill.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.mh_depth_fill_status.argtypes = [vp]
    L.mh_depth_fill_set_mode.argtypes = [vp, i32]
    L.mh_depth_fill_get_mode.argtypes = [vp, vp]
    L.mh_depth_fill_stats.argtypes = [vp, i32, vp]
    # (EXPORTS lists it and build() insists on it; absent only in the parent's build that scripts/ab_lib.sh names through
    #  MH_LIB_PATH to measure it against this one)
    if hasattr(L, "mh_depth_fill_batch"):
        L.mh_depth_fill_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, i32, vp]
    L.mh_depth_fill_host.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.mh_frame_set_cluster_linkage.argtypes = [vp, C.POINTER(mh_linkage_params)]
    if hasattr(L, "mh_linkage_set_mode"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_linkage_set_mode.argtypes = [vp, i32]
        L.mh_linkage_get_mode.argtypes = [vp, vp]
        L.mh_linkage_stats.argtypes = [vp, vp, i32]
    L.mh_cluster_linkage.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_linkage_params), vp, vp, vp]
    if hasattr(L, "mh_linkage_debug_matrix"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_linkage_debug_matrix.argtypes = [vp, vp, vp, i32, C.POINTER(mh_linkage_params), vp, vp]
        L.mh_linkage_debug_agglomerate.argtypes = [vp, vp, i32, f32, i32, i32, vp, vp, C.POINTER(C.c_int32)]
        L.mh_frame_debug_fetch_clusters_slot.argtypes = [vp, i32, vp, vp, vp, i32, i32, C.POINTER(C.c_int32)]
        L.mh_frame_debug_fetch_cluster_table_slot.argtypes = [vp, i32, vp, vp, vp, i32, C.POINTER(C.c_int32),
                                                              C.POINTER(C.c_int32)]
    if hasattr(L, "mh_cluster_wms"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_cluster_wms.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_wms_params), vp, vp, i32, vp, i32, vp]
        L.mh_wms_debug_state.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_wms_params), vp, vp, vp, vp]
        L.mh_frame_set_cluster_wms.argtypes = [vp, C.POINTER(mh_wms_params)]
    if hasattr(L, "mh_pose_debug_rows"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_pose_debug_rows.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.mh_pose_debug_step.argtypes = [vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp]
    L.mh_frame_set_depth_rules.argtypes = [vp, C.POINTER(mh_depth_rules), vp]
    L.mh_frame_enqueue_rest_strided.argtypes = [vp, vp, i32, vp, i32, i32, C.POINTER(mh_cam),
                                                C.POINTER(mh_frame_params), C.c_uint64]
    L.mh_frame_result_copy_dev.argtypes = [vp, vp, i32]
    L.mh_frame_enqueue_rest_batch.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, C.POINTER(mh_cam),
                                              C.POINTER(mh_frame_params), C.c_uint64]
    L.mh_frame_fetch_slot.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_int32), vp]
    L.mh_frame_result_copy_slots_dev.argtypes = [vp, vp, i32, i32]
    L.mh_frame_fetch_matches.argtypes = [vp, vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_features_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.mh_frame_keypoints.argtypes = [vp, C.POINTER(C.c_int32)]
    L.mh_models_create.argtypes = [C.POINTER(vp), C.c_char_p]
    L.mh_models_destroy.argtypes = [vp]
    L.mh_models_destroy.restype = None
    L.mh_models_last_error.argtypes = [vp]
    L.mh_models_last_error.restype = C.c_char_p
    L.mh_models_add_xml.argtypes = [vp, C.c_char_p]
    L.mh_models_add_xml_buffer.argtypes = [vp, C.c_char_p, C.c_int64]
    L.mh_models_count.argtypes = [vp]
    L.mh_models_rows.argtypes = [vp]
    L.mh_models_rows.restype = C.c_int64
    L.mh_models_name.argtypes = [vp, i32]
    L.mh_models_name.restype = C.c_char_p
    L.mh_models_range.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp]
    L.mh_models_desc.argtypes = [vp]
    L.mh_models_desc.restype = vp
    L.mh_models_xyz.argtypes = [vp]
    L.mh_models_xyz.restype = vp
    L.mh_models_save.argtypes = [vp, C.c_char_p]
    L.mh_models_load.argtypes = [C.POINTER(vp), C.c_char_p]
    L.mh_db_upload_models.argtypes = [vp, vp, i32, i32]
    L.mh_db_upload_raw.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32]
    L.mh_frame_set_depth_image.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32]
    L.mh_frame_enqueue_match_local.argtypes = [vp, vp, i32, vp]
    L.mh_frame_enqueue_rest.argtypes = [vp, vp, i32, vp, i32, C.POINTER(mh_cam),
                                        C.POINTER(mh_frame_params), C.c_uint64]
    L.mh_frame_fetch.argtypes = [vp, vp, i32, C.POINTER(C.c_int32), vp]
    L.mh_frame_result_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.mh_db_share.argtypes = [vp, vp]
    L.mh_db_splice.argtypes = [vp, i32, i32, vp, vp, i32, i32, i32]
    L.mh_db_reserve.argtypes = [vp, C.c_int64, i32]
    L.mh_db_adopt.argtypes = [vp, vp]
    L.mh_db_generation.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mh_db_model_rows.argtypes = [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.mh_db_splice_models.argtypes = [vp, i32, i32, vp, i32]
    L.mh_db_debug_fetch.argtypes = [vp, i32, vp, C.c_size_t]
    L.mh_depth_rules_debug_fetch.argtypes = [vp, i32, i32, vp, C.c_size_t]
    L.mh_depth_filter.argtypes = [vp, vp, i32, i32, vp, i32, f32, vp, vp, i32, vp]
    L.mh_depth_prop.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp]
    L.mh_frame_run_kinect_host.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params),
                                           i32, i32, i32, f32, f32, C.c_uint64, vp, i32, C.POINTER(C.c_int32), vp]
    if hasattr(L, "mh_depth_map_from_raw_dev"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        rd = C.POINTER(mh_raw_depth)
        L.mh_depth_map_from_raw_dev.argtypes = [vp, vp, rd, vp, vp, i32, i32]
        L.mh_depth_map_from_raw_batch_dev.argtypes = [vp, C.POINTER(vp), rd, vp, C.POINTER(vp), i32, i32, i32]
        L.mh_depth_map_from_raw_host.argtypes = [vp, vp, rd, vp, vp, i32, i32]
        L.mh_frame_run_kinect_raw_host.argtypes = [vp, vp, vp, rd, vp, vp, i32, i32, i32, i32, C.POINTER(mh_cam),
                                                   C.POINTER(mh_frame_params), i32, i32, i32, f32, f32, C.c_uint64, vp, i32,
                                                   C.POINTER(C.c_int32), vp]
    if hasattr(L, "mh_image_gray_dev"):   # (the same)
        ri = C.POINTER(mh_raw_image)
        L.mh_image_gray_dev.argtypes = [vp, vp, ri, vp]
        L.mh_image_gray_batch_dev.argtypes = [vp, C.POINTER(vp), ri, C.POINTER(vp), i32]
        L.mh_image_gray_host.argtypes = [vp, vp, ri, vp]
        L.mh_frame_set_image_format.argtypes = [vp, ri]
    L.mh_db_debug_screen.argtypes = [vp, vp]
    L.mh_db_debug_route.argtypes = [vp, i32]
    L.mh_db_edit_ms.argtypes = [vp, C.POINTER(f32)]
    L.mh_match_stats.argtypes = [vp, i32, vp, i32]
    L.mh_match_set_mode.argtypes = [vp, i32]
    L.mh_match_launches.argtypes = [vp, vp]
    L.mh_pose_set_split.argtypes = [vp, i32]
    L.mh_frame_counters.argtypes = [vp, vp]
    L.mh_frame_set_images.argtypes = [vp, vp, vp, i32]
    L.mh_filter_images.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp, i32, i32, f32, f32,
                                   vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
    L.mh_pose_ransac_images.argtypes = [vp, vp, vp, vp, i32, vp, i32, C.POINTER(mh_pose_params),
                                        C.c_uint64, vp, C.POINTER(C.c_int32)]
    L.mh_match_timing.argtypes = [vp, vp]
    L.mh_screen_margin.argtypes = [f32, f32]
    L.mh_screen_margin.restype = f32
    L.mh_enable_timing.argtypes = [vp, i32]
    L.mh_timing.argtypes = [vp, C.POINTER(mh_times)]
    L.mh_comm_unique_id.argtypes = [vp]
    L.mh_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.mh_comm_create_all.argtypes = [C.POINTER(vp), i32, C.POINTER(vp)]
    L.mh_comm_create_host.argtypes = [vp, i32, i32, ALLGATHER_FN, vp, C.POINTER(vp)]
    L.mh_comm_destroy.argtypes = [vp]
    L.mh_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.mh_frame_enqueue_sharded.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params), C.c_uint64]
    L.mh_frame_enqueue_sharded_batch.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(mh_cam),
                                                 C.POINTER(mh_frame_params), C.POINTER(C.c_uint64)]
    L.mh_frame_enqueue_sharded_all.argtypes = [C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp), i32, i32,
                                               C.POINTER(mh_cam), C.POINTER(mh_frame_params), C.POINTER(C.c_uint64)]
    L.mh_frame_enqueue_batch.argtypes = [vp, vp, vp, i32, i32, C.POINTER(mh_cam), C.POINTER(mh_frame_params),
                                         C.POINTER(C.c_uint64)]
    L.mh_frame_set_depth_image_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, f32, f32]
    L.mh_frame_previous_objects.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_gather_objects.argtypes = [vp, vp, i32, vp, i32, C.POINTER(C.c_int32)]
    L.mh_pose_kernel_info.argtypes = [vp, i32, vp]
    L.mh_frame_fetch_matches_slot.argtypes = [vp, i32, vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_fetch_match_reps_slot.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_fetch_match_points.argtypes = [vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_enqueue_rest_frames.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, C.POINTER(mh_cam),
                                               C.POINTER(mh_frame_params), C.POINTER(C.c_uint64)]
    L.mh_screen_values.argtypes = [vp, vp, i32, i32, vp, C.POINTER(f32), C.POINTER(f32), i32]
    L.mh_screen_record_value.argtypes = [f32, f32]
    L.mh_screen_record_value.restype = C.c_uint16
    L.mh_screen_record_bounds.argtypes = [C.c_uint16, C.c_uint32, f32, f32, i32, f32, C.POINTER(f32), C.POINTER(f32)]
    L.mh_screen_record_bounds.restype = None
    if hasattr(L, "mh_screen_pack_value"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_screen_pack_value.argtypes = [f32, C.c_uint32, i32]
        L.mh_screen_pack_value.restype = f32
        L.mh_screen_pack_pert.argtypes = [f32, f32, i32]
        L.mh_screen_pack_pert.restype = f32
        L.mh_screen_sample_bounds.argtypes = [C.c_uint16, f32, f32, f32, C.POINTER(f32), C.POINTER(f32)]
        L.mh_screen_sample_bounds.restype = None
        L.mh_screen_launch_plan.argtypes = [i32, i32, i32, vp]
        L.mh_screen_launch_plan.restype = None
        L.mh_match_incomplete.argtypes = [vp, C.POINTER(C.c_uint32), i32]
    if hasattr(L, "mh_screen_reject_proved"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_screen_reject_proved.argtypes = [f32, f32, f32, f32, f32, f32]
        L.mh_match_set_accept.argtypes = [vp, f32]
        L.mh_match_prerejected.argtypes = [vp, C.POINTER(C.c_uint32), i32]
    if hasattr(L, "mh_screen_sample_values"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_screen_sample_values.argtypes = [vp, vp, i32, vp, vp]
        L.mh_match_query_candidates.argtypes = [vp, i32, vp]
    L.mh_db_upload_blocks.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, i32, i32]
    L.mh_frame_block_stride.argtypes = [i32]
    L.mh_frame_block_stride.restype = C.c_size_t
    L.mh_frame_fetch_batch_async.argtypes = [vp, i32, i32, vp, C.c_uint32]
    L.mh_frame_fetch_previous_async.argtypes = [vp, i32, vp, C.c_uint32]
    L.mh_frame_fetch_wait.argtypes = [vp, C.POINTER(C.c_int32)]
    L.mh_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.mh_host_free.argtypes = [vp, vp]
    L.mh_frame_wait_descriptors.argtypes = [vp]
    if hasattr(L, "mh_step_match"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_set_linkage_scratch_limit.argtypes = [vp, C.c_size_t]
        L.mh_step_match.argtypes = [vp, vp, vp, i32, C.POINTER(mh_cam), f32, i32]
        L.mh_step_match_fetch.argtypes = [vp, vp, vp, vp, i32, C.POINTER(C.c_int32)]
        L.mh_step_cluster.argtypes = [vp, f32, f32, i32, i32, vp, vp, vp, i32, i32, C.POINTER(C.c_int32)]
        L.mh_step_pose.argtypes = [vp, i32, C.POINTER(mh_pose_params), C.c_uint64, vp, i32, C.POINTER(C.c_int32)]
        L.mh_step_filter.argtypes = [vp, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_int32)]
    L.mh_frame_fetch_query.argtypes = [vp]
    if hasattr(L, "mh_undistort"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_undistort_map.argtypes = [vp, i32, i32, vp, vp, vp, vp]
        L.mh_undistort.argtypes = [vp, vp, vp, i32, i32, vp, vp]
        L.mh_undistort_dev.argtypes = [vp, vp, vp, i32, i32, vp, vp]
        L.mh_frame_set_undistort.argtypes = [vp, vp]
    if hasattr(L, "mh_frame_enqueue_images"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_frame_enqueue_images.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, C.POINTER(mh_frame_params), C.c_uint64]
        L.mh_frame_enqueue_images_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, C.POINTER(mh_frame_params), vp]
        L.mh_frame_set_undistort_images.argtypes = [vp, vp, i32]
        L.mh_frame_image_counts.argtypes = [vp, vp, i32, C.POINTER(C.c_int32)]
        L.mh_frame_features_image_dev.argtypes = [vp, C.POINTER(vp)]
    if hasattr(L, "mh_filter_depth"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_filter_depth_set_points.argtypes = [vp, vp, vp, i32]
        L.mh_filter_depth.argtypes = [vp, vp, vp, i32, vp, vp, i32, C.POINTER(mh_cam), i32, f32, f32, C.POINTER(mh_cam),
                                      C.POINTER(mh_filter_depth_params), vp, vp, vp, vp, vp, C.POINTER(C.c_int32), vp, vp, vp]
        L.mh_frame_set_filter_depth.argtypes = [vp, C.POINTER(mh_filter_depth_params), C.POINTER(mh_filter_depth_params),
                                                C.POINTER(mh_cam)]
    if hasattr(L, "mh_frame_route"):   # (the same)
        L.mh_frame_route.argtypes = [vp, vp]
        L.mh_filter_depth_debug_form.argtypes = [vp, i32]
    if hasattr(L, "mh_planar_rows_dev"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_planar_rows_dev.argtypes = [vp, vp, vp, vp, i32, C.POINTER(mh_planar_spec), vp, vp, i32, vp, vp]
        L.mh_planar_rows_batch_dev.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(mh_planar_spec), vp, vp, i32, vp, vp]
        L.mh_db_splice_image.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, C.POINTER(mh_planar_spec),
                                         C.POINTER(C.c_int32), vp, vp, vp, i32]
        L.mh_db_splice_images.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, C.POINTER(mh_planar_spec), vp, vp, vp, vp, i32]
        L.mh_models_add_rows.argtypes = [vp, C.c_char_p, vp, vp, C.c_int64]
        L.mh_models_write_xml.argtypes = [vp, i32, C.c_char_p]
    if hasattr(L, "mh_view_rows_dev"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        pv, ps, pd = C.POINTER(mh_view), C.POINTER(mh_view_spec), C.POINTER(mh_view_dup)
        L.mh_view_rows_dev.argtypes = [vp, vp, vp, vp, i32, pv, i32, i32, ps, pd, vp, vp, i32, vp, vp, vp]
        L.mh_view_rows_batch_dev.argtypes = [vp, vp, vp, vp, i32, i32, pv, i32, i32, ps, pd, vp, vp, i32, vp, vp, vp]
        L.mh_db_append.argtypes = [vp, i32, vp, vp, i32, i32, i32]
        L.mh_db_splice_view.argtypes = [vp, i32, i32, vp, pv, i32, i32, i32, i32, ps, C.POINTER(C.c_int32), vp, vp, vp, vp, i32]
        L.mh_db_append_view.argtypes = [vp, i32, vp, pv, i32, i32, i32, i32, ps, C.POINTER(C.c_int32), vp, vp, vp, vp, i32]
        L.mh_db_splice_views.argtypes = [vp, i32, vp, pv, i32, i32, i32, i32, i32, ps, vp, vp, vp, vp, vp, i32]
    if hasattr(L, "mh_view_merge_dev"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        pv, ps, pd, pi = C.POINTER(mh_view), C.POINTER(mh_view_spec), C.POINTER(mh_view_dup), C.POINTER(C.c_int32)
        L.mh_view_merge_dev.argtypes = [vp, vp, vp, vp, vp, i32, pv, i32, i32, ps, pd, vp, vp, vp, vp, vp, i32, vp, vp]
        L.mh_db_merge_view.argtypes = [vp, i32, vp, pv, i32, i32, i32, i32, ps, vp, i32, pi, pi, vp, vp, vp, vp, i32,
                                       vp, vp, vp, i32, vp, i32]
        L.mh_db_keep_rows.argtypes = [vp, i32, vp, i32, pi, vp]
    if hasattr(L, "mh_depth_verify"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_depth_verify.argtypes = [vp, vp, vp, i32, vp, vp, i32, C.POINTER(mh_cam), C.POINTER(mh_cam),
                                      C.POINTER(mh_depth_verify_params), vp]
        L.mh_depth_verify_debug_form.argtypes = [vp, i32]
        L.mh_frame_set_depth_verify.argtypes = [vp, C.POINTER(mh_depth_verify_params), C.POINTER(mh_cam)]
        L.mh_frame_fetch_verify_slot.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_int32)]
        L.mh_frame_fetch_verify.argtypes = [vp, i32, vp, C.POINTER(C.c_int32)]
    if hasattr(L, "mh_object_hulls"):   # (absent only in an older build named by MH_LIB_PATH for an A/B run)
        L.mh_object_hulls.argtypes = [vp, vp, vp, i32, C.POINTER(mh_cam), i32, vp, vp, vp, vp]
        L.mh_hull_debug_form.argtypes = [vp, i32]
        L.mh_frame_set_hulls.argtypes = [vp, i32, i32]
        L.mh_frame_fetch_hulls_slot.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        L.mh_frame_fetch_hulls.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        L.mh_frame_hull_block_stride.argtypes = [i32, i32]
        L.mh_frame_hull_block_stride.restype = C.c_size_t
        L.mh_frame_fetch_batch_hulls_async.argtypes = [vp, i32, i32, vp]
    _lib = L
    return L


def _calib(v):
    a = np.ascontiguousarray(v, np.float32).reshape(-1)
    if a.size != 4:
        raise ValueError("a calibration has 4 values")
    return a


def make_cam(K, cam) -> mh_cam:
    c = mh_cam()
    c.K[:] = [float(x) for x in K]
    c.cam[:] = [float(x) for x in cam]
    return c


def make_cams(Ks, cams):
    """Array of mh_cam for a frame with several images: Ks [n,4], cams [n,7]."""
    arr = (mh_cam * len(Ks))()
    for i, (K, c) in enumerate(zip(Ks, cams)):
        arr[i] = make_cam(K, c)
    return arr


def make_pose_params(n_hypotheses=1024, max_objects_per_cluster=4, n_pts_align=5,
                     min_n_pts_object=6, error_threshold=10.0, lm_iters_l2=2, lm_iters_l4=10):
    return mh_pose_params(n_hypotheses, max_objects_per_cluster, n_pts_align, min_n_pts_object,
                          error_threshold, lm_iters_l2, lm_iters_l4)


def default_frame_params() -> mh_frame_params:
    p = mh_frame_params()
    load().mh_frame_default_params(C.byref(p))
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_depth(world, wgt) -> np.ndarray:
    n = len(world)
    d = np.zeros(n, DEPTH_DTYPE)
    if n:
        world = np.asarray(world, np.float32)
        d["wx"], d["wy"], d["wz"] = world[:, 0], world[:, 1], world[:, 2]
        d["w"] = np.asarray(wgt, np.float32)
    return d


def pack_corr(uv, xyz) -> np.ndarray:
    n = len(uv)
    c = np.zeros(n, CORR_DTYPE)
    if n:
        uv = np.asarray(uv, np.float32)
        xyz = np.asarray(xyz, np.float32)
        c["u"], c["v"] = uv[:, 0], uv[:, 1]
        c["x"], c["y"], c["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return c


def screen_record_bounds(value_bits, row0, tau, spread, N, dmax):
    """mh_screen_record_bounds (host arithmetic): (lo, hi) of the largest screen value among a record's rows."""
    lo, hi = C.c_float(0), C.c_float(0)
    load().mh_screen_record_bounds(int(value_bits), int(row0), float(tau), float(spread), int(N), float(dmax),
                                   C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def screen_sample_bounds(value_bits, tau, pert, dmax):
    """mh_screen_sample_bounds (host arithmetic): (lo, hi) of the largest screen value of a sampled tile's block."""
    lo, hi = C.c_float(0), C.c_float(0)
    load().mh_screen_sample_bounds(int(value_bits), float(tau), float(pert), float(dmax), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def screen_launch_plan(Q, N, q_expected=0) -> dict:
    """mh_screen_launch_plan (host arithmetic): how a two-stage MATCH of Q queries against N rows is launched; all zero
    when it does not run on the 16x16x32 passes."""
    o = np.zeros(8, np.int32)
    load().mh_screen_launch_plan(int(Q), int(q_expected), int(N), _ptr(o))
    keys = ("onesweep", "tile_first", "tile_stride", "sampled_tiles", "splits_a", "pack_bits", "splits_b", "tiles_b")
    return {k: int(v) for k, v in zip(keys, o)}


SCREEN_PLAN_KEYS = ("family", "nqb", "a_tile_first", "a_stride", "a_tiles", "a_splits", "pack_bits", "onesweep",
                    "b_tiles", "b_splits", "sub_cap", "skip_first", "skip_stride", "n_slots")


def screen_plan(Q, N, q_expected=0) -> dict:
    """mh_screen_plan (host arithmetic): the whole launch plan of a two-stage MATCH of Q queries against N rows, for either
    kernel family (family = 32: the 32x32x16 passes, 16: the 16x16x32 passes)."""
    o = np.zeros(len(SCREEN_PLAN_KEYS), np.int32)
    f = load().mh_screen_plan   # (bound here, like mh_screen_park_places)
    f.argtypes, f.restype = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p], None
    f(int(Q), int(q_expected), int(N), _ptr(o))
    return {k: int(v) for k, v in zip(SCREEN_PLAN_KEYS, o)}


def screen_park_places() -> int:
    """mh_screen_park_places: hits a wavefront of pass B of the 16x16x32 launches parks before it appends from the hit path."""
    f = load().mh_screen_park_places   # (bound here, not in load(): A/B runs load older builds of the library by MH_LIB_PATH)
    f.argtypes, f.restype = [], C.c_int
    return int(f())


FRAME_HEAD_DTYPE = np.dtype([("n_objects", "<i4"), ("flags", "<i4"), ("counts", "<i4", (4,)), ("tag", "<u4"), ("frame", "<i4")])


def frame_block_dtype(max_objects: int) -> np.dtype:
    """One record of a delivery block (mh_frame_fetch_batch_async): mh_frame_head + mh_object[max_objects]."""
    return np.dtype([("head", FRAME_HEAD_DTYPE), ("objects", OBJECT_DTYPE, (max_objects,))])


def hull_block_dtype(max_objects: int, max_vertices: int) -> np.dtype:
    """One frame of a hull delivery block (mh_frame_fetch_batch_hulls_async): max_objects records, object o's at [o]."""
    rec = np.dtype([("n_vertices", np.int32), ("n_behind", np.int32), ("bbox_uv", np.float32, (8, 2)),
                    ("hull_xy", np.float32, (max_vertices, 2))])
    assert rec.itemsize * max_objects == load().mh_frame_hull_block_stride(max_objects, max_vertices)
    return np.dtype([("objects", rec, (max_objects,))])


def frame_block_bytes(B: int, max_objects: int) -> int:
    return B * (FRAME_HEAD_DTYPE.itemsize + OBJECT_DTYPE.itemsize * max_objects)


def comm_unique_id() -> bytes:
    """mh_comm_unique_id: rank 0 makes it, the launcher hands it to the other ranks."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    if load().mh_comm_unique_id(buf) != MH_OK:
        raise MhError("mh_comm_unique_id failed: RCCL not loadable?")
    return buf.raw


class Lane:
    """mh_lane: streams for the chip-filling MATCH passes of all contexts of a device (CU-masked or low priority)."""

    def __init__(self, device=0, n_streams=4, reserve_cus_per_xcd=2, low_priority=False):
        self.L = load()
        if not hasattr(self.L, "mh_lane_create"):
            raise MhError("lanes exist only in experiment builds of the library (make EXTRA=-DMH_EXPERIMENTS; MH_LIB_PATH)")
        h = C.c_void_p()
        rc = self.L.mh_lane_create(device, n_streams, reserve_cus_per_xcd, int(low_priority), C.byref(h))
        if rc != MH_OK:
            raise MhError(f"mh_lane_create -> {rc}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mh_lane_destroy(self.h)
            self.h = None


class Comm:
    """mh_comm of one rank: RCCL (`create`), or a host transport (`create_host`: fn(send: bytes) -> bytes of all
    ranks in rank order -- ranks that share a device, test rigs)."""

    def __init__(self, handle, keep=None):
        self.L = load()
        self.h = handle
        self._keep = keep   # the ctypes callback must outlive the communicator

    @classmethod
    def create(cls, ctx: "Context", unique_id: bytes, rank: int, world: int) -> "Comm":
        h = C.c_void_p()
        buf = C.create_string_buffer(unique_id, COMM_ID_BYTES)
        ctx._ck(ctx.L.mh_comm_create(ctx.h, buf, rank, world, C.byref(h)), "mh_comm_create")
        return cls(h)

    @classmethod
    def create_host(cls, ctx: "Context", rank: int, world: int, allgather) -> "Comm":
        def _cb(_user, send, recv, nbytes):
            try:
                out = allgather(C.string_at(send, nbytes))
                if len(out) != nbytes * world:
                    return 1
                C.memmove(recv, out, len(out))
                return 0
            except Exception:   # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        fn = ALLGATHER_FN(_cb)
        h = C.c_void_p()
        ctx._ck(ctx.L.mh_comm_create_host(ctx.h, rank, world, fn, None, C.byref(h)), "mh_comm_create_host")
        return cls(h, keep=fn)

    @classmethod
    def create_all(cls, ctxs) -> "list[Comm]":
        n = len(ctxs)
        hs = (C.c_void_p * n)(*[c.h for c in ctxs])
        out = (C.c_void_p * n)()
        ctxs[0]._ck(ctxs[0].L.mh_comm_create_all(hs, n, out), "mh_comm_create_all")
        return [cls(C.c_void_p(out[i])) for i in range(n)]

    def info(self):
        r, w, k = C.c_int(0), C.c_int(0), C.c_int(0)
        self.L.mh_comm_info(self.h, C.byref(r), C.byref(w), C.byref(k))
        return r.value, w.value, bool(k.value)

    def close(self):
        if getattr(self, "h", None):
            self.L.mh_comm_destroy(self.h)
            self.h = None


def frame_enqueue_sharded_all(ctxs, comms, q_desc_ptrs, q_uv_ptrs, Q, B, K, cam, params, seeds):
    """mh_frame_enqueue_sharded_all: one host thread, one context + communicator per device."""
    n = len(ctxs)
    c = make_cam(K, cam)
    sd = (C.c_uint64 * B)(*[int(x) for x in seeds])
    rc = ctxs[0].L.mh_frame_enqueue_sharded_all((C.c_void_p * n)(*[x.h for x in ctxs]), (C.c_void_p * n)(*[x.h for x in comms]),
                                                n, (C.c_void_p * n)(*q_desc_ptrs), (C.c_void_p * n)(*q_uv_ptrs), Q, B,
                                                C.byref(c), C.byref(params), sd)
    if rc != MH_OK:
        msgs = [x.L.mh_last_error(x.h).decode() for x in ctxs]
        raise MhError(f"mh_frame_enqueue_sharded_all -> {rc}: {msgs}")


class Context:
    """One mh_ctx.  Host-array methods mirror the per-step C entry points."""

    def __init__(self, device: int = 0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.mh_create(device, C.byref(h))
        if rc != MH_OK:
            raise MhError(f"mh_create(device={device}) failed with {rc}: no gfx950 device?")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mh_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc, what):
        if rc != MH_OK:
            raise MhError(f"{what} -> {rc}: {self.L.mh_last_error(self.h).decode()}")

    # ---- context ----
    def set_stream(self, stream_ptr):
        self._ck(self.L.mh_set_stream(self.h, C.c_void_p(stream_ptr)), "mh_set_stream")

    def synchronize(self):
        self._ck(self.L.mh_synchronize(self.h), "mh_synchronize")

    def set_lane(self, lane: "Lane | None"):
        self._ck(self.L.mh_set_lane(self.h, lane.h if lane is not None else None), "mh_set_lane")

    def reserve(self, max_queries, max_clusters=1024, max_objects=4096):
        self._ck(self.L.mh_reserve(self.h, max_queries, max_clusters, max_objects), "mh_reserve")

    def reserve_batch(self, queries_per_frame, frames, max_clusters=1024, max_objects=4096):
        self._ck(self.L.mh_reserve_batch(self.h, queries_per_frame, frames, max_clusters, max_objects), "mh_reserve_batch")

    def enable_timing(self, on=True):
        self._ck(self.L.mh_enable_timing(self.h, int(on)), "mh_enable_timing")

    def timing(self) -> dict:
        t = mh_times()
        self._ck(self.L.mh_timing(self.h, C.byref(t)), "mh_timing")
        return {n: getattr(t, n) for n, _ in mh_times._fields_}

    # ---- DB / MATCH ----
    def db_upload(self, desc, model_of, xyz, n_models, index_base=0):
        desc = np.ascontiguousarray(desc, np.float32)
        model_of = np.ascontiguousarray(model_of, np.int32)
        xyz = np.ascontiguousarray(xyz, np.float32)
        self._ck(self.L.mh_db_upload(self.h, _ptr(desc), _ptr(model_of), _ptr(xyz), desc.shape[0],
                                     n_models, index_base), "mh_db_upload")

    def db_upload_blocks(self, desc, model_of, xyz, n_models, block_global_row, block_rows, normalize=False):
        """A shard whose rows are several runs of global rows (round-robin model assignment): mh_db_upload_blocks."""
        desc = np.ascontiguousarray(desc, np.float32)
        model_of = np.ascontiguousarray(model_of, np.int32)
        xyz = np.ascontiguousarray(xyz, np.float32)
        g = np.ascontiguousarray(block_global_row, np.int32)
        r = np.ascontiguousarray(block_rows, np.int32)
        self._ck(self.L.mh_db_upload_blocks(self.h, _ptr(desc), _ptr(model_of), _ptr(xyz), desc.shape[0], n_models,
                                            _ptr(g), _ptr(r), len(g), int(normalize)), "mh_db_upload_blocks")

    def db_share(self, src: "Context"):
        """Use the database `src` holds (no copy; one store per GPU for all frames in flight)."""
        self._ck(self.L.mh_db_share(self.h, src.h), "mh_db_share")

    # ---- edits of the resident DB (mh_db_splice and friends) ----
    def db_splice(self, op, model, desc=None, xyz=None, normalize=False, on_device=False, n_rows=None):
        """mh_db_splice: op = DB_INSERT / DB_REPLACE / DB_REMOVE of model `model`.  desc [n][128], xyz [n][3]: host
        arrays, or device pointers (ints) with on_device and n_rows."""
        if op == DB_REMOVE:
            self._ck(self.L.mh_db_splice(self.h, op, int(model), None, None, 0, 0, 0), "mh_db_splice")
            return
        if on_device:
            self._ck(self.L.mh_db_splice(self.h, op, int(model), C.c_void_p(desc), C.c_void_p(xyz), int(n_rows),
                                         int(normalize), 1), "mh_db_splice")
            return
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, DIM)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        assert desc.shape[0] == xyz.shape[0]
        self._ck(self.L.mh_db_splice(self.h, op, int(model), _ptr(desc), _ptr(xyz), desc.shape[0], int(normalize), 0),
                 "mh_db_splice")

    def db_splice_models(self, op, model, models: "ModelSet | None" = None, set_index=0):
        """mh_db_splice_models: the rows of model `set_index` of a parsed set, normalised on the device."""
        self._ck(self.L.mh_db_splice_models(self.h, op, int(model), models.h if models is not None else None, int(set_index)),
                 "mh_db_splice_models")

    # ---- planar models from images: createPlanarModelsFromImages (moped.cpp:196-236) ----
    def planar_rows_dev(self, desc_ptr, xy_ptr, n_ptr, cap, spec: mh_planar_spec, desc_out_ptr, xyz_out_ptr, out_cap,
                        n_out_ptr, bbox_ptr, n_images=1):
        """mh_planar_rows_dev (n_images > 1: mh_planar_rows_batch_dev) on device arrays; asynchronous."""
        a = [C.c_void_p(desc_ptr), C.c_void_p(xy_ptr), C.c_void_p(n_ptr)]
        b = [int(cap), C.byref(spec) if spec is not None else None, C.c_void_p(desc_out_ptr), C.c_void_p(xyz_out_ptr),
             int(out_cap), C.c_void_p(n_out_ptr), C.c_void_p(bbox_ptr)]
        if n_images == 1:
            self._ck(self.L.mh_planar_rows_dev(self.h, *a, *b), "mh_planar_rows_dev")
        else:
            self._ck(self.L.mh_planar_rows_batch_dev(self.h, *a, int(n_images), *b), "mh_planar_rows_batch_dev")

    def db_splice_image(self, op, model, gray_ptr, w, h, spec: mh_planar_spec, double_size=True, max_keypoints=4096,
                        want_rows=False):
        """mh_db_splice_image: the device image becomes model `model` (DB_INSERT / DB_REPLACE).  -> (n_rows, bbox[6]) or,
        with want_rows, (n_rows, bbox, desc [n,128], xyz [n,3]) -- the selected rows, descriptors as FEAT made them."""
        n = C.c_int32(0)
        bbox = np.zeros(6, np.float32)
        d = np.zeros((max_keypoints, DIM), np.float32) if want_rows else None
        x = np.zeros((max_keypoints, 3), np.float32) if want_rows else None
        rc = self.L.mh_db_splice_image(self.h, int(op), int(model), C.c_void_p(gray_ptr), w, h, int(double_size),
                                       int(max_keypoints), C.byref(spec) if spec is not None else None, C.byref(n),
                                       _ptr(bbox), _ptr(d) if want_rows else None, _ptr(x) if want_rows else None,
                                       max_keypoints if want_rows else 0)
        # MH_ERR_CAPACITY: the edit is made, from the first max_keypoints keypoints of the list
        self.planar_truncated = rc == MH_ERR_CAPACITY
        self._ck(MH_OK if self.planar_truncated else rc, "mh_db_splice_image")
        if want_rows:
            return int(n.value), bbox, d[:n.value].copy(), x[:n.value].copy()
        return int(n.value), bbox

    def db_splice_images(self, model_first, gray_ptrs, w, h, spec: mh_planar_spec, double_size=True, max_keypoints=4096,
                         want_rows=False):
        """mh_db_splice_images: len(gray_ptrs) device images of one size become models model_first .. (INSERT), FEAT as
        one batch, one selection launch.  -> (n_rows [n], bbox [n,6]) and, with want_rows, lists of desc and xyz."""
        k = len(gray_ptrs)
        g = (C.c_void_p * k)(*gray_ptrs)
        n = np.zeros(k, np.int32)
        bbox = np.zeros((k, 6), np.float32)
        d = np.zeros((k, max_keypoints, DIM), np.float32) if want_rows else None
        x = np.zeros((k, max_keypoints, 3), np.float32) if want_rows else None
        rc = self.L.mh_db_splice_images(self.h, int(model_first), g, k, w, h, int(double_size), int(max_keypoints),
                                        C.byref(spec) if spec is not None else None, _ptr(n), _ptr(bbox),
                                        _ptr(d) if want_rows else None, _ptr(x) if want_rows else None,
                                        max_keypoints if want_rows else 0)
        self.planar_truncated = rc == MH_ERR_CAPACITY
        self._ck(MH_OK if self.planar_truncated else rc, "mh_db_splice_images")
        if want_rows:
            return n, bbox, [d[i, :n[i]].copy() for i in range(k)], [x[i, :n[i]].copy() for i in range(k)]
        return n, bbox

    # ---- 3-D models from Kinect views (mh_view_rows_dev and friends) ----
    def view_rows_dev(self, desc_ptr, xy_ptr, n_ptr, cap, view: mh_view, w, h, spec: mh_view_spec, desc_out_ptr, xyz_out_ptr,
                      out_cap, n_out_ptr, bbox_ptr, stats_ptr, dup: "mh_view_dup | None" = None):
        """mh_view_rows_dev on device arrays; asynchronous."""
        self._ck(self.L.mh_view_rows_dev(
            self.h, C.c_void_p(desc_ptr), C.c_void_p(xy_ptr), C.c_void_p(n_ptr), int(cap),
            C.byref(view) if view is not None else None, int(w), int(h), C.byref(spec) if spec is not None else None,
            C.byref(dup) if dup is not None else None, C.c_void_p(desc_out_ptr), C.c_void_p(xyz_out_ptr), int(out_cap),
            C.c_void_p(n_out_ptr), C.c_void_p(bbox_ptr), C.c_void_p(stats_ptr)), "mh_view_rows_dev")

    def view_rows_batch_dev(self, desc_ptr, xy_ptr, n_ptr, cap, views, w, h, spec: mh_view_spec, desc_out_ptr, xyz_out_ptr,
                            out_cap, n_out_ptr, bbox_ptr, stats_ptr, dup: "mh_view_dup | None" = None):
        """mh_view_rows_batch_dev: len(views) lists, one mh_view each, in one launch; asynchronous."""
        vs = (mh_view * len(views))(*views)
        self._ck(self.L.mh_view_rows_batch_dev(
            self.h, C.c_void_p(desc_ptr), C.c_void_p(xy_ptr), C.c_void_p(n_ptr), len(views), int(cap), vs, int(w), int(h),
            C.byref(spec) if spec is not None else None, C.byref(dup) if dup is not None else None, C.c_void_p(desc_out_ptr),
            C.c_void_p(xyz_out_ptr), int(out_cap), C.c_void_p(n_out_ptr), C.c_void_p(bbox_ptr), C.c_void_p(stats_ptr)),
            "mh_view_rows_batch_dev")

    def db_append(self, model, desc, xyz, normalize=False, on_device=False, n_rows=None):
        """mh_db_append: rows behind the last row of model `model`.  desc [n][128], xyz [n][3]: host arrays, or device
        pointers (ints) with on_device and n_rows."""
        if on_device:
            self._ck(self.L.mh_db_append(self.h, int(model), C.c_void_p(desc), C.c_void_p(xyz), int(n_rows), int(normalize), 1),
                     "mh_db_append")
            return
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, DIM)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        assert desc.shape[0] == xyz.shape[0]
        self._ck(self.L.mh_db_append(self.h, int(model), _ptr(desc), _ptr(xyz), desc.shape[0], int(normalize), 0), "mh_db_append")

    def _view_edit(self, name, head, gray_ptr, view, w, h, spec, double_size, max_keypoints, want_rows):
        n = C.c_int32(0)
        bbox = np.zeros(6, np.float32)
        stats = np.zeros(8, np.int32)
        d = np.zeros((max_keypoints, DIM), np.float32) if want_rows else None
        x = np.zeros((max_keypoints, 3), np.float32) if want_rows else None
        rc = getattr(self.L, name)(self.h, *head, C.c_void_p(gray_ptr), C.byref(view) if view is not None else None, w, h,
                                   int(double_size), int(max_keypoints), C.byref(spec) if spec is not None else None,
                                   C.byref(n), _ptr(bbox), _ptr(stats), _ptr(d) if want_rows else None,
                                   _ptr(x) if want_rows else None, max_keypoints if want_rows else 0)
        # MH_ERR_CAPACITY: the edit is made, from the first max_keypoints keypoints of the list
        self.planar_truncated = rc == MH_ERR_CAPACITY
        self._ck(MH_OK if self.planar_truncated else rc, name)
        if want_rows:
            return int(n.value), bbox, stats, d[:n.value].copy(), x[:n.value].copy()
        return int(n.value), bbox, stats

    def db_splice_view(self, op, model, gray_ptr, view: mh_view, w, h, spec: mh_view_spec, double_size=True,
                       max_keypoints=4096, want_rows=False):
        """mh_db_splice_view: the device image + depth map + pose become model `model` (DB_INSERT / DB_REPLACE).
        -> (n_rows, bbox[6], stats[8]) or, with want_rows, (n_rows, bbox, stats, desc [n,128], xyz [n,3])."""
        return self._view_edit("mh_db_splice_view", (int(op), int(model)), gray_ptr, view, w, h, spec, double_size,
                               max_keypoints, want_rows)

    def db_append_view(self, model, gray_ptr, view: mh_view, w, h, spec: mh_view_spec, double_size=True, max_keypoints=4096,
                       want_rows=False):
        """mh_db_append_view: a further view of model `model`; the keypoints it already holds are left out when the
        spec's duplicate test is on.  Returns as db_splice_view: n_rows = rows added, bbox = the whole model's."""
        return self._view_edit("mh_db_append_view", (int(model),), gray_ptr, view, w, h, spec, double_size, max_keypoints,
                               want_rows)

    def view_merge_dev(self, desc_ptr, qn_ptr, xy_ptr, n_ptr, cap, view: mh_view, w, h, spec: mh_view_spec, dup: mh_view_dup,
                       old_desc_ptr, views_in_ptr, merged_idx_ptr, merged_desc_ptr, merged_xyz_ptr, merged_cap, n_merged_ptr,
                       views_out_ptr):
        """mh_view_merge_dev on device arrays: the keypoints rule 7 drops, folded into the rows they re-observe;
        asynchronous."""
        self._ck(self.L.mh_view_merge_dev(
            self.h, C.c_void_p(desc_ptr), C.c_void_p(qn_ptr), C.c_void_p(xy_ptr), C.c_void_p(n_ptr), int(cap),
            C.byref(view) if view is not None else None, int(w), int(h), C.byref(spec) if spec is not None else None,
            C.byref(dup) if dup is not None else None, C.c_void_p(old_desc_ptr), C.c_void_p(views_in_ptr),
            C.c_void_p(merged_idx_ptr), C.c_void_p(merged_desc_ptr), C.c_void_p(merged_xyz_ptr), int(merged_cap),
            C.c_void_p(n_merged_ptr), C.c_void_p(views_out_ptr)), "mh_view_merge_dev")

    def db_merge_view(self, model, gray_ptr, view: mh_view, w, h, spec: mh_view_spec, double_size=True, max_keypoints=4096,
                      views_in=None, want_rows=True):
        """mh_db_merge_view: a further view of model `model`; the keypoints the model already holds are folded into their
        rows.  views_in: the model's view counts (None: all ones).  -> (n_added, n_merged, bbox[6], stats[8], views_out
        [rows after], merged_idx [m], merged_desc [m,128] (s, not normalised), merged_xyz [m,3], desc [n,128], xyz [n,3]);
        the last five are None without want_rows."""
        _, rows = self.db_model_rows(model)
        vin = None if views_in is None else np.ascontiguousarray(views_in, np.int32)
        limit = min(max_keypoints, spec.max_rows) if spec is not None and spec.max_rows > 0 else max_keypoints
        vout = np.zeros(rows + limit, np.int32)
        na, nm = C.c_int32(0), C.c_int32(0)
        bbox = np.zeros(6, np.float32)
        stats = np.zeros(8, np.int32)
        mcap = min(rows, max_keypoints) if want_rows else 0
        d = np.zeros((max_keypoints, DIM), np.float32) if want_rows else None
        x = np.zeros((max_keypoints, 3), np.float32) if want_rows else None
        mi = np.zeros(max(mcap, 1), np.int32) if want_rows else None
        md = np.zeros((max(mcap, 1), DIM), np.float32) if want_rows else None
        mx = np.zeros((max(mcap, 1), 3), np.float32) if want_rows else None
        opt = lambda a: _ptr(a) if a is not None else None
        rc = self.L.mh_db_merge_view(self.h, int(model), C.c_void_p(gray_ptr), C.byref(view) if view is not None else None, w, h,
                                     int(double_size), int(max_keypoints), C.byref(spec) if spec is not None else None,
                                     opt(vin), 0 if vin is None else len(vin), C.byref(na), C.byref(nm), _ptr(bbox), _ptr(stats),
                                     opt(d), opt(x), max_keypoints if want_rows else 0, opt(mi), opt(md), opt(mx), mcap,
                                     _ptr(vout), len(vout))
        # MH_ERR_CAPACITY: the edit is made, from the first max_keypoints keypoints of the list
        self.planar_truncated = rc == MH_ERR_CAPACITY
        self._ck(MH_OK if self.planar_truncated else rc, "mh_db_merge_view")
        n, m = int(na.value), int(nm.value)
        vout = vout[:rows + n].copy()
        if want_rows:
            return n, m, bbox, stats, vout, mi[:m].copy(), md[:m].copy(), mx[:m].copy(), d[:n].copy(), x[:n].copy()
        return n, m, bbox, stats, vout, None, None, None, None, None

    def db_keep_rows(self, model, keep):
        """mh_db_keep_rows: model `model` keeps the rows whose flag is set, in order.  -> (n_rows, bbox[6])."""
        keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        n = C.c_int32(0)
        bbox = np.zeros(6, np.float32)
        self._ck(self.L.mh_db_keep_rows(self.h, int(model), _ptr(keep) if len(keep) else None, len(keep), C.byref(n), _ptr(bbox)),
                 "mh_db_keep_rows")
        return int(n.value), bbox

    def db_splice_views(self, model_first, gray_ptrs, views, w, h, spec: mh_view_spec, double_size=True, max_keypoints=4096,
                        want_rows=False):
        """mh_db_splice_views: len(views) views of one size become models model_first .. (INSERT), FEAT as one batch, one
        selection launch.  -> (n_rows [n], bbox [n,6], stats [n,8]) and, with want_rows, lists of desc and xyz."""
        k = len(gray_ptrs)
        assert len(views) == k
        g = (C.c_void_p * k)(*gray_ptrs)
        vs = (mh_view * k)(*views)
        n = np.zeros(k, np.int32)
        bbox = np.zeros((k, 6), np.float32)
        stats = np.zeros((k, 8), np.int32)
        d = np.zeros((k, max_keypoints, DIM), np.float32) if want_rows else None
        x = np.zeros((k, max_keypoints, 3), np.float32) if want_rows else None
        rc = self.L.mh_db_splice_views(self.h, int(model_first), g, vs, k, w, h, int(double_size), int(max_keypoints),
                                       C.byref(spec) if spec is not None else None, _ptr(n), _ptr(bbox), _ptr(stats),
                                       _ptr(d) if want_rows else None, _ptr(x) if want_rows else None,
                                       max_keypoints if want_rows else 0)
        self.planar_truncated = rc == MH_ERR_CAPACITY
        self._ck(MH_OK if self.planar_truncated else rc, "mh_db_splice_views")
        if want_rows:
            return n, bbox, stats, [d[i, :n[i]].copy() for i in range(k)], [x[i, :n[i]].copy() for i in range(k)]
        return n, bbox, stats

    def db_reserve(self, max_rows, max_models):
        self._ck(self.L.mh_db_reserve(self.h, int(max_rows), int(max_models)), "mh_db_reserve")

    def db_adopt(self, src: "Context"):
        """Stream-ordered db_share: take the store `src` holds now; no host wait."""
        self._ck(self.L.mh_db_adopt(self.h, src.h), "mh_db_adopt")

    def db_generation(self) -> int:
        g = C.c_uint64(0)
        self._ck(self.L.mh_db_generation(self.h, C.byref(g)), "mh_db_generation")
        return int(g.value)

    def db_size(self):
        n, m = C.c_int(0), C.c_int(0)
        self._ck(self.L.mh_db_size(self.h, C.byref(n), C.byref(m)), "mh_db_size")
        return n.value, m.value

    def db_model_rows(self, model):
        """(row_begin, n_rows) of a model of the resident store."""
        b, n = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.mh_db_model_rows(self.h, int(model), C.byref(b), C.byref(n)), "mh_db_model_rows")
        return b.value, n.value

    def db_debug_screen(self) -> dict:
        """ScreenDb's scalars as bit patterns (mh_db_debug_screen)."""
        o = np.zeros(8, np.uint32)
        self._ck(self.L.mh_db_debug_screen(self.h, _ptr(o)), "mh_db_debug_screen")
        names = ("dmax_bits", "spread_bits", "zero_idx", "zero_d1_bits", "zero_d2_bits", "usable", "has_image", "N")
        return dict(zip(names, (int(v) for v in o)))

    def db_debug_fetch(self, which: str) -> np.ndarray:
        """Everything the store defines of one array, as raw bytes viewed in the array's type: 'desc', 'norm', 'xyz',
        'model', 'desc_h' (uint16 bit patterns), 'neg_h' (the last two empty when the store has no f16 image)."""
        sc = self.db_debug_screen()
        N, img = sc["N"], sc["has_image"]
        n_pad = (N + 127) // 128 * 128
        k, dt, n = {"desc": (0, np.float32, n_pad * DIM), "norm": (1, np.float32, n_pad), "xyz": (2, np.float32, N * 3),
                    "model": (3, np.int32, N), "desc_h": (4, np.uint16, n_pad * DIM if img else 0),
                    "neg_h": (5, np.float32, n_pad // 128 * 192 if img else 0)}[which]
        out = np.zeros(n, dt)
        self._ck(self.L.mh_db_debug_fetch(self.h, k, _ptr(out), out.nbytes), "mh_db_debug_fetch")
        return out

    def db_debug_route(self, route: int):
        self._ck(self.L.mh_db_debug_route(self.h, int(route)), "mh_db_debug_route")

    def db_edit_ms(self) -> float:
        ms = C.c_float(0)
        self._ck(self.L.mh_db_edit_ms(self.h, C.byref(ms)), "mh_db_edit_ms")
        return float(ms.value)

    def frame_counters(self) -> dict:
        """Device-side counters of the last frame on this context (see mh_frame_counters)."""
        c = np.zeros(8, np.int32)
        self._ck(self.L.mh_frame_counters(self.h, _ptr(c)), "mh_frame_counters")
        names = ("matches", "clusters", "r2", "r3", "r4", "pose_tasks", "error", "hypotheses")
        return dict(zip(names, (int(v) for v in c)))

    def pose_kernel_info(self, kind=0):
        """mh_pose_kernel_info: registers / LDS / threads / residency of the RANSAC kernel on this device."""
        o = np.zeros(8, np.int32)
        self._ck(self.L.mh_pose_kernel_info(self.h, int(kind), _ptr(o)), "mh_pose_kernel_info")
        waves = int(o[5])
        return {"vgprs": int(o[0]), "lds_bytes": int(o[1]), "threads": int(o[2]), "workgroups_per_cu": int(o[3]),
                "scratch_bytes": int(o[4]), "waves_per_workgroup": waves,
                "waves_per_simd": int(o[3]) * waves / 4.0}

    def match_timing(self) -> dict:
        """Per-kernel GPU times (ms) of the last two-stage MATCH (after enable_timing)."""
        t = np.zeros(5, np.float32)
        self._ck(self.L.mh_match_timing(self.h, _ptr(t)), "mh_match_timing")
        return dict(zip(("prepare_ms", "pass_a_ms", "thresholds_ms", "pass_b_ms", "pass_c_ms"), (float(v) for v in t)))

    def screen_values(self, qn, n_rows, shape=0):
        """mh_screen_values: [Q][n_rows] screen values as the matrix pipe computes them, + (dmax, spread) of the DB.
        shape: 0 = the MFMA shape the large launches use, 1 = 32x32x16, 2 = 16x16x32."""
        qn = np.ascontiguousarray(qn, np.float32)
        out = np.zeros((qn.shape[0], n_rows), np.float32)
        dmax, spread = C.c_float(0), C.c_float(0)
        self._ck(self.L.mh_screen_values(self.h, _ptr(qn), qn.shape[0], n_rows, _ptr(out), C.byref(dmax), C.byref(spread),
                                         int(shape)), "mh_screen_values")
        return out, dmax.value, spread.value

    def screen_sample_values(self, qn, row0):
        """mh_screen_sample_values: [Q][2][8] -- for query q the screen values of the 8 rows of the lane blocks row0[q][0]
        and row0[q][1] (bit b = row row0 + (b & 3) + 16 (b >> 2)), from the code pass C names a sampled record's rows with."""
        qn = np.ascontiguousarray(qn, np.float32)
        row0 = np.ascontiguousarray(row0, np.int32)
        assert row0.shape == (qn.shape[0], 2)
        out = np.zeros((qn.shape[0], 2, 8), np.float32)
        self._ck(self.L.mh_screen_sample_values(self.h, _ptr(qn), qn.shape[0], _ptr(row0), _ptr(out)), "mh_screen_sample_values")
        return out

    def match_set_mode(self, mode: int):
        """-1 auto, 0 exact f32 kernels only, 1 two-stage (f16 screen + exact rescoring) whenever possible,
        2 / 3 the exact VALU / f32 matrix-pipe kernel whatever the query count."""
        self._ck(self.L.mh_match_set_mode(self.h, int(mode)), "mh_match_set_mode")

    def pose_set_split(self, on: bool):
        """POSE of the frame paths as two launches (hypotheses, then one-wavefront refines; the default) or as one."""
        self._ck(self.L.mh_pose_set_split(self.h, int(bool(on))), "mh_pose_set_split")

    def match_kernel_launches(self) -> dict:
        """MATCH launch sequences of this context by the kernel that searched (mh_match_launches)."""
        o = np.zeros(3, np.uint32)
        self._ck(self.L.mh_match_launches(self.h, _ptr(o)), "mh_match_launches")
        return {"valu": int(o[0]), "mfma": int(o[1]), "screen": int(o[2])}

    def match_stats(self, Q=0, reset=False) -> dict:
        """Two-stage MATCH statistics since the last reset + which path Q queries would take."""
        st = np.zeros(4, np.uint32)
        self._ck(self.L.mh_match_stats(self.h, int(Q), _ptr(st), int(reset)), "mh_match_stats")
        return {"candidates": int(st[0]), "brute_force_queries": int(st[1]), "queries": int(st[2]),
                "two_stage": bool(st[3])}

    def match_query_candidates(self, Q):
        """mh_match_query_candidates: per query, the rows that ran pass C's canonical chain since the last match_stats reset."""
        out = np.zeros(int(Q), np.uint32)
        self._ck(self.L.mh_match_query_candidates(self.h, int(Q), _ptr(out)), "mh_match_query_candidates")
        return out

    def match_incomplete(self, reset=False) -> int:
        """Queries since the last reset whose sampled-tile records were incomplete and that took pass C's bounded
        sweep of a lane slot's rows instead (mh_match_incomplete)."""
        n = C.c_uint32(0)
        self._ck(self.L.mh_match_incomplete(self.h, C.byref(n), int(reset)), "mh_match_incomplete")
        return int(n.value)

    def match_set_accept(self, ratio: float):
        """mh_match_set_accept: 0 = the default (resident frames hand MATCH their ratio, match() gets every exact triple);
        r > 0 = match() hands it r as well, so that the raw triple of a query r rejects may read (-1, inf, inf);
        -1 = nobody does (frames included)."""
        self._ck(self.L.mh_match_set_accept(self.h, float(ratio)), "mh_match_set_accept")

    def match_prerejected(self, reset=False) -> int:
        """Queries since the last reset that pass C answered (-1, inf, inf) because their records proved that the
        ratio test rejects them (mh_match_prerejected)."""
        n = C.c_uint32(0)
        self._ck(self.L.mh_match_prerejected(self.h, C.byref(n), int(reset)), "mh_match_prerejected")
        return int(n.value)

    def normalize(self, desc):
        d = np.ascontiguousarray(desc, np.float32).copy()
        self._ck(self.L.mh_normalize(self.h, _ptr(d), d.shape[0]), "mh_normalize")
        return d

    def match(self, q, ratio=0.8):
        q = np.ascontiguousarray(q, np.float32)
        Q = q.shape[0]
        acc = np.full(Q, -1, np.int32)
        raw = np.full(Q, -1, np.int32)
        d1 = np.zeros(Q, np.float32)
        d2 = np.zeros(Q, np.float32)
        self._ck(self.L.mh_match(self.h, _ptr(q), Q, ratio, _ptr(acc), _ptr(raw), _ptr(d1), _ptr(d2)), "mh_match")
        return acc, raw, d1, d2

    def normalize_match(self, q, ratio=0.8):
        """mh_normalize + mh_match in one call: -> (normalised copy of q, acc, raw, d1, d2)."""
        q = np.ascontiguousarray(q, np.float32).copy()
        Q = q.shape[0]
        acc = np.full(Q, -1, np.int32)
        raw = np.full(Q, -1, np.int32)
        d1 = np.zeros(Q, np.float32)
        d2 = np.zeros(Q, np.float32)
        self._ck(self.L.mh_normalize_match(self.h, _ptr(q), Q, ratio, _ptr(acc), _ptr(raw), _ptr(d1), _ptr(d2)),
                 "mh_normalize_match")
        return q, acc, raw, d1, d2

    # ---- CLUSTER ----
    def meanshift(self, pts, radius=200.0, merge=20.0, min_pts=7, max_iter=100):
        pts = np.ascontiguousarray(pts, np.float32)
        n = pts.shape[0]
        dim = pts.shape[1] if pts.ndim == 2 else 2
        label = np.full(max(n, 1), -1, np.int32)
        order = np.full(max(n, 1), -1, np.int32)
        ncl = C.c_int32(0)
        self._ck(self.L.mh_meanshift(self.h, _ptr(pts), n, dim, radius, merge, min_pts, max_iter,
                                     _ptr(label), _ptr(order), C.byref(ncl)), "mh_meanshift")
        label = label[:n]
        clusters, pos = [], 0
        for c in range(ncl.value):
            sz = int((label == c).sum())
            clusters.append(order[pos:pos + sz].copy())
            pos += sz
        return clusters, label

    def meanshift_batch(self, problems, radius=200.0, merge=20.0, min_pts=7, max_iter=100):
        """problems: list of [n_p, dim] point arrays (same dim) -> list of (clusters, label) like meanshift()."""
        dim = 2
        for p in problems:
            if np.asarray(p).ndim == 2 and np.asarray(p).shape[0]:
                dim = np.asarray(p).shape[1]
        sizes = [int(np.asarray(p).shape[0]) for p in problems]
        off = np.zeros(len(problems) + 1, np.int32)
        off[1:] = np.cumsum(sizes)
        total = int(off[-1])
        pts = (np.concatenate([np.asarray(p, np.float32).reshape(-1, dim) for p in problems])
               if total else np.zeros((0, dim), np.float32))
        pts = np.ascontiguousarray(pts, np.float32)
        label = np.full(max(total, 1), -1, np.int32)
        order = np.full(max(total, 1), -1, np.int32)
        ncl = np.zeros(max(len(problems), 1), np.int32)
        self._ck(self.L.mh_meanshift_batch(self.h, _ptr(pts), _ptr(off), len(problems), dim, radius, merge,
                                           min_pts, max_iter, _ptr(label), _ptr(order), _ptr(ncl)),
                 "mh_meanshift_batch")
        out = []
        for i in range(len(problems)):
            b, e = int(off[i]), int(off[i + 1])
            lab, ordr = label[b:e], order[b:e]
            clusters, pos = [], 0
            for c in range(int(ncl[i])):
                sz = int((lab == c).sum())
                clusters.append(ordr[pos:pos + sz].copy())
                pos += sz
            out.append((clusters, lab.copy()))
        return out

    # ---- POSE ----
    def pose_ransac(self, corr, cluster_off, K, cam, params: mh_pose_params, seed=1):
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        cluster_off = np.ascontiguousarray(cluster_off, np.int32)
        ncl = len(cluster_off) - 1
        R = max(params.max_objects_per_cluster, 1)
        out = np.zeros(max(ncl * R, 1), POSE_OUT_DTYPE)
        n_out = C.c_int32(0)
        c = make_cam(K, cam)
        self._ck(self.L.mh_pose_ransac(self.h, _ptr(corr), _ptr(cluster_off), ncl, C.byref(c),
                                       C.byref(params), seed, _ptr(out), C.byref(n_out)), "mh_pose_ransac")
        return out[:n_out.value].copy()

    def pose_ransac_images(self, corr, image_of, cluster_off, Ks, cams, params: mh_pose_params, seed=1):
        """pose_ransac with every correspondence in its own image (Ks [n,4], cams [n,7])."""
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        image_of = np.ascontiguousarray(image_of, np.int32)
        cluster_off = np.ascontiguousarray(cluster_off, np.int32)
        ncl = len(cluster_off) - 1
        R = max(params.max_objects_per_cluster, 1)
        out = np.zeros(max(ncl * R, 1), POSE_OUT_DTYPE)
        n_out = C.c_int32(0)
        arr = make_cams(Ks, cams)
        self._ck(self.L.mh_pose_ransac_images(self.h, _ptr(corr), _ptr(image_of), _ptr(cluster_off), ncl, arr, len(Ks),
                                              C.byref(params), seed, _ptr(out), C.byref(n_out)), "mh_pose_ransac_images")
        return out[:n_out.value].copy()

    def frame_set_images(self, q_image_ptr, Ks=None, cams=None):
        """Frames with several images: q_image_ptr = device int32[Q] (image of every query); 0 / None: one image again."""
        if not q_image_ptr or Ks is None or len(Ks) <= 1:
            self._ck(self.L.mh_frame_set_images(self.h, None, None, 1), "mh_frame_set_images")
            return
        arr = make_cams(Ks, cams)
        self._ck(self.L.mh_frame_set_images(self.h, C.c_void_p(q_image_ptr), arr, len(Ks)), "mh_frame_set_images")

    def pose_ransac_depth(self, corr, depth, cluster_off, K, cam, params: mh_pose_params, kind, alpha=0.5, seed=1):
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        depth = np.ascontiguousarray(depth, DEPTH_DTYPE)
        cluster_off = np.ascontiguousarray(cluster_off, np.int32)
        ncl = len(cluster_off) - 1
        R = max(params.max_objects_per_cluster, 1)
        out = np.zeros(max(ncl * R, 1), POSE_OUT_DTYPE)
        n_out = C.c_int32(0)
        c = make_cam(K, cam)
        self._ck(self.L.mh_pose_ransac_depth(self.h, _ptr(corr), _ptr(depth), _ptr(cluster_off), ncl, C.byref(c),
                                             C.byref(params), kind, alpha, seed, _ptr(out), C.byref(n_out)),
                 "mh_pose_ransac_depth")
        return out[:n_out.value].copy()

    def frame_set_depth(self, q_depth_ptr, kind, alpha=0.5):
        self._ck(self.L.mh_frame_set_depth(self.h, C.c_void_p(q_depth_ptr) if q_depth_ptr else None, kind, alpha),
                 "mh_frame_set_depth")

    def frame_set_depth_image(self, depth_ptr, fill_ptr, width, height, kind, alpha=0.5, cauchy_scale=0.1):
        self._ck(self.L.mh_frame_set_depth_image(self.h, C.c_void_p(depth_ptr) if depth_ptr else None,
                                                 C.c_void_p(fill_ptr) if fill_ptr else None, width, height, kind,
                                                 alpha, cauchy_scale), "mh_frame_set_depth_image")

    def depth_fill_dev(self, depth_ptr, width, height, K, fill_ptr, scale=8, bilinear=False):
        """moped3d's DEPTHFILL on a device depth map [h, w, 4], in place, + its distance map [h, w]; asynchronous.
        -> the scale factor used."""
        k = np.ascontiguousarray(K, np.float32)
        used = C.c_int(0)
        self._ck(self.L.mh_depth_fill(self.h, C.c_void_p(depth_ptr), width, height, int(scale), 1 if bilinear else 0,
                                      _ptr(k), C.c_void_p(fill_ptr), C.byref(used)), "mh_depth_fill")
        return used.value

    def depth_fill_batch_dev(self, depth_ptrs, fill_ptrs, width, height, K, scale=8, bilinear=False):
        """DEPTHFILL of len(depth_ptrs) device maps of one size, each in place with its own distance map: one launch per
        stage for all of them; asynchronous (depth_fill_status reports a ring overflow of any of them)."""
        n = len(depth_ptrs)
        if len(fill_ptrs) != n:
            raise ValueError("one distance map per depth map")
        k = np.ascontiguousarray(K, np.float32)
        d = (C.c_void_p * max(n, 1))(*depth_ptrs)
        f = (C.c_void_p * max(n, 1))(*fill_ptrs)
        self._ck(self.L.mh_depth_fill_batch(self.h, d, f, n, width, height, int(scale), 1 if bilinear else 0, _ptr(k)),
                 "mh_depth_fill_batch")

    def depth_fill_set_mode(self, mode: int):
        """DEPTH_FILL_REPLAY (0, the default: one wavefront replays the queue; downscaled maps of up to 8192 pixels) or
        DEPTH_FILL_LEVELS (1: the queue generation by generation, the same bytes, downscaled maps of up to 2^21 pixels)."""
        self._ck(self.L.mh_depth_fill_set_mode(self.h, int(mode)), "mh_depth_fill_set_mode")

    def depth_fill_get_mode(self) -> int:
        mode = C.c_int(0)
        self._ck(self.L.mh_depth_fill_get_mode(self.h, C.byref(mode)), "mh_depth_fill_get_mode")
        return mode.value

    def depth_fill_stats(self, frame=0):
        """Of frame `frame` of the last fill (a DEPTH_FILL_LEVELS one): -> (non-empty generations, largest generation,
        elements over all generations, overflowed).  Synchronises the context."""
        out = np.zeros(4, np.int32)
        self._ck(self.L.mh_depth_fill_stats(self.h, int(frame), _ptr(out)), "mh_depth_fill_stats")
        return tuple(int(v) for v in out)

    def depth_fill_status(self):
        self._ck(self.L.mh_depth_fill_status(self.h), "mh_depth_fill_status")

    def depth_fill(self, depth_img, K, scale=8, bilinear=False):
        """The same on a host map: -> (filled copy [h, w, 4], distance map [h, w], scale used)."""
        d = np.ascontiguousarray(depth_img, np.float32).copy()
        h, w = d.shape[:2]
        dist = np.zeros((h, w), np.float32)
        k = np.ascontiguousarray(K, np.float32)
        used = C.c_int(0)
        self._ck(self.L.mh_depth_fill_host(self.h, _ptr(d), w, h, int(scale), 1 if bilinear else 0, _ptr(k), _ptr(dist),
                                           C.byref(used)), "mh_depth_fill_host")
        return d, dist, used.value

    # ---- the depth map from raw sensor depth (moped3d/moped3d.cpp:279-333) ----
    def depth_map_from_raw_dev(self, raw_ptr, raw: mh_raw_depth, K, depth_ptr, width, height):
        """A device buffer of raw sensor depth (make_raw_depth) -> the device map [height, width, 4]; asynchronous."""
        k = np.ascontiguousarray(K, np.float32)
        self._ck(self.L.mh_depth_map_from_raw_dev(self.h, C.c_void_p(raw_ptr) if raw_ptr else None, C.byref(raw), _ptr(k),
                                                  C.c_void_p(depth_ptr) if depth_ptr else None, width, height),
                 "mh_depth_map_from_raw_dev")

    def depth_map_from_raw_batch_dev(self, raw_ptrs, raw: mh_raw_depth, K, depth_ptrs, width, height):
        """len(raw_ptrs) raw buffers of one description -> a map each, one launch; asynchronous."""
        n = len(raw_ptrs)
        if len(depth_ptrs) != n:
            raise ValueError("one map per raw buffer")
        k = np.ascontiguousarray(K, np.float32)
        r = (C.c_void_p * max(n, 1))(*raw_ptrs)
        d = (C.c_void_p * max(n, 1))(*depth_ptrs)
        self._ck(self.L.mh_depth_map_from_raw_batch_dev(self.h, r, C.byref(raw), _ptr(k), d, n, width, height),
                 "mh_depth_map_from_raw_batch_dev")

    def depth_map_from_raw(self, raw_buf, raw: mh_raw_depth, K, width, height):
        """The same on a host buffer (any contiguous array holding the bytes `raw` describes) -> the map [height, width, 4]."""
        b = np.ascontiguousarray(raw_buf)
        k = np.ascontiguousarray(K, np.float32)
        out = np.zeros((height, width, 4), np.float32)
        self._ck(self.L.mh_depth_map_from_raw_host(self.h, _ptr(b), C.byref(raw), _ptr(k), _ptr(out), width, height),
                 "mh_depth_map_from_raw_host")
        return out

    # ---- the gray image from what a camera delivers (moped3d/moped3d.cpp:249) ----
    def image_gray_dev(self, raw_ptr, fmt: mh_raw_image, gray_ptr):
        """A device buffer as `fmt` (make_raw_image) describes it -> the packed device gray image [height, width];
        asynchronous."""
        self._ck(self.L.mh_image_gray_dev(self.h, C.c_void_p(raw_ptr) if raw_ptr else None,
                                          C.byref(fmt) if fmt is not None else None,
                                          C.c_void_p(gray_ptr) if gray_ptr else None), "mh_image_gray_dev")

    def image_gray_batch_dev(self, raw_ptrs, fmt: mh_raw_image, gray_ptrs):
        """len(raw_ptrs) raw buffers of one description -> a gray image each, one launch; asynchronous."""
        n = len(raw_ptrs)
        if len(gray_ptrs) != n:
            raise ValueError("one gray image per raw buffer")
        r = (C.c_void_p * max(n, 1))(*raw_ptrs)
        g = (C.c_void_p * max(n, 1))(*gray_ptrs)
        self._ck(self.L.mh_image_gray_batch_dev(self.h, r, C.byref(fmt) if fmt is not None else None, g, n),
                 "mh_image_gray_batch_dev")

    def image_gray(self, raw_buf, fmt: mh_raw_image):
        """The same on a host buffer (any contiguous array holding the bytes `fmt` describes) -> gray [height, width]."""
        b = np.ascontiguousarray(raw_buf)
        if b.nbytes < raw_image_bytes(fmt):
            raise ValueError("the buffer is shorter than the description's extent")
        out = np.zeros((max(fmt.height, 0), max(fmt.width, 0)), np.uint8)
        self._ck(self.L.mh_image_gray_host(self.h, _ptr(b), C.byref(fmt), _ptr(out)), "mh_image_gray_host")
        return out

    def frame_set_image_format(self, fmt):
        """The image pointers of frame_enqueue_image[_batch] / frame_enqueue_images[_batch] (and the gray arrays of
        frame_run_kinect[_raw]_host) are raw buffers as `fmt` (make_raw_image) describes them from now on: converted by
        one launch per call in front of undistortion and FEAT.  None = packed 8-bit gray, the default."""
        self._ck(self.L.mh_frame_set_image_format(self.h, C.byref(fmt) if fmt is not None else None),
                 "mh_frame_set_image_format")
        self._image_fmt = None if fmt is None else mh_raw_image(fmt.format, fmt.width, fmt.height, fmt.row_stride, fmt.offset)

    def _host_image(self, gray, size):
        """The `gray` argument of frame_run_kinect[_raw]_host -> (contiguous uint8 array, w, h).  While a format is set the
        array is the camera's buffer: it must hold the format's extent, which is what the library copies from it."""
        g = np.ascontiguousarray(gray, np.uint8)
        fmt = getattr(self, "_image_fmt", None)
        if fmt is None:
            w, h = size if size is not None else g.shape[::-1]
            if g.size != w * h:
                raise ValueError("gray must hold width x height bytes")
            return g, w, h
        if g.nbytes < raw_image_bytes(fmt):
            raise ValueError("the buffer is shorter than the extent of the image format that is set")
        w, h = size if size is not None else (fmt.width, fmt.height)
        return g, w, h

    def frame_set_depth_image_batch(self, depth_ptrs, fill_ptrs, width, height, kind, alpha=0.5, cauchy_scale=0.1):
        """One depth map (+ distance map, or None for all) per frame of the following batches."""
        n = len(depth_ptrs)
        d = (C.c_void_p * n)(*depth_ptrs)
        f = (C.c_void_p * n)(*fill_ptrs) if fill_ptrs else None
        self._ck(self.L.mh_frame_set_depth_image_batch(self.h, d, f, n, width, height, kind, alpha, cauchy_scale),
                 "mh_frame_set_depth_image_batch")

    # ---- FEAT ----
    def sift(self, gray, double_size=True, cap=16384):
        """-> (xy [n,2] = (col,row), scale_ori [n,2], desc [n,128]) in the reference's list order."""
        g = np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        xy = np.zeros((cap, 2), np.float32)
        so = np.zeros((cap, 2), np.float32)
        d = np.zeros((cap, 128), np.float32)
        n = C.c_int32(0)
        self._ck(self.L.mh_sift_extract(self.h, _ptr(g), w, h, int(double_size), _ptr(xy), _ptr(so), _ptr(d), cap,
                                        C.byref(n)), "mh_sift_extract")
        return xy[:n.value].copy(), so[:n.value].copy(), d[:n.value].copy()

    def sift_dev(self, gray_ptr, w, h, double_size, desc_ptr, xy_ptr, scale_ori_ptr, cap, n_ptr):
        self._ck(self.L.mh_sift_extract_dev(self.h, C.c_void_p(gray_ptr), w, h, int(double_size), C.c_void_p(desc_ptr),
                                            C.c_void_p(xy_ptr), C.c_void_p(scale_ori_ptr) if scale_ori_ptr else None,
                                            cap, C.c_void_p(n_ptr)), "mh_sift_extract_dev")

    def sift_batch_dev(self, gray_ptrs, w, h, double_size, desc_ptr, xy_ptr, cap, counts_ptr):
        """FEAT alone on len(gray_ptrs) device images of one size, one launch per stage; asynchronous."""
        n = len(gray_ptrs)
        g = (C.c_void_p * n)(*gray_ptrs)
        self._ck(self.L.mh_sift_extract_batch_dev(self.h, g, n, w, h, int(double_size), C.c_void_p(desc_ptr),
                                                  C.c_void_p(xy_ptr), cap, C.c_void_p(counts_ptr)),
                 "mh_sift_extract_batch_dev")

    # the stages of the last extraction, for verification (mh_sift_debug_*)
    def sift_debug_plan(self):
        """-> (image slots of the last launch, [(rows, cols)] per octave)."""
        ni, no = C.c_int32(0), C.c_int32(0)
        rows, cols = np.zeros(SIFT_MAX_OCTAVES, np.int32), np.zeros(SIFT_MAX_OCTAVES, np.int32)
        self._ck(self.L.mh_sift_debug_plan(self.h, C.addressof(ni), C.addressof(no), _ptr(rows), _ptr(cols)),
                 "mh_sift_debug_plan")
        return ni.value, [(int(rows[o]), int(cols[o])) for o in range(no.value)]

    def sift_debug_level(self, octave, kind, level, shape, slot=0):
        """Gaussian (kind 0) / DoG (kind 1) level 0..4 of `octave` -> float32 [rows, cols] (shape from sift_debug_plan)."""
        out = np.zeros(shape, np.float32)
        self._ck(self.L.mh_sift_debug_level(self.h, slot, octave, kind, level, _ptr(out)), "mh_sift_debug_level")
        return out

    def sift_debug_candidates(self, slot=0, cap=65536):
        """-> (candidates [n] SIFT_CANDIDATE_DTYPE in the kernel's (any) order, won [n] bool)."""
        out = np.zeros(cap, SIFT_CANDIDATE_DTYPE)
        won = np.zeros(cap, np.uint8)
        n = C.c_int32(0)
        self._ck(self.L.mh_sift_debug_candidates(self.h, slot, _ptr(out), _ptr(won), cap, C.byref(n)),
                 "mh_sift_debug_candidates")
        if n.value > cap:
            raise MhError(f"mh_sift_debug_candidates: {n.value} candidates, room for {cap}")
        return out[:n.value].copy(), won[:n.value].astype(bool)

    def sift_debug_keys(self, slot=0, cap=16384):
        """-> keys [n] SIFT_KEY_DTYPE in the kernel's (any) order."""
        out = np.zeros(cap, SIFT_KEY_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_sift_debug_keys(self.h, slot, _ptr(out), cap, C.byref(n)), "mh_sift_debug_keys")
        if n.value > cap:
            raise MhError(f"mh_sift_debug_keys: {n.value} keys, room for {cap}")
        return out[:n.value].copy()

    def sift_debug_describe(self, keys, workgroups=0, slot=0):
        """The shipped descriptor kernel alone on `keys` (SIFT_KEY_DTYPE, distinct `order`) over the pyramid the last
        extraction left in `slot`, on `workgroups` workgroups (0: production's 4 096) -> (xy [n,2], scale_ori [n,2], desc
        [n,128]); place i = the key with i keys of larger order.  The context's own keys and outputs stay untouched."""
        k = np.ascontiguousarray(keys, SIFT_KEY_DTYPE)
        n = len(k)
        xy = np.zeros((n, 2), np.float32)
        so = np.zeros((n, 2), np.float32)
        d = np.zeros((n, 128), np.float32)
        self._ck(self.L.mh_sift_debug_describe(self.h, slot, _ptr(k), n, workgroups, _ptr(d), _ptr(xy), _ptr(so)),
                 "mh_sift_debug_describe")
        return xy, so, d

    def sift_debug_blur(self, variant, src, sigma, half=False, want_dog=True, want_half=False):
        """One blur level of a float32 image through kernel `variant` (mh_sift_debug_blur) -> (dst, dog or None,
        half-size copy or None).  A variant that cannot take the arguments raises MhError."""
        a = np.ascontiguousarray(src, np.float32)
        shape = (a.shape[0] >> 1, a.shape[1] >> 1) if half else a.shape
        dst = np.zeros(shape, np.float32)
        dog = np.zeros(shape, np.float32) if want_dog else None
        hd = np.zeros(shape, np.float32) if want_half else None
        self._ck(self.L.mh_sift_debug_blur(self.h, variant, _ptr(a), a.shape[0], a.shape[1], sigma, int(half), _ptr(dst),
                                           _ptr(dog) if want_dog else None, _ptr(hd) if want_half else None),
                 "mh_sift_debug_blur")
        return dst, dog, hd

    # ---- UNDISTORTED_IMAGE (UTIL_UNDISTORT) ----
    def undistort(self, gray, K, dist):
        """-> the 8-bit image undistorted as UTIL_UNDISTORT::process leaves it (K = fx, fy, cx, cy; dist = k1, k2, p1, p2)."""
        g = np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        out = np.empty_like(g)
        k, d = _calib(K), _calib(dist)
        self._ck(self.L.mh_undistort(self.h, _ptr(g), _ptr(out), w, h, _ptr(k), _ptr(d)), "mh_undistort")
        return out

    def undistort_dev(self, src_ptr, dst_ptr, w, h, K, dist):
        """The same on device images (dst != src), stream-ordered."""
        k, d = _calib(K), _calib(dist)
        self._ck(self.L.mh_undistort_dev(self.h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), w, h, _ptr(k), _ptr(d)),
                 "mh_undistort_dev")

    def undistort_map(self, w, h, K, dist):
        """-> (mapx, mapy) float32 [h, w]: the maps UTIL_UNDISTORT::init builds."""
        mx = np.empty((h, w), np.float32)
        my = np.empty((h, w), np.float32)
        k, d = _calib(K), _calib(dist)
        self._ck(self.L.mh_undistort_map(self.h, w, h, _ptr(k), _ptr(d), _ptr(mx), _ptr(my)), "mh_undistort_map")
        return mx, my

    def frame_set_undistort(self, dist):
        """Undistort the images of frame_enqueue_image[_batch] with the frame camera's K and these k1, k2, p1, p2
        before FEAT; None = off."""
        d = None if dist is None else _calib(dist)
        self._ck(self.L.mh_frame_set_undistort(self.h, None if d is None else _ptr(d)), "mh_frame_set_undistort")

    def project_test(self, pose7, corr, K, cam, thr):
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        n = corr.shape[0]
        inl = np.zeros(max(n, 1), np.uint8)
        e2 = np.zeros(max(n, 1), np.float32)
        cnt = C.c_int32(0)
        p = np.ascontiguousarray(pose7, np.float32)
        c = make_cam(K, cam)
        self._ck(self.L.mh_project_test(self.h, _ptr(p), _ptr(corr), n, C.byref(c), thr, _ptr(inl),
                                        _ptr(e2), C.byref(cnt)), "mh_project_test")
        return cnt.value, inl[:n].astype(bool), e2[:n]

    def pose_debug_rows(self, kind, res, phase, alpha, R, t, cams, pts, lst):
        """The LM refine's residual rows, Jacobians, cost and normal equations at pose (R [3,3], t [3]) as the shipped device
        functions compute them (mh_pose_debug_rows).  cams: [(K, cam7), ...]; pts: the kernel's own layout, float32 words
        [n_pts, POSE_POINT_STRIDE[kind]]; lst: point indices.  -> dict of nrows [n], r [n,4], J [n,4,6] (uint32 words:
        rows a model does not have hold POSE_DEBUG_FILL), cost, H [21], g [6] (uint32 words) and devcams [n_images,16]
        (K, Rc, tc as the kernels got them)."""
        R = np.ascontiguousarray(R, np.float32).reshape(9)
        t = np.ascontiguousarray(t, np.float32).reshape(3)
        pts = np.ascontiguousarray(pts, np.float32)
        lst = np.ascontiguousarray(lst, np.int32)
        arr = (mh_cam * max(len(cams), 1))(*[make_cam(K, cam) for K, cam in cams])
        n = len(lst)
        nrows = np.zeros(n, np.int32)
        r = np.zeros((n, 4), np.uint32)
        J = np.zeros((n, 4, 6), np.uint32)
        sums = np.zeros(28, np.uint32)
        dc = np.zeros((len(cams), 16), np.float32)
        self._ck(self.L.mh_pose_debug_rows(self.h, kind, res, phase, alpha, _ptr(R), _ptr(t), C.cast(arr, C.c_void_p), len(cams),
                                           _ptr(pts), len(pts), _ptr(lst), n, _ptr(nrows), _ptr(r), _ptr(J), _ptr(sums),
                                           _ptr(sums[1:]), _ptr(sums[22:]), _ptr(dc)), "mh_pose_debug_rows")
        return dict(nrows=nrows, r=r, J=J, cost=sums[0], H=sums[1:22].copy(), g=sums[22:28].copy(), devcams=dc)

    def pose_debug_step(self, H, g, mu, R, t):
        """One LM step's linear algebra on the device (mh_pose_debug_step): solve6(H [21], g [6], mu), rotate_left(dx, R),
        t + dx[3:] -> (solved, dx [6], Rn [3,3], tn [3], lanes_agree); without a solution the floats hold
        POSE_DEBUG_FILL."""
        H = np.ascontiguousarray(H, np.float32).reshape(21)
        g = np.ascontiguousarray(g, np.float32).reshape(6)
        R = np.ascontiguousarray(R, np.float32).reshape(9)
        t = np.ascontiguousarray(t, np.float32).reshape(3)
        dx, Rn, tn = np.zeros(6, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
        ok, agree = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.mh_pose_debug_step(self.h, _ptr(H), _ptr(g), mu, _ptr(R), _ptr(t), C.byref(ok), _ptr(dx), _ptr(Rn),
                                           _ptr(tn), C.byref(agree)), "mh_pose_debug_step")
        return bool(ok.value), dx, Rn.reshape(3, 3), tn, bool(agree.value)

    # ---- FILTER ----
    def filter(self, corr, model_off, obj_model, obj_pose, K, cam, min_points, feature_distance, min_score):
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        model_off = np.ascontiguousarray(model_off, np.int32)
        obj_model = np.ascontiguousarray(obj_model, np.int32)
        obj_pose = np.ascontiguousarray(obj_pose, np.float32)
        n_obj = obj_model.shape[0]
        M = corr.shape[0]
        score = np.zeros(max(n_obj, 1), np.float32)
        keep = np.zeros(max(n_obj, 1), np.uint8)
        order = np.zeros(max(n_obj, 1), np.int32)
        members = np.zeros(max(M, 1), np.int32)
        off = np.zeros(n_obj + 2, np.int32)
        kept = C.c_int32(0)
        c = make_cam(K, cam)
        self._ck(self.L.mh_filter(self.h, _ptr(corr), _ptr(model_off), len(model_off) - 1, _ptr(obj_model),
                                  _ptr(obj_pose), n_obj, C.byref(c), min_points, feature_distance,
                                  min_score, _ptr(score), _ptr(keep), _ptr(order), _ptr(members),
                                  _ptr(off), C.byref(kept)), "mh_filter")
        k = kept.value
        clusters = [members[off[i]:off[i + 1]].copy() for i in range(k)]
        return score[:n_obj], keep[:n_obj].astype(bool), order[:k].copy(), clusters

    def filter_images(self, corr, image_of, model_off, obj_model, obj_pose, Ks, cams, min_points, feature_distance,
                      min_score):
        """filter() for matches that come from several images (image_of[i] = image of match i)."""
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        image_of = np.ascontiguousarray(image_of, np.int32)
        model_off = np.ascontiguousarray(model_off, np.int32)
        obj_model = np.ascontiguousarray(obj_model, np.int32)
        obj_pose = np.ascontiguousarray(obj_pose, np.float32)
        n_obj = obj_model.shape[0]
        M = corr.shape[0]
        score = np.zeros(max(n_obj, 1), np.float32)
        keep = np.zeros(max(n_obj, 1), np.uint8)
        order = np.zeros(max(n_obj, 1), np.int32)
        members = np.zeros(max(M, 1), np.int32)
        off = np.zeros(n_obj + 2, np.int32)
        kept = C.c_int32(0)
        arr = make_cams(Ks, cams)
        self._ck(self.L.mh_filter_images(self.h, _ptr(corr), _ptr(image_of), _ptr(model_off), len(model_off) - 1,
                                         _ptr(obj_model), _ptr(obj_pose), n_obj, arr, len(Ks), min_points,
                                         feature_distance, min_score, _ptr(score), _ptr(keep), _ptr(order),
                                         _ptr(members), _ptr(off), C.byref(kept)), "mh_filter_images")
        k = kept.value
        clusters = [members[off[i]:off[i + 1]].copy() for i in range(k)]
        return score[:n_obj], keep[:n_obj].astype(bool), order[:k].copy(), clusters

    # ---- FILTER, depth class (moped3d FILTER_PROJECTION_DEPTH_CPU) ----
    def filter_depth_set_points(self, points_xyz, points_off):
        """The models' test points: points_xyz [total, 3], points_off [n_models + 1] (model m's slice in the order the
        reference walks TestPoints[m]).  None / an empty offset list clears them.  To be set again after a DB edit."""
        if points_off is None or len(points_off) <= 1:
            self._ck(self.L.mh_filter_depth_set_points(self.h, None, None, 0), "mh_filter_depth_set_points")
            return
        off = np.ascontiguousarray(points_off, np.int32)
        xyz = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        if off[-1] != len(xyz):
            raise ValueError("points_off[-1] is not the number of points")
        self._ck(self.L.mh_filter_depth_set_points(self.h, _ptr(xyz), _ptr(off), len(off) - 1), "mh_filter_depth_set_points")

    def filter_depth(self, corr, model_off, obj_model, obj_pose, K, cam, min_points, feature_distance, min_score,
                     depth_K, depth_cam, params):
        """filter() of the depth class on the depth map the context holds (frame_set_depth_image[_host]) -> (score, keep,
        order, clusters, incorrect_score, used, plausible); params: (PlausibleSqDistance, DepthFraction,
        MinKeypointFraction)."""
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        model_off = np.ascontiguousarray(model_off, np.int32)
        obj_model = np.ascontiguousarray(obj_model, np.int32)
        obj_pose = np.ascontiguousarray(obj_pose, np.float32)
        n_obj = obj_model.shape[0]
        M = corr.shape[0]
        score = np.zeros(max(n_obj, 1), np.float32)
        keep = np.zeros(max(n_obj, 1), np.uint8)
        order = np.zeros(max(n_obj, 1), np.int32)
        members = np.zeros(max(M, 1), np.int32)
        off = np.zeros(n_obj + 2, np.int32)
        inc = np.zeros(max(n_obj, 1), np.float32)
        used = np.zeros(max(n_obj, 1), np.int32)
        plausible = np.zeros(max(n_obj, 1), np.int32)
        kept = C.c_int32(0)
        c, dc = make_cam(K, cam), make_cam(depth_K, depth_cam)
        prm = make_filter_depth_params(params)
        self._ck(self.L.mh_filter_depth(self.h, _ptr(corr), _ptr(model_off), len(model_off) - 1, _ptr(obj_model),
                                        _ptr(obj_pose), n_obj, C.byref(c), min_points, feature_distance, min_score,
                                        C.byref(dc), C.byref(prm), _ptr(score), _ptr(keep), _ptr(order), _ptr(members),
                                        _ptr(off), C.byref(kept), _ptr(inc), _ptr(used), _ptr(plausible)), "mh_filter_depth")
        k = kept.value
        clusters = [members[off[i]:off[i + 1]].copy() for i in range(k)]
        return (score[:n_obj], keep[:n_obj].astype(bool), order[:k].copy(), clusters, inc[:n_obj], used[:n_obj],
                plausible[:n_obj])

    def frame_set_depth_image_host(self, depth_img, fill_img, kind=DEPTH_BACKPROJECTION, alpha=0.5, cauchy_scale=0.1):
        """The frame's depth map [h, w, 4] (+ fill-distance map [h, w] or None) from host arrays, copied into the
        context; depth_img None: no map."""
        if depth_img is None:
            self._ck(self.L.mh_frame_set_depth_image_host(self.h, None, None, 0, 0, 0, alpha, cauchy_scale),
                     "mh_frame_set_depth_image_host")
            return
        d = np.ascontiguousarray(depth_img, np.float32)
        h, w = d.shape[:2]
        f = None if fill_img is None else np.ascontiguousarray(fill_img, np.float32).reshape(h, w)
        self._ck(self.L.mh_frame_set_depth_image_host(self.h, _ptr(d), _ptr(f), w, h, kind, alpha, cauchy_scale),
                 "mh_frame_set_depth_image_host")

    def depth_filter(self, depth_img, K, patch_size, density, uv, group_off=None):
        """moped3d's DEPTHFILTER on the caller's points uv [n, 2]: keep [n] bool.  group_off None: one group, ToFilter = 1
        (the detected features); else [n_groups + 1], ToFilter = 2 (every model's matches counted by themselves).
        depth_img [h, w, 4], or None = the map the context holds (frame_set_depth_image[_host])."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = len(uv)
        off = np.ascontiguousarray(group_off if group_off is not None else [0, n], np.int32)
        if off[-1] != n:
            raise ValueError("group_off must end at the number of points")
        d, h, w = None, 0, 0
        if depth_img is not None:
            d = np.ascontiguousarray(depth_img, np.float32)
            h, w = d.shape[:2]
        k = np.ascontiguousarray(K, np.float32)
        keep = np.zeros(max(n, 1), np.uint8)
        self._ck(self.L.mh_depth_filter(self.h, _ptr(d), w, h, _ptr(k), int(patch_size), float(density), _ptr(uv), _ptr(off),
                                        len(off) - 1, _ptr(keep)), "mh_depth_filter")
        return keep[:n].astype(bool)

    def depth_prop(self, depth_img, fill_img, uv) -> np.ndarray:
        """moped3d's DEPTHMAP_PROP on the caller's points uv [n, 2]: DEPTH_INFO_DTYPE [n] (Match::depthInformation).
        depth_img [h, w, 4] + fill_img [h, w] or None (fillDistance -1); depth_img None = the context's maps."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = len(uv)
        d, f, h, w = None, None, 0, 0
        if depth_img is not None:
            d = np.ascontiguousarray(depth_img, np.float32)
            h, w = d.shape[:2]
            f = None if fill_img is None else np.ascontiguousarray(fill_img, np.float32).reshape(h, w)
        out = np.zeros(max(n, 1), DEPTH_INFO_DTYPE)
        self._ck(self.L.mh_depth_prop(self.h, _ptr(d), _ptr(f), w, h, _ptr(uv), n, _ptr(out)), "mh_depth_prop")
        return out[:n]

    def frame_run_kinect_host(self, gray, depth_img, fill_img, K, cam, params: mh_frame_params, seed, fill_scale=8,
                              bilinear=False, double_size=True, max_keypoints=2048, kind=DEPTH_BACKPROJECTION, alpha=0.5,
                              cauchy_scale=0.1, max_objects=4096, size=None):
        """One Kinect frame from host arrays in one call: gray [h, w] uint8, depth_img [h, w, 4]; fill_scale 0: the maps
        arrive filled (fill_img [h, w] or None), else DEPTHFILL on the device first.  With frame_set_image_format on,
        `gray` is the camera's raw buffer (at least the format's extent) and size = (w, h), default the format's, its size.
        -> (objects, counts, the depth map and the distance map as the frame used them)."""
        g, w, h = self._host_image(gray, size)
        d = np.ascontiguousarray(depth_img, np.float32).reshape(h, w, 4).copy()
        if fill_scale:
            f = np.zeros((h, w), np.float32)
        else:
            f = None if fill_img is None else np.ascontiguousarray(fill_img, np.float32).reshape(h, w).copy()
        c = make_cam(K, cam)
        objs = np.zeros(max_objects, OBJECT_DTYPE)
        n = C.c_int32(0)
        counts = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_run_kinect_host(self.h, _ptr(g), _ptr(d), _ptr(f), w, h, 1 if double_size else 0,
                                                 int(max_keypoints), C.byref(c), C.byref(params), int(fill_scale),
                                                 1 if bilinear else 0, kind, alpha, cauchy_scale, seed, _ptr(objs),
                                                 max_objects, C.byref(n), _ptr(counts)), "mh_frame_run_kinect_host")
        return objs[:min(n.value, max_objects)].copy(), counts, d, f

    def frame_run_kinect_raw_host(self, gray, raw_buf, raw: mh_raw_depth, K, cam, params: mh_frame_params, seed,
                                  fill_scale=8, bilinear=False, double_size=True, max_keypoints=2048,
                                  kind=DEPTH_BACKPROJECTION, alpha=0.5, cauchy_scale=0.1, max_objects=4096, maps_back=True,
                                  size=None):
        """One Kinect frame from what the sensor delivers: gray [h, w] uint8 and the raw depth buffer `raw` describes; the
        map [h, w, 4] is built on the device (K), then the frame runs as frame_run_kinect_host's does.  With
        frame_set_image_format on, `gray` is the camera's raw buffer (at least the format's extent) and size = (w, h), default the format's, its size.
        -> (objects, counts, the depth map and the distance map as the frame used them; None, None without maps_back,
        and no distance map with fill_scale 0)."""
        g, w, h = self._host_image(gray, size)
        b = np.ascontiguousarray(raw_buf)
        d = np.zeros((h, w, 4), np.float32) if maps_back else None
        f = np.zeros((h, w), np.float32) if maps_back and fill_scale else None
        c = make_cam(K, cam)
        objs = np.zeros(max_objects, OBJECT_DTYPE)
        n = C.c_int32(0)
        counts = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_run_kinect_raw_host(self.h, _ptr(g), _ptr(b), C.byref(raw), _ptr(d), _ptr(f), w, h,
                                                     1 if double_size else 0, int(max_keypoints), C.byref(c),
                                                     C.byref(params), int(fill_scale), 1 if bilinear else 0, kind, alpha,
                                                     cauchy_scale, seed, _ptr(objs), max_objects, C.byref(n), _ptr(counts)),
                 "mh_frame_run_kinect_raw_host")
        return objs[:min(n.value, max_objects)].copy(), counts, d, f

    def frame_set_filter_depth(self, f1=None, f2=None, depth_K=None, depth_cam=None):
        """FILTER (f1) / FILTER2 (f2) of the frames enqueued from now on as the depth class; None: that slot stays plain,
        both None: off.  f1, f2: (PlausibleSqDistance, DepthFraction, MinKeypointFraction)."""
        p1, p2 = make_filter_depth_params(f1), make_filter_depth_params(f2)
        dc = make_cam(depth_K, depth_cam) if depth_K is not None else None
        self._ck(self.L.mh_frame_set_filter_depth(self.h, C.byref(p1) if p1 is not None else None,
                                                  C.byref(p2) if p2 is not None else None,
                                                  C.byref(dc) if dc is not None else None), "mh_frame_set_filter_depth")

    def frame_route(self):
        """How the last frame or batch enqueued went through CLUSTER .. FILTER2 (mh_frame_route) -> int32 [4]: frames,
        1 = they shared their launches, 1 = the FILTER steps ran in the POSE tails, depth class bits (1 FILTER, 2 FILTER2).
        Host bookkeeping: no synchronisation."""
        o = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_route(self.h, _ptr(o)), "mh_frame_route")
        return o

    def filter_depth_debug_form(self, form):
        """Debug: the device form filter_depth() scores with -- 0 the workgroup form (default), 1 the wave form the fused
        POSE tails run.  Frames ignore it."""
        self._ck(self.L.mh_filter_depth_debug_form(self.h, int(form)), "mh_filter_depth_debug_form")

    # ---- DEPTH_VERIFY ----
    def depth_verify(self, corr, model_off, obj_model, obj_pose, K, cam, depth_K, depth_cam, params):
        """mh_depth_verify: DEPTH_VERIFY_CPU::process for every object against the depth map the context holds
        (frame_set_depth_image[_host]) and the resident store's keypoints -> records [n_obj] (VERIFY_DTYPE), nothing
        erased; params: (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction)."""
        corr = np.ascontiguousarray(corr, CORR_DTYPE)
        model_off = np.ascontiguousarray(model_off, np.int32)
        obj_model = np.ascontiguousarray(obj_model, np.int32).reshape(-1)
        obj_pose = np.ascontiguousarray(obj_pose, np.float32).reshape(-1, 7)
        n = obj_model.shape[0]
        assert obj_pose.shape[0] == n
        rec = np.zeros(max(n, 1), VERIFY_DTYPE)
        c, dc = make_cam(K, cam), make_cam(depth_K, depth_cam)
        prm = make_depth_verify_params(params)
        self._ck(self.L.mh_depth_verify(self.h, _ptr(corr), _ptr(model_off), len(model_off) - 1, _ptr(obj_model),
                                        _ptr(obj_pose), n, C.byref(c), C.byref(dc), C.byref(prm), _ptr(rec)), "mh_depth_verify")
        return rec[:n]

    def frame_set_depth_verify(self, params, depth_K=None, depth_cam=None):
        """mh_frame_set_depth_verify: frames and batches enqueued afterwards run DEPTH_VERIFY behind FILTER2 and deliver
        the objects it leaves; params: (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction) or None = off;
        depth_K, depth_cam: the depth map's camera."""
        prm = make_depth_verify_params(params)
        if prm is None:
            self._ck(self.L.mh_frame_set_depth_verify(self.h, None, None), "mh_frame_set_depth_verify")
            return
        dc = make_cam(depth_K, depth_cam)
        self._ck(self.L.mh_frame_set_depth_verify(self.h, C.byref(prm), C.byref(dc)), "mh_frame_set_depth_verify")

    def frame_fetch_verify(self, slot=0, max_records=4096):
        """mh_frame_fetch_verify_slot: the records (VERIFY_DTYPE) of the frame in result slot `slot`, one per object that
        left FILTER2, in that order; the frame's fetched objects are those with keep = 1."""
        rec = np.zeros(max(max_records, 1), VERIFY_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_verify_slot(self.h, int(slot), int(max_records), _ptr(rec), C.byref(n)),
                 "mh_frame_fetch_verify_slot")
        return rec[:min(n.value, max_records)].copy()

    def depth_verify_debug_form(self, form):
        """mh_depth_verify_debug_form: 0 a workgroup per object (default), 1 a wavefront per object."""
        self._ck(self.L.mh_depth_verify_debug_form(self.h, int(form)), "mh_depth_verify_debug_form")

    # ---- object hulls ----
    def object_hulls(self, obj_model, obj_pose, K, cam, max_vertices=64):
        """mh_object_hulls: Object::getObjectHull of every object in the image (K, cam) + the projected corners of the
        models' bounding boxes.  -> (hulls, n_vertices [n], n_behind [n], bbox_uv [n, 8, 2]); hulls[o] is [k, 2] with
        k = min(n_vertices[o], max_vertices), in the reference's vertex order."""
        obj_model = np.ascontiguousarray(obj_model, np.int32).reshape(-1)
        obj_pose = np.ascontiguousarray(obj_pose, np.float32).reshape(-1, 7)
        n = obj_model.shape[0]
        assert obj_pose.shape[0] == n
        xy = np.zeros((max(n, 1), max(int(max_vertices), 1), 2), np.float32)
        nv = np.zeros(max(n, 1), np.int32)
        nb = np.zeros(max(n, 1), np.int32)
        bb = np.zeros((max(n, 1), 8, 2), np.float32)
        c = make_cam(K, cam)
        self._ck(self.L.mh_object_hulls(self.h, _ptr(obj_model), _ptr(obj_pose), n, C.byref(c), int(max_vertices), _ptr(xy),
                                        _ptr(nv), _ptr(nb), _ptr(bb)), "mh_object_hulls")
        hulls = [xy[o, :min(int(nv[o]), int(max_vertices))].copy() for o in range(n)]
        return hulls, nv[:n], nb[:n], bb[:n]

    def frame_set_hulls(self, max_vertices, image=0):
        """mh_frame_set_hulls: frames and batches enqueued afterwards compute their objects' hulls (0 = off)."""
        self._ck(self.L.mh_frame_set_hulls(self.h, int(max_vertices), int(image)), "mh_frame_set_hulls")

    def frame_fetch_hulls(self, slot=None, max_objects=4096, max_vertices=64):
        """mh_frame_fetch_hulls[_slot]: the hulls of the frame in result slot `slot` (None: mh_frame_fetch's frame), in the
        order of its objects.  -> (hulls, n_vertices [n], n_behind [n], bbox_uv [n, 8, 2]) as object_hulls gives them."""
        xy = np.zeros((max(max_objects, 1), max(int(max_vertices), 1), 2), np.float32)
        nv = np.zeros(max(max_objects, 1), np.int32)
        nb = np.zeros(max(max_objects, 1), np.int32)
        bb = np.zeros((max(max_objects, 1), 8, 2), np.float32)
        n = C.c_int32(0)
        if slot is None:
            self._ck(self.L.mh_frame_fetch_hulls(self.h, max_objects, int(max_vertices), _ptr(xy), _ptr(nv), _ptr(nb), _ptr(bb),
                                                 C.byref(n)), "mh_frame_fetch_hulls")
        else:
            self._ck(self.L.mh_frame_fetch_hulls_slot(self.h, int(slot), max_objects, int(max_vertices), _ptr(xy), _ptr(nv), _ptr(nb),
                                                      _ptr(bb), C.byref(n)), "mh_frame_fetch_hulls_slot")
        k = min(n.value, max_objects)
        return [xy[o, :min(int(nv[o]), int(max_vertices))].copy() for o in range(k)], nv[:k].copy(), nb[:k].copy(), bb[:k].copy()

    def frame_fetch_batch_hulls_async(self, B, max_objects, host_ptr):
        """mh_frame_fetch_batch_hulls_async: B frames' hull records into the caller's pinned block (hull_block_dtype);
        frame_fetch_wait() waits for it."""
        self._ck(self.L.mh_frame_fetch_batch_hulls_async(self.h, B, max_objects, C.c_void_p(host_ptr)),
                 "mh_frame_fetch_batch_hulls_async")

    def hull_debug_form(self, form):
        """Debug: the device form object_hulls() runs -- 0 the octagon prefilter (default), 1 sort and chain every point."""
        self._ck(self.L.mh_hull_debug_form(self.h, int(form)), "mh_hull_debug_form")

    # ---- frame (device pointers as ints) ----
    def frame_enqueue(self, q_desc_ptr, q_uv_ptr, Q, K, cam, params: mh_frame_params, seed=1):
        c = make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue(self.h, C.c_void_p(q_desc_ptr), C.c_void_p(q_uv_ptr), Q,
                                         C.byref(c), C.byref(params), seed), "mh_frame_enqueue")

    def frame_run_host(self, q_desc, q_uv, Ks, cams, params: mh_frame_params, seed=1, q_image=None, write_back=True,
                       max_objects=4096):
        """The whole frame from host arrays, objects back on return (mh_frame_run_host: what FRAME_RESIDENT_HIP calls).
        q_desc [Q,128] float32 C-contiguous (normalised in place if write_back), q_uv [Q,2]; Ks [n,4], cams [n,7];
        q_image [Q] int32 when n > 1.  -> (objects, counts)."""
        assert q_desc.dtype == np.float32 and q_desc.flags.c_contiguous and q_desc.shape[1] == 128
        uv = np.ascontiguousarray(q_uv, np.float32)
        arr = make_cams(Ks, cams)
        img = None if q_image is None else np.ascontiguousarray(q_image, np.int32)
        objs = np.zeros(max_objects, OBJECT_DTYPE)
        n = C.c_int32(0)
        counts = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_run_host(self.h, _ptr(q_desc), _ptr(uv), None if img is None else _ptr(img), q_desc.shape[0],
                                          arr, len(Ks), C.byref(params), C.c_uint64(int(seed)), int(bool(write_back)),
                                          _ptr(objs), max_objects, C.byref(n), _ptr(counts)), "mh_frame_run_host")
        return objs[:min(n.value, max_objects)].copy(), counts

    def host_alloc(self, nbytes):
        """Page-locked host memory from the library (mh_host_alloc) as a uint8 array; host_free(array) releases it."""
        p = C.c_void_p()
        self._ck(self.L.mh_host_alloc(self.h, C.c_size_t(int(nbytes)), C.byref(p)), "mh_host_alloc")
        a = np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(p.value))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        self._ck(self.L.mh_host_free(self.h, C.c_void_p(self._pinned.pop(a.ctypes.data))), "mh_host_free")

    def frame_run_host_begin(self, q_desc, q_uv, Ks, cams, params: mh_frame_params, seed=1, q_image=None, write_back=True):
        """mh_frame_run_host in halves: upload + enqueue (returns at once); then frame_wait_descriptors(), frame_fetch().
        The arrays must stay alive and untouched until then."""
        assert q_desc.dtype == np.float32 and q_desc.flags.c_contiguous and q_desc.shape[1] == 128
        assert q_uv.dtype == np.float32 and q_uv.flags.c_contiguous
        arr = make_cams(Ks, cams)
        self._rh_keep = (q_desc, q_uv, q_image, arr)
        self._ck(self.L.mh_frame_run_host_begin(self.h, _ptr(q_desc), _ptr(q_uv), None if q_image is None else _ptr(q_image),
                                                q_desc.shape[0], arr, len(Ks), C.byref(params), C.c_uint64(int(seed)),
                                                int(bool(write_back))), "mh_frame_run_host_begin")

    def frame_wait_descriptors(self):
        self._ck(self.L.mh_frame_wait_descriptors(self.h), "mh_frame_wait_descriptors")

    # ---- the six slots one call each on a frame that stays on the device (mh_step_*: the per-step plugins' hand-over) ----
    def step_match(self, q_desc, q_uv, K, cam, ratio=0.8, write_back=True):
        """MATCH: upload, normalise, search, ratio test, per-model lists on the device -> (model_off [n_models + 1],
        match_query [M], match_pts [M] CORR_DTYPE).  q_desc is normalised in place if write_back."""
        assert q_desc.dtype == np.float32 and q_desc.flags.c_contiguous and q_desc.shape[1] == 128
        uv = np.ascontiguousarray(q_uv, np.float32)
        Q = q_desc.shape[0]
        c = make_cam(K, cam)
        self._ck(self.L.mh_step_match(self.h, _ptr(q_desc), _ptr(uv), Q, C.byref(c), C.c_float(ratio), int(bool(write_back))),
                 "mh_step_match")
        if write_back:
            self.frame_wait_descriptors()
        nn_, nm_ = C.c_int(0), C.c_int(0)
        self._ck(self.L.mh_db_size(self.h, C.byref(nn_), C.byref(nm_)), "mh_db_size")
        nm = nm_.value
        off = np.zeros(nm + 1, np.int32)
        mq = np.zeros(Q, np.int32)
        pts = np.zeros(Q, CORR_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_step_match_fetch(self.h, _ptr(off), _ptr(mq), _ptr(pts), Q, C.byref(n)), "mh_step_match_fetch")
        return off, mq[:n.value].copy(), pts[:n.value].copy()

    def step_cluster(self, radius=200.0, merge=20.0, min_pts=7, max_iter=100, cap_clusters=1024, cap_members=1 << 16):
        """CLUSTER on the resident lists -> (cl_model [n], cl_off [n + 1], members [cl_off[n]]: indices into matches[model])."""
        cm = np.zeros(cap_clusters, np.int32)
        co = np.zeros(cap_clusters + 1, np.int32)
        mem = np.zeros(cap_members, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.mh_step_cluster(self.h, C.c_float(radius), C.c_float(merge), int(min_pts), int(max_iter), _ptr(cm), _ptr(co),
                                        _ptr(mem), cap_clusters, cap_members, C.byref(n)), "mh_step_cluster")
        return cm[:n.value].copy(), co[:n.value + 1].copy(), mem[:co[n.value]].copy()

    def step_pose(self, which, prm: mh_pose_params, seed, cap=4096):
        """POSE (which = 1) / POSE2 (2) on the resident clusters -> the objects the step appends (STEP_OBJECT_DTYPE)."""
        out = np.zeros(cap, STEP_OBJECT_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_step_pose(self.h, int(which), C.byref(prm), C.c_uint64(int(seed)), _ptr(out), cap, C.byref(n)),
                 "mh_step_pose")
        return out[:n.value].copy()

    def step_filter(self, which, min_points, feature_distance, min_score, n_objects, cap_members=1 << 16):
        """FILTER (1) / FILTER2 (2) on the resident objects -> (score [n_objects], keep [n_objects], out_order [kept],
        cl_off [kept + 1], members)."""
        score = np.zeros(max(n_objects, 1), np.float32)
        keep = np.zeros(max(n_objects, 1), np.uint8)
        order = np.zeros(max(n_objects, 1), np.int32)
        co = np.zeros(n_objects + 1, np.int32)
        mem = np.zeros(cap_members, np.int32)
        kept = C.c_int32(0)
        self._ck(self.L.mh_step_filter(self.h, int(which), int(min_points), C.c_float(feature_distance), C.c_float(min_score),
                                       int(n_objects), _ptr(score), _ptr(keep), _ptr(order), _ptr(mem), _ptr(co), cap_members,
                                       C.byref(kept)), "mh_step_filter")
        k = kept.value
        return score[:n_objects].copy(), keep[:n_objects].copy(), order[:k].copy(), co[:k + 1].copy(), mem[:co[k]].copy()

    def frame_enqueue_image(self, gray_ptr, w, h, double_size, max_keypoints, K, cam, params: mh_frame_params,
                            seed=1, _cam_struct=None):
        """FEAT -> FILTER2 of a device-resident 8-bit image; nothing goes through the host."""
        c = _cam_struct or make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue_image(self.h, C.c_void_p(gray_ptr), w, h, int(double_size), max_keypoints,
                                               C.byref(c), C.byref(params), seed), "mh_frame_enqueue_image")

    def frame_enqueue_image_batch(self, gray_ptrs, w, h, double_size, max_keypoints, K, cam, params: mh_frame_params, seeds,
                                  _cam_struct=None):
        """FEAT of B device images, ONE MATCH launch sequence over all their keypoints, CLUSTER..FILTER2 image after
        image into result slots 0..B-1 (frame_fetch_slot)."""
        c = _cam_struct or make_cam(K, cam)
        B = len(gray_ptrs)
        g = (C.c_void_p * B)(*gray_ptrs)
        sd = (C.c_uint64 * B)(*[int(x) for x in seeds])
        self._ck(self.L.mh_frame_enqueue_image_batch(self.h, g, B, w, h, int(double_size), max_keypoints, C.byref(c),
                                                     C.byref(params), sd), "mh_frame_enqueue_image_batch")

    def frame_enqueue_images(self, gray_ptrs, w, h, double_size, max_keypoints_per_image, Ks, cams,
                             params: mh_frame_params, seed=1, _cam_structs=None):
        """ONE frame seen by len(gray_ptrs) cameras, images resident on the device (Ks [n,4], cams [n,7]): FEAT of every
        image, the lists packed on the device, MATCH..FILTER2 with every keypoint in its own image."""
        n = len(gray_ptrs)
        arr = _cam_structs or make_cams(Ks, cams)
        if len(arr) != n:
            raise ValueError("one camera per image")
        g = (C.c_void_p * max(n, 1))(*gray_ptrs)
        self._ck(self.L.mh_frame_enqueue_images(self.h, g, n, w, h, int(double_size), max_keypoints_per_image, arr,
                                                C.byref(params), seed), "mh_frame_enqueue_images")

    def frame_enqueue_images_batch(self, gray_ptrs, n_images, w, h, double_size, max_keypoints_per_image, Ks, cams,
                                   params: mh_frame_params, seeds, _cam_structs=None):
        """len(gray_ptrs) / n_images frames of one rig (frame f's images: gray_ptrs[f n_images : (f + 1) n_images]) into
        result slots 0.. (frame_fetch_slot)."""
        n_frames, rest = divmod(len(gray_ptrs), max(n_images, 1))
        arr = _cam_structs or make_cams(Ks, cams)
        if rest or len(arr) != n_images or len(seeds) != n_frames:
            raise ValueError("n_images images and one seed per frame, one camera per image of the rig")
        g = (C.c_void_p * max(len(gray_ptrs), 1))(*gray_ptrs)
        sd = (C.c_uint64 * max(n_frames, 1))(*[int(x) for x in seeds])
        self._ck(self.L.mh_frame_enqueue_images_batch(self.h, g, n_frames, n_images, w, h, int(double_size),
                                                      max_keypoints_per_image, arr, C.byref(params), sd),
                 "mh_frame_enqueue_images_batch")

    def frame_set_undistort_images(self, dists):
        """Undistort the images of frame_enqueue_images[_batch], camera i with its K and dists[i] = k1, k2, p1, p2;
        None = off."""
        if dists is None or len(dists) == 0:
            self._ck(self.L.mh_frame_set_undistort_images(self.h, None, 0), "mh_frame_set_undistort_images")
            return
        d = np.ascontiguousarray(dists, np.float32).reshape(-1, 4)
        self._ck(self.L.mh_frame_set_undistort_images(self.h, _ptr(d), len(d)), "mh_frame_set_undistort_images")

    def frame_image_counts(self):
        """Keypoints every image contributed to the frame last fetched (after clamping to the per-image capacity)."""
        out = np.zeros(8, np.int32)   # MH_MAX_IMAGES
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_image_counts(self.h, _ptr(out), len(out), C.byref(n)), "mh_frame_image_counts")
        return out[:n.value].copy()

    def frame_features_image_dev(self):
        """Device int32 pointer: the image index of every row of the list frame_features_dev hands out."""
        q = C.c_void_p()
        self._ck(self.L.mh_frame_features_image_dev(self.h, C.byref(q)), "mh_frame_features_image_dev")
        return q.value

    def set_linkage_scratch_limit(self, nbytes):
        """Bound of the linkage clusterer's similarity-matrix scratch for this context (0: the default, 4 GiB)."""
        self._ck(self.L.mh_set_linkage_scratch_limit(self.h, C.c_size_t(int(nbytes))), "mh_set_linkage_scratch_limit")

    def frame_set_cluster_linkage(self, params: "mh_linkage_params | None"):
        """CLUSTER of the next frames: moped3d's linkage clusterer (None: mean shift again)."""
        self._ck(self.L.mh_frame_set_cluster_linkage(self.h, C.byref(params) if params is not None else None),
                 "mh_frame_set_cluster_linkage")

    def cluster_linkage(self, problems, params=None):
        """problems: list of (uv [n,2], model_xyz [n,3], world_xyz [n,3]) -> list of (clusters, label);
        the depth map must have been set with frame_set_depth_image."""
        prm = params or default_linkage_params()
        sizes = [len(p[0]) for p in problems]
        off = np.zeros(len(problems) + 1, np.int32)
        off[1:] = np.cumsum(sizes)
        total = int(off[-1])
        if total:
            corr = np.concatenate([pack_corr(np.asarray(p[0], np.float32), np.asarray(p[1], np.float32)) for p in problems if len(p[0])])
            dep = np.concatenate([pack_depth(np.asarray(p[2], np.float32), np.ones(len(p[2]), np.float32)) for p in problems if len(p[0])])
        else:
            corr, dep = np.zeros(0, CORR_DTYPE), pack_depth(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
        corr, dep = np.ascontiguousarray(corr), np.ascontiguousarray(dep)
        label = np.full(max(total, 1), -1, np.int32)
        order = np.full(max(total, 1), -1, np.int32)
        ncl = np.zeros(max(len(problems), 1), np.int32)
        self._ck(self.L.mh_cluster_linkage(self.h, _ptr(corr), _ptr(dep), _ptr(off), len(problems), C.byref(prm),
                                           _ptr(label), _ptr(order), _ptr(ncl)), "mh_cluster_linkage")
        out = []
        for i in range(len(problems)):
            b, e = int(off[i]), int(off[i + 1])
            lab, ordr = label[b:e], order[b:e]
            clusters, pos = [], 0
            for c in range(int(ncl[i])):
                sz = int((lab == c).sum())
                clusters.append(ordr[pos:pos + sz].copy())
                pos += sz
            out.append((clusters, lab.copy()))
        return out

    # moped3d's weighted mean shift (CLUSTER_WEIGHTED_MEAN_SHIFT_CPU) on its own
    @staticmethod
    def _wms_pack(problems):
        sizes = [len(p[0]) for p in problems]
        off = np.zeros(len(problems) + 1, np.int32)
        off[1:] = np.cumsum(sizes)
        total = int(off[-1])
        xyz, fill = np.zeros((max(total, 1), 3), np.float32), np.zeros(max(total, 1), np.float32)
        for p, b in zip(problems, off):
            if len(p[0]):
                xyz[b:b + len(p[0])] = np.asarray(p[0], np.float32).reshape(-1, 3)
                fill[b:b + len(p[0])] = np.asarray(p[1], np.float32)
        return off, xyz, fill

    def frame_set_cluster_wms(self, params: "mh_wms_params | None"):
        """CLUSTER of the following single-camera frames: the weighted mean shift over the depth map's points (None: off;
        it and frame_set_cluster_linkage exclude each other, the one set last is on)."""
        self._ck(self.L.mh_frame_set_cluster_wms(self.h, C.byref(params) if params is not None else None),
                 "mh_frame_set_cluster_wms")

    def cluster_wms_raw(self, problems, params, cap_clusters, cap_members):
        """mh_cluster_wms as it is -> (status, n_clusters [problems], cl_off [cap_clusters + 1], members [cap_members],
        needed (clusters, members)); the arrays are pre-filled with -1 so that a test sees what was written."""
        off, xyz, fill = self._wms_pack(problems)
        ncl = np.full(max(len(problems), 1), -1, np.int32)
        cl_off = np.full(cap_clusters + 1, -1, np.int32)
        members = np.full(max(cap_members, 1), -1, np.int32)
        needed = np.zeros(2, np.int64)
        rc = self.L.mh_cluster_wms(self.h, _ptr(xyz), _ptr(fill), _ptr(off), len(problems), C.byref(params), _ptr(ncl),
                                   _ptr(cl_off), int(cap_clusters), _ptr(members), int(cap_members), _ptr(needed))
        return rc, ncl[:len(problems)], cl_off, members[:cap_members], (int(needed[0]), int(needed[1]))

    def cluster_wms(self, problems, params=None):
        """problems: list of (xyz [n, 3] camera-frame points, fill [n] fill distances), one per (model, image), each of up
        to WMS_MAX_POINTS points -> per problem the list of clusters in the reference's order, each an int32 array of
        problem-local indices, descending.  Clusters may overlap."""
        prm = params or mh_wms_params()
        total = sum(len(p[0]) for p in problems)
        cap_c, cap_m = max(total, 1), max(4 * total, 1)
        for _ in range(2):
            rc, ncl, cl_off, members, needed = self.cluster_wms_raw(problems, prm, cap_c, cap_m)
            if rc != MH_ERR_CAPACITY:
                break
            cap_c, cap_m = max(needed[0], 1), max(needed[1], 1)   # (overlap beyond four memberships per point: ask again)
        self._ck(rc, "mh_cluster_wms")
        out, k = [], 0
        for p in range(len(problems)):
            out.append([members[cl_off[k + c]:cl_off[k + c + 1]].copy() for c in range(int(ncl[p]))])
            k += int(ncl[p])
        return out

    def wms_debug_state(self, problems, params=None):
        """The same problems through the same kernel -> per problem (weight [n], centre [n, 3], active [n] bool,
        iterations): the weights, the final centres, which canopies survived, the reference's nIter."""
        prm = params or mh_wms_params()
        off, xyz, fill = self._wms_pack(problems)
        total = int(off[-1])
        weight, centre = np.zeros(max(total, 1), np.float32), np.zeros((max(total, 1), 3), np.float32)
        active, iters = np.zeros(max(total, 1), np.int32), np.zeros(max(len(problems), 1), np.int32)
        self._ck(self.L.mh_wms_debug_state(self.h, _ptr(xyz), _ptr(fill), _ptr(off), len(problems), C.byref(prm), _ptr(weight),
                                           _ptr(centre), _ptr(active), _ptr(iters)), "mh_wms_debug_state")
        return [(weight[b:e].copy(), centre[b:e].copy(), active[b:e].astype(bool), int(iters[p]))
                for p, (b, e) in enumerate(zip(off[:-1], off[1:]))]

    def linkage_set_mode(self, mode: int):
        """LINKAGE_SCAN (0, the default: one workgroup per problem rescans every live pair per merge; up to 1024 points)
        or LINKAGE_ROWMAX (1: the matrix stage on the whole grid, the merge loop over cached row maxima -- the same
        matrices and clusters, up to LINKAGE_MAX_POINTS points).  For cluster_linkage, the debug entries and the frames."""
        self._ck(self.L.mh_linkage_set_mode(self.h, int(mode)), "mh_linkage_set_mode")

    def linkage_get_mode(self) -> int:
        mode = C.c_int(0)
        self._ck(self.L.mh_linkage_get_mode(self.h, C.byref(mode)), "mh_linkage_get_mode")
        return mode.value

    def linkage_stats(self, reset=False):
        """What the LINKAGE_ROWMAX kernels counted on the device since the last reset -> (problems clustered, merges,
        rows rescanned, largest n).  Synchronises the context."""
        out = np.zeros(4, np.int64)
        self._ck(self.L.mh_linkage_stats(self.h, _ptr(out), 1 if reset else 0), "mh_linkage_stats")
        return tuple(int(v) for v in out)

    # the clusterer's two halves on their own, for verification (mh_linkage_debug_*)
    def linkage_debug_matrix(self, uv, model_xyz, world_xyz, params=None):
        """One problem as cluster_linkage takes it -> (A, K) float32 [n, n]: the 3-D side after pass 2 (before the
        division by its maximum) and the final similarity as the agglomeration first sees it."""
        prm = params or default_linkage_params()
        n = len(uv)
        corr = np.ascontiguousarray(pack_corr(np.asarray(uv, np.float32), np.asarray(model_xyz, np.float32)))
        dep = np.ascontiguousarray(pack_depth(np.asarray(world_xyz, np.float32), np.ones(n, np.float32)))
        A, K = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
        self._ck(self.L.mh_linkage_debug_matrix(self.h, _ptr(corr), _ptr(dep), n, C.byref(prm), _ptr(A), _ptr(K)),
                 "mh_linkage_debug_matrix")
        return A, K

    def linkage_debug_agglomerate(self, Km, cutoff=0.1, min_pts=7, linkage_type=1):
        """The agglomeration alone over a symmetric similarity matrix [n, n] -> (clusters, label) as cluster_linkage's."""
        Km = np.ascontiguousarray(Km, np.float32)
        n = len(Km)
        if Km.shape != (n, n):
            raise ValueError("linkage_debug_agglomerate: a square matrix")
        label, order = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
        ncl = C.c_int32(0)
        self._ck(self.L.mh_linkage_debug_agglomerate(self.h, _ptr(Km), n, C.c_float(cutoff), int(min_pts), int(linkage_type),
                                                     _ptr(label), _ptr(order), C.byref(ncl)), "mh_linkage_debug_agglomerate")
        label = label[:n]
        clusters, pos = [], 0
        for c in range(ncl.value):
            sz = int((label == c).sum())
            clusters.append(order[pos:pos + sz].copy())
            pos += sz
        return clusters, label.copy()

    def frame_debug_fetch_clusters_slot(self, slot=0, cap_clusters=4096, cap_members=1 << 16):
        """CLUSTER's result of frame `slot` of the last frame / batch -> list of (model, member indices inside that model's
        match list, in the clusterer's order), clusters in (model, emission) order."""
        cm, co = np.zeros(cap_clusters, np.int32), np.zeros(cap_clusters + 1, np.int32)
        mem = np.zeros(cap_members, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_debug_fetch_clusters_slot(self.h, int(slot), _ptr(cm), _ptr(co), _ptr(mem), cap_clusters,
                                                           cap_members, C.byref(n)), "mh_frame_debug_fetch_clusters_slot")
        return [(int(cm[c]), mem[co[c]:co[c + 1]].copy()) for c in range(n.value)]

    def frame_debug_fetch_cluster_table_slot(self, slot=0, cap_clusters=4096):
        """The flat cluster table of frame `slot` as the device holds it (the arrays POSE walks) -> (cl_model, cl_begin,
        cl_count, n_now): the rows CLUSTER published (FrameCounts::n_clusters of them; cl_begin = absolute position in the
        frame's match list) and the device's current row count (fs->n_clusters: 0 once a FILTER2 has kept nothing)."""
        cm, cb, cc = (np.zeros(cap_clusters, np.int32) for _ in range(3))
        n, now = C.c_int32(0), C.c_int32(0)
        self._ck(self.L.mh_frame_debug_fetch_cluster_table_slot(self.h, int(slot), _ptr(cm), _ptr(cb), _ptr(cc), cap_clusters,
                                                                C.byref(n), C.byref(now)),
                 "mh_frame_debug_fetch_cluster_table_slot")
        return cm[:n.value].copy(), cb[:n.value].copy(), cc[:n.value].copy(), now.value

    def frame_set_depth_rules(self, K=None, patch_size=64, feature_density=-1.0, match_density=-1.0, ratio_table=None,
                              maximum_depth=4.0, default_depth=1.0, cauchy_scale=0.1, off=False):
        """moped3d's DEPTHFILTER / DEPTHFILTER2 / adaptive ratio inside the frame (needs frame_set_depth_image)."""
        if off:
            self._ck(self.L.mh_frame_set_depth_rules(self.h, None, None), "mh_frame_set_depth_rules")
            return
        r = mh_depth_rules(patch_size, feature_density, match_density, None, 0, maximum_depth, default_depth, cauchy_scale)
        tab = None
        if ratio_table is not None:
            tab = np.ascontiguousarray(ratio_table, np.float32)
            r.ratio_table = tab.ctypes.data
            r.n_models = tab.shape[0]
        k = np.ascontiguousarray(K if K is not None else [0, 0, 0, 0], np.float32)
        self._ck(self.L.mh_frame_set_depth_rules(self.h, C.byref(r), _ptr(k)), "mh_frame_set_depth_rules")

    def depth_rules_debug_fetch(self, which: str, slot=0, n=None) -> np.ndarray:
        """What the depth front end left for frame `slot` (mh_depth_rules_debug_fetch): 'inv_size' float64 [n = pw ph],
        'keep1' uint8 [n = Q], 'm_depth' DEPTH_DTYPE [n = the frame's match count, default: asked from the lists]."""
        k, dt = {"inv_size": (0, np.float64), "keep1": (1, np.uint8), "m_depth": (2, DEPTH_DTYPE)}[which]
        if n is None:
            assert which == "m_depth", "inv_size and keep1 need their length"
            n = len(self.frame_fetch_matches_slot(slot)[0])
        out = np.zeros(int(n), dt)
        self._ck(self.L.mh_depth_rules_debug_fetch(self.h, k, int(slot), _ptr(out) if n else None, out.nbytes),
                 "mh_depth_rules_debug_fetch")
        return out

    def frame_fetch_matches(self, cap=1 << 16):
        q = np.zeros(cap, np.int32)
        m = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_matches(self.h, _ptr(q), _ptr(m), cap, C.byref(n)), "mh_frame_fetch_matches")
        return q[:min(n.value, cap)].copy(), m[:min(n.value, cap)].copy()

    def frame_fetch_matches_slot(self, slot, cap=1 << 16):
        """Accepted matches of frame `slot` of the last batch: (query, model), sorted by (model, query)."""
        q = np.zeros(cap, np.int32)
        m = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_matches_slot(self.h, slot, _ptr(q), _ptr(m), cap, C.byref(n)),
                 "mh_frame_fetch_matches_slot")
        return q[:min(n.value, cap)].copy(), m[:min(n.value, cap)].copy()

    def frame_fetch_match_points(self, cap=1 << 16):
        """The last frame's accepted matches as correspondences (u, v of the query, x, y, z of its row), list order."""
        c = np.zeros(cap, CORR_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_match_points(self.h, _ptr(c), cap, C.byref(n)), "mh_frame_fetch_match_points")
        return c[:min(n.value, cap)].copy()

    def frame_fetch_match_reps(self, slot=None, cap=1 << 16):
        """Representatives of the list entries of frame `slot` of the last batch (None: the last frame): the first
        entry with the same pixel (and image) -- the key of FILTER's bestPoints map."""
        r = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_match_reps_slot(self.h, -1 if slot is None else slot, _ptr(r), cap, C.byref(n)),
                 "mh_frame_fetch_match_reps_slot")
        return r[:min(n.value, cap)].copy()

    def frame_enqueue_rest_frames(self, q_uv_ptr, Q, gathered_ptr, n_shards, stride_words, plane_words, B, K, cam,
                                  params: mh_frame_params, seeds, _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        sd = (C.c_uint64 * B)(*[int(x) for x in seeds])
        self._ck(self.L.mh_frame_enqueue_rest_frames(self.h, C.c_void_p(q_uv_ptr), Q, C.c_void_p(gathered_ptr), n_shards,
                                                     stride_words, plane_words, B, C.byref(c), C.byref(params), sd),
                 "mh_frame_enqueue_rest_frames")

    def frame_features_dev(self):
        d, u, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self.L.mh_frame_features_dev(self.h, C.byref(d), C.byref(u), C.byref(n)), "mh_frame_features_dev")
        return d.value, u.value, n.value

    def frame_keypoints(self):
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_keypoints(self.h, C.byref(n)), "mh_frame_keypoints")
        return n.value

    def frame_enqueue_match_local(self, q_desc_ptr, Q, top2_ptr):
        """top2_ptr: device block of [3][Q] 32-bit words (idx1, d1 bits, d2 bits)."""
        self._ck(self.L.mh_frame_enqueue_match_local(self.h, C.c_void_p(q_desc_ptr), Q, C.c_void_p(top2_ptr)),
                 "mh_frame_enqueue_match_local")

    def frame_enqueue_rest(self, q_uv_ptr, Q, gathered_ptr, n_shards, K, cam, params: mh_frame_params,
                           seed=1, _cam_struct=None):
        """gathered_ptr: device block of [n_shards][3][Q] words (rank order)."""
        c = _cam_struct or make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue_rest(self.h, C.c_void_p(q_uv_ptr), Q, C.c_void_p(gathered_ptr),
                                              n_shards, C.byref(c), C.byref(params), seed),
                 "mh_frame_enqueue_rest")

    def frame_enqueue_rest_strided(self, q_uv_ptr, Q, gathered_ptr, n_shards, stride_words, K, cam,
                                   params: mh_frame_params, seed=1, _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue_rest_strided(self.h, C.c_void_p(q_uv_ptr), Q, C.c_void_p(gathered_ptr), n_shards,
                                                      stride_words, C.byref(c), C.byref(params), seed),
                 "mh_frame_enqueue_rest_strided")

    def frame_enqueue_rest_batch(self, q_uv_ptr, Q, gathered_ptr, n_shards, stride_words, plane_words, slot, K, cam,
                                 params: mh_frame_params, seed=1, _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue_rest_batch(self.h, C.c_void_p(q_uv_ptr), Q, C.c_void_p(gathered_ptr), n_shards,
                                                    stride_words, plane_words, slot, C.byref(c), C.byref(params), seed),
                 "mh_frame_enqueue_rest_batch")

    def frame_enqueue_batch(self, q_desc_ptr, q_uv_ptr, Q, B, K, cam, params: mh_frame_params, seeds, _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        sd = (C.c_uint64 * B)(*[int(x) for x in seeds])
        self._ck(self.L.mh_frame_enqueue_batch(self.h, C.c_void_p(q_desc_ptr), C.c_void_p(q_uv_ptr), Q, B, C.byref(c),
                                               C.byref(params), sd), "mh_frame_enqueue_batch")

    def frame_enqueue_sharded(self, comm: Comm, q_desc_ptr, q_uv_ptr, Q, K, cam, params: mh_frame_params, seed=1,
                              _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        self._ck(self.L.mh_frame_enqueue_sharded(self.h, comm.h, C.c_void_p(q_desc_ptr), C.c_void_p(q_uv_ptr), Q,
                                                 C.byref(c), C.byref(params), seed), "mh_frame_enqueue_sharded")

    def frame_enqueue_sharded_batch(self, comm: Comm, q_desc_ptr, q_uv_ptr, Q, B, K, cam, params: mh_frame_params,
                                    seeds, _cam_struct=None):
        c = _cam_struct or make_cam(K, cam)
        sd = (C.c_uint64 * B)(*[int(x) for x in seeds])
        self._ck(self.L.mh_frame_enqueue_sharded_batch(self.h, comm.h, C.c_void_p(q_desc_ptr), C.c_void_p(q_uv_ptr), Q, B,
                                                       C.byref(c), C.byref(params), sd),
                 "mh_frame_enqueue_sharded_batch")

    def frame_previous_objects(self, frame_in_batch=0, cap=8 * EX2_OBJECTS):
        objs = np.zeros(cap, OBJECT_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_previous_objects(self.h, frame_in_batch, _ptr(objs), cap, C.byref(n)),
                 "mh_frame_previous_objects")
        if n.value > cap:
            return self.frame_previous_objects(frame_in_batch, n.value)
        return objs[:n.value].copy()

    def frame_gather_objects(self, comm: Comm, slot=0, cap=4096):
        objs = np.zeros(cap, OBJECT_DTYPE)
        n = C.c_int32(0)
        self._ck(self.L.mh_frame_gather_objects(self.h, comm.h, slot, _ptr(objs), cap, C.byref(n)),
                 "mh_frame_gather_objects")
        return objs[:min(n.value, cap)].copy()

    def frame_fetch_slot(self, slot, max_objects=4096):
        objs = np.zeros(max_objects, OBJECT_DTYPE)
        n = C.c_int32(0)
        counts = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_fetch_slot(self.h, slot, _ptr(objs), max_objects, C.byref(n), _ptr(counts)),
                 "mh_frame_fetch_slot")
        return objs[:min(n.value, max_objects)].copy(), counts

    # ---- delivery of whole batches into pinned host memory (mh_frame_fetch_batch_async) ----
    def frame_fetch_batch_async(self, B, max_objects, host_ptr, tag=0):
        self._ck(self.L.mh_frame_fetch_batch_async(self.h, B, max_objects, C.c_void_p(host_ptr), tag & 0xFFFFFFFF),
                 "mh_frame_fetch_batch_async")

    def frame_fetch_previous_async(self, max_objects, host_ptr, tag=0):
        self._ck(self.L.mh_frame_fetch_previous_async(self.h, max_objects, C.c_void_p(host_ptr), tag & 0xFFFFFFFF),
                 "mh_frame_fetch_previous_async")

    def frame_fetch_wait(self):
        """Blocks until the context's pending delivery has landed; raises on capacity / exchange flags."""
        fl = C.c_int32(0)
        self._ck(self.L.mh_frame_fetch_wait(self.h, C.byref(fl)), "mh_frame_fetch_wait")

    def frame_fetch_query(self) -> bool:
        """True when the pending delivery (if any) has landed."""
        rc = self.L.mh_frame_fetch_query(self.h)
        if rc < 0:
            self._ck(rc, "mh_frame_fetch_query")
        return rc == 0

    def frame_result_copy_slots_dev(self, dst_ptr, n_slots, max_objects):
        self._ck(self.L.mh_frame_result_copy_slots_dev(self.h, C.c_void_p(dst_ptr), n_slots, max_objects),
                 "mh_frame_result_copy_slots_dev")

    def frame_result_copy_dev(self, dst_ptr, max_objects):
        self._ck(self.L.mh_frame_result_copy_dev(self.h, C.c_void_p(dst_ptr), max_objects), "mh_frame_result_copy_dev")

    def frame_fetch(self, max_objects=4096):
        objs = np.zeros(max_objects, OBJECT_DTYPE)
        n = C.c_int32(0)
        counts = np.zeros(4, np.int32)
        self._ck(self.L.mh_frame_fetch(self.h, _ptr(objs), max_objects, C.byref(n), _ptr(counts)), "mh_frame_fetch")
        return objs[:min(n.value, max_objects)].copy(), counts

    def frame_result_dev(self):
        p = C.c_void_p()
        b = C.c_int64(0)
        self._ck(self.L.mh_frame_result_dev(self.h, C.byref(p), C.byref(b)), "mh_frame_result_dev")
        return p.value, b.value

    def match_local_dev(self, qn_ptr, qnorm_ptr, Q, idx_ptr, d1_ptr, d2_ptr):
        self._ck(self.L.mh_match_local_dev(self.h, C.c_void_p(qn_ptr), C.c_void_p(qnorm_ptr), Q,
                                           C.c_void_p(idx_ptr), C.c_void_p(d1_ptr), C.c_void_p(d2_ptr)),
                 "mh_match_local_dev")

    def match_local_counted_dev(self, qn_ptr, qnorm_ptr, Q, q_count_ptr, q_expected, idx_ptr, d1_ptr, d2_ptr):
        """match_local_dev for Q rows of capacity, the number of queries among them read on the device."""
        self._ck(self.L.mh_match_local_counted_dev(self.h, C.c_void_p(qn_ptr), C.c_void_p(qnorm_ptr), Q, C.c_void_p(q_count_ptr),
                                                   int(q_expected), C.c_void_p(idx_ptr), C.c_void_p(d1_ptr), C.c_void_p(d2_ptr)),
                 "mh_match_local_counted_dev")

    def match_merge_dev(self, idx_s_ptr, d1_s_ptr, d2_s_ptr, n_shards, Q, idx_ptr, d1_ptr, d2_ptr):
        self._ck(self.L.mh_match_merge_dev(self.h, C.c_void_p(idx_s_ptr), C.c_void_p(d1_s_ptr),
                                           C.c_void_p(d2_s_ptr), n_shards, Q, C.c_void_p(idx_ptr),
                                           C.c_void_p(d1_ptr), C.c_void_p(d2_ptr)), "mh_match_merge_dev")

    def normalize_dev(self, q_ptr, qnorm_ptr, Q):
        self._ck(self.L.mh_normalize_dev(self.h, C.c_void_p(q_ptr), C.c_void_p(qnorm_ptr), Q), "mh_normalize_dev")


class ModelSet:
    """Host-side models (include/moped_hip.h "model files"): parsed `.moped.xml` files or a
    mapped `.mopeddb` container.  Host code only -- usable without a GPU."""

    def __init__(self, desc_type: str = "SIFT", _handle=None):
        self.L = load()
        if _handle is None:
            h = C.c_void_p()
            if self.L.mh_models_create(C.byref(h), desc_type.encode()) != 0:
                raise MhError("mh_models_create")
            _handle = h
        self.h = _handle

    @classmethod
    def load(cls, path: str) -> "ModelSet":
        L = load()
        h = C.c_void_p()
        if L.mh_models_load(C.byref(h), path.encode()) != 0:
            raise MhError(f"mh_models_load: not a valid .mopeddb file: {path}")
        return cls(_handle=h)

    def _ck(self, rc, what):
        if rc != 0:
            raise MhError(f"{what}: {self.L.mh_models_last_error(self.h).decode('latin-1')}")

    def add_xml(self, path: str):
        self._ck(self.L.mh_models_add_xml(self.h, path.encode()), "mh_models_add_xml")

    def add_xml_buffer(self, data: bytes):
        self._ck(self.L.mh_models_add_xml_buffer(self.h, data, len(data)), "mh_models_add_xml_buffer")

    def save(self, path: str):
        self._ck(self.L.mh_models_save(self.h, path.encode()), "mh_models_save")

    def add_rows(self, name: str, desc, xyz):
        """A model from rows (desc [n,128] kept as given, xyz [n,3]); a known name replaces that model."""
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, DIM)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        if desc.shape[0] != xyz.shape[0]:
            raise ValueError("one xyz per descriptor")
        self._ck(self.L.mh_models_add_rows(self.h, name.encode("latin-1"), _ptr(desc), _ptr(xyz), desc.shape[0]),
                 "mh_models_add_rows")

    def write_xml(self, i: int, path: str):
        """Model i as the `.moped.xml` file createModels writes (mh_models_write_xml)."""
        if self.L.mh_models_write_xml(self.h, int(i), path.encode()) != 0:
            raise MhError(f"mh_models_write_xml: no model {i}, or cannot write {path}")

    @property
    def n_models(self) -> int:
        return int(self.L.mh_models_count(self.h))

    @property
    def n_rows(self) -> int:
        return int(self.L.mh_models_rows(self.h))

    def name(self, i: int) -> str:
        return self.L.mh_models_name(self.h, i).decode("latin-1")

    def model_range(self, i: int):
        b, n = C.c_int64(0), C.c_int64(0)
        bbox = np.zeros(6, np.float32)
        self._ck(self.L.mh_models_range(self.h, i, C.byref(b), C.byref(n), _ptr(bbox)), "mh_models_range")
        return int(b.value), int(n.value), bbox

    def _view(self, ptr, cols):
        n = self.n_rows
        if n == 0 or not ptr:
            return np.zeros((0, cols), np.float32)
        buf = (C.c_float * (n * cols)).from_address(ptr)
        return np.frombuffer(buf, np.float32).reshape(n, cols)

    @property
    def desc(self) -> np.ndarray:
        """[rows,128] view (as parsed, not normalised); valid while the set lives and is not modified."""
        return self._view(self.L.mh_models_desc(self.h), 128)

    @property
    def xyz(self) -> np.ndarray:
        return self._view(self.L.mh_models_xyz(self.h), 3)

    @property
    def model_of(self) -> np.ndarray:
        out = np.zeros(self.n_rows, np.int32)
        for i in range(self.n_models):
            b, n, _ = self.model_range(i)
            out[b:b + n] = i
        return out

    def upload(self, ctx: "Context", first_model: int = 0, n_models: int | None = None):
        """Update() for a block of models: rows normalised on the device, ids stay global."""
        n_models = self.n_models - first_model if n_models is None else n_models
        ctx._ck(self.L.mh_db_upload_models(ctx.h, self.h, first_model, n_models), "mh_db_upload_models")

    def splice(self, ctx: "Context", op: int, model: int, set_index: int = 0):
        """addModel / removeModel on the resident DB: model `set_index` of this set -> Context.db_splice_models."""
        ctx.db_splice_models(op, model, self, set_index)

    def close(self):
        if self.h:
            self.L.mh_models_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
