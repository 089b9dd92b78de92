"""Frames with several cameras from device images (mh_frame_enqueue_images[_batch]), what needs no device:
the numpy restatement of the packing (tests/images_pack_ref.py, which the GPU tests take their expected lists from) on
hand-written cases, the new entry points in the built library and the Python bindings, the header under -std=gnu++98."""
import ctypes
import os
import subprocess

import numpy as np

import images_pack_ref as ref
from moped_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
NEW = ["mh_frame_enqueue_images", "mh_frame_enqueue_images_batch", "mh_frame_set_undistort_images", "mh_frame_image_counts"]


def _stage(n_images_total, cap, width=128):
    """A staging area whose every element names its place: row r, column c -> r * 1000 + c."""
    rows = n_images_total * cap
    desc = (np.arange(rows)[:, None] * 1000 + np.arange(width)[None, :]).astype(np.float32)
    xy = np.stack([np.arange(rows) + 0.25, np.arange(rows) + 0.5], 1).astype(np.float32)
    return desc, xy


def test_two_images_by_hand():
    cap = 4
    desc, xy = _stage(2, cap)
    d, u, img, clamped, totals = ref.pack(desc, xy, [3, 2], cap, 2)
    assert clamped.tolist() == [[3, 2]] and totals.tolist() == [5]
    # image 0's rows 0, 1, 2 then image 1's rows 4, 5 of the staging area
    assert d[:5, 0].tolist() == [0, 1000, 2000, 4000, 5000]
    assert u[:5, 0].tolist() == [0.25, 1.25, 2.25, 4.25, 5.25]
    assert img.tolist() == [0, 0, 0, 1, 1, -1, -1, -1]
    assert np.isnan(d[5:]).all() and np.isnan(u[5:]).all()            # rows past the total are not written


def test_clamping_and_empty_images():
    cap = 3
    desc, xy = _stage(3, cap)
    d, u, img, clamped, totals = ref.pack(desc, xy, [7, 0, 3], cap, 3)        # 7 > cap: the first 3; nothing of image 1
    assert clamped.tolist() == [[3, 0, 3]] and totals.tolist() == [6]
    assert d[:6, 0].tolist() == [0, 1000, 2000, 6000, 7000, 8000]
    assert img[:6].tolist() == [0, 0, 0, 2, 2, 2] and (img[6:] == -1).all()
    # nothing at all, and a count below zero counts as none
    d, u, img, clamped, totals = ref.pack(desc, xy, [0, -2, 0], cap, 3)
    assert totals.tolist() == [0] and (img == -1).all() and clamped.tolist() == [[0, 0, 0]]
    # an empty image in front and at the end
    _, _, img, clamped, totals = ref.pack(desc, xy, [0, 2, 0], cap, 3)
    assert img[:2].tolist() == [1, 1] and totals.tolist() == [2]


def test_eight_images_and_frame_strides():
    cap, n = 5, 8
    counts = [1, 0, 5, 9, 2, 0, 0, 3,      # frame 0: 1 + 0 + 5 + 5 + 2 + 0 + 0 + 3 = 16
              0, 0, 0, 0, 0, 0, 0, 0,      # frame 1: empty
              5, 5, 5, 5, 5, 5, 5, 5]      # frame 2: full
    desc, xy = _stage(3 * n, cap)
    d, u, img, clamped, totals = ref.pack(desc, xy, counts, cap, n)
    Q = n * cap
    assert totals.tolist() == [16, 0, 40]
    assert clamped[0].tolist() == [1, 0, 5, 5, 2, 0, 0, 3]
    assert img[:16].tolist() == [0] + [2] * 5 + [3] * 5 + [4] * 2 + [7] * 3
    want0 = [0] + [10 + k for k in range(5)] + [15 + k for k in range(5)] + [20, 21] + [35, 36, 37]
    assert (d[:16, 0] / 1000).astype(int).tolist() == want0
    assert (img[Q:2 * Q] == -1).all()                                 # frame 1 starts at row Q and holds nothing
    assert (d[2 * Q:3 * Q, 0] / 1000).astype(int).tolist() == list(range(2 * Q, 3 * Q))   # a full frame is a plain copy
    assert img[2 * Q:3 * Q].tolist() == list(np.repeat(np.arange(8), 5))
    assert np.array_equal(d[2 * Q:3 * Q, 1:] - d[2 * Q:3 * Q, :1], np.tile(np.arange(1, 128, dtype=np.float32), (Q, 1)))
    # layout() and pack_lists() tell the same story
    _, _, rows = ref.layout(counts, cap, n)
    lists = [(desc[j * cap:j * cap + max(c, 0)] if c <= cap else np.concatenate([desc[j * cap:(j + 1) * cap]] * 2),
              xy[j * cap:j * cap + max(c, 0)] if c <= cap else np.concatenate([xy[j * cap:(j + 1) * cap]] * 2))
             for j, c in enumerate(counts)]
    for f, (pd, pu, pi, pc) in enumerate(ref.pack_lists(lists, cap, n)):
        t = totals[f]
        assert np.array_equal(pd, d[f * Q:f * Q + t]) and np.array_equal(pu, u[f * Q:f * Q + t])
        assert np.array_equal(pi, img[f * Q:f * Q + t]) and np.array_equal(pi, rows[f][0])
        assert pc.tolist() == clamped[f].tolist()


def test_entry_points_are_exported_and_refuse_a_null_context():
    for name in NEW:
        assert name in capi.EXPORTS, name
    lib = ctypes.CDLL(capi.LIB_PATH)      # no compute call: there is no GPU here
    for name in NEW + ["mh_frame_features_image_dev"]:
        assert hasattr(lib, name), name
    MH_ERR_ARG = -1
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.mh_frame_enqueue_images.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, ctypes.c_uint64]
    lib.mh_frame_enqueue_images_batch.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.mh_frame_set_undistort_images.argtypes = [vp, vp, i32]
    lib.mh_frame_image_counts.argtypes = [vp, vp, i32, vp]
    lib.mh_frame_features_image_dev.argtypes = [vp, vp]
    assert lib.mh_frame_enqueue_images(None, None, 2, 640, 480, 1, 256, None, None, 1) == MH_ERR_ARG
    assert lib.mh_frame_enqueue_images_batch(None, None, 2, 2, 640, 480, 1, 256, None, None, None) == MH_ERR_ARG
    assert lib.mh_frame_set_undistort_images(None, None, 0) == MH_ERR_ARG
    n = ctypes.c_int32(0)
    assert lib.mh_frame_image_counts(None, None, 0, ctypes.byref(n)) == MH_ERR_ARG
    assert lib.mh_frame_features_image_dev(None, None) == MH_ERR_ARG
    for name in ("frame_enqueue_images", "frame_enqueue_images_batch", "frame_set_undistort_images", "frame_image_counts"):
        assert callable(getattr(capi.Context, name))
    from moped_amd.pipeline import FramePipeline
    assert callable(FramePipeline.enqueue_images) and callable(FramePipeline.enqueue_images_batch)


def test_header_still_compiles_as_gnu98():
    out = subprocess.run(["make", "-s", "-B", "-C", HOST, "check98", "check_ref"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
