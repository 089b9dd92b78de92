"""A model taught from one Kinect view is recognised: frame 0 over the relief under the trap pose goes in through
FramePipeline.add_kinect_model, then (a) a moped2 image frame of the same image (mean shift, no depth map) and (b) a
Kinect frame of the same image and map (moped3d's linkage clusterer, which needs the map; depth rules at their default,
off) must each report the taught model with a pose that reprojects the taught rows onto their keypoints within the
project's criterion: mean reprojection error below 1 px (README, "Parity").

The taught points are those of the keypoints' truncated pixels, so even the true pose leaves the fractional part of
(u, v) as error -- 0.38 px in the mean once a pose has absorbed its offset; the criterion has room for that."""
import os

import numpy as np
import pytest

import view_model_ref as ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
H, W = GOLD["gray0"].shape
CAP = 2048
POSE = ref.trap_pose()


def reprojection_error(pose, xyz, uv):
    """Mean pixel distance between the taught keypoints and their model points seen under `pose` by the camera K."""
    q = np.asarray(pose[:4], np.float64)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    p = xyz.astype(np.float64) @ R.T + np.asarray(pose[4:7], np.float64)
    proj = np.stack([p[:, 0] / p[:, 2] * K[0] + K[2], p[:, 1] / p[:, 2] * K[1] + K[3]], 1)
    return float(np.linalg.norm(proj - uv.astype(np.float64), axis=1).mean())


@pytest.fixture(scope="module")
def taught():
    import torch
    from moped_amd.pipeline import FramePipeline, ShardedDB
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x91A2)
    desc = np.abs(rng.normal(size=(800, 128))).astype(np.float32)   # two models nobody sees
    xyz = rng.uniform(-0.1, 0.1, (800, 3)).astype(np.float32)
    db = ShardedDB(desc, xyz, np.repeat(np.arange(2, dtype=np.int32), [300, 500]), 2)
    relief = ref.relief_map(W, H, tuple(K))
    gray = torch.from_numpy(np.ascontiguousarray(GOLD["gray0"])).to(dev)
    depth = torch.from_numpy(relief).to(dev)
    fill = torch.zeros((H, W), dtype=torch.float32, device=dev)   # every pixel measured
    torch.cuda.synchronize()
    pipe = FramePipeline(0, db, depth=1, max_queries=CAP, K=K, cam=CAM0)
    i, n, bbox, stats = pipe.add_kinect_model(gray, depth, name="relief", pose=POSE, max_keypoints=CAP)
    # the rows and the keypoints they came from, by the reference on FEAT's own list
    xy, _, d = pipe.ctxs[0].sift(GOLD["gray0"])
    wd, wx, wb, ws, idx = ref.rows(d, xy, len(xy), relief, None, POSE)
    assert i == 2 and n == len(idx) == len(xy) > 500 and np.array_equal(stats, ws)
    assert np.array_equal(pipe.db.xyz[800:].view(np.uint32), wx.view(np.uint32))
    # the true pose itself: what the truncation alone leaves
    assert reprojection_error(POSE, wx, xy[idx]) < 0.9
    yield dict(pipe=pipe, gray=gray, depth=depth, fill=fill, xyz=wx, uv=xy[idx])
    pipe.close()


def recognised(t, objs, counts, what):
    print(what, "objects", len(objs), "counters", list(counts))
    assert len(objs) >= 1, (what, "no object", list(counts))
    o = objs[np.argmax(objs["score"])]
    err = reprojection_error(o["pose"], t["xyz"], t["uv"])
    print(what, "model", int(o["model"]), "pose", o["pose"].tolist(), "mean reprojection error", err, "px")
    assert o["model"] == 2, (what, list(counts))
    assert err < 1.0, (what, err)


def test_image_frame_finds_the_taught_model(taught):
    c = taught["pipe"].ctxs[0]
    c.frame_enqueue_image(taught["gray"].data_ptr(), W, H, True, CAP, K, CAM0, taught["pipe"].params, seed=5)
    objs, counts = taught["pipe"].fetch(0)
    recognised(taught, objs, counts, "image frame")


def test_kinect_frame_finds_the_taught_model(taught):
    c = taught["pipe"].ctxs[0]
    c.frame_set_depth_image(taught["depth"].data_ptr(), taught["fill"].data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
    c.frame_set_cluster_linkage(capi.default_linkage_params())
    try:
        c.frame_enqueue_image(taught["gray"].data_ptr(), W, H, True, CAP, K, CAM0, taught["pipe"].params, seed=5)
        objs, counts = taught["pipe"].fetch(0)
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
    recognised(taught, objs, counts, "Kinect frame")
