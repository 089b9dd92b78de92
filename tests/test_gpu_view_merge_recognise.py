"""A model merged from two Kinect views and pruned to the rows both saw is recognised: frame 0 over the relief under the
trap pose goes in through FramePipeline.add_kinect_model, frame 3 through merge_kinect_view, then prune_model(min_views =
2).  An image frame and a Kinect frame of frame 0 and an image frame of frame 3 must each report the model with a pose
that reprojects the pruned rows onto the keypoints they came from within the project's criterion, mean reprojection
error below 1 px (README, "Parity"): frame 0's own keypoints for frame 0, the observing keypoints for frame 3.  The
fixture and `recognised` are those of tests/test_gpu_view_recognise.py."""
import os

import numpy as np
import pytest

import view_merge_ref as mref
import view_model_ref as ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
H, W = GOLD["gray0"].shape
CAP = 2048
POSE = ref.trap_pose()
MERGE = dict(merge_ratio=0.8, merge_dist=0.002)


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
    gray = {k: torch.from_numpy(np.ascontiguousarray(GOLD[k])).to(dev) for k in ("gray0", "gray3")}
    depth = torch.from_numpy(relief).to(dev)
    fill = torch.zeros((H, W), dtype=torch.float32, device=dev)   # every pixel measured
    torch.cuda.synchronize()
    pipe = FramePipeline(0, db, depth=2, max_queries=CAP, K=K, cam=CAM0)
    c2 = capi.Context(0)
    try:
        i, n0, bbox, stats = pipe.add_kinect_model(gray["gray0"], depth, name="relief", pose=POSE, max_keypoints=CAP)
        assert i == 2 and n0 == 586 and np.all(pipe.model_views(2) == 1)
        # who observes whom, by the reference on FEAT's own lists and MATCH's answer against the store as it is now
        xy0 = pipe.ctxs[0].sift(GOLD["gray0"])[0]
        xy3, _, d3 = pipe.ctxs[0].sift(GOLD["gray3"])
        d, x, mo = (np.ascontiguousarray(v) for v in (pipe.db.desc, pipe.db.xyz, pipe.db.model_of))
        assert c2.L.mh_db_upload_raw(c2.h, capi._ptr(d), capi._ptr(mo), capi._ptr(x), len(mo), 3, 0, 1) == 0
        _, acc, raw, d1, d2 = c2.normalize_match(d3, 0.8)
        dup = dict(idx=raw, d1=d1, d2=d2, model_of=mo, xyz=x, model=2, row_begin=800, row_end=800 + n0)
        why, _ = ref.verdicts(xy3, len(xy3), relief, None, POSE, dup=dup, **MERGE)
        obs = mref.observations(why, raw, 800, 800 + n0)
        gens = [c.db_generation() for c in pipe.ctxs]
        i, added, merged, bbox, stats = pipe.merge_kinect_view(2, gray["gray3"], depth, pose=POSE, max_keypoints=CAP, **MERGE)
        assert [c.db_generation() for c in pipe.ctxs] == [g + 1 for g in gens]   # the other slot adopted
        views = pipe.model_views(2)
        assert merged == len(obs) >= 300 and added == int((why == ref.KEEP).sum()) >= 100 and stats[ref.DUP] == (why == ref.DUP).sum()
        assert len(views) == n0 + added and np.array_equal(np.nonzero(views == 2)[0], sorted(obs)) and np.all(views[n0:] == 1)
        i, n_rows, bbox = pipe.prune_model(2, 2)
        assert n_rows == merged and pipe.ctxs[1].db_size() == (800 + merged, 3) and np.all(pipe.model_views(2) == 2)
        rows = np.array(sorted(obs))
        pts = pipe.db.xyz[800:]
        assert len(pts) == merged and np.array_equal(bbox[:3], pts.min(0)) and np.array_equal(bbox[3:], pts.max(0))
        # the store holds what the mirror says
        assert np.array_equal(pipe.ctxs[1].db_debug_fetch("xyz").view(np.uint32), pipe.db.xyz.view(np.uint32).reshape(-1))
        uv0 = xy0[rows]
        uv3 = xy3[[obs[r][0] for r in rows]]
        # the true pose itself: what the truncation and the averaging leave
        assert reprojection_error(POSE, pts, uv0) < 0.9 and reprojection_error(POSE, pts, uv3) < 0.9
        yield dict(pipe=pipe, gray=gray, depth=depth, fill=fill, xyz=pts, uv={"gray0": uv0, "gray3": uv3})
    finally:
        c2.close()
        pipe.close()


def recognised(t, objs, counts, what, image):
    print(what, "objects", len(objs), "counters", list(counts))
    assert len(objs) >= 1, (what, "no object", list(counts))
    o = objs[np.argmax(objs["score"])]
    err = reprojection_error(o["pose"], t["xyz"], t["uv"][image])
    print(what, "model", int(o["model"]), "pose", o["pose"].tolist(), "mean reprojection error", err, "px")
    assert o["model"] == 2, (what, list(counts))
    assert err < 1.0, (what, err)


@pytest.mark.parametrize("image", ["gray0", "gray3"])
def test_image_frame_finds_the_merged_model(taught, image):
    c = taught["pipe"].ctxs[0]
    c.frame_enqueue_image(taught["gray"][image].data_ptr(), W, H, True, CAP, K, CAM0, taught["pipe"].params, seed=5)
    objs, counts = taught["pipe"].fetch(0)
    recognised(taught, objs, counts, "image frame of " + image, image)


def test_kinect_frame_finds_the_merged_model(taught):
    c = taught["pipe"].ctxs[0]
    c.frame_set_depth_image(taught["depth"].data_ptr(), taught["fill"].data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
    c.frame_set_cluster_linkage(capi.default_linkage_params())
    try:
        c.frame_enqueue_image(taught["gray"]["gray0"].data_ptr(), W, H, True, CAP, K, CAM0, taught["pipe"].params, seed=5)
        objs, counts = taught["pipe"].fetch(0)
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
    recognised(taught, objs, counts, "Kinect frame", "gray0")
