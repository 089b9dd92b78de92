"""Hulls behind the frames (mh_frame_set_hulls, csrc/hull.hip's frame launch): with hulls on a frame's objects and counts
are bit for bit those of the same frame with hulls off; its hulls equal mh_object_hulls of the fetched objects, which
equal the float32 restatement of getConvexHull (tests/hull_ref.py); in a batch of 3 slot f equals frame f alone; a
frame without objects works; run_stage2 = 0 puts the launch behind POSE; the asynchronous block delivery equals the
per-slot fetches; a fetch after a frame with hulls off, a sharded enqueue with hulls on and a camera that the frame
does not have are refused."""
import ctypes as C

import numpy as np
import pytest

import hull_ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
Q = 2000
MAXV = 48
CAP = 16     # objects a fetch takes


@pytest.fixture(scope="module")
def scene():
    import torch
    db = synth.make_db(8, 2000)
    frames = [synth.make_frame(db, n_vis=n, seed=900 + i, Q=Q) for i, n in enumerate((2, 0, 3))]
    dev = torch.device("cuda:0")
    qd = torch.cat([torch.from_numpy(f.desc) for f in frames]).to(dev)
    uv = torch.cat([torch.from_numpy(f.uv) for f in frames]).to(dev)
    c = capi.Context(0)
    c.db_upload(db.desc, db.model_of, db.xyz, db.n_models)
    c.reserve_batch(Q, len(frames), 256, 64)
    yield db, frames, torch, qd, uv, c
    c.close()


def _alone(scene, f, prm, hulls):
    """Frame f alone on the scene's context, hulls on (MAXV) or off: (objects, counts[, hulls])."""
    db, frames, torch, qd, uv, c = scene
    work = qd[f * Q:(f + 1) * Q].clone()      # (the frame normalises its descriptors in place)
    torch.cuda.synchronize()
    c.frame_set_hulls(MAXV if hulls else 0)
    c.frame_enqueue(work.data_ptr(), uv[f * Q:(f + 1) * Q].data_ptr(), Q, synth.K_DEFAULT, synth.CAM_IDENTITY, prm, 77 + f)
    objs, counts = c.frame_fetch(CAP)
    return (objs, counts, c.frame_fetch_hulls(None, CAP, MAXV)) if hulls else (objs, counts)


def _same_objects(a, b):
    return (len(a) == len(b) and np.array_equal(a["model"], b["model"]) and
            np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32)) and
            np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32)) and np.array_equal(a["n_points"], b["n_points"]))


def _same_hulls(a, b):
    return (len(a[0]) == len(b[0]) and all(hull_ref.same_vertices(x, y) for x, y in zip(a[0], b[0])) and
            np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))


def _check_against_the_restatement(scene, objs, hulls):
    db, frames, torch, qd, uv, c = scene
    assert len(hulls[0]) == len(objs)
    direct = c.object_hulls(objs["model"], objs["pose"], synth.K_DEFAULT, synth.CAM_IDENTITY, MAXV)
    assert _same_hulls(hulls, direct)
    for o, ob in enumerate(objs):
        xyz = db.xyz[db.model_of == ob["model"]]
        want, behind = hull_ref.object_hull(ob["pose"], xyz, synth.K_DEFAULT, synth.CAM_IDENTITY)
        assert hulls[1][o] == len(want) <= MAXV and hulls[2][o] == behind
        assert hull_ref.same_vertices(hulls[0][o], want)
        assert np.array_equal(hulls[3][o], hull_ref.bbox_corners(ob["pose"], xyz, synth.K_DEFAULT, synth.CAM_IDENTITY))


@pytest.mark.parametrize("stage2", [1, 0])
def test_frame_with_hulls_is_the_frame_without_plus_its_hulls(scene, stage2):
    prm = capi.default_frame_params()
    prm.run_stage2 = stage2
    off = _alone(scene, 0, prm, False)
    on = _alone(scene, 0, prm, True)
    assert len(off[0]) >= 2
    assert _same_objects(on[0], off[0]) and np.array_equal(on[1], off[1])
    _check_against_the_restatement(scene, on[0], on[2])
    none = _alone(scene, 1, prm, True)        # the frame that shows no model
    assert len(none[0]) == 0 and len(none[2][0]) == 0


def test_batch_slots_equal_the_frames_alone_and_the_block_delivery_equals_the_fetches(scene):
    db, frames, torch, qd, uv, c = scene
    prm = capi.default_frame_params()
    alone = [_alone(scene, f, prm, True) for f in range(3)]
    B = 3
    work = qd.clone()
    torch.cuda.synchronize()
    c.frame_set_hulls(MAXV)
    c.frame_enqueue_batch(work.data_ptr(), uv.data_ptr(), Q, B, synth.K_DEFAULT, synth.CAM_IDENTITY, prm, [77 + f for f in range(B)])
    dt = capi.hull_block_dtype(CAP, MAXV)
    block = c.host_alloc(B * dt.itemsize)
    block[:] = 0xAB
    try:
        c.frame_fetch_batch_hulls_async(B, CAP, block.ctypes.data)
        with pytest.raises(capi.MhError, match="not been waited for"):
            c.frame_fetch_batch_hulls_async(B, CAP, block.ctypes.data)
        c.frame_fetch_wait()
        recs = block.view(dt)
        total = 0
        for f in range(B):
            objs, counts = c.frame_fetch_slot(f, CAP)
            hulls = c.frame_fetch_hulls(f, CAP, MAXV)
            assert _same_objects(objs, alone[f][0]) and np.array_equal(counts, alone[f][1]), f
            assert _same_hulls(hulls, alone[f][2]), f
            _check_against_the_restatement(scene, objs, hulls)
            for o in range(len(objs)):
                r = recs[f]["objects"][o]
                assert r["n_vertices"] == hulls[1][o] and r["n_behind"] == hulls[2][o]
                assert np.array_equal(r["bbox_uv"], hulls[3][o])
                assert np.array_equal(r["hull_xy"][:len(hulls[0][o])], hulls[0][o])
            total += len(objs)
        assert total >= 4 and len(alone[1][0]) == 0
    finally:
        c.host_free(block)


def test_refusals(scene):
    db, frames, torch, qd, uv, c = scene
    prm = capi.default_frame_params()
    good = _alone(scene, 2, prm, True)
    # a frame with hulls off: its slot holds none
    _alone(scene, 2, prm, False)
    with pytest.raises(capi.MhError, match="without hulls"):
        c.frame_fetch_hulls(None, CAP, MAXV)
    with pytest.raises(capi.MhError, match="without hulls"):
        c.frame_fetch_batch_hulls_async(1, CAP, 1 << 20)
    # hulls on: the sharded entry points and a camera the frame does not have are refused before anything is enqueued
    c.frame_set_hulls(MAXV)
    launches = c.match_kernel_launches()
    gathered = torch.zeros(3 * Q, dtype=torch.int32, device=qd.device)
    with pytest.raises(capi.MhError, match="sharded"):
        c.frame_enqueue_rest(uv.data_ptr(), Q, gathered.data_ptr(), 1, synth.K_DEFAULT, synth.CAM_IDENTITY, prm, 5)
    with pytest.raises(capi.MhError, match="sharded"):
        c.frame_enqueue_rest_frames(uv.data_ptr(), Q, gathered.data_ptr(), 1, 3 * Q, Q, 2, synth.K_DEFAULT, synth.CAM_IDENTITY, prm, [5, 6])
    c.frame_set_hulls(MAXV, image=1)
    work = qd[2 * Q:3 * Q].clone()
    with pytest.raises(capi.MhError, match="camera"):
        c.frame_enqueue(work.data_ptr(), uv[2 * Q:].data_ptr(), Q, synth.K_DEFAULT, synth.CAM_IDENTITY, prm, 79)
    assert c.match_kernel_launches() == launches              # no MATCH was launched for any of them
    assert c.L.mh_frame_set_hulls(c.h, -1, 0) == capi.MH_ERR_ARG and c.L.mh_frame_set_hulls(c.h, 8, 8) == capi.MH_ERR_ARG   # (8: MH_MAX_IMAGES)
    again = _alone(scene, 2, prm, True)                        # the context is as it was
    assert _same_objects(again[0], good[0]) and _same_hulls(again[2], good[2])
    c.frame_set_hulls(0)


def test_hulls_in_the_second_camera_of_a_two_camera_frame():
    """mh_frame_set_hulls' `image`: the hulls of a several-camera frame are those of its objects in THAT camera; a
    camera the frame does not have is refused."""
    db = synth.make_db(6, 1500, seed=8)
    cams = [synth.camera_pose(0.0), synth.camera_pose(-0.12, (0.10, 0.0, 0.0))]
    fr = synth.make_frame_images(db, cams, n_vis=2, seed=5, q_per_image=900, pts_per_obj=130)
    prm = capi.default_frame_params()
    c = capi.Context(0)
    try:
        c.db_upload(db.desc, db.model_of, db.xyz, db.n_models)
        off = c.frame_run_host(fr.desc.copy(), fr.uv, fr.Ks, fr.cams, prm, 9, fr.image, max_objects=CAP)
        assert len(off[0]) >= 2
        for image in (0, 1):
            c.frame_set_hulls(MAXV, image)
            objs, counts = c.frame_run_host(fr.desc.copy(), fr.uv, fr.Ks, fr.cams, prm, 9, fr.image, max_objects=CAP)
            assert _same_objects(objs, off[0]) and np.array_equal(counts, off[1])
            hulls = c.frame_fetch_hulls(None, CAP, MAXV)
            assert _same_hulls(hulls, c.object_hulls(objs["model"], objs["pose"], fr.Ks[image], fr.cams[image], MAXV))
            for o, ob in enumerate(objs):
                want, _ = hull_ref.object_hull(ob["pose"], db.xyz[db.model_of == ob["model"]], fr.Ks[image], fr.cams[image])
                assert hull_ref.same_vertices(hulls[0][o], want)
        c.frame_set_hulls(MAXV, 2)
        with pytest.raises(capi.MhError, match="camera"):
            c.frame_run_host(fr.desc.copy(), fr.uv, fr.Ks, fr.cams, prm, 9, fr.image, max_objects=CAP)
    finally:
        c.close()
