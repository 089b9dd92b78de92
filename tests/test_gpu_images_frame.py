"""Frames with several cameras from device images (mh_frame_enqueue_images[_batch]): images in, objects out, the
keypoint counts never on the host.  Everything is compared bit for bit with the path the suite already trusts for a host
that knows the counts: Context.sift per image, the lists concatenated on the host (tests/images_pack_ref.py),
mh_frame_set_images + mh_frame_enqueue.

Scene: the planted planar model of tests/test_gpu_image_frame.py (model 0 = frame 0's keypoints at z = 0.8, model 1 =
500 clutter rows); images: the two bundled 640x480 frames (586 and 599 keypoints) and a constant-grey one (none)."""
import json
import os

import numpy as np
import pytest

import images_pack_ref as ref
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
CAP = 1024
H, W = GOLD["gray0"].shape


class Scene:
    pass


@pytest.fixture(scope="module")
def scene():
    import torch
    s = Scene()
    s.torch = torch
    s.dev = torch.device("cuda:0")
    s.c = c = capi.Context(0)
    s.prm = capi.default_frame_params()
    gray = {"g0": GOLD["gray0"], "g3": GOLD["gray3"], "blank": np.full((H, W), 128, np.uint8)}
    s.lists = {}
    for name, g in gray.items():                              # FEAT on the host's side, once: (desc, xy) in list order
        xy, _, desc = c.sift(g)
        s.lists[name] = (desc, xy)
    assert [len(s.lists[n][0]) for n in ("g0", "g3", "blank")] == [586, 599, 0]
    s.img = {name: torch.from_numpy(g).to(s.dev) for name, g in gray.items()}
    desc0, xy0 = s.lists["g0"]
    z = np.float32(0.8)
    xyz = np.stack([(xy0[:, 0] - K[2]) / K[0] * z, (xy0[:, 1] - K[3]) / K[1] * z, np.full(len(xy0), z)], 1).astype(np.float32)
    rng = np.random.default_rng(7)
    clutter = np.abs(rng.normal(size=(500, 128))).astype(np.float32)
    c.db_upload(orclib.normalize(np.concatenate([desc0, clutter])),
                np.concatenate([np.zeros(len(xy0), np.int32), np.ones(500, np.int32)]),
                np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)]), 2)
    c.reserve(3 * 2 * CAP)                                    # the largest call below: 3 frames x 2 cameras
    torch.cuda.synchronize()
    s.memo = {}
    yield s
    c.close()


def rig(n, K1=None):
    Ks = [K.copy() for _ in range(n)]
    if K1 is not None:
        Ks[1] = np.asarray(K1, np.float32)
    return Ks, [CAM0.copy() for _ in range(n)]


def reference(s, names, Ks, cams, seed, cap=CAP):
    """The host round trip: the packed list built from the per-image lists with the counts known, then
    mh_frame_set_images + mh_frame_enqueue.  -> (objects, counts, normalised descriptors, uv, image index); computed
    once per case and shared."""
    torch, c = s.torch, s.c
    key = (tuple(names), tuple(np.concatenate(Ks).tolist()), seed, cap)
    if key in s.memo:
        return s.memo[key]
    (desc, xy, image, _), = ref.pack_lists([s.lists[n] for n in names], cap, len(names))
    q_desc, q_uv, q_img = (torch.from_numpy(a).to(s.dev) for a in (desc, xy, image))
    torch.cuda.synchronize()
    c.frame_set_images(q_img.data_ptr(), Ks, cams)
    try:
        c.frame_enqueue(q_desc.data_ptr(), q_uv.data_ptr(), len(desc), Ks[0], cams[0], s.prm, seed)
        objs, counts = c.frame_fetch()
    finally:
        c.frame_set_images(None)
    s.memo[key] = (objs, counts, q_desc.cpu().numpy(), xy, image)
    return s.memo[key]


def device_list(s, n):
    """The first n rows of the frame's device-side list: (descriptors, uv, image index)."""
    from moped_amd.pipeline import _DevMem
    torch, c = s.torch, s.c
    d_ptr, u_ptr, _ = c.frame_features_dev()
    i_ptr = c.frame_features_image_dev()
    if n == 0:
        return np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.int32)
    get = lambda p, shape, t: torch.as_tensor(_DevMem(p, shape, t), device=s.dev).cpu().numpy()
    return get(d_ptr, (n, 128), "<f4"), get(u_ptr, (n, 2), "<f4"), get(i_ptr, (n,), "<i4")


def enqueue(s, names, Ks, cams, seed, cap=CAP):
    s.c.frame_enqueue_images([s.img[n].data_ptr() for n in names], W, H, True, cap, Ks, cams, s.prm, seed)
    return s.c.frame_fetch()


def check_against_reference(s, names, Ks, cams, seed, cap=CAP, repeats=2):
    want, want_counts, want_desc, want_uv, want_img = reference(s, names, Ks, cams, seed, cap)
    for _ in range(repeats):                                  # (the second launch is sized by the first frame's count)
        got, got_counts = enqueue(s, names, Ks, cams, seed, cap)
        print(f"{names} cap {cap}: objects {len(got)} / {len(want)}, counts {got_counts.tolist()} / {want_counts.tolist()}")
        assert np.array_equal(got_counts, want_counts)
        assert got.tobytes() == want.tobytes()
        assert s.c.frame_keypoints() == len(want_img)
        assert s.c.frame_image_counts().tolist() == [min(len(s.lists[n][0]), cap) for n in names]
        dd, uu, ii = device_list(s, len(want_img))
        assert np.array_equal(dd.view(np.uint32), want_desc.view(np.uint32))
        assert np.array_equal(uu.view(np.uint32), want_uv.view(np.uint32))
        assert np.array_equal(ii, want_img)
    return got, got_counts


def test_two_cameras_equal_the_host_round_trip(scene):
    s = scene
    Ks, cams = rig(2)
    got, counts = check_against_reference(s, ["g0", "g3"], Ks, cams, seed=11)
    assert s.c.frame_keypoints() == 586 + 599 and s.c.frame_image_counts().tolist() == [586, 599]
    _, _, ii = device_list(s, 586 + 599)
    assert ii.tolist() == [0] * 586 + [1] * 599
    assert len(got) >= 1 and (got["model"] == 0).any()        # both bundled frames show the planted plane
    # every image goes through its OWN camera: another K for camera 1 -- still equal, and other objects
    Ks2, _ = rig(2, K1=[K[0], K[1], K[2] + 7, K[3]])
    got2, _ = check_against_reference(s, ["g0", "g3"], Ks2, cams, seed=11)
    assert got2.tobytes() != got.tobytes()


@pytest.mark.parametrize("cap", [256, 200])                   # (200: no multiple of the 64 rows a workgroup packs)
def test_clamping_and_an_empty_camera(scene, cap):
    s = scene
    Ks, cams = rig(3)
    names = ["g3", "blank", "g0"]
    check_against_reference(s, names, Ks, cams, seed=12, cap=cap)
    assert s.c.frame_image_counts().tolist() == [cap, 0, cap] and s.c.frame_keypoints() == 2 * cap
    dd, uu, ii = device_list(s, 2 * cap)
    assert ii.tolist() == [0] * cap + [2] * cap               # the first `cap` of image 0, nothing of image 1, image 2's
    assert np.array_equal(uu, np.concatenate([s.lists["g3"][1][:cap], s.lists["g0"][1][:cap]]))


def test_a_rig_that_sees_nothing(scene):
    s = scene
    Ks, cams = rig(2)
    objs, counts = enqueue(s, ["blank", "blank"], Ks, cams, seed=13)
    assert len(objs) == 0 and counts[0] == 0
    assert s.c.frame_keypoints() == 0 and s.c.frame_image_counts().tolist() == [0, 0]


def test_one_image_is_the_single_image_path(scene):
    s = scene
    c = s.c
    c.frame_enqueue_image(s.img["g0"].data_ptr(), W, H, True, CAP, K, CAM0, s.prm, seed=14)
    want, want_counts = c.frame_fetch()
    from moped_amd.pipeline import _DevMem
    d_ptr, u_ptr, _ = c.frame_features_dev()
    want_desc = s.torch.as_tensor(_DevMem(d_ptr, (586, 128), "<f4"), device=s.dev).cpu().numpy()
    for _ in range(2):
        got, got_counts = enqueue(s, ["g0"], [K], [CAM0], seed=14)
        assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts)
        assert c.frame_keypoints() == 586 and c.frame_image_counts().tolist() == [586]
        dd, _, ii = device_list(s, 586)
        assert np.array_equal(dd.view(np.uint32), want_desc.view(np.uint32)) and not ii.any()
    assert len(want) >= 1


def test_batch_equals_its_frames_alone(scene):
    s = scene
    c = s.c
    Ks, cams = rig(2)
    c.frame_enqueue_image(s.img["g0"].data_ptr(), W, H, True, CAP, K, CAM0, s.prm, seed=20)
    plain = c.frame_fetch()
    frames = [["g0", "g3"], ["g3", "blank"], ["blank", "g0"]]
    seeds = [21, 22, 23]
    alone = [enqueue(s, names, Ks, cams, seed) for names, seed in zip(frames, seeds)]
    ptrs = [s.img[n].data_ptr() for names in frames for n in names]
    for _ in range(2):                                        # twice over the same arenas
        c.frame_enqueue_images_batch(ptrs, 2, W, H, True, CAP, Ks, cams, s.prm, seeds)
        for f, (want, want_counts) in enumerate(alone):
            got, got_counts = c.frame_fetch_slot(f)
            print(f"slot {f}: objects {len(got)} / {len(want)}, counts {got_counts.tolist()} / {want_counts.tolist()}")
            assert np.array_equal(got_counts, want_counts)
            assert got.tobytes() == want.tobytes()
    assert all(len(a[0]) >= 1 for a in alone)
    # the frames alone are the host round trip's (so the batch is, too)
    for names, seed, (got, got_counts) in zip(frames, seeds, alone):
        want, want_counts, *_ = reference(s, names, Ks, cams, seed)
        assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts)
    # the context is a one-camera context again: no image index of the batch is left behind
    c.frame_enqueue_image(s.img["g0"].data_ptr(), W, H, True, CAP, K, CAM0, s.prm, seed=20)
    again = c.frame_fetch()
    assert again[0].tobytes() == plain[0].tobytes() and np.array_equal(again[1], plain[1])
    # ... and so is a frame from features
    desc, xy = s.lists["g0"]
    q_desc, q_uv = s.torch.from_numpy(desc).to(s.dev), s.torch.from_numpy(xy).to(s.dev)
    s.torch.cuda.synchronize()
    c.frame_enqueue(q_desc.data_ptr(), q_uv.data_ptr(), len(desc), K, CAM0, s.prm, seed=20)
    feat = c.frame_fetch()
    assert feat[0].tobytes() == plain[0].tobytes() and np.array_equal(feat[1], plain[1])


def test_undistortion_per_camera(scene):
    s = scene
    torch, c = s.torch, s.c
    cal = json.load(open(os.path.join(HERE, "golden", "undistort_cameras.json")))
    a, b = cal["launch"], cal["kinect_rgb"]
    Ks = [np.array(a["K"], np.float32), np.array(b["K"], np.float32)]
    dists = [np.array(a["dist"], np.float32), np.array(b["dist"], np.float32)]
    cams = [CAM0.copy(), CAM0.copy()]
    names = ["g0", "g3"]
    ptrs = [s.img[n].data_ptr() for n in names]

    def remapped_first(ds):
        out = [torch.empty_like(s.img[n]) for n in names]
        for n, o, k, d in zip(names, out, Ks, ds):
            c.undistort_dev(s.img[n].data_ptr(), o.data_ptr(), W, H, k, d)
        c.frame_set_undistort_images(None)
        c.frame_enqueue_images([o.data_ptr() for o in out], W, H, True, CAP, Ks, cams, s.prm, 31)
        return c.frame_fetch()

    def on_the_way(ds):
        c.frame_set_undistort_images(ds)
        try:
            c.frame_enqueue_images(ptrs, W, H, True, CAP, Ks, cams, s.prm, 31)
            return c.frame_fetch(), c.frame_image_counts().tolist()
        finally:
            c.frame_set_undistort_images(None)

    want, want_counts = remapped_first(dists)
    (got, got_counts), per_image = on_the_way(dists)
    print(f"undistorted rig: objects {len(got)} / {len(want)}, counts {got_counts.tolist()}, keypoints {per_image}")
    assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts)
    assert min(per_image) > 100
    # the coefficients belong to their cameras: swapped, the frame is another one
    (swapped, swapped_counts), per_image_swapped = on_the_way(dists[::-1])
    want_s, want_s_counts = remapped_first(dists[::-1])
    assert swapped.tobytes() == want_s.tobytes() and np.array_equal(swapped_counts, want_s_counts)
    assert (swapped.tobytes(), swapped_counts.tolist(), per_image_swapped) != (got.tobytes(), got_counts.tolist(), per_image)
    # coefficients for another number of cameras are refused, and off is off
    c.frame_set_undistort_images(dists + dists[:1])
    with pytest.raises(capi.MhError):
        c.frame_enqueue_images(ptrs, W, H, True, CAP, Ks, cams, s.prm, 31)
    c.frame_set_undistort_images(None)
    Ks1, cams1 = rig(2)
    check_against_reference(s, names, Ks1, cams1, seed=11, repeats=1)


def test_refusals_leave_the_context_as_it_was(scene):
    s = scene
    torch, c = s.torch, s.c
    Ks, cams = rig(2)
    g = s.img["g0"].data_ptr()
    with pytest.raises(capi.MhError):                         # 9 cameras
        K9, c9 = rig(9)
        c.frame_enqueue_images([g] * 9, W, H, True, 64, K9, c9, s.prm, 1)
    check_against_reference(s, ["g0", "g3"], Ks, cams, seed=11, repeats=1)
    with pytest.raises(capi.MhError):                         # 17 frames x 2 cameras: more images than one FEAT launch takes
        c.frame_enqueue_images_batch([g] * 34, 2, W, H, True, 64, Ks, cams, s.prm, list(range(17)))
    check_against_reference(s, ["g0", "g3"], Ks, cams, seed=11, repeats=1)
    depth = torch.zeros((H, W, 4), dtype=torch.float32, device=s.dev)
    c.frame_set_depth_image(depth.data_ptr(), 0, W, H, capi.DEPTH_BACKPROJECTION)
    try:
        with pytest.raises(capi.MhError):                     # a depth map belongs to one camera
            c.frame_enqueue_images([g, g], W, H, True, CAP, Ks, cams, s.prm, 1)
        with pytest.raises(capi.MhError):
            c.frame_enqueue_images_batch([g, g], 2, W, H, True, CAP, Ks, cams, s.prm, [1])
    finally:
        c.frame_set_depth_image(0, 0, W, H, capi.DEPTH_BACKPROJECTION)
    check_against_reference(s, ["g0", "g3"], Ks, cams, seed=11, repeats=1)
