"""UNDISTORTED_IMAGE on the device (moped_amd/csrc/undistort.hip) against tests/undistort_ref.py, the restatement of
UTIL_UNDISTORT (src/util/UTIL_UNDISTORT.hpp): the float maps bit for bit, the undistorted bytes bit for bit, the
resident image path equal to the host steps, and a distorted scene that is found only with undistortion."""
import ctypes as C
import os

import numpy as np
import pytest

import orclib
import undistort_ref as ur
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
CAMS = ur.cameras()
LAUNCH_K, LAUNCH_D = CAMS["launch"]
CAM0 = synth.CAM_IDENTITY
CAP = 4096


def _random_cameras(n, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        f = rng.uniform(300, 1200)
        K = [f, f * rng.uniform(0.97, 1.03), rng.uniform(250, 390), rng.uniform(190, 290)]
        dist = [rng.uniform(-0.4, 0.3), rng.uniform(-0.2, 0.3), rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3)]
        out.append((K, dist))
    return out


CAMERAS = [
    (LAUNCH_K, [0, 0, 0, 0]),                               # zero
    CAMS["node_default"],                                   # the ROS node's 1e-12
    (LAUNCH_K, LAUNCH_D),                                   # moped2/startmoped.launch
    ([300.0, 300.0, 320.0, 240.0], [-0.5, 0, 0, 0]),        # strong barrel: folds, maps outside the frame
    (LAUNCH_K, [0.2, 0, 0, 0]),                             # pincushion
    (LAUNCH_K, [0, 0, 0.01, -0.008]),                       # tangential only
] + _random_cameras(8)


def _images():
    rng = np.random.default_rng(5)
    return [GOLD["gray0"], GOLD["gray3"], synth.textured_image(3), rng.integers(0, 256, (480, 640), dtype=np.uint8)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def test_maps_equal_the_restatement_bit_for_bit(ctx):
    for w, h in [(640, 480), (641, 479), (1280, 960), (13, 17)]:
        for K, dist in CAMERAS:
            mx, my = ctx.undistort_map(w, h, K, dist)
            ex, ey = ur.maps(w, h, K, dist)
            assert mx.view(np.uint32).tobytes() == ex.view(np.uint32).tobytes(), (w, h, K, dist)
            assert my.view(np.uint32).tobytes() == ey.view(np.uint32).tobytes(), (w, h, K, dist)
    # the strong barrel camera does reach outside the frame at 1280x960
    mx, _ = ctx.undistort_map(1280, 960, *CAMERAS[3])
    assert (mx < 0).any() or (mx >= 1280).any()


def test_bytes_equal_the_restatement_host_dev_and_in_place(ctx, torch_dev):
    torch, dev = torch_dev
    imgs = _images()
    want = {(a, b): ur.undistort(img, *CAMERAS[b]) for a, img in enumerate(imgs) for b in range(len(CAMERAS))}
    src = [torch.from_numpy(img).to(dev) for img in imgs]
    dst = torch.empty((480, 640), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # twice round 14 cameras on one context: more often than its cache of 8 holds
    for rep in range(2):
        for b, (K, dist) in enumerate(CAMERAS):
            for a, img in enumerate(imgs):
                e = want[(a, b)]
                if (a + rep) % 2 == 0:
                    assert np.array_equal(ctx.undistort(img, K, dist), e), (a, b)
                else:
                    ctx.undistort_dev(src[a].data_ptr(), dst.data_ptr(), 640, 480, K, dist)
                    ctx.synchronize()
                    assert np.array_equal(dst.cpu().numpy(), e), (a, b)
    # in place: out == in through the C entry point
    buf = np.ascontiguousarray(imgs[0]).copy()
    k, d = np.float32(LAUNCH_K), np.float32(LAUNCH_D)
    rc = ctx.L.mh_undistort(ctx.h, capi._ptr(buf), capi._ptr(buf), 640, 480, capi._ptr(k), capi._ptr(d))
    assert rc == capi.MH_OK and np.array_equal(buf, want[(0, 2)])
    # other sizes, host path
    rng = np.random.default_rng(9)
    for w, h in [(641, 479), (13, 17)]:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for K, dist in CAMERAS[:6]:
            assert np.array_equal(ctx.undistort(img, K, dist), ur.undistort(img, K, dist)), (w, h, K, dist)


def test_zero_distortion_is_the_identity(ctx):
    for img in _images():
        assert np.array_equal(ctx.undistort(img, LAUNCH_K, [0, 0, 0, 0]), img)
        assert np.array_equal(ctx.undistort(img, *CAMS["node_default"]), img)


def _scene_db(c, gray, K):
    """The planar model of test_gpu_image_frame.py: the image's keypoints back-projected to z = 0.8, plus clutter."""
    xy, _, desc = c.sift(gray)
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1)
    rng = np.random.default_rng(7)
    clutter = np.abs(rng.normal(size=(500, 128))).astype(np.float32)
    db_desc = orclib.normalize(np.concatenate([desc, clutter]))
    db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3))]).astype(np.float32)
    model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
    c.db_upload(db_desc, model_of, db_xyz, 2)
    c.reserve(4 * CAP)
    return db_desc, model_of, db_xyz


def test_resident_path_equals_the_host_steps(torch_dev):
    torch, dev = torch_dev
    K = np.float32(LAUNCH_K)
    c = capi.Context(0)
    try:
        db = _scene_db(c, GOLD["gray0"], K)
        prm = capi.default_frame_params()
        imgs = [GOLD["gray0"], GOLD["gray3"], synth.textured_image(4, fine=0.25), GOLD["gray0"]]
        g = [torch.from_numpy(x).to(dev) for x in imgs]
        torch.cuda.synchronize()
        want = []
        for f, img in enumerate(imgs):
            und = c.undistort(img, K, LAUNCH_D)                    # UNDISTORTED_IMAGE, then FEAT, then the frame
            xy, _, desc = c.sift(und)
            q_desc, q_uv = torch.from_numpy(desc).to(dev), torch.from_numpy(xy).to(dev)
            torch.cuda.synchronize()
            c.frame_enqueue(q_desc.data_ptr(), q_uv.data_ptr(), len(xy), K, CAM0, prm, seed=20 + f)
            objs, counts = c.frame_fetch()
            want.append((objs, counts, len(xy)))
        c.frame_set_undistort(LAUNCH_D)
        for f in range(len(imgs)):
            c.frame_enqueue_image(g[f].data_ptr(), 640, 480, True, CAP, K, CAM0, prm, seed=20 + f)
            objs, counts = c.frame_fetch()
            assert c.frame_keypoints() == want[f][2]
            assert np.array_equal(counts, want[f][1]) and objs.tobytes() == want[f][0].tobytes(), f
        assert len(want[0][0]) >= 1
        c.frame_enqueue_image_batch([x.data_ptr() for x in g], 640, 480, True, CAP, K, CAM0, prm, [20, 21, 22, 23])
        for f in range(len(imgs)):
            objs, counts = c.frame_fetch_slot(f)
            assert np.array_equal(counts, want[f][1]) and objs.tobytes() == want[f][0].tobytes(), f
        # off again: what a fresh context gives
        c.frame_set_undistort(None)
        c.frame_enqueue_image(g[1].data_ptr(), 640, 480, True, CAP, K, CAM0, prm, seed=30)
        got = c.frame_fetch()
    finally:
        c.close()
    fresh = capi.Context(0)
    try:
        fresh.db_upload(*db[:2], db[2], 2)
        fresh.reserve(4 * CAP)
        fresh.frame_enqueue_image(g[1].data_ptr(), 640, 480, True, CAP, K, CAM0, prm, seed=30)
        ref = fresh.frame_fetch()
    finally:
        fresh.close()
    assert np.array_equal(got[1], ref[1]) and got[0].tobytes() == ref[0].tobytes()


def _distort_scene(K, dist, w=640, h=480, margin=48):
    """A planar texture seen through the camera: the pinhole image is the canvas's middle; every distorted pixel
    samples the canvas where the distortion model sends it back (fixed-point iteration in float64)."""
    canvas = synth.textured_image(6, h + 2 * margin, w + 2 * margin, fine=0.25).astype(np.float64)
    fx, fy, cx, cy = np.float64(K)
    k1, k2, p1, p2 = np.float64(dist)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xd, yd = (j - cx) / fx, (i - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(100):
        r2 = x * x + y * y
        kr = 1 + k1 * r2 + k2 * r2 * r2
        x = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / kr
        y = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / kr
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 * r2
    u = fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
    v = fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
    assert np.hypot(u - j, v - i).max() < 1e-6
    X, Y = fx * x + cx + margin, fy * y + cy + margin          # canvas coordinates of the undistorted point
    assert X.min() >= 0 and Y.min() >= 0 and X.max() < w + 2 * margin - 1 and Y.max() < h + 2 * margin - 1
    x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
    ax, ay = X - x0, Y - y0
    s = (canvas[y0, x0] * (1 - ax) * (1 - ay) + canvas[y0, x0 + 1] * ax * (1 - ay) + canvas[y0 + 1, x0] * (1 - ax) * ay +
         canvas[y0 + 1, x0 + 1] * ax * ay)
    pinhole = canvas[margin:margin + h, margin:margin + w]
    return np.clip(np.rint(s), 0, 255).astype(np.uint8), np.rint(pinhole).astype(np.uint8)


def test_distorted_scene_is_found_with_undistortion(torch_dev):
    torch, dev = torch_dev
    K = np.float32(LAUNCH_K)
    distorted, pinhole = _distort_scene(K, LAUNCH_D)
    c = capi.Context(0)
    try:
        _scene_db(c, pinhole, K)
        prm = capi.default_frame_params()
        g = torch.from_numpy(distorted).to(dev)
        torch.cuda.synchronize()
        inliers = []
        for dist in (LAUNCH_D, None):
            c.frame_set_undistort(dist)
            c.frame_enqueue_image(g.data_ptr(), 640, 480, True, CAP, K, CAM0, prm, seed=3)
            objs, _ = c.frame_fetch()
            mine = objs[objs["model"] == 0]
            if dist is not None:
                assert len(mine) >= 1
            if not len(mine):
                inliers.append(0)
                continue
            best = mine[np.argmax(mine["score"])]
            if dist is not None:
                assert np.abs(best["pose"][4:7]).max() < 0.05 and abs(abs(best["pose"][3]) - 1) < 0.01
            # inliers of object 0: its matches within POSE2's radius (sqrt 5 px) of the pose the frame found
            _, model = c.frame_fetch_matches()
            corr = c.frame_fetch_match_points()[model == 0]
            inliers.append(c.project_test(best["pose"], corr, K, CAM0, 5.0)[0])
        print(f"object 0 inliers within sqrt(5) px: with undistortion {inliers[0]}, without {inliers[1]}")
        assert inliers[1] < inliers[0]
    finally:
        c.close()


def test_bad_arguments_are_refused(ctx, torch_dev):
    torch, dev = torch_dev
    L, h = ctx.L, ctx.h
    img = np.zeros((8, 8), np.uint8)
    out = np.zeros((8, 8), np.uint8)
    mx = np.zeros((8, 8), np.float32)
    K, d = np.float32(LAUNCH_K), np.float32(LAUNCH_D)
    p = capi._ptr
    ARG = -1   # MH_ERR_ARG

    src_t = torch.zeros((8, 8), dtype=torch.uint8, device=dev)
    dst_t = torch.zeros((8, 8), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sd, dd_ = C.c_void_p(src_t.data_ptr()), C.c_void_p(dst_t.data_ptr())

    def all_three(w, hh, k, dd):
        return [L.mh_undistort(h, p(img), p(out), w, hh, k, dd), L.mh_undistort_map(h, w, hh, k, dd, p(mx), p(mx)),
                L.mh_undistort_dev(h, sd, dd_, w, hh, k, dd)]

    # null pointers
    assert L.mh_undistort(h, None, p(out), 8, 8, p(K), p(d)) == ARG
    assert L.mh_undistort(h, p(img), None, 8, 8, p(K), p(d)) == ARG
    assert L.mh_undistort_map(h, 8, 8, p(K), p(d), None, p(mx)) == ARG
    assert L.mh_undistort_map(h, 8, 8, p(K), p(d), p(mx), None) == ARG
    assert L.mh_undistort_dev(h, None, dd_, 8, 8, p(K), p(d)) == ARG
    assert L.mh_undistort_dev(h, sd, None, 8, 8, p(K), p(d)) == ARG
    assert all_three(8, 8, None, p(d)) == [ARG] * 3
    assert all_three(8, 8, p(K), None) == [ARG] * 3
    assert L.mh_undistort(None, p(img), p(out), 8, 8, p(K), p(d)) == ARG
    assert L.mh_undistort_dev(None, sd, dd_, 8, 8, p(K), p(d)) == ARG
    assert L.mh_undistort_map(None, 8, 8, p(K), p(d), p(mx), p(mx)) == ARG
    assert L.mh_frame_set_undistort(None, p(d)) == ARG
    # sizes
    for w, hh in [(0, 8), (8, 0), (-1, 8), (8, -3), (32768, 1), (1, 32768)]:
        assert all_three(w, hh, p(K), p(d)) == [ARG] * 3, (w, hh)
    # non-finite calibration, fx or fy = 0
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(4):
            k2, d2 = K.copy(), d.copy()
            k2[i] = bad
            d2[i] = bad
            assert all_three(8, 8, p(k2), p(d)) == [ARG] * 3
            assert all_three(8, 8, p(K), p(d2)) == [ARG] * 3
            assert L.mh_frame_set_undistort(h, p(d2)) == ARG
    for i in (0, 1):
        k2 = K.copy()
        k2[i] = 0
        assert all_three(8, 8, p(k2), p(d)) == [ARG] * 3
    # the device entry with out == in
    assert L.mh_undistort_dev(h, sd, sd, 8, 8, p(K), p(d)) == ARG
    # still usable
    rng = np.random.default_rng(3)
    g = rng.integers(0, 256, (17, 13), dtype=np.uint8)
    assert np.array_equal(ctx.undistort(g, LAUNCH_K, LAUNCH_D), ur.undistort(g, LAUNCH_K, LAUNCH_D))
