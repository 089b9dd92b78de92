"""Kinect frames from what the sensor delivers: FramePipeline.enqueue_kinect_raw_batch and mh_frame_run_kinect_raw_host
build the depth map on the device (moped_amd/csrc/depthmap.hip) and then run what the calls that take the finished map
run.  Both must give, byte for byte, what those calls give when they are fed the restatement's map
(tests/depthmap_ref.py) -- the same launches behind the map, so no tolerance.

The scene is tests/test_gpu_kinect_image_batch.py's: bundled frame 0's keypoints on a plane 0.8 m in front of the camera
are model 0; the raw depth is that plane with NaN rows, sensor-like holes (NaN) or a far corner."""
import numpy as np
import pytest

import depthmap_ref as ref
from moped_amd import capi
from test_gpu_depthfill import holes
from test_gpu_kinect_image_batch import CAM0, CAP, H, K, W, World

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def raw_z():
    z = np.full((H, W), 0.8, f32)
    z_nan, z_far, z_blobs = z.copy(), z.copy(), z.copy()
    z_nan[:40] = np.nan
    z_far[300:, :200] = 5.0
    z_blobs[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = np.nan
    return {"nan": z_nan, "far": z_far, "blobs": z_blobs}


def fetch_all(c, B):
    out = []
    for slot in range(B):
        objs, counts = c.frame_fetch_slot(slot)
        mq, mm = c.frame_fetch_matches_slot(slot)
        out.append((objs.tobytes(), counts.tolist(), mq.tobytes(), mm.tobytes()))
    return out


def test_raw_batch_equals_the_map_batch_fed_the_restatement(world):
    w = world
    torch = w.torch
    order = [("f0", "blobs"), ("f3", "nan"), ("thin", "far")]
    B = len(order)
    z = raw_z()
    maps = {k: ref.depth_map(*ref.plain(v), K, W, H) for k, v in z.items()}
    assert (maps["blobs"][..., 2] < 0).sum() > 1000 and (maps["nan"][:40, :, 2] < 0).all()
    grays = [w.t_gray[i].data_ptr() for i, _ in order]
    seeds = [w.seed(i, m) for i, m in order]
    # the existing route, fed the restatement's maps (filled in place: copies)
    t_d = [torch.from_numpy(maps[m]).to(w.dev) for _, m in order]
    t_f = [torch.empty((H, W), dtype=torch.float32, device=w.dev) for _ in order]
    torch.cuda.synchronize()
    w.pipe.enqueue_kinect_batch(0, grays, [t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], W, H, seeds,
                                fill_scale=8, max_keypoints=CAP, keep=(t_d, t_f))
    want = fetch_all(w.c, B)
    w.c.depth_fill_status()
    want_maps = [t.cpu().numpy() for t in t_d]
    want_dist = [t.cpu().numpy() for t in t_f]
    assert sum(len(x[0]) > 0 for x in want) >= 2            # the model is found: the comparison is not of empty lists
    assert len({x[2] for x in want}) == B                   # ... and the frames differ
    # the raw route, twice (the second time the slot's tensors exist already and hold the first run's maps)
    t_raw = [torch.from_numpy(z[m]).to(w.dev) for _, m in order]
    torch.cuda.synchronize()
    fmt = capi.make_raw_depth(capi.RAW_DEPTH_F32_M, W, H)
    for rep in range(2):
        got_maps, got_dist = w.pipe.enqueue_kinect_raw_batch(0, grays, [t.data_ptr() for t in t_raw], fmt, W, H, seeds,
                                                             fill_scale=8, max_keypoints=CAP, keep=t_raw)
        got = fetch_all(w.c, B)
        w.c.depth_fill_status()
        for f in range(B):
            assert got[f] == want[f], (rep, f)
            assert got_maps[f].cpu().numpy().tobytes() == want_maps[f].tobytes(), (rep, f)
            assert got_dist[f].cpu().numpy().tobytes() == want_dist[f].tobytes(), (rep, f)
    # fill_scale=None: no DEPTHFILL, no distance maps -- the existing route fed the unfilled maps and none either
    t_d = [torch.from_numpy(maps[m]).to(w.dev) for _, m in order]
    torch.cuda.synchronize()
    w.c.frame_set_depth_image_batch([t.data_ptr() for t in t_d], None, W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
    w.c.frame_enqueue_image_batch(grays, W, H, True, CAP, K, CAM0, w.prm, seeds)
    want = fetch_all(w.c, B)
    got_maps, got_dist = w.pipe.enqueue_kinect_raw_batch(0, grays, [t.data_ptr() for t in t_raw], fmt, W, H, seeds,
                                                         fill_scale=None, max_keypoints=CAP, keep=t_raw)
    assert got_dist is None
    assert fetch_all(w.c, B) == want
    for f in range(B):
        assert got_maps[f].cpu().numpy().tobytes() == maps[order[f][1]].tobytes(), f


def test_qvga_u16_frame_from_host_equals_the_map_frame(world):
    """320 x 240 uint16 millimetres beside the 640 x 480 image, host memory in: mh_frame_run_kinect_raw_host against
    mh_frame_run_kinect_host on the restatement's map -- objects, counts and both maps copied back."""
    w = world
    c = w.c
    mm = np.full((H // 2, W // 2), 800, np.uint16)
    mm[:20] = 0
    mm[100:130, 150:200] = 0
    mm[239, 319] = 0
    m = ref.depth_map(*ref.plain(mm), K, W, H)
    assert 10000 < (m[..., 2] < 0).sum() < W * H // 2
    gray = w.gray["f0"]
    seed = w.seed("f0", "nan")
    want_objs, want_counts, want_d, want_f = c.frame_run_kinect_host(gray, m, None, K, CAM0, w.prm, seed, fill_scale=8,
                                                                     max_keypoints=CAP)
    assert len(want_objs) >= 1 and want_f.max() > 0 and not (want_d[..., 2] < 0).any()
    fmt = capi.make_raw_depth(capi.RAW_DEPTH_U16_MM, W // 2, H // 2)
    for rep in range(2):
        objs, counts, d, f = c.frame_run_kinect_raw_host(gray, mm, fmt, K, CAM0, w.prm, seed, fill_scale=8,
                                                         max_keypoints=CAP)
        assert np.array_equal(counts, want_counts) and objs.tobytes() == want_objs.tobytes(), rep
        assert d.tobytes() == want_d.tobytes() and f.tobytes() == want_f.tobytes(), rep
    # the outputs are optional: nothing copied back, the same objects
    objs, counts, d, f = c.frame_run_kinect_raw_host(gray, mm, fmt, K, CAM0, w.prm, seed, fill_scale=8, max_keypoints=CAP,
                                                     maps_back=False)
    assert d is None and f is None
    assert np.array_equal(counts, want_counts) and objs.tobytes() == want_objs.tobytes()
    # fill_scale 0: the map as built is the frame's map, no distance map
    want0 = c.frame_run_kinect_host(gray, m, None, K, CAM0, w.prm, seed, fill_scale=0, max_keypoints=CAP)
    objs, counts, d, f = c.frame_run_kinect_raw_host(gray, mm, fmt, K, CAM0, w.prm, seed, fill_scale=0, max_keypoints=CAP)
    assert f is None and d.tobytes() == m.tobytes()
    assert np.array_equal(counts, want0[1]) and objs.tobytes() == want0[0].tobytes()
