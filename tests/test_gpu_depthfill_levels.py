"""MH_DEPTH_FILL_LEVELS (mh_depth_fill_set_mode): moped3d's DEPTHFILL with the FIFO queue run generation by generation.
The oracle is orclib.depth_fill, the restatement of DEPTH_FILL_EXACT_CPU; depth maps and distance maps are compared as
uint32 views, so every bit counts.  Where the replay (the default mode) takes the map, the two modes must give the same
bytes; the other cases are the ground the replay refuses: downscaled maps of more than 8192 pixels (640 x 480 at factors 4,
2; 320 x 240 at factor 1, where pixel indices pass 16 bits; moped3d's own 1280 x 960 at its factor 8), the reference's
automatic factor for an ordinary share of holes, batches and the Kinect batch path at factor 4, the STEP plugin."""
import os
import subprocess

import numpy as np
import pytest

import orclib
from moped_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
K = np.array([525.0, 525.0, 319.5, 239.5], np.float32)
REPLAY, LEVELS = 0, 1


def make_map(h, w, z):
    d = np.zeros((h, w, 4), np.float32)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    d[..., 2] = z
    d[..., 0] = (u - K[2]) / K[0] * z
    d[..., 1] = (v - K[3]) / K[1] * z
    d[..., 3] = np.sqrt((d[..., :3] ** 2).sum(-1))
    return d


def holes(kind, h, w, rng=None):
    rng = np.random.default_rng(h + w) if rng is None else rng
    z = (rng.uniform(0.5, 3.5, size=(h, w)) + 0.3 * np.sin(np.arange(w) / 40.0)[None, :]).astype(np.float32)
    if kind == "sparse":
        z[rng.random((h, w)) < 0.05] = -1.0
    elif kind == "dense":
        z[rng.random((h, w)) < 0.7] = -1.0
    elif kind == "blobs":          # sensor-like: shadows beside objects, a dead border, speckle
        for _ in range(25):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(5, 70)
            yy, xx = np.ogrid[:h, :w]
            z[(yy - cy) ** 2 + ((xx - cx) * rng.uniform(0.3, 1.0)) ** 2 < r * r] = -1.0
        z[:, :12] = -1.0
        z[-9:, :] = -1.0
        z[rng.random((h, w)) < 0.01] = -1.0
    elif kind == "grid":           # every downscaled pixel next to a valid one: the most seeds a map can have
        z[::2, :] = -1.0
    elif kind == "none":
        pass
    elif kind == "all":
        z[:] = -1.0
    elif kind == "one_valid":
        z[:] = -1.0
        z[h // 2 // 16 * 16, w // 3 // 16 * 16] = 2.0
    elif kind == "nan":            # NaN depths are holes (`>= 0` is false)
        z[rng.random((h, w)) < 0.2] = np.nan
    return make_map(h, w, z)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture
def lv(ctx):
    """The session's context in LEVELS mode; the default mode afterwards, whatever the test did."""
    ctx.depth_fill_set_mode(LEVELS)
    yield ctx
    ctx.depth_fill_set_mode(REPLAY)


def stats_ok(c, h, w, scale, frame=0):
    """Item 5's second half, after every LEVELS fill of items 1-3: no overflow, no generation above dw * dh."""
    gens, largest, elements, overflowed = c.depth_fill_stats(frame)
    print("stats", (h, w, scale), "generations", gens, "largest", largest, "elements", elements)
    assert overflowed == 0
    assert largest <= (w // scale) * (h // scale)
    assert gens <= elements and largest <= elements
    return gens, largest, elements


def fill_and_check(c, d, scale, bilinear):
    """A LEVELS fill of host map d against the oracle -> (filled, distance)."""
    h, w = d.shape[:2]
    want, want_dist, _ = orclib.depth_fill(d, K, scale, bilinear)
    got, got_dist, used = c.depth_fill(d, K, scale, bilinear)
    assert used == scale
    stats_ok(c, h, w, scale)
    assert same(got_dist, want_dist), (h, w, scale, bilinear, int((got_dist != want_dist).sum()))
    assert same(got, want), (h, w, scale, bilinear)
    return got, got_dist


@pytest.mark.parametrize("kind", ["sparse", "dense", "blobs", "grid", "none", "all", "one_valid", "nan"])
@pytest.mark.parametrize("scale,bilinear", [(8, False), (8, True), (16, False)])
def test_same_bytes_where_both_modes_work(ctx, kind, scale, bilinear):
    d = holes(kind, 480, 640)
    try:
        ctx.depth_fill_set_mode(REPLAY)
        rep, rep_dist, _ = ctx.depth_fill(d, K, scale, bilinear)
        ctx.depth_fill_set_mode(LEVELS)
        got, got_dist = fill_and_check(ctx, d, scale, bilinear)      # == the oracle
        assert same(got, rep) and same(got_dist, rep_dist)
    finally:
        ctx.depth_fill_set_mode(REPLAY)


@pytest.mark.parametrize("h,w,scale,kind", [(480, 640, 4, "blobs"), (480, 640, 4, "nan"), (480, 640, 4, "sparse"),
                                            (480, 640, 4, "grid"), (480, 640, 4, "one_valid"), (480, 640, 2, "blobs"),
                                            (240, 320, 1, "blobs"), (960, 1280, 8, "blobs")])
def test_ground_the_replay_refuses(lv, h, w, scale, kind):
    d = holes(kind, h, w)
    for bilinear in (False, True):
        got, got_dist = fill_and_check(lv, d, scale, bilinear)
    if scale == 1:   # the reference never hands the filled depths back at factor 1: only the distance map is written
        assert same(got, d) and got_dist.max() > 0
    if kind == "grid":   # at factor 4 only hole rows are sampled: no valid pixel, no seed, every hole at distance 1e30
        assert np.all(got_dist[d[..., 2] < 0] == np.float32(1e30)) and same(got, d)
    lv.depth_fill_set_mode(REPLAY)
    with pytest.raises(capi.MhError):
        lv.depth_fill(d, K, scale, False)


def edge_maps():
    z33 = np.full((3, 3), -1.0, np.float32)
    z33[0, 0] = 1.5
    z140 = np.full((1, 40), -1.0, np.float32)
    z140[0, 5], z140[0, 30] = 1.0, 2.5
    z88 = np.full((8, 8), -1.0, np.float32)
    z88[0, 0] = 0.75
    return {"3x3 one valid corner": (make_map(3, 3, z33), 1), "1x40 two valid": (make_map(1, 40, z140), 1),
            "8x8 at 8, valid": (make_map(8, 8, z88), 8), "8x8 at 8, hole": (make_map(8, 8, -z88), 8),
            "8x8 at 8, sparse": (holes("sparse", 8, 8), 8), "100x36 at 3": (holes("blobs", 100, 36), 3),
            "483x642 at 8": (holes("blobs", 483, 642), 8)}


@pytest.mark.parametrize("name", list(edge_maps()))
def test_edges(lv, name):
    d, scale = edge_maps()[name]
    for bilinear in (False, True):
        fill_and_check(lv, d, scale, bilinear)


def test_automatic_factor(lv):
    rng = np.random.default_rng(480 + 640)
    z = rng.uniform(0.5, 3.5, size=(480, 640)).astype(np.float32)
    z[rng.random((480, 640)) < 0.3] = -1.0
    d = make_map(480, 640, z)
    want, want_dist, s = orclib.depth_fill(d, K, -1)
    assert s == 4
    got, got_dist, used = lv.depth_fill(d, K, -1)
    assert used == 4 and same(got, want) and same(got_dist, want_dist)
    lv.depth_fill_set_mode(REPLAY)
    with pytest.raises(capi.MhError):
        lv.depth_fill(d, K, -1)
    lv.depth_fill_set_mode(LEVELS)
    got, got_dist, used = lv.depth_fill(d, K, -1)
    assert used == 4 and same(got, want) and same(got_dist, want_dist)


def test_stats_count_the_generations(lv):
    d = holes("one_valid", 480, 640)
    fill_and_check(lv, d, 4, False)
    gens, largest, elements, overflowed = lv.depth_fill_stats()
    assert gens >= 100          # the valid pixel is 107 Chebyshev steps from the far edge of the 160 x 120 map
    assert overflowed == 0 and 1 <= largest <= 160 * 120 and elements >= gens
    lv.depth_fill_set_mode(REPLAY)
    lv.depth_fill(d, K, 8, False)
    with pytest.raises(capi.MhError):   # the stats are those of a LEVELS fill
        lv.depth_fill_stats()
    assert lv.depth_fill_get_mode() == REPLAY
    lv.depth_fill_set_mode(LEVELS)
    assert lv.depth_fill_get_mode() == LEVELS
    with pytest.raises(capi.MhError):
        lv.depth_fill_set_mode(2)
    assert lv.depth_fill_get_mode() == LEVELS
    # a refused LEVELS call (more than 2^21 downscaled pixels, before any launch) leaves no stats to read either
    lv.depth_fill(d, K, 4, False)
    assert lv.depth_fill_stats()[0] >= 100
    wide = np.zeros((1, (1 << 21) + 1, 4), np.float32)
    with pytest.raises(capi.MhError) as e:
        lv.depth_fill(wide, K, 1, False)
    assert "-> -3:" in str(e.value)
    with pytest.raises(capi.MhError):
        lv.depth_fill_stats()
    fill_and_check(lv, d, 4, False)              # the context keeps working


def batch_fill(c, maps, scale, bilinear=False):
    import torch
    dev = torch.device("cuda:0")
    h, w = maps[0].shape[:2]
    t_d = [torch.from_numpy(m).to(dev) for m in maps]
    t_f = [torch.empty((h, w), dtype=torch.float32, device=dev) for _ in maps]
    torch.cuda.synchronize()
    c.depth_fill_batch_dev([t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], w, h, K, scale, bilinear)
    c.depth_fill_status()
    return [t.cpu().numpy() for t in t_d], [t.cpu().numpy() for t in t_f]


def test_batches(lv):
    import torch
    maps = [holes(k, 480, 640) for k in ("blobs", "nan", "sparse")]
    got, got_dist = batch_fill(lv, maps, 4)
    for f, m in enumerate(maps):
        stats_ok(lv, 480, 640, 4, f)
    for f, m in enumerate(maps):
        want, want_dist, _ = orclib.depth_fill(m, K, 4, False)
        one, one_dist, _ = lv.depth_fill(m, K, 4, False)
        assert same(got[f], want) and same(got_dist[f], want_dist), f
        assert same(got[f], one) and same(got_dist[f], one_dist), f
    # sixteen maps at a factor both modes take
    maps = [holes("blobs", 480, 640, np.random.default_rng(100 + i)) for i in range(16)]
    got, got_dist = batch_fill(lv, maps, 8, True)
    for f in range(16):
        stats_ok(lv, 480, 640, 8, f)
    lv.depth_fill_set_mode(REPLAY)
    rep, rep_dist = batch_fill(lv, maps, 8, True)
    lv.depth_fill_set_mode(LEVELS)
    for f in range(16):
        assert same(got[f], rep[f]) and same(got_dist[f], rep_dist[f]), f
    assert any((d > 0).any() for d in got_dist)
    # a map handed in twice, the automatic factor: MH_ERR_ARG as in the default mode
    dev = torch.device("cuda:0")
    t_d = torch.from_numpy(maps[0]).to(dev)
    t_f = [torch.empty((480, 640), dtype=torch.float32, device=dev) for _ in range(2)]
    with pytest.raises(capi.MhError) as e:
        lv.depth_fill_batch_dev([t_d.data_ptr(), t_d.data_ptr()], [t.data_ptr() for t in t_f], 640, 480, K, 4)
    assert "-> -1:" in str(e.value)
    t_d2 = torch.from_numpy(maps[1]).to(dev)
    with pytest.raises(capi.MhError) as e:
        lv.depth_fill_batch_dev([t_d.data_ptr(), t_d2.data_ptr()], [t.data_ptr() for t in t_f], 640, 480, K, -1)
    assert "-> -1:" in str(e.value)


def test_kinect_batch_through_the_pipeline_at_factor_4():
    """FramePipeline.set_depth_fill_mode + enqueue_kinect_batch(fill_scale=4) on the bundled-frame scene of
    tests/test_gpu_kinect_image_batch.py (its three-frame batch): the objects, counts, match lists and keep flags of every
    frame equal those of the frame alone under the oracle's factor-4 fill of its raw map, and so do the batch's objects
    when the maps arrive filled by the oracle (fill_scale=None)."""
    import test_gpu_kinect_image_batch as kb
    w = kb.World()
    try:
        torch = w.torch
        order = [("f0", "blobs"), ("f3", "nan"), ("thin", "far")]
        filled = {k: orclib.depth_fill(w.raw[k], kb.K, 4, False)[:2] for _, k in order}
        t_filled = {k: (torch.from_numpy(m).to(w.dev), torch.from_numpy(f).to(w.dev)) for k, (m, f) in filled.items()}
        want = [w.alone(i, m, kb.BACK, t_filled) for i, m in order]
        assert len(want[0]["objs"]) >= 1 and len(want[1]["objs"]) >= 1
        grays, seeds = [w.t_gray[i].data_ptr() for i, _ in order], [w.seed(i, m) for i, m in order]
        # the maps filled on the host, handed in filled
        w.pipe.enqueue_kinect_batch(0, grays, [t_filled[m][0].data_ptr() for _, m in order],
                                    [t_filled[m][1].data_ptr() for _, m in order], kb.W, kb.H, seeds, fill_scale=None,
                                    max_keypoints=kb.CAP)
        host_filled = [w.c.frame_fetch_slot(s) for s in range(len(order))]
        for slot in range(len(order)):
            w.check_slot(slot, want[slot], tag="filled on the host")
        # raw maps, filled by the batch itself
        t_d = [torch.from_numpy(w.raw[m]).to(w.dev) for _, m in order]
        t_f = [torch.empty((kb.H, kb.W), dtype=torch.float32, device=w.dev) for _ in order]
        torch.cuda.synchronize()
        with pytest.raises(capi.MhError):   # the default mode refuses factor 4
            w.pipe.enqueue_kinect_batch(0, grays, [t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], kb.W, kb.H, seeds,
                                        fill_scale=4, max_keypoints=kb.CAP, keep=(t_d, t_f))
        w.pipe.set_depth_fill_mode(LEVELS)
        w.pipe.enqueue_kinect_batch(0, grays, [t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], kb.W, kb.H, seeds,
                                    fill_scale=4, max_keypoints=kb.CAP, keep=(t_d, t_f))
        for slot in range(len(order)):
            w.check_slot(slot, want[slot], tag="kinect at 4")
            objs, counts = w.c.frame_fetch_slot(slot)
            assert objs.tobytes() == host_filled[slot][0].tobytes() and np.array_equal(counts, host_filled[slot][1])
        w.c.depth_fill_status()
        for t, f, (_, m) in zip(t_d, t_f, order):
            assert same(t.cpu().numpy(), filled[m][0]) and same(f.cpu().numpy(), filled[m][1])
    finally:
        w.close()


def test_plugin_level_fill(tmp_path):
    """DEPTH_FILL_EXACT_HIP(4, false, levelFill) in moped3d's DEPTHFILL slot gives the oracle's bytes on a 640 x 480 map;
    without the argument the step warns, appends no distance map and reports itself not capable, as before."""
    subprocess.check_call(["make", "-s", "-C", HOST, "moped3d_depthfill_test"])
    exe = os.path.join(HOST, "moped3d_depthfill_test")
    h, w = 480, 640
    d = holes("blobs", h, w)
    src, dst = str(tmp_path / "depth_in.bin"), str(tmp_path / "depth_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([w, h], np.int32).tobytes() + K.tobytes() + d.tobytes())
    for bilinear in (0, 1):
        subprocess.check_call([exe, src, dst, "4", str(bilinear), "1"])
        raw = np.fromfile(dst, np.float32)
        got, got_dist = raw[:h * w * 4].reshape(h, w, 4), raw[h * w * 4:].reshape(h, w)
        want, want_dist, _ = orclib.depth_fill(d, K, 4, bool(bilinear))
        assert same(got, want) and same(got_dist, want_dist)
    for args in (["4", "0"], ["4", "0", "0"]):
        r = subprocess.run([exe, src, str(tmp_path / "none.bin"), *args], capture_output=True, text=True)
        assert r.returncode == 4 and "distance map" in r.stderr, (r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "none.bin"))
