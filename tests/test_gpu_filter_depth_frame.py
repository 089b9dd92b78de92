"""The depth FILTER inside frames (mh_frame_set_filter_depth / FramePipeline.set_filter_depth): a planted object that the
depth map confirms is delivered with the restatement's score, the same object in front of a surface three times
further away is gone, batches equal their frames alone, switching the feature off leaves no trace, and the frames it
cannot serve are refused before anything is enqueued.

The scene is tests/test_gpu_kinect_image_batch.py's: the keypoints of bundled frame 0 on a plane 0.8 m in front of the
camera are model 0, 500 clutter rows model 1; the image is bundled frame 0 through mh_frame_enqueue_image.  The depth
residual of POSE looks every match up at its own truncated pixel (DEPTHMAP_PROP, no interpolation), so map (b) leaves
exactly the keypoints' pixels at 0.8 m and puts every other measured depth at three times its value: POSE reads the
same numbers from both maps and delivers the same pose, and only the FILTER's test points -- plane points between the
keypoints -- see the far surface.  What the depth class must then do is asserted with the restatement before the device
is trusted."""
import numpy as np
import pytest

import filter_depth_ref as fdr
import test_gpu_kinect_image_batch as kib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
K, CAM0, W, H, CAP = kib.K, kib.CAM0, kib.W, kib.H, kib.CAP
BACK = capi.DEPTH_BACKPROJECTION
PRM = (4096.0, 0.02, 0.1)          # PlausibleSqDistance, DepthFraction, MinKeypointFraction
SEED = 11


class World:
    def __init__(self):
        import torch
        from moped_amd.pipeline import FramePipeline, ShardedDB
        self.torch, self.dev = torch, torch.device("cuda:0")
        gray = kib.GOLD["gray0"]
        probe = capi.Context(0)
        xy, desc = probe.sift(gray)[::2]
        probe.close()
        z = f32(0.8)
        xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(f32)
        rng = np.random.default_rng(7)
        self.db = (np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(f32)]),
                   np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(f32)]),
                   np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)]))
        self.pipe = self.pipeline()
        self.c = self.pipe.ctxs[0]
        self.prm = self.pipe.params
        # maps: (a) the plane; (b) three times as far everywhere but at the keypoints' own pixels
        kp = np.zeros((H, W), bool)
        kp[xy[:, 1].astype(int), xy[:, 0].astype(int)] = True
        za = np.full((H, W), 0.8, f32)
        zb = np.where(kp, f32(0.8), f32(2.4)).astype(f32)
        self.maps = {"a": kib.plane(za), "b": kib.plane(zb)}
        assert np.array_equal(self.maps["a"][kp], self.maps["b"][kp])
        self.fill = np.zeros((H, W), f32)
        # test points of model 0: plane points at pixel centres at least two pixels from every keypoint's pixel
        near = np.zeros((H, W), bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                near |= np.roll(np.roll(kp, dy, 0), dx, 1)
        u, v = np.meshgrid(np.arange(30, W - 30, 19), np.arange(30, H - 30, 17))
        u, v = u.ravel(), v.ravel()
        free = ~near[v, u]
        u, v = u[free][:300], v[free][:300]
        assert len(u) == 300
        self.pts = np.stack([(u + 0.5 - K[2]) / K[0] * z, (v + 0.5 - K[3]) / K[1] * z, np.full(len(u), z)], 1).astype(f32)
        self.pts_off = np.array([0, 300, 300], np.int32)
        self.t_gray = torch.from_numpy(gray).to(self.dev)
        self.t_maps = {k: torch.from_numpy(m).to(self.dev) for k, m in self.maps.items()}
        self.t_fill = torch.from_numpy(self.fill).to(self.dev)
        torch.cuda.synchronize()

    def pipeline(self):
        from moped_amd.pipeline import FramePipeline, ShardedDB
        return FramePipeline(0, ShardedDB(self.db[0], self.db[1], self.db[2], 2), depth=1, max_queries=3 * CAP, batch=3)

    def on(self, pipe=None):
        (pipe or self.pipe).set_filter_depth(self.pts, self.pts_off, f1=PRM, f2=PRM, depth_cam=(K, CAM0))

    def off(self, pipe=None):
        (pipe or self.pipe).set_filter_depth(None, None)

    def frame(self, name, seed=SEED):
        """One frame alone with map `name` -> (objects, counts)."""
        c = self.c
        c.frame_set_depth_image(self.t_maps[name].data_ptr(), self.t_fill.data_ptr(), W, H, BACK, 0.5, 0.1)
        c.frame_enqueue_image(self.t_gray.data_ptr(), W, H, True, CAP, K, CAM0, self.prm, seed)
        return c.frame_fetch()

    def batch(self, names, seeds, pipe=None):
        pipe = pipe or self.pipe
        pipe.enqueue_kinect_batch(0, [self.t_gray.data_ptr()] * len(names), [self.t_maps[n].data_ptr() for n in names],
                                  [self.t_fill.data_ptr()] * len(names), W, H, seeds, fill_scale=None, max_keypoints=CAP)
        return pipe.fetch_batch(0, len(names))

    def restated(self, name, obj):
        """The depth class on the last frame's match lists with one object at a delivered pose -> (score, IS, used)."""
        corr = self.c.frame_fetch_match_points()
        _, mm = self.c.frame_fetch_matches()
        model_off = np.concatenate([[0], np.cumsum(np.bincount(mm, minlength=2))]).astype(np.int32)
        uv = np.stack([corr["u"], corr["v"]], 1)
        xyz = np.stack([corr["x"], corr["y"], corr["z"]], 1)
        r = fdr.filter_projection_depth(uv, xyz, model_off, np.array([obj["model"]], np.int32), obj["pose"][None].astype(f32), K,
                                        CAM0, 0, self.prm.f2_feature_distance, -1e30, self.pts, self.pts_off,
                                        self.maps[name], self.fill, K, CAM0, *PRM)
        return r[0][0], r[4][0], r[5][0]

    def close(self):
        self.off()
        self.c.frame_set_depth_image(0, 0, 0, 0, 0)
        self.pipe.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def _same(a, b, tag):
    (oa, ca), (ob, cb) = a, b
    assert np.array_equal(ca, cb), ("counts", tag, ca, cb)
    assert oa.tobytes() == ob.tobytes(), ("objects", tag)


def test_planted_object_confirmed_refuted_and_left_alone(world):
    w = world
    w.off()
    plain_a, plain_b = w.frame("a"), w.frame("b")
    assert len(plain_a[0]) == 1 and plain_a[0][0]["model"] == 0
    _same(plain_a, plain_b, "POSE reads the same pixels of both maps")
    w.on()
    # (a) the map agrees: delivered, at the pose the plain class delivers, with the restatement's score
    objs, counts = w.frame("a")
    assert len(objs) == 1 and objs[0]["model"] == 0
    assert np.array_equal(objs["pose"].view(np.uint32), plain_a[0]["pose"].view(np.uint32))
    score, inc, used = w.restated("a", objs[0])
    print("map a: score", float(objs[0]["score"]), "restated", float(score), "IS", float(inc), "used", int(used))
    assert used > 250 and score > w.prm.f2_min_score
    assert f32(objs[0]["score"]).view(np.uint32) == f32(score).view(np.uint32)
    # (b) the surface is three times as far: by the restatement the penalty takes the score below MinScore ...
    score_b, inc_b, used_b = w.restated("b", objs[0])
    print("map b: restated", float(score_b), "IS", float(inc_b), "used", int(used_b))
    assert used_b > 250 and score_b < w.prm.f1_min_score
    # ... and the object is gone
    objs_b, counts_b = w.frame("b")
    assert len(objs_b) == 0 and counts_b[2] >= 1     # (POSE had made it)
    # the feature off again: delivered as before
    w.off()
    _same(w.frame("b"), plain_b, "feature off")


def test_batch_equals_the_frames_alone_and_off_leaves_no_trace(world):
    w = world
    names, seeds = ["a", "b", "a"], [21, 22, 23]
    w.on()
    alone = [w.frame(n, s) for n, s in zip(names, seeds)]
    assert [len(o) for o, _ in alone] == [1, 0, 1]
    got = w.batch(names, seeds)
    for f in range(3):
        _same(got[f], alone[f], ("batch frame", f))
    # both slots None after that batch: the objects of a pipeline that never had the feature on
    w.off()
    got = w.batch(names, seeds)
    fresh = w.pipeline()
    try:
        want = w.batch(names, seeds, fresh)
    finally:
        fresh.close()
    for f in range(3):
        _same(got[f], want[f], ("feature off, frame", f))
    assert [len(o) for o, _ in got] == [1, 1, 1]


def test_refusals(world):
    w, c, torch = world, world.c, world.torch
    w.on()
    g = w.t_gray.data_ptr()
    before = w.frame("a")                       # a frame's results on the device: no refusal below may touch them
    state = lambda: (c.frame_fetch(), c.frame_counters(), c.frame_fetch_match_points().tobytes())

    def untouched(was):
        now = state()
        _same(now[0], was[0], "result slot after a refusal")
        assert now[1] == was[1] and now[2] == was[2], "counters / match lists after a refusal"

    was = state()
    _same(was[0], before, "fetch twice")
    try:
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        with pytest.raises(capi.MhError, match="no depth map"):
            c.frame_enqueue_image(g, W, H, True, CAP, K, CAM0, w.prm, 1)
        untouched(was)
        c.frame_set_depth_image(w.t_maps["a"].data_ptr(), w.t_fill.data_ptr(), W, H, BACK, 0.5, 0.1)
        with pytest.raises(capi.MhError, match="one camera per frame"):
            c.frame_enqueue_images([g, g], W, H, True, CAP, [K, K], [CAM0, synth.camera_pose(-0.1, (0.1, 0.0, 0.0))], w.prm, 1)
        qd = torch.zeros((64, 128), dtype=torch.float32, device=w.dev)
        uv = torch.zeros((64, 2), dtype=torch.float32, device=w.dev)
        comm = capi.Comm.create_host(c, 0, 1, lambda blob: blob)
        try:
            with pytest.raises(capi.MhError, match="sharded"):
                c.frame_enqueue_sharded(comm, qd.data_ptr(), uv.data_ptr(), 64, K, CAM0, w.prm, 1)
        finally:
            comm.close()
        gathered = torch.zeros(3 * 64, dtype=torch.int32, device=w.dev)
        with pytest.raises(capi.MhError, match="sharded"):
            c.frame_enqueue_rest(uv.data_ptr(), 64, gathered.data_ptr(), 1, K, CAM0, w.prm, 1)
        # stale points after a DB edit
        w.pipe.replace_model(1, w.db[0][-100:], w.db[1][-100:])
        untouched(was)
        with pytest.raises(capi.MhError, match="mh_filter_depth_set_points again"):
            c.frame_enqueue_image(g, W, H, True, CAP, K, CAM0, w.prm, 1)
        untouched(was)                           # nothing was launched: FEAT, MATCH and the rest chain all write these
        with pytest.raises(ValueError):
            w.pipe.exchange = True
            try:
                w.on()
            finally:
                w.pipe.exchange = False
    finally:
        w.off()
    # a refused frame left nothing behind: the plain frame still runs
    assert len(w.frame("a")[0]) == 1
