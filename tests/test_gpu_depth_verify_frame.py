"""DEPTH_VERIFY behind the frames (mh_frame_set_depth_verify / FramePipeline.set_depth_verify): a planted object that the
depth map confirms is delivered, the same object in front of a surface three times as far is erased; the records and the
delivered objects equal the stand-alone call on the frame's own match lists and on the objects FILTER2 left; batches equal
their frames alone; the hulls follow the surviving objects; switching the feature off leaves no trace; the frames it
cannot serve are refused before anything is enqueued.

The scene is tests/test_gpu_filter_depth_frame.py's: the keypoints of bundled frame 0 on a plane 0.8 m in front of the
camera are model 0, 500 clutter rows model 1, the image is bundled frame 0 through mh_frame_enqueue_image.  Here model 0's
rows are off their true places by about 0.7 px (so that the quality score of a correct pose is about 0.6, not 1), and it
gets 300 more rows: plane points at pixel centres at least two pixels from every keypoint's pixel, with clutter
descriptors that never match.  POSE looks every match's depth up at the IMAGE keypoint's own pixel, and map (b) leaves
exactly those pixels at 0.8 m and puts every other depth at 2.4 m: POSE reads the same numbers from both maps and
delivers the same pose, and only the verification -- which walks every row of the model -- sees the far surface.  What the
class must then do is asserted with the restatement before the device is trusted."""
import numpy as np
import pytest

import depth_verify_ref as dvr
import test_gpu_kinect_image_batch as kib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
K, CAM0, W, H, CAP = kib.K, kib.CAM0, kib.W, kib.H, kib.CAP
BACK = capi.DEPTH_BACKPROJECTION
PRM = (4096.0, 3.0, 0.0, 0.02)     # FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction
SEED = 11


class World:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        gray = kib.GOLD["gray0"]
        probe = capi.Context(0)
        xy, desc = probe.sift(gray)[::2]
        probe.close()
        z = f32(0.8)
        rng = np.random.default_rng(7)
        off = rng.normal(0, 0.7, (len(xy), 2))         # pixels
        xyz = np.stack([(xy[:, 0] + off[:, 0] - K[2]) / K[0] * z, (xy[:, 1] + off[:, 1] - K[3]) / K[1] * z,
                        np.full(len(xy), z)], 1).astype(f32)
        kp = np.zeros((H, W), bool)
        kp[xy[:, 1].astype(int), xy[:, 0].astype(int)] = True
        near = np.zeros((H, W), bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                near |= np.roll(np.roll(kp, dy, 0), dx, 1)
        u, v = np.meshgrid(np.arange(30, W - 30, 19), np.arange(30, H - 30, 17))
        u, v = u.ravel(), v.ravel()
        free = ~near[v, u]
        u, v = u[free][:300], v[free][:300]
        assert len(u) == 300
        plane = np.stack([(u + 0.5 - K[2]) / K[0] * z, (v + 0.5 - K[3]) / K[1] * z, np.full(len(u), z)], 1).astype(f32)
        clutter = lambda n: np.abs(rng.normal(size=(n, 128))).astype(f32)
        self.n0 = len(xy) + 300
        self.db = (np.concatenate([desc, clutter(300), clutter(500)]),
                   np.concatenate([xyz, plane, rng.uniform(-0.1, 0.1, (500, 3)).astype(f32)]),
                   np.concatenate([np.zeros(self.n0, np.int32), np.ones(500, np.int32)]))
        self.kp_off = np.array([0, self.n0, self.n0 + 500], np.int32)
        self.pipe = self.pipeline()
        self.c = self.pipe.ctxs[0]
        self.prm = self.pipe.params
        za = np.full((H, W), 0.8, f32)
        zb = np.where(kp, f32(0.8), f32(2.4)).astype(f32)
        self.maps = {"a": kib.plane(za), "b": kib.plane(zb)}
        assert np.array_equal(self.maps["a"][kp], self.maps["b"][kp])
        self.fill = np.zeros((H, W), f32)
        self.t_gray = torch.from_numpy(gray).to(self.dev)
        self.t_maps = {k: torch.from_numpy(m).to(self.dev) for k, m in self.maps.items()}
        self.t_fill = torch.from_numpy(self.fill).to(self.dev)
        torch.cuda.synchronize()

    def pipeline(self):
        from moped_amd.pipeline import FramePipeline, ShardedDB
        return FramePipeline(0, ShardedDB(self.db[0], self.db[1], self.db[2], 2), depth=1, max_queries=4 * CAP, batch=4)

    def on(self, pipe=None):
        (pipe or self.pipe).set_depth_verify(PRM, depth_cam=(K, CAM0))

    def off(self, pipe=None):
        (pipe or self.pipe).set_depth_verify(None)

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

    def lists(self):
        """The match lists of the last frame -> (corr, model_off)."""
        corr = self.c.frame_fetch_match_points()
        mm = self.c.frame_fetch_matches()[1]
        return corr, np.concatenate([[0], np.cumsum(np.bincount(mm, minlength=2))]).astype(np.int32)

    def restated(self, name, objs, corr, model_off):
        uv = np.stack([corr["u"], corr["v"]], 1)
        xyz = np.stack([corr["x"], corr["y"], corr["z"]], 1)
        return dvr.depth_verify(uv, xyz, model_off, self.db[1], self.kp_off, objs["model"], objs["pose"].astype(f32), K, CAM0,
                                self.maps[name], self.fill, K, CAM0, PRM)

    def close(self):
        self.off()
        self.pipe.set_hulls(0)
        self.c.frame_set_depth_image(0, 0, 0, 0, 0)
        self.pipe.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def _same(a, b, tag):
    (oa, ca), (ob, cb) = a[:2], b[:2]
    assert np.array_equal(ca, cb), ("counts", tag, ca, cb)
    assert oa.tobytes() == ob.tobytes(), ("objects", tag)


def _records_equal(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k in dvr.WORDS:
        a, b = got[k], want[k]
        if a.dtype.kind == "f":
            a, b = np.array(a, f32), np.array(b, f32)
            a[np.isnan(a)] = np.nan
            b[np.isnan(b)] = np.nan
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (tag, k, got[k], want[k])


def test_planted_object_kept_erased_and_equal_to_the_stand_alone_call(world):
    w, c = world, world.c
    w.off()
    plain = {n: w.frame(n) for n in "ab"}
    assert len(plain["a"][0]) == 1 and plain["a"][0][0]["model"] == 0
    _same(plain["a"], plain["b"], "POSE reads the same pixels of both maps")
    with pytest.raises(capi.MhError, match="ran without DEPTH_VERIFY"):
        c.frame_fetch_verify(0)
    # the restatement first: on the plain frame's lists and objects, (a) keeps and (b) erases
    corr, model_off = w.lists()
    want = {n: w.restated(n, plain[n][0], corr, model_off) for n in "ab"}
    for n in "ab":
        r = want[n][0]
        print("map", n, "QS", float(r["qs"]), "IS", float(r["is"]), "used", int(r["used"]), "of", int(r["keypoints"]),
              "plausible", int(r["plausible"]))
    assert want["a"]["keep"].tolist() == [1] and want["b"]["keep"].tolist() == [0]
    assert want["a"][0]["keypoints"] == w.n0 and want["a"][0]["used"] > 0.9 * w.n0
    w.on()
    for n in "ab":
        objs, counts = w.frame(n)
        rec = c.frame_fetch_verify(0)
        assert np.array_equal(counts, plain[n][1])       # counts[] stay: counts[3] = objects after FILTER2's erase
        # the stand-alone call on the frame's own lists and the objects FILTER2 left (the plain frame's: same seed)
        corr_n, off_n = w.lists()
        assert corr_n.tobytes() == corr.tobytes() and np.array_equal(off_n, model_off)
        alone = c.depth_verify(corr_n, off_n, plain[n][0]["model"], plain[n][0]["pose"], K, CAM0, K, CAM0, PRM)
        _records_equal(rec, alone, ("frame vs stand-alone", n))
        _records_equal(rec, want[n], ("frame vs restatement", n))
        assert objs.tobytes() == plain[n][0][rec["keep"] == 1].tobytes(), ("delivered", n)
    assert len(w.frame("a")[0]) == 1 and len(w.frame("b")[0]) == 0
    # the feature off again: delivered as before, and no records
    w.off()
    _same(w.frame("b"), plain["b"], "feature off")
    with pytest.raises(capi.MhError, match="ran without DEPTH_VERIFY"):
        c.frame_fetch_verify(0)


@pytest.mark.parametrize("names", [["a", "b", "a", "b"], ["b", "b", "a", "a"]])
def test_batch_of_four_equals_its_frames_alone(world, names):
    w, c = world, world.c
    seeds = [31, 32, 33, 34]
    w.on()
    try:
        alone, recs = [], []
        for n, s in zip(names, seeds):
            alone.append(w.frame(n, s))
            recs.append(c.frame_fetch_verify(0))
        assert [len(o) for o, _ in alone] == [1 if n == "a" else 0 for n in names]
        got = w.batch(names, seeds)
        assert c.frame_route()[:2].tolist() == [4, 1], c.frame_route()      # a merged Kinect batch stays merged
        for f in range(4):
            _same(got[f], alone[f], ("batch frame", f))
            _records_equal(c.frame_fetch_verify(f), recs[f], ("batch records", f))
            assert len(recs[f]) == 1
    finally:
        w.off()


def test_hulls_follow_the_surviving_objects(world):
    w, c = world, world.c
    names, seeds = ["a", "b", "a", "b"], [41, 42, 43, 44]
    w.on()
    w.pipe.set_hulls(32)
    try:
        got = w.batch(names, seeds)
        for f, n in enumerate(names):
            objs, counts, hulls = got[f]
            assert len(objs) == (1 if n == "a" else 0) and len(hulls[0]) == len(objs), (f, n)
            if len(objs):
                want = c.object_hulls(objs["model"], objs["pose"], K, CAM0, 32)
                assert hulls[0][0].tobytes() == want[0][0].tobytes() and np.array_equal(hulls[1], want[1])
    finally:
        w.pipe.set_hulls(0)
        w.off()


def test_set_and_cleared_equals_never_set(world):
    w = world
    names, seeds = ["a", "b", "a", "b"], [51, 52, 53, 54]
    w.on()
    assert [len(o) for o, _ in w.batch(names, seeds)] == [1, 0, 1, 0]
    w.off()
    got = w.batch(names, seeds)
    one = w.frame("b", 55)
    fresh = w.pipeline()
    try:
        want = w.batch(names, seeds, fresh)
        c0, w.c = w.c, fresh.ctxs[0]
        try:
            one_fresh = w.frame("b", 55)
        finally:
            w.c = c0
    finally:
        fresh.close()
    for f in range(4):
        _same(got[f], want[f], ("feature off, frame", f))
    _same(one, one_fresh, "feature off, one frame")
    assert [len(o) for o, _ in got] == [1, 1, 1, 1]


def test_refused_frame_kinds_enqueue_nothing(world):
    w, c, torch = world, world.c, world.torch
    w.on()
    g = w.t_gray.data_ptr()
    before = w.frame("a")
    state = lambda: (c.frame_fetch(), c.frame_counters(), c.frame_fetch_match_points().tobytes(), c.frame_fetch_verify(0).tobytes())

    def untouched(was):
        now = state()
        _same(now[0], was[0], "result slot after a refusal")
        assert now[1] == was[1] and now[2] == was[2] and now[3] == was[3], "counters / match lists / records after a refusal"

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
        untouched(was)
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
        untouched(was)
        with pytest.raises(ValueError):
            w.pipe.exchange = True
            try:
                w.on()
            finally:
                w.pipe.exchange = False
    finally:
        w.off()
    assert len(w.frame("a")[0]) == 1
