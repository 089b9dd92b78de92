"""The depth FILTER in the POSE tails (filter_depth_score_wave behind the refine and in pose_kept_f1, csrc/pose.hip) and
in merged batches (FilterFuseDepth's table of maps, csrc/steps.h), against the route that test_gpu_filter_depth_frame.py
holds to the restatement: the same context with stage timing on keeps the frames apart and the FILTERs as launches of
their own.  Objects (bytes), score bits and counts must be equal; Context.frame_route() says which way a frame went.

Image path: the scene of test_gpu_filter_depth_frame.py (its World: one planted object, map "a" confirms it, map "b"
refutes it while POSE reads the same numbers from both).  Descriptor path: six models of 1 500 points with 0, 1, 63, 64,
65 and 130 test points, five frames with 2, 0, 3, 1 and 6 visible objects and synth.depth_image maps -- a background 1.5 m
away behind objects at 0.5 .. 1.0 m, which the depth class refutes wherever a model has test points -- except the last
frame's, where the objects' own test points are drawn into the map (nearest surface per pixel, the keypoints' pixels left
as they are, so POSE reads what it read before): there the depth class keeps what it finds."""
import numpy as np
import pytest

import test_gpu_filter_depth_frame as fdf
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
K, CAM0, W, H, CAP, PRM = fdf.K, fdf.CAM0, fdf.W, fdf.H, fdf.CAP, fdf.PRM
SLOTS = {"both": (PRM, PRM), "f1": (PRM, None), "f2": (None, PRM), "neither": (None, None)}
BITS = {"both": 3, "f1": 1, "f2": 2, "neither": 0}


def _same(a, b, tag):
    fdf._same(a, b, tag)


def _timed(c, run):
    """run() with stage timing on: frames one after the other, FILTER and FILTER2 as launches of their own."""
    c.enable_timing(True)
    try:
        return run()
    finally:
        c.enable_timing(False)


# ------------------------------------------------------------------------------------------------------- image path
@pytest.fixture(scope="module")
def world():
    w = fdf.World()
    yield w
    w.c.enable_timing(False)
    w.close()


def _set(w, which, pipe=None):
    f1, f2 = SLOTS[which]
    if f1 is None and f2 is None:
        w.off(pipe)
    else:
        (pipe or w.pipe).set_filter_depth(w.pts, w.pts_off, f1=f1, f2=f2, depth_cam=(K, CAM0))


def _frame_on(w, c, name, seed=fdf.SEED):
    c.frame_set_depth_image(w.t_maps[name].data_ptr(), w.t_fill.data_ptr(), W, H, fdf.BACK, 0.5, 0.1)
    c.frame_enqueue_image(w.t_gray.data_ptr(), W, H, True, CAP, K, CAM0, w.prm, seed)
    return c.frame_fetch()


def test_frame_route_says_which_way_the_frames_went(world):
    w, c = world, world.c
    names, seeds = ["a", "b", "a"], [21, 22, 23]
    _set(w, "both")
    w.frame("a")
    assert c.frame_route().tolist() == [1, 0, 1, 0b11]           # a frame alone: fused
    w.batch(names, seeds)
    assert c.frame_route().tolist() == [3, 1, 1, 0b11]           # a map per frame: merged and fused
    _timed(c, lambda: w.frame("a"))
    assert c.frame_route().tolist() == [1, 0, 0, 0b11]           # timing on: launches of their own
    _timed(c, lambda: w.batch(names, seeds))
    assert c.frame_route().tolist() == [3, 0, 0, 0b11]           # ... and frame after frame
    # POSE as one launch: its kernel does not carry the depth class -- FILTER as launches of its own, the same objects
    fused = w.frame("a")
    c.pose_set_split(False)
    try:
        apart = w.frame("a")
        assert c.frame_route().tolist() == [1, 0, 0, 0b11]
        w.batch(names, seeds)
        assert c.frame_route().tolist() == [3, 0, 0, 0b11]
    finally:
        c.pose_set_split(True)
    _same(fused, apart, "POSE as one launch")
    for which in ("f1", "f2"):
        _set(w, which)
        w.frame("a")
        assert c.frame_route().tolist() == [1, 0, 1, BITS[which]], which
        w.batch(names, seeds)
        assert c.frame_route().tolist() == [3, 1, 1, BITS[which]], which
    # feature off: what a pipeline that never had it on reports for the same calls
    _set(w, "neither")
    fresh = w.pipeline()
    try:
        fc = fresh.ctxs[0]
        assert fc.frame_route().tolist() == [0, 0, 0, 0]         # nothing enqueued yet
        w.frame("a")
        _frame_on(w, fc, "a")
        assert c.frame_route().tolist() == fc.frame_route().tolist() and c.frame_route()[3] == 0
        w.batch(names, seeds)
        w.batch(names, seeds, fresh)
        assert c.frame_route().tolist() == fc.frame_route().tolist() and c.frame_route()[3] == 0
        assert c.frame_route()[0] == 3
    finally:
        fresh.close()


@pytest.mark.parametrize("which", list(SLOTS))
def test_a_frame_alone_equals_the_stand_alone_route(world, which):
    w, c = world, world.c
    _set(w, which)
    for name in ("a", "b"):
        fused = w.frame(name)
        assert c.frame_route().tolist() == [1, 0, 1, BITS[which]]
        apart = _timed(c, lambda: w.frame(name))
        assert c.frame_route().tolist() == [1, 0, 0, BITS[which]]
        print(which, name, "objects", len(fused[0]), "counts", fused[1], "scores", fused[0]["score"])
        _same(fused, apart, (which, name))
        if which == "both" and name == "a":
            assert len(fused[0]) == 1 and fused[0][0]["model"] == 0
            score, inc, used = w.restated("a", fused[0][0])
            assert used > 250 and inc >= 0
            assert f32(fused[0][0]["score"]).view(np.uint32) == f32(score).view(np.uint32)
        if which == "both" and name == "b":
            assert len(fused[0]) == 0 and fused[1][2] >= 1       # (POSE had made it)
        if which == "neither":
            assert len(fused[0]) == 1


def test_merged_batch_of_images_every_frame_with_its_own_map(world):
    w, c = world, world.c
    _set(w, "both")
    seeds = [31, 32, 33]
    for names, n_objs in ((["a", "b", "a"], [1, 0, 1]), (["b", "a", "b"], [0, 1, 0])):   # the same arenas, the maps swapped
        alone = [w.frame(n, s) for n, s in zip(names, seeds)]
        got = w.batch(names, seeds)
        assert c.frame_route().tolist() == [3, 1, 1, 0b11]
        assert [len(o) for o, _ in got] == n_objs, names        # a frame that read a neighbour's map cannot pass
        for f in range(3):
            _same(got[f], alone[f], (names, f))


def test_switching_on_off_on(world):
    w, c = world, world.c
    names, seeds = ["a", "b", "a"], [41, 42, 43]
    _set(w, "both")
    first = w.batch(names, seeds), w.frame("b", 44)
    _set(w, "neither")
    off = w.batch(names, seeds), w.frame("b", 44)
    fresh = w.pipeline()
    try:
        never = w.batch(names, seeds, fresh), _frame_on(w, fresh.ctxs[0], "b", 44)
    finally:
        fresh.close()
    for f in range(3):
        _same(off[0][f], never[0][f], ("off, batch frame", f))
    _same(off[1], never[1], "off, a frame alone")
    assert [len(o) for o, _ in off[0]] == [1, 1, 1] and len(off[1][0]) == 1
    _set(w, "both")
    again = w.batch(names, seeds), w.frame("b", 44)
    for f in range(3):
        _same(again[0][f], first[0][f], ("on again, batch frame", f))
    _same(again[1], first[1], "on again, a frame alone")
    assert [len(o) for o, _ in again[0]] == [1, 0, 1] and len(again[1][0]) == 0


# -------------------------------------------------------------------------------------------------- descriptor path
N_VIS = (2, 0, 3, 1, 6)
N_TEST = (0, 1, 63, 64, 65, 130)
Q = 1500
PRM_D = (4096.0, 0.1, 0.1)


def _draw_objects(db, fr, img, fill, pts, pts_off):
    """The visible objects' test points into the map at their true poses: the nearest surface per pixel over the 3 x 3
    pixels about each point, measured (fill 0); the keypoints' own pixels stay as they are."""
    keep = np.zeros((480, 640), bool)
    keep[np.clip(fr.uv[:, 1].astype(int), 0, 479), np.clip(fr.uv[:, 0].astype(int), 0, 639)] = True
    zbuf = np.full((480, 640), np.inf)
    for m, pose in zip(fr.visible, fr.poses):
        k = pts[pts_off[m]:pts_off[m + 1]].astype(np.float64)
        if not len(k):
            continue
        p = k @ synth.quat_to_R(pose[:4]).T + pose[4:].astype(np.float64)
        u = (p[:, 0] / p[:, 2] * K[0] + K[2]).astype(int)
        v = (p[:, 1] / p[:, 2] * K[1] + K[3]).astype(int)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y = u + dx, v + dy
                ok = (x >= 0) & (x < 640) & (y >= 0) & (y < 480)
                np.minimum.at(zbuf, (y[ok], x[ok]), p[ok, 2] * 1.002)
    yy, xx = np.nonzero(np.isfinite(zbuf) & ~keep)
    z = zbuf[yy, xx]
    img[yy, xx, 0] = (xx + 0.5 - K[2]) / K[0] * z
    img[yy, xx, 1] = (yy + 0.5 - K[3]) / K[1] * z
    img[yy, xx, 2] = z
    img[yy, xx, 3] = np.sqrt((img[yy, xx, :3].astype(np.float64) ** 2).sum(-1))
    fill[yy, xx] = 0.0
    return len(yy)


class Scene:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        db = self.db = synth.make_db(6, 1500, seed=2)
        self.frs = [synth.make_frame(db, n_vis=n, seed=60 + i, Q=Q, pts_per_obj=130) for i, n in enumerate(N_VIS)]
        # test points: the first N_TEST[m] of model m's own points
        self.pts_off = np.concatenate([[0], np.cumsum(N_TEST)]).astype(np.int32)
        self.pts = np.concatenate([db.xyz[db.model_of == m][:n] for m, n in enumerate(N_TEST)]).astype(f32)
        self.maps = []
        for i, f in enumerate(self.frs):
            img, fill = synth.depth_image(db, f, seed=10 + i, fill_max=0.3)
            if i == len(self.frs) - 1:
                assert _draw_objects(db, f, img, fill, self.pts, self.pts_off) > 1000
            self.maps.append((torch.from_numpy(img).to(self.dev), torch.from_numpy(fill).to(self.dev)))
        self.uv = [torch.from_numpy(f.uv).to(self.dev) for f in self.frs]
        self.uv_all = torch.cat([torch.from_numpy(f.uv) for f in self.frs]).to(self.dev)
        self.prm = capi.default_frame_params()
        self.seeds = [5 + i for i in range(len(self.frs))]

    def context(self, linkage):
        from moped_amd import moped3d
        c = capi.Context(0)
        c.db_upload(c.normalize(self.db.desc), self.db.model_of, self.db.xyz, self.db.n_models)
        c.reserve(len(self.frs) * Q)
        if linkage:
            table = moped3d.ratio_table(self.db.xyz, self.db.model_of, self.db.n_models, synth.K_DEFAULT)
            c.frame_set_depth_rules(synth.K_DEFAULT, 64, 0.05, 0.01, table)
            c.frame_set_cluster_linkage(capi.default_linkage_params())
        return c

    def depth(self, c, f1, f2):
        if f1 is not None or f2 is not None:
            c.filter_depth_set_points(self.pts, self.pts_off)
        c.frame_set_filter_depth(f1, f2, synth.K_DEFAULT, synth.CAM_IDENTITY)

    def alone(self, c):
        out = []
        for i in range(len(self.frs)):
            c.frame_set_depth_image(self.maps[i][0].data_ptr(), self.maps[i][1].data_ptr(), 640, 480, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
            qd = self.torch.from_numpy(self.frs[i].desc).to(self.dev)   # (MATCH normalises the descriptors in place: a fresh copy)
            c.frame_enqueue(qd.data_ptr(), self.uv[i].data_ptr(), Q, synth.K_DEFAULT, synth.CAM_IDENTITY, self.prm, self.seeds[i])
            out.append(c.frame_fetch())
        return out

    def batch(self, c):
        B = len(self.frs)
        c.frame_set_depth_image_batch([m[0].data_ptr() for m in self.maps], [m[1].data_ptr() for m in self.maps], 640, 480,
                                      capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        qd = self.torch.cat([self.torch.from_numpy(f.desc) for f in self.frs]).to(self.dev)
        c.frame_enqueue_batch(qd.data_ptr(), self.uv_all.data_ptr(), Q, B, synth.K_DEFAULT, synth.CAM_IDENTITY, self.prm, self.seeds)
        return [c.frame_fetch_slot(f) for f in range(B)]


@pytest.fixture(scope="module")
def scene():
    return Scene()


def _equal(got, want, tag):
    (o, n), (a, an) = got, want
    assert np.array_equal(n, an), ("counts", tag, n, an)
    assert np.array_equal(o["model"], a["model"]), ("model", tag)
    assert np.array_equal(o["pose"].view(np.uint32), a["pose"].view(np.uint32)), ("pose", tag)
    assert np.array_equal(o["score"].view(np.uint32), a["score"].view(np.uint32)), ("score", tag)


@pytest.mark.parametrize("linkage", [False, True], ids=["mean_shift", "linkage_and_rules"])
def test_merged_batch_of_descriptor_frames_twice(scene, linkage):
    s = scene
    c = s.context(linkage)
    try:
        # the stand-alone route (timing on), feature off and on: what the depth class does to these frames
        s.depth(c, None, None)
        plain = _timed(c, lambda: s.alone(c))
        s.depth(c, PRM_D, PRM_D)
        apart = _timed(c, lambda: s.alone(c))
        assert c.frame_route().tolist() == [1, 0, 0, 0b11]
        removed = [sorted(set(p[0]["model"].tolist()) - set(a[0]["model"].tolist())) for p, a in zip(plain, apart)]
        kept = [sorted(set(p[0]["model"].tolist()) & set(a[0]["model"].tolist())) for p, a in zip(plain, apart)]
        print("plain", [p[0]["model"].tolist() for p in plain], "depth class", [a[0]["model"].tolist() for a in apart],
              "counts", [a[1].tolist() for a in apart])
        assert any(removed) and any(kept), (removed, kept)
        assert any(N_TEST[m] >= 63 for r in removed for m in r), removed      # (by test points, not by an empty list)
        assert any(N_TEST[m] >= 63 for k in kept for m in k), kept
        # the frames alone, fused
        fused = s.alone(c)
        assert c.frame_route().tolist() == [1, 0, 1, 0b11]
        for f in range(len(N_VIS)):
            _equal(fused[f], apart[f], ("alone, fused", f))
        # the batch, twice over the same arenas
        for rep in range(2):
            got = s.batch(c)
            assert c.frame_route().tolist() == [len(N_VIS), 1, 1, 0b11]
            for f in range(len(N_VIS)):
                _equal(got[f], apart[f], ("batch", rep, f))
    finally:
        c.close()


def test_kept_slots_across_workgroups_in_filter2(scene):
    """FILTER2 scores the objects FILTER kept again (pose_kept_f1: four slots per workgroup): more than four of them, the
    depth class in FILTER2 alone."""
    s = scene
    c = s.context(False)
    try:
        s.depth(c, None, PRM_D)
        apart = _timed(c, lambda: s.alone(c))
        assert apart[-1][1][3] >= 5, apart[-1][1]                 # objects kept by FILTER in the frame with six
        assert len(apart[-1][0]) >= 5
        fused = s.alone(c)
        assert c.frame_route().tolist() == [1, 0, 1, 0b10]
        got = s.batch(c)
        assert c.frame_route().tolist() == [len(N_VIS), 1, 1, 0b10]
        for f in range(len(N_VIS)):
            _equal(fused[f], apart[f], ("alone", f))
            _equal(got[f], apart[f], ("batch", f))
    finally:
        c.close()
