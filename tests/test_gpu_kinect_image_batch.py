"""Kinect frames in batches: a gray image and a depth map per frame, both on the device, in -- objects out.
mh_frame_enqueue_image_batch with the maps of mh_frame_set_depth_image_batch runs moped3d's front end
(moped3d/libmoped/src/config.hpp:38-49: DEPTHFILTER x 2, the adaptive ratio, DEPTHMAP_PROP, CLUSTER_LINKAGE, the depth
residual) behind FEAT for B frames with one launch per stage.  Every frame must give, bit for bit, what the path that is
pinned already gives it alone: mh_sift_extract -> mh_frame_set_depth_image -> mh_frame_enqueue with the host-known
keypoint count -- the same kernels and arithmetic on both sides, so no tolerance.

The scene is tests/test_gpu_image_frame.py's: the keypoints of bundled frame 0 on a plane 0.8 m in front of the camera are
model 0, 500 clutter rows model 1.  The images are bundled frames 0 and 3, a blank image and "thinned" (frame 0 with every
second 64-pixel column band painted gray).  The depth maps are that plane with a defect each, so that a frame that reads
another frame's map gives something else: NaN rows, a corner beyond MaximumDepth, sensor-like holes that DEPTHFILL
filled first.  (The planar model needs no relief: its control points come from the largest face of its bounding box,
which is the plane itself.)

FeatureDensity is 0.8, not the configuration's 0.05: on this scene 0.05 keeps 99.7 % of the keypoints and would test
nothing, 0.8 keeps 79 / 80 / 61 % (frames 0, 3, thinned on the plain plane) -- the test asserts that share with the
oracle before it trusts the device.

The trap for a DEPTHFILTER that ignores the frames' counts: a frame's keypoints lie at a stride of the capacity, and the
rows behind its count hold what an earlier batch left there.  The second order puts thinned (fewer keypoints) into the
slot that held frame 3 in the first: frame 3's last rows behind thinned's count change dozens of thinned's keep
verdicts if they are counted -- asserted on the CPU, so the trap is live."""
import os
import re
import types

import numpy as np
import pytest

import orclib
from moped_amd import capi, moped3d, synth
from test_gpu_depth_rules import _oracle_lists
from test_gpu_depthfill import holes

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
W, H = 640, 480
CAP = 1024                                   # rows per frame; every image has fewer keypoints
FEATURE_DENSITY, MATCH_DENSITY = 0.8, 0.01
BACK, REPRO = capi.DEPTH_BACKPROJECTION, capi.DEPTH_REPROJECTION
# (image, map) per slot.  B puts thinned where A had frame 3, and gives every image another map than A did.
ORDER_A = [("f0", "nan"), ("f3", "far"), ("blank", "far"), ("thin", "blobs"), ("f0", "blobs")]
ORDER_B = [("f0", "far"), ("thin", "nan"), ("blank", "nan"), ("f3", "blobs"), ("f0", "nan")]
# frame by frame only the last frame's lists and keep flags remain: thinned last, where A had frame 0 (more keypoints too)
ORDER_T = [("f0", "far"), ("f3", "blobs"), ("blank", "nan"), ("f0", "nan"), ("thin", "nan")]


def plane(z):
    """[H, W, 4] depth map (x, y, z, norm) of depths z [H, W] under K."""
    d = np.zeros((H, W, 4), np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    d[..., 2] = z
    d[..., 0] = (u - K[2]) / K[0] * z
    d[..., 1] = (v - K[3]) / K[1] * z
    d[..., 3] = np.sqrt((d[..., :3] ** 2).sum(-1))
    return d


def raw_maps():
    """The z = 0.8 plane with a defect per map, as a sensor would deliver them (before DEPTHFILL)."""
    z = np.full((H, W), 0.8, np.float32)
    z_nan, z_far, z_blobs = z.copy(), z.copy(), z.copy()
    z_nan[:40] = np.nan
    z_far[300:, :200] = 5.0                                   # beyond MaximumDepth (4 m)
    z_blobs[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = -1.0
    return {"nan": plane(z_nan), "far": plane(z_far), "blobs": plane(z_blobs), "plain": plane(z)}


def images():
    f0 = GOLD["gray0"]
    thin = f0.copy()
    for band in (1, 3, 5, 7, 9):
        thin[:, 64 * band:64 * (band + 1)] = 128
    return {"f0": f0, "f3": GOLD["gray3"], "blank": np.zeros_like(f0), "thin": thin}


class World:
    """One pipeline slot with the scene's DB, the images and maps on the device, and the frames alone (cached)."""

    def __init__(self):
        import torch
        from moped_amd.pipeline import FramePipeline, ShardedDB
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.gray = images()
        probe = capi.Context(0)
        self.kp = {k: probe.sift(g)[::2] for k, g in self.gray.items()}          # name -> (xy, raw descriptors)
        probe.close()
        xy, desc = self.kp["f0"]
        z = np.float32(0.8)
        xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
        rng = np.random.default_rng(7)
        clutter = np.abs(rng.normal(size=(500, 128))).astype(np.float32)          # a second model nobody sees
        self.db_desc = np.concatenate([desc, clutter])
        self.db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)])
        self.model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
        self.table = moped3d.ratio_table(self.db_xyz, self.model_of, 2, K)
        self.pipe = FramePipeline(0, ShardedDB(self.db_desc, self.db_xyz, self.model_of, 2), depth=1,
                                  max_queries=5 * CAP, batch=5)
        self.c = self.pipe.ctxs[0]
        self.prm = self.pipe.params
        # the maps as the frames see them: sensor-like holes filled (the oracle's DEPTHFILL; the device's own batch fill
        # must give the same bytes, checked in the fixture), the other defects as they are, distance 0
        self.raw = raw_maps()
        filled, dist, _ = orclib.depth_fill(self.raw["blobs"], K, 8, False)
        self.maps = {"nan": (self.raw["nan"], np.zeros((H, W), np.float32)),
                     "far": (self.raw["far"], np.zeros((H, W), np.float32)), "blobs": (filled, dist)}
        self.t_gray = {k: torch.from_numpy(g).to(self.dev) for k, g in self.gray.items()}
        self.t_maps = {k: (torch.from_numpy(m).to(self.dev), torch.from_numpy(f).to(self.dev)) for k, (m, f) in self.maps.items()}
        torch.cuda.synchronize()
        self._alone = {}
        self.front_end(True)

    def front_end(self, linkage):
        self.c.frame_set_depth_rules(K, 64, FEATURE_DENSITY, MATCH_DENSITY, self.table)
        self.c.frame_set_cluster_linkage(capi.default_linkage_params() if linkage else None)
        self.linkage = linkage

    def seed(self, img, mp):
        return 100 + 7 * sorted(self.gray).index(img) + sorted(self.raw).index(mp)

    def alone(self, img, mp, kind=BACK, maps=None):
        """The frame through the pinned path: host-known keypoints and count, its map set for one frame.
        -> dict(objs, counts, mq, mm, keep, n)."""
        key = (img, mp, kind, self.linkage, maps is not None)
        if key in self._alone:
            return self._alone[key]
        c, torch = self.c, self.torch
        xy, desc = self.kp[img]
        n = len(xy)
        if n == 0:   # (mh_frame_enqueue takes no empty frame: nothing in, nothing out)
            r = dict(objs=None, counts=np.zeros(4, np.int32), mq=np.zeros(0, np.int32), mm=np.zeros(0, np.int32),
                     keep=np.zeros(0, np.uint8), n=0)
        else:
            t_m, t_f = (maps or self.t_maps)[mp]
            c.frame_set_depth_image(t_m.data_ptr(), t_f.data_ptr(), W, H, kind, 0.5, 0.1)
            qd, uv = torch.from_numpy(desc).to(self.dev), torch.from_numpy(xy).to(self.dev)
            torch.cuda.synchronize()
            c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), n, K, CAM0, self.prm, self.seed(img, mp))
            objs, counts = c.frame_fetch()
            mq, mm = c.frame_fetch_matches()
            r = dict(objs=objs, counts=counts, mq=mq, mm=mm, keep=c.depth_rules_debug_fetch("keep1", 0, n), n=n)
        self._alone[key] = r
        return r

    def set_maps(self, order, kind=BACK, maps=None):
        t = maps or self.t_maps
        self.c.frame_set_depth_image_batch([t[m][0].data_ptr() for _, m in order], [t[m][1].data_ptr() for _, m in order],
                                           W, H, kind, 0.5, 0.1)

    def batch(self, order, kind=BACK):
        self.set_maps(order, kind)
        self.c.frame_enqueue_image_batch([self.t_gray[i].data_ptr() for i, _ in order], W, H, True, CAP, K, CAM0, self.prm,
                                         [self.seed(i, m) for i, m in order])

    def check_slot(self, slot, want, lists=True, tag=None):
        c = self.c
        objs, counts = c.frame_fetch_slot(slot)
        assert np.array_equal(counts, want["counts"]), (tag, slot, counts, want["counts"])
        if want["objs"] is None:
            assert len(objs) == 0, (tag, slot)
        else:
            assert objs.tobytes() == want["objs"].tobytes(), (tag, slot)
        if lists:
            mq, mm = c.frame_fetch_matches_slot(slot)
            assert np.array_equal(mq, want["mq"]) and np.array_equal(mm, want["mm"]), (tag, slot)
            keep = c.depth_rules_debug_fetch("keep1", slot, CAP)
            assert np.array_equal(keep[:want["n"]], want["keep"]), (tag, slot, int((keep[:want["n"]] != want["keep"]).sum()))

    def close(self):
        self.c.frame_set_depth_rules(off=True)
        self.c.frame_set_cluster_linkage(None)
        self.c.frame_set_depth_image(0, 0, 0, 0, 0)
        self.pipe.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def test_the_scene_bites_before_the_device_is_trusted(world):
    """CPU side: FeatureDensity 0.8 keeps and drops more than 15 % of every non-blank frame's keypoints, the stale-row
    trap is live, and the device's batch fill of the holed map gives the oracle's bytes (what the frames read)."""
    w = world
    plain = w.raw["plain"]
    for name in ("f0", "f3", "thin"):
        xy = w.kp[name][0]
        share = orclib.depthfilter_keep(plain, K, 64, FEATURE_DENSITY, xy).mean()
        print(name, len(xy), "keypoints, kept", round(float(share), 3))
        assert 0.15 < share < 0.85, (name, share)
    assert len(w.kp["blank"][0]) == 0
    # thinned's list with frame 3's last rows behind its count, as slot 1 of ORDER_B finds them after ORDER_A
    xy_t, xy_3 = w.kp["thin"][0], w.kp["f3"][0]
    assert len(xy_t) + 50 < len(xy_3) < CAP
    m = w.maps["nan"][0]
    right = orclib.depthfilter_keep(m, K, 64, FEATURE_DENSITY, xy_t)
    stale = orclib.depthfilter_keep(m, K, 64, FEATURE_DENSITY, np.concatenate([xy_t, xy_3[len(xy_t):]]))[:len(xy_t)]
    print("stale rows change", int((right != stale).sum()), "of", len(xy_t), "verdicts")
    assert int((right != stale).sum()) >= 10
    # ... and with frame 0's last rows behind it, as the last slot of ORDER_T finds them after ORDER_A
    xy_0 = w.kp["f0"][0]
    stale0 = orclib.depthfilter_keep(m, K, 64, FEATURE_DENSITY, np.concatenate([xy_t, xy_0[len(xy_t):]]))[:len(xy_t)]
    print("frame 0's stale rows change", int((right != stale0).sum()), "of", len(xy_t), "verdicts")
    assert int((right != stale0).sum()) >= 10
    # DEPTHFILL of the holed map on the device, in a batch beside the two others (whose NaN rows it fills too: copies)
    torch = w.torch
    t_d = [torch.from_numpy(w.raw[k]).to(w.dev) for k in ("blobs", "nan")]
    t_f = [torch.empty((H, W), dtype=torch.float32, device=w.dev) for _ in t_d]
    torch.cuda.synchronize()
    w.c.depth_fill_batch_dev([t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], W, H, K, 8, False)
    w.c.depth_fill_status()
    assert np.array_equal(t_d[0].cpu().numpy().view(np.uint32), w.maps["blobs"][0].view(np.uint32))
    assert np.array_equal(t_f[0].cpu().numpy().view(np.uint32), w.maps["blobs"][1].view(np.uint32))
    assert w.maps["blobs"][1].max() > 0 and not (w.maps["blobs"][0][..., 2] < 0).any()


def test_the_frames_alone_find_the_model_and_depend_on_their_maps(world):
    w = world
    for img in ("f0", "f3"):
        for mp in ("nan", "far", "blobs"):
            a = w.alone(img, mp)
            assert len(a["objs"]) >= 1 and a["counts"][0] > 50, (img, mp, a["counts"])
            best = a["objs"][np.argmax(a["objs"]["score"])]
            assert best["model"] == 0
            assert np.abs(best["pose"][4:7]).max() < 0.05 and abs(abs(best["pose"][3]) - 1) < 0.01
        lists = [w.alone(img, mp)["mq"].tobytes() for mp in ("nan", "far", "blobs")]
        assert len(set(lists)) == 3, img     # a frame that read another frame's map would show
    assert 0.15 < w.alone("thin", "nan")["keep"].mean() < 0.85


def test_batches_of_five_in_two_orders_twice_equal_the_frames_alone(world):
    w = world
    for tag, order in (("A", ORDER_A), ("B", ORDER_B)):
        want = [w.alone(i, m) for i, m in order]
        for rep in range(2):
            w.batch(order)
            for slot in range(len(order)):
                w.check_slot(slot, want[slot], tag=(tag, rep))


def test_one_slot_against_the_oracle(world):
    """Not device against device only: frame 3 under the map with the far corner -- keep flags = the oracle's
    DEPTHFILTER on that map and the frame's keypoints, match list = the oracle's selection from its exact 2-NN search."""
    w = world
    order = ORDER_A
    slot = 1
    img, mp = order[slot]
    w.batch(order)
    xy, desc = w.kp[img]
    n = len(xy)
    m, f = w.maps[mp]
    keep = w.c.depth_rules_debug_fetch("keep1", slot, CAP)[:n]
    assert np.array_equal(keep.astype(bool), orclib.depthfilter_keep(m, K, 64, FEATURE_DENSITY, xy))
    idx, d1, d2 = orclib.match_2nn(orclib.normalize(w.db_desc), orclib.normalize(desc))
    s = dict(db=types.SimpleNamespace(model_of=w.model_of, n_models=2), fr=types.SimpleNamespace(uv=xy), idx=idx, d1=d1,
             d2=d2, img=m, fill=f)
    want_q, want_m = _oracle_lists(s, FEATURE_DENSITY, MATCH_DENSITY, w.table)
    got_q, got_m = w.c.frame_fetch_matches_slot(slot)
    assert len(want_q) > 50
    assert np.array_equal(got_q, want_q) and np.array_equal(got_m, want_m)


def test_frame_by_frame_form_with_timing_on(world):
    """mh_enable_timing keeps the frames apart: each runs its own launches with its own map and count.  The frames then
    share one set of working arrays, so only the last one's lists and keep flags remain to be fetched: thinned is last,
    behind its count the rows frame 0 left in that slot."""
    w = world
    want = [w.alone(i, m) for i, m in ORDER_T]         # (the frames alone run as they always do, before timing is on)
    w.batch(ORDER_A)
    w.c.enable_timing(True)
    try:
        w.batch(ORDER_T)
        for slot in range(len(ORDER_T)):
            w.check_slot(slot, want[slot], lists=slot == len(ORDER_T) - 1, tag="timing")
    finally:
        w.c.enable_timing(False)


@pytest.mark.parametrize("variant", ["meanshift", "reprojection"])
def test_mean_shift_and_the_reprojection_residual(world, variant):
    w = world
    kind = REPRO if variant == "reprojection" else BACK
    order = [("f3", "far"), ("thin", "blobs"), ("f0", "nan")]
    try:
        if variant == "meanshift":
            w.front_end(False)
        want = [w.alone(i, m, kind) for i, m in order]
        assert any(len(a["objs"]) >= 1 for a in want)
        w.batch(ORDER_A)
        w.batch(order, kind)
        for slot in range(len(order)):
            w.check_slot(slot, want[slot], tag=variant)
    finally:
        w.front_end(True)


def test_enqueue_kinect_batch_fills_the_maps_itself(world):
    """FramePipeline.enqueue_kinect_batch: raw sensor maps in; DEPTHFILL of the batch, the maps' hand-over and the image
    batch on the slot's stream.  Every frame equals the frame alone under the oracle's fill of its raw map (NaN depths
    are holes to the fill)."""
    w = world
    torch = w.torch
    order = [("f0", "blobs"), ("f3", "nan"), ("thin", "far")]
    filled = {k: orclib.depth_fill(w.raw[k], K, 8, False)[:2] for _, k in order}
    t_filled = {k: (torch.from_numpy(m).to(w.dev), torch.from_numpy(f).to(w.dev)) for k, (m, f) in filled.items()}
    want = [w.alone(i, m, BACK, t_filled) for i, m in order]
    assert len(want[0]["objs"]) >= 1 and len(want[1]["objs"]) >= 1
    for rep in range(2):
        t_d = [torch.from_numpy(w.raw[m]).to(w.dev) for _, m in order]
        t_f = [torch.empty((H, W), dtype=torch.float32, device=w.dev) for _ in order]
        torch.cuda.synchronize()
        w.pipe.enqueue_kinect_batch(0, [w.t_gray[i].data_ptr() for i, _ in order], [t.data_ptr() for t in t_d],
                                    [t.data_ptr() for t in t_f], W, H, [w.seed(i, m) for i, m in order], fill_scale=8,
                                    max_keypoints=CAP, keep=(t_d, t_f))
        for slot in range(len(order)):
            w.check_slot(slot, want[slot], tag=("kinect", rep))
        w.c.depth_fill_status()
        for t, (_, m) in zip(t_d, order):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), filled[m][0].view(np.uint32))
    # fill_scale=None: the maps arrive filled
    w.pipe.enqueue_kinect_batch(0, [w.t_gray[i].data_ptr() for i, _ in order], [t_filled[m][0].data_ptr() for _, m in order],
                                [t_filled[m][1].data_ptr() for _, m in order], W, H, [w.seed(i, m) for i, m in order],
                                fill_scale=None, max_keypoints=CAP)
    for slot in range(len(order)):
        w.check_slot(slot, want[slot], tag="filled")


def test_single_image_with_a_map_and_rules_equals_the_two_step_path(world):
    """mh_frame_enqueue_image with a depth map, the rules and the linkage clusterer -- after frame 3, so that thinned
    finds frame 3's rows behind its count."""
    w = world
    c = w.c
    for img, mp in (("f3", "far"), ("thin", "nan"), ("blank", "nan"), ("f0", "blobs")):
        want = w.alone(img, mp)
        t_m, t_f = w.t_maps[mp]
        c.frame_set_depth_image(t_m.data_ptr(), t_f.data_ptr(), W, H, BACK, 0.5, 0.1)
        c.frame_enqueue_image(w.t_gray[img].data_ptr(), W, H, True, CAP, K, CAM0, w.prm, w.seed(img, mp))
        objs, counts = c.frame_fetch()
        assert c.frame_keypoints() == want["n"]
        assert np.array_equal(counts, want["counts"]), (img, mp)
        if want["objs"] is None:
            assert len(objs) == 0
            continue
        assert objs.tobytes() == want["objs"].tobytes(), (img, mp)
        mq, mm = c.frame_fetch_matches()
        assert np.array_equal(mq, want["mq"]) and np.array_equal(mm, want["mm"])
        assert np.array_equal(c.depth_rules_debug_fetch("keep1", 0, CAP)[:want["n"]], want["keep"])
    # a batch of one image with the single frame's map counts too
    want = w.alone("f3", "far")
    t_m, t_f = w.t_maps["far"]
    c.frame_set_depth_image(t_m.data_ptr(), t_f.data_ptr(), W, H, BACK, 0.5, 0.1)
    c.frame_enqueue_image_batch([w.t_gray["f3"].data_ptr()], W, H, True, CAP, K, CAM0, w.prm, [w.seed("f3", "far")])
    w.check_slot(0, want, tag="B=1")


def test_refusals_and_the_plain_image_batch_afterwards(world):
    w = world
    c, torch = w.c, w.torch
    grays = [w.t_gray[i].data_ptr() for i, _ in ORDER_A]
    seeds = [w.seed(i, m) for i, m in ORDER_A]

    def refused(names):
        with pytest.raises(capi.MhError) as e:
            c.frame_enqueue_image_batch(grays, W, H, True, CAP, K, CAM0, w.prm, seeds)
        msg = str(e.value)
        assert "-> -1:" in msg and any(re.search(n + r"(?![_\w])", msg) for n in names), msg

    w.set_maps(ORDER_A[:2])                                   # two maps, five images
    refused(["mh_frame_set_depth_image_batch"])
    attrs = torch.zeros((5 * CAP, 4), dtype=torch.float32, device=w.dev)
    w.set_maps(ORDER_A)
    c.frame_set_depth(attrs.data_ptr(), BACK)                 # per-query attributes: nobody has them for device-made queries
    refused(["mh_frame_set_depth_image_batch", "mh_frame_set_depth"])
    c.frame_set_depth(0, BACK)
    q_img = torch.zeros(5 * CAP, dtype=torch.int32, device=w.dev)
    w.set_maps(ORDER_A)
    c.frame_set_images(q_img.data_ptr(), [K, K], [CAM0, CAM0])   # a per-query image index with two images
    refused(["mh_frame_enqueue_images_batch"])
    c.frame_set_images(0)
    c.frame_set_depth_image(0, 0, 0, 0, 0)                    # the rules without any depth map
    refused(["mh_frame_set_depth_image_batch"])
    # the context is as it was: the depth batch still runs and gives the frames alone
    want = [w.alone(i, m) for i, m in ORDER_A]
    w.batch(ORDER_A)
    for slot in range(len(ORDER_A)):
        w.check_slot(slot, want[slot], tag="after refusals")
    # and without the front end the plain image batch is the images alone (test_batch_of_images_equals_the_images_alone)
    c.frame_set_depth_rules(off=True)
    c.frame_set_cluster_linkage(None)
    c.frame_set_depth_image(0, 0, 0, 0, 0)
    try:
        alone = []
        for i, (img, mp) in enumerate(ORDER_A):
            c.frame_enqueue_image(w.t_gray[img].data_ptr(), W, H, True, CAP, K, CAM0, w.prm, seeds[i])
            alone.append(c.frame_fetch())
        c.frame_enqueue_image_batch(grays, W, H, True, CAP, K, CAM0, w.prm, seeds)
        for slot, (objs, counts) in enumerate(alone):
            got, got_counts = c.frame_fetch_slot(slot)
            assert np.array_equal(got_counts, counts) and got.tobytes() == objs.tobytes(), slot
        assert len(alone[0][0]) >= 1 and len(alone[2][0]) == 0
    finally:
        w.front_end(True)
