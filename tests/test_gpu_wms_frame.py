"""moped3d's weighted mean shift as the CLUSTER step of single-camera frames (mh_frame_set_cluster_wms): whole frames --
descriptors in, objects out -- over the 20-model frames and per-frame depth / fill maps of tests/test_gpu_linkage_stages.py.

What a frame's CLUSTER left (mh_frame_debug_fetch_clusters_slot: the per-model lists; mh_frame_debug_fetch_cluster_table_slot:
the flat table POSE walks) must equal the float32 restatement of the reference's class (tests/wms_ref.py) run on the frame's
OWN fetched matches: points = the depth map's pixel under ((int) u, (int) v), fill distances = the fill map's there, both
clamped to the map.  Exact: members, member order (descending), cluster order, table rows.  A model's clusters may overlap and
hold up to MH_WMS_MEMBER_FACTOR x its matches; the first that would pass that is dropped whole with the later ones (restated
below) and the frame's capacity flag is set."""
import numpy as np
import pytest

import orclib
import wms_ref
from moped_amd import capi, synth
from test_gpu_linkage_stages import H, K, CAM0, N_MODELS, PLANTED, Q_FRAME, W, counted_frame, frame_maps

pytestmark = pytest.mark.gpu
FACTOR = capi.WMS_MEMBER_FACTOR
DEFAULT = (0.1, 0.02, 7, 100, 10.0)      # Radius, Merge (metres), MinPts, MaxIterations, halfWeightDistance (pixels)
OVERLAP = (0.15, 0.005, 7, 100, 10.0)    # canopies that hold each other's points: up to 2.2 memberships per match (frame 0)
AT_FACTOR = (0.12, 0.01, 5, 50, 25.0)    # frame 0: one model's clusters hold exactly FACTOR x its matches -- kept, `>` decides
EXCEED = (0.3, 0.02, 7, 0, 10.0)         # MaxIterations 0: a cluster around every match -- n x ~n members for n matches


def restated(fr, img, fill, mq, mm, prm):
    """-> (rows [(model, members)], cl_begin per row, models that passed the factor): the frame's cluster table by the
    restatement, over the fetched match lists (queries mq of models mm, model after model)."""
    R, M, min_pts, max_iter, hwd = prm
    rows, begin, over = [], [], []
    for m in range(N_MODELS):
        pos = np.flatnonzero(mm == m)
        n = len(pos)
        if n <= min_pts:
            continue
        uv = fr.uv[mq[pos]]
        world, _ = orclib.depthmap_prop(img, fill, uv, 0.1)
        ix = np.clip(uv[:, 0].astype(np.int32), 0, W - 1)
        iy = np.clip(uv[:, 1].astype(np.int32), 0, H - 1)
        clusters, _, _, _ = wms_ref.weighted_mean_shift(world, wms_ref.cauchy_weight(fill[iy, ix], hwd), R, M, min_pts, max_iter)
        used = 0
        for cl in clusters:
            if used + len(cl) > FACTOR * n:      # dropped whole, with the model's later ones
                over.append(m)
                break
            rows.append((m, cl.tolist()))
            begin.append(FACTOR * int(pos[0]) + used)
            used += len(cl)
    return rows, begin, over


class Frames:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.db = synth.make_db(N_MODELS, 400, seed=11)
        rot = lambda k: PLANTED[k:] + PLANTED[:k]
        self.frames = [counted_frame(self.db, rot(7 * f), 40 + f) for f in range(3)]
        self.maps = [frame_maps(self.db, fr, f) for f, fr in enumerate(self.frames)]
        self.t_maps = [(torch.from_numpy(m).to(self.dev), torch.from_numpy(f).to(self.dev)) for m, f in self.maps]
        torch.cuda.synchronize()

    def context(self, reserve, prm=DEFAULT):
        c = capi.Context(0)
        c.db_upload(c.normalize(self.db.desc), self.db.model_of, self.db.xyz, self.db.n_models)
        c.reserve(reserve, max_clusters=4096)
        if prm is not None:
            c.frame_set_cluster_wms(capi.mh_wms_params(*prm))
        return c

    @staticmethod
    def params(silent):
        """silent: POSE .. FILTER2 report nothing (no cluster is large enough for an object), so that the flat cluster table
        is still CLUSTER's when the frame is through -- FILTER rewrites it for POSE2 otherwise"""
        p = capi.default_frame_params()
        if silent:
            for pose in (p.pose1, p.pose2):
                pose.n_hypotheses, pose.max_objects_per_cluster, pose.min_n_pts_object = 256, 1, 1 << 20
        return p

    def enqueue(self, c, f, seed=5, with_map=True, silent=False):
        torch = self.torch
        if with_map:
            m, fl = self.t_maps[f]
            c.frame_set_depth_image(m.data_ptr(), fl.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        fr = self.frames[f]
        qd, uv = torch.from_numpy(fr.desc).to(self.dev), torch.from_numpy(fr.uv).to(self.dev)
        torch.cuda.synchronize()
        c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), Q_FRAME, K, CAM0, self.params(silent), seed + f)

    def check(self, c, f, prm, counts, what="", table=True, slot=0):
        """the last frame's lists and table (it went into `slot`) against the restatement on its own matches -> (rows, over, mm)"""
        mq, mm = c.frame_fetch_matches_slot(slot)
        rows, begin, over = restated(self.frames[f], *self.maps[f], mq, mm, prm)
        got = [(m, mem.tolist()) for m, mem in c.frame_debug_fetch_clusters_slot(slot, cap_members=1 << 18)]
        assert len(got) == len(rows), (what, len(got), len(rows))
        for k, (a, b) in enumerate(zip(got, rows)):
            assert a == b, (what, "per-model lists, row", k, a[0], b[0])
        if table:
            cm, cb, cc, _ = c.frame_debug_fetch_cluster_table_slot(slot)
            assert np.array_equal(cm, [r[0] for r in rows]), (what, "cl_model")
            assert np.array_equal(cb, begin), (what, "cl_begin")
            assert np.array_equal(cc, [len(r[1]) for r in rows]), (what, "cl_count")
        if counts is not None:
            assert counts[0] == len(mq) and counts[1] == len(rows), (what, counts)
        return rows, over, mm

    def alone(self, c, f, prm, what=""):
        """the frame twice: silent, for the lists and the flat table as CLUSTER left them; then as a user runs it, for the
        objects (the lists once more) -> (objs, counts, rows, mm)"""
        self.enqueue(c, f, silent=True)
        objs, counts = c.frame_fetch()
        assert len(objs) == 0
        rows, over, mm = self.check(c, f, prm, counts, what)
        assert not over, what
        self.enqueue(c, f)
        objs, counts = c.frame_fetch()
        assert self.check(c, f, prm, counts, what, table=False)[0] == rows
        return objs, counts, rows, mm


@pytest.fixture(scope="module")
def frames():
    return Frames()


def _close(c):
    c.frame_set_cluster_wms(None)
    c.frame_set_cluster_linkage(None)
    c.frame_set_depth_image(0, 0, 0, 0, 0)
    c.close()


def test_lists_and_table_equal_the_restatement(frames):
    w = frames
    c = w.context(Q_FRAME)
    try:
        for f in range(3):
            objs, counts, rows, mm = w.alone(c, f, DEFAULT, f)
            print(f, "clusters", len(rows), "objects", len(objs))
            assert len(rows) >= 10 and len({m for m, _ in rows}) >= 8 and len(objs) >= 1
        again = w.alone(c, 0, DEFAULT, "again")
        assert again[2] == w.alone(c, 0, DEFAULT, "and again")[2]
    finally:
        _close(c)


def test_overlap_inside_the_factor(frames):
    w = frames
    c = w.context(Q_FRAME, OVERLAP)
    try:
        objs, counts, rows, mm = w.alone(c, 0, OVERLAP, "overlap")
        ratio = {m: sum(len(r[1]) for r in rows if r[0] == m) / int((mm == m).sum()) for m in {r[0] for r in rows}}
        print("memberships per match", {m: round(v, 2) for m, v in ratio.items()})
        assert max(ratio.values()) > 1.0 and max(ratio.values()) <= FACTOR      # a match in several clusters, no model cut
        # some match really is in two clusters of its model
        m = max(ratio, key=ratio.get)
        members = np.concatenate([r[1] for r in rows if r[0] == m])
        assert len(np.unique(members)) < len(members)
        assert len(objs) >= 1
        c.frame_set_cluster_wms(capi.mh_wms_params(*AT_FACTOR))
        objs, counts, rows, mm = w.alone(c, 0, AT_FACTOR, "at the factor")
        assert max(sum(len(r[1]) for r in rows if r[0] == m) / int((mm == m).sum()) for m in {r[0] for r in rows}) == FACTOR
    finally:
        _close(c)


def test_past_the_factor_whole_clusters_the_flag_and_a_clean_next_frame(frames):
    w = frames
    c = w.context(Q_FRAME, EXCEED)
    try:
        w.enqueue(c, 0, silent=True)
        with pytest.raises(capi.MhError, match="capacity"):
            c.frame_fetch()
        rows, over, mm = w.check(c, 0, EXCEED, None, "past the factor")   # (the fetch that raised delivered no counts)
        assert len(over) >= 5                                     # models whose clusters were cut ...
        for m in over:                                            # ... hold whole clusters inside FACTOR x their matches
            n = int((mm == m).sum())
            used = sum(len(r[1]) for r in rows if r[0] == m)
            assert 0 < used <= FACTOR * n
        c.frame_set_cluster_wms(capi.mh_wms_params(*DEFAULT))
        w.alone(c, 0, DEFAULT, "the next frame")                  # no flag, the right table
    finally:
        _close(c)


def test_a_batch_of_three_equals_the_frames_one_by_one(frames):
    w, torch = frames, frames.torch
    c = w.context(3 * Q_FRAME)
    try:
        alone = [w.alone(c, f, DEFAULT, f) for f in range(3)]
        c.frame_set_depth_image_batch([m.data_ptr() for m, _ in w.t_maps], [fl.data_ptr() for _, fl in w.t_maps], W, H,
                                      capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        uv = torch.cat([torch.from_numpy(fr.uv) for fr in w.frames]).to(w.dev)
        qd = torch.cat([torch.from_numpy(fr.desc) for fr in w.frames]).to(w.dev)
        torch.cuda.synchronize()
        c.frame_enqueue_batch(qd.data_ptr(), uv.data_ptr(), Q_FRAME, 3, K, CAM0, capi.default_frame_params(), [5, 6, 7])
        assert c.frame_route()[1] == 0                            # frame by frame: the members' buffer is the context's
        for f in range(3):
            objs, counts = c.frame_fetch_slot(f)
            assert np.array_equal(counts, alone[f][1]), f
            assert objs.tobytes() == alone[f][0].tobytes(), f
        w.check(c, 2, DEFAULT, alone[2][1], "the batch's last frame", table=False, slot=2)   # (frame by frame only the last frame's lists remain)
    finally:
        _close(c)


def test_mode_off_and_the_linkage_setter_afterwards(frames):
    w = frames
    c = w.context(Q_FRAME, None)
    try:
        def run():
            w.enqueue(c, 0)
            objs, counts = c.frame_fetch()
            return objs.tobytes(), counts.tolist(), [(m, mem.tolist()) for m, mem in c.frame_debug_fetch_clusters_slot(0)], \
                [a.tolist() for a in c.frame_debug_fetch_cluster_table_slot(0)[:3]]
        plain = run()                                             # mean shift: the parent's table
        c.frame_set_cluster_wms(capi.mh_wms_params(*DEFAULT))
        assert w.alone(c, 0, DEFAULT, "on")[2] != plain[2]
        c.frame_set_cluster_wms(None)
        assert run() == plain                                     # off again: nothing has changed
        c.frame_set_cluster_linkage(capi.default_linkage_params())
        linkage = run()
        c.frame_set_cluster_wms(capi.mh_wms_params(*DEFAULT))     # the one set last is on ...
        w.alone(c, 0, DEFAULT, "after linkage")
        c.frame_set_cluster_linkage(capi.default_linkage_params())   # ... and the linkage setter takes over again
        assert run() == linkage and linkage[2] != plain[2]
    finally:
        _close(c)


def test_refusals(frames):
    w, torch = frames, frames.torch
    c = w.context(Q_FRAME)
    try:
        for bad in (dict(radius=float("nan")), dict(merge=-1.0), dict(half_weight_distance=float("nan")), dict(max_iter=-1)):
            with pytest.raises(capi.MhError, match="-> -1: mh_frame_set_cluster_wms: " + next(iter(bad))):
                c.frame_set_cluster_wms(capi.mh_wms_params(**bad))
        # no depth map
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        with pytest.raises(capi.MhError, match="-> -1:.*no depth map"):
            w.enqueue(c, 0, with_map=False)
        # the sharded entry points: a gathered block in place of the context's own MATCH
        m, fl = w.t_maps[0]
        c.frame_set_depth_image(m.data_ptr(), fl.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        words = torch.zeros(3 * Q_FRAME, dtype=torch.int32, device=w.dev)
        uv = torch.from_numpy(w.frames[0].uv).to(w.dev)
        torch.cuda.synchronize()
        with pytest.raises(capi.MhError, match="-> -1:.*sharded"):
            c.frame_enqueue_rest(uv.data_ptr(), Q_FRAME, words.data_ptr(), 1, K, CAM0, capi.default_frame_params(), 1)
        # several cameras
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        qi = torch.zeros(Q_FRAME, dtype=torch.int32, device=w.dev)
        torch.cuda.synchronize()
        c.frame_set_images(qi.data_ptr(), [K] * 2, [CAM0] * 2)
        with pytest.raises(capi.MhError, match="-> -1:"):
            w.enqueue(c, 0, with_map=False)
        c.frame_set_images(0)
        w.alone(c, 0, DEFAULT, "after the refusals")              # the context goes on
    finally:
        _close(c)


def test_the_bundled_kinect_scene_reports_the_planted_object():
    """Bundled frame 0 over the filled "blobs" map (tests/test_gpu_kinect_image_batch.py's scene, depth rules on): one
    planar model of ~590 keypoints spanning about a metre -- a Radius that holds it -- within that module's pose bar."""
    from test_gpu_kinect_image_batch import World
    w = World()
    try:
        w.c.frame_set_cluster_wms(capi.mh_wms_params(0.7, 0.05, 7, 100, 10.0))
        w.linkage = "wms"
        a = w.alone("f0", "blobs")
        assert len(a["objs"]) >= 1 and a["counts"][0] > 50, a["counts"]
        best = a["objs"][np.argmax(a["objs"]["score"])]
        print("pose", best["pose"], "matches", a["counts"][0])
        assert best["model"] == 0
        assert np.abs(best["pose"][4:7]).max() < 0.05 and abs(abs(best["pose"][3]) - 1) < 0.01
    finally:
        w.c.frame_set_cluster_wms(None)
        w.close()
