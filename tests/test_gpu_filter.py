"""The stand-alone FILTER launch (mh_filter / mh_filter_images: filter_kernel, csrc/filter.hip + filter_dev.h) against
the oracle's FILTER_PROJECTION_CPU::process (orclib.filter_projection / filter_images) bit for bit, over generated
cases at the sizes the kernel treats differently (tests/filter_cases.py): object slots past FL_SLOTS = 256 and the
FILTER_GRID = 128 grid stride, models past the 2 048-match in-cluster cache, equal scores on both sides of slots 128
and 256, (0.0, y) against (-0.0, y), points behind the camera; thresholds placed exactly on values the oracle
produced; and calls on one context that must not see each other."""
import numpy as np
import pytest

import filter_cases as fc
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu


def _device(ctx, c, **over):
    a = dict(c, **over)
    corr = capi.pack_corr(a["uv"], a["xyz"])
    if len(a["Ks"]) == 1:
        return ctx.filter(corr, a["model_off"], a["obj_model"], a["obj_pose"], a["Ks"][0], a["cams"][0], a["min_points"],
                          a["fd"], a["min_score"])
    return ctx.filter_images(corr, a["img"], a["model_off"], a["obj_model"], a["obj_pose"], a["Ks"], a["cams"],
                             a["min_points"], a["fd"], a["min_score"])


@pytest.mark.parametrize("n_images,block", [(1, b) for b in range(6)] + [(2, 0), (2, 1), (8, 0),
                                                                           (8, 1)])   # 8: MH_MAX_IMAGES
def test_filter_kernel_equals_the_oracle(ctx, n_images, block):
    rng = np.random.default_rng([0xF11, n_images, block])
    reached = fc.Regimes()
    other_image = same_image = 0
    for case in range(250):
        c = fc.make_case(rng, n_images)
        o = fc.oracle(c)
        fc.same(_device(ctx, c), o, (n_images, block, case))
        reached.add(c, o)
        if n_images > 1 and len(c["uv"]):
            keys = np.concatenate([(c["uv"] + np.float32(0)).view(np.uint32), c["img"][:, None].view(np.uint32)], 1)
            n_uv, n_key = len(np.unique(keys[:, :2], axis=0)), len(np.unique(keys, axis=0))
            other_image += n_key > n_uv                 # one coordinate in two images: two keys
            same_image += n_key < len(keys)             # one coordinate twice in one image: one key
    # the block reached what it is for
    assert reached.kept_past_256 and reached.big_cluster and reached.tie_128 and reached.tie_256, vars(reached)
    assert reached.signed_zero_owned and reached.empty_model_obj and reached.kept > 1000 and reached.erased > 1000, vars(reached)
    if n_images > 1:
        assert other_image > 20 and same_image > 20


def _pick(score, want):
    """The last object the oracle scored above 0 among those `want` takes (None: none)."""
    cand = [o for o in np.nonzero(score > 0)[0] if want(int(o))]
    return int(cand[-1]) if cand else None


@pytest.mark.parametrize("n_images", [1, 2])
def test_thresholds_exactly_on_values_the_oracle_produced(ctx, n_images):
    """min_score == an object's exact score keeps it, nextafter(score, inf) erases it; min_points == its owned count
    keeps it, one more erases it; feature_distance == one match's err2 leaves the match out (strict '<'), nextafter up
    takes it in.  The oracle's answer must change at each step (the threshold bites), the device's must follow."""
    rng = np.random.default_rng([0x7E5, n_images])
    hits = dict(score=0, points=0, dist=0, past_256=0, past_2048=0)
    for case in range(40):
        c = fc.make_case(rng, n_images, n_obj=[4, 129, 257, 600][case % 4])
        base = fc.oracle(c, min_points=0, min_score=0.0)
        if not len(base[2]):
            continue
        score = base[0]
        sizes = np.diff(c["model_off"])
        o = _pick(score, lambda o: o >= 256)
        o = _pick(score, lambda o: True) if o is None else o
        if o is None:
            continue
        hits["past_256"] += o >= 256
        # min_score on the score (min_points 0: every object owns enough)
        s = float(score[o])
        for ms, kept in ((s, True), (float(np.nextafter(np.float32(s), np.float32(np.inf))), False)):
            r = fc.oracle(c, min_points=0, min_score=ms)
            assert bool(r[1][o]) == kept
            fc.same(_device(ctx, c, min_points=0, min_score=ms), r, ("min_score", case, kept))
        hits["score"] += 1
        # min_points on its owned count (min_score 0: every object is kept in the base run)
        owned = len(base[3][int(np.nonzero(base[2] == o)[0][0])])
        for mp, kept in ((owned, True), (owned + 1, False)):
            r = fc.oracle(c, min_points=mp, min_score=0.0)
            assert bool(r[1][o]) == kept
            fc.same(_device(ctx, c, min_points=mp, min_score=0.0), r, ("min_points", case, kept))
        hits["points"] += 1
        # feature_distance on one match's err2: the last one with 0 < err2 < 10 (a term the score cannot lose), of an
        # object on a model of more than 2 048 matches when there is one
        ob = _pick(score, lambda o: sizes[c["obj_model"][o]] > 2048)
        ob = o if ob is None else ob
        e = fc.err2(c, ob)
        ok = np.nonzero((e > 0) & (e < 10))[0]
        if not len(ok):
            continue
        i = int(ok[-1])
        hits["past_2048"] += i >= 2048
        d = float(e[i])
        res = []
        for fd in (d, float(np.nextafter(np.float32(d), np.float32(np.inf)))):
            r = fc.oracle(c, min_points=0, min_score=0.0, fd=fd)
            fc.same(_device(ctx, c, min_points=0, min_score=0.0, fd=fd), r, ("feature_distance", case, fd))
            res.append(r)
        assert res[0][0][ob] != res[1][0][ob]                       # the match went in: the score moved
        hits["dist"] += 1
    assert hits["score"] >= 20 and hits["dist"] >= 20 and hits["past_256"] >= 5 and hits["past_2048"] >= 2, hits


def test_calls_on_one_context_do_not_see_each_other():
    """Growing, then shrinking match and object counts on one context, a whole frame in between: every call equals the
    same call on a fresh context (and the oracle) -- the claim table and the slot scratch hold nothing over."""
    rng = np.random.default_rng(0x415)
    db = synth.make_db(6, 800, seed=3)
    fr = synth.make_frame(db, n_vis=3, seed=4, Q=1500)
    prm = capi.default_frame_params()
    c = capi.Context(0)
    c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
    c.reserve(1500)
    cases = []
    while len(cases) < 8:       # M ascending then descending, object counts up then down
        cs = fc.make_case(rng, 1 + 7 * (len(cases) % 3 == 2), n_obj=[4, 129, 257, 600, 600, 256, 127, 1][len(cases)])
        cases.append(cs)
    order = sorted(range(4), key=lambda i: len(cases[i]["uv"])) + sorted(range(4, 8), key=lambda i: -len(cases[i]["uv"]))
    assert len(cases[order[3]]["uv"]) > 0
    try:
        for j, i in enumerate(order):
            got = _device(c, cases[i])
            fresh = capi.Context(0)
            try:
                want = _device(fresh, cases[i])
            finally:
                fresh.close()
            fc.same(got, want, ("fresh context", j))
            fc.same(got, fc.oracle(cases[i]), ("oracle", j))
            if j % 2 == 0:
                objs, counts = c.frame_run_host(fr.desc.copy(), fr.uv, [synth.K_DEFAULT], [synth.CAM_IDENTITY], prm, seed=j)
                assert len(objs) >= 1
    finally:
        c.close()


# ---------------------------------------------------------------------------------------- the fused FILTER tail
def _same_frame(a, b, tag):
    """Two runs of one frame: the per-stage counts first (matches, clusters, objects after POSE -- a failure names its
    stage), then every count, then the delivered (model, pose, score, n_points) bits."""
    (oa, ca), (ob, cb) = a, b
    assert np.array_equal(ca[:3], cb[:3]), ("counts up to POSE", tag, ca, cb)
    assert np.array_equal(ca, cb), ("counts", tag, ca, cb)
    assert np.array_equal(oa["model"], ob["model"]), tag
    assert np.array_equal(oa["pose"].view(np.uint32), ob["pose"].view(np.uint32)), tag
    assert np.array_equal(oa["score"].view(np.uint32), ob["score"].view(np.uint32)), tag
    assert np.array_equal(oa["n_points"], ob["n_points"]), tag


def _contexts(db, Q):
    """A default context (FILTER fused into the POSE launches) and one with stage timing (FILTER as its own filter_kernel
    launch, the un-merged batch path, the one-launch POSE)."""
    out = []
    for timing in (False, True):
        c = capi.Context(0)
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        c.reserve(Q)
        c.enable_timing(timing)
        out.append(c)
    return out


@pytest.mark.parametrize("name", ["duplicates", "duplicates_big", "slots", "pose2_none"])
def test_fused_filter_equals_the_filter_launch(name):
    db, fr, uv, Kx = fc.frame_scene(name)
    prm = capi.default_frame_params()
    fused, timed = _contexts(db, len(fr.desc))
    try:
        for seed in (3, 4):
            res = [c.frame_run_host(fr.desc.copy(), uv, [Kx], [synth.CAM_IDENTITY], prm, seed=seed) for c in (fused, timed)]
            _same_frame(res[0], res[1], (name, seed))
            assert len(res[0][0]) >= 1
        if name == "slots":
            assert res[0][1][2] > 256
    finally:
        fused.close()
        timed.close()


def test_fused_filter_equals_the_filter_launch_with_two_cameras():
    db = synth.make_db(6, 1500, seed=8)
    cams = [synth.camera_pose(0.0), synth.camera_pose(-0.12, (0.10, 0.0, 0.0))]
    fr = synth.make_frame_images(db, cams, n_vis=3, seed=15, q_per_image=900, pts_per_obj=130)
    prm = capi.default_frame_params()
    fused, timed = _contexts(db, len(fr.desc))
    try:
        res = [c.frame_run_host(fr.desc.copy(), fr.uv, fr.Ks, fr.cams, prm, seed=6, q_image=fr.image) for c in (fused, timed)]
    finally:
        fused.close()
        timed.close()
    _same_frame(res[0], res[1], "two cameras")
    assert len(res[0][0]) >= 2


def test_fused_batch_equals_the_frames_alone_with_the_filter_launch():
    """Distinct frames as one merged batch (fused FILTER tails) against the same frames one by one on a timing context
    (stand-alone FILTER launches)."""
    import torch
    from moped_amd.pipeline import FramePipeline, ShardedDB
    db = synth.make_db(12, 2000, seed=71)
    frs = [synth.make_frame(db, n_vis=n, seed=72 + i, Q=2000) for i, n in enumerate((1, 4, 0, 8, 2, 6))]
    B, Q = len(frs), 2000
    dev = torch.device("cuda:0")
    pipe = FramePipeline(0, ShardedDB(db.desc, db.xyz, db.model_of, db.n_models), depth=1, max_queries=B * Q, batch=B)
    _, timed = _contexts(db, Q)
    try:
        prm = pipe.params
        alone = [timed.frame_run_host(f.desc.copy(), f.uv, [synth.K_DEFAULT], [synth.CAM_IDENTITY], prm, seed=90 + i)
                 for i, f in enumerate(frs)]
        qd = torch.cat([torch.from_numpy(f.desc) for f in frs]).to(dev)
        uv = torch.cat([torch.from_numpy(f.uv) for f in frs]).to(dev)
        pipe.enqueue_batch(0, qd, uv, B, [90 + i for i in range(B)])
        batch = pipe.fetch_batch(0, B)
    finally:
        pipe.close()
        timed.close()
    for f in range(B):
        _same_frame(batch[f], alone[f], ("batch frame", f))
    assert sum(len(o) for o, _ in batch) >= 15


@pytest.mark.parametrize("kind", [capi.DEPTH_BACKPROJECTION, capi.DEPTH_REPROJECTION])
def test_fused_filter_equals_the_filter_launch_with_depth(kind):
    import torch
    from moped_amd.pipeline import FramePipeline, ShardedDB
    K = synth.K_DEFAULT
    db = synth.make_db(6, 2000, seed=81)
    fr = synth.make_frame(db, n_vis=3, seed=82, Q=1500, pts_per_obj=120)
    Q = len(fr.uv)
    world = np.stack([(fr.uv[:, 0] - K[2]) / K[0], (fr.uv[:, 1] - K[3]) / K[1], np.ones(Q)], 1).astype(np.float32)
    for j, m in enumerate(fr.visible):   # planted features: their true camera-frame point; clutter: a plane at 1 m
        rows = np.nonzero((fr.src_point >= 0) & (db.model_of[np.maximum(fr.src_point, 0)] == m) & ~fr.is_outlier)[0]
        R = synth.quat_to_R(fr.poses[j][:4])
        world[rows] = (db.xyz[fr.src_point[rows]].astype(np.float64) @ R.T + fr.poses[j][4:]).astype(np.float32)
    depth = capi.pack_depth(world, np.ones(Q, np.float32))
    dev = torch.device("cuda:0")
    pipe = FramePipeline(0, ShardedDB(db.desc, db.xyz, db.model_of, db.n_models), depth=1, max_queries=Q)
    try:
        c = pipe.ctxs[0]
        tdepth = torch.from_numpy(depth.view(np.float32).reshape(Q, 4)).to(dev)
        c.frame_set_depth(tdepth.data_ptr(), kind, 0.5)
        res = []
        for timing in (False, True):
            c.enable_timing(timing)
            pipe.enqueue(0, torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev), seed=9)
            res.append(pipe.fetch(0))
        c.enable_timing(False)
        c.frame_set_depth(0, 0)
    finally:
        pipe.close()
    _same_frame(res[0], res[1], ("depth", kind))
    assert len(res[0][0]) >= 2
