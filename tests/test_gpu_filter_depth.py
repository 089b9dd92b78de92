"""mh_filter_depth (filter_depth_kernel, csrc/filter_depth.hip) against the restatement of moped3d's
FILTER_PROJECTION_DEPTH_CPU::process (tests/filter_depth_ref.py) bit for bit: score, incorrect score, used and plausible
counts, keep flags, order and clusters, over generated cases (make_depth_case: a 40 x 30 map with holes, NaN and filled
pixels, a depth camera that is not the identity, test points per model at the chunk boundaries of the ordered chain,
object counts past a wavefront, the FILTER_GRID stride and FL_SLOTS); thresholds placed exactly on values the
restatement produced; calls on one context that must not see each other; stale test points after a DB edit.

A NaN has no defined bit pattern across the two machines (0/0 is 0xFFC00000 on x86 and 0x7FC00000 on the GPU): NaN
scores are compared as "NaN on both sides", everything else at the bits."""
import numpy as np
import pytest

import filter_depth_ref as fdr
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(a):
    a = np.array(a, f32)
    a[np.isnan(a)] = np.nan            # one pattern for every NaN
    return a.view(np.uint32)


def _device(ctx, c, **over):
    a = dict(c, **over)
    ctx.frame_set_depth_image_host(a["depth_img"], a["fill_img"])
    ctx.filter_depth_set_points(a["pts_xyz"], a["pts_off"])
    return ctx.filter_depth(capi.pack_corr(a["uv"], a["xyz"]), a["model_off"], a["obj_model"], a["obj_pose"], a["K"], a["cam"],
                            a["min_points"], a["fd"], a["min_score"], a["depth_K"], a["depth_cam"],
                            (a["psd"], a["depth_fraction"], a["min_kp_fraction"]))


def _ref(c, **over):
    a = dict(c, **over)
    return fdr.filter_projection_depth(a["uv"], a["xyz"], a["model_off"], a["obj_model"], a["obj_pose"], a["K"], a["cam"],
                                       a["min_points"], a["fd"], a["min_score"], a["pts_xyz"], a["pts_off"], a["depth_img"],
                                       a["fill_img"], a["depth_K"], a["depth_cam"], a["psd"], a["depth_fraction"],
                                       a["min_kp_fraction"])


def same(g, o, tag=None):
    for name, i in (("score", 0), ("incorrect_score", 4)):
        bad = np.nonzero(_bits(g[i]) != _bits(o[i]))[0]
        assert not len(bad), (name, tag, bad[:5], g[i][bad[:5]], o[i][bad[:5]])
    assert np.array_equal(g[5], o[5]), ("used", tag)
    assert np.array_equal(g[6], o[6]), ("plausible", tag)
    assert np.array_equal(g[1], o[1]), ("keep", tag)
    assert np.array_equal(g[2], o[2]), ("order", tag)
    assert len(g[3]) == len(o[3]), ("kept", tag)
    for k, (a, b) in enumerate(zip(g[3], o[3])):
        assert np.array_equal(a, b), ("members", k, tag)


@pytest.fixture(scope="module")
def dctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("block", [0, 1])
def test_filter_depth_kernel_equals_the_restatement(dctx, block):
    rng = np.random.default_rng([0xD3F, block])
    n_objs, n_pts = set(), set()
    kept = erased = penalised = nans = zeroed = 0
    for case in range(200):
        # every listed object count and test-point count comes round in every block, the rest is the generator's choice
        c = fdr.make_depth_case(rng, n_obj=fdr.N_OBJ[case // 8 % 4] if case % 8 == 0 else None,
                                n_pts=fdr.N_PTS[case % 7])
        o = _ref(c)
        same(_device(dctx, c), o, (block, case))
        n_objs.add(len(c["obj_model"]))
        n_pts.update(np.diff(c["pts_off"]).tolist())
        kept += int(o[1].sum())
        erased += int((~o[1]).sum())
        penalised += int((o[4] > 0).sum())
        zeroed += int(((o[4] == 0) & (o[5] > 0)).sum())
        nans += int(np.isnan(o[0]).sum())
    assert n_objs >= set(fdr.N_OBJ) and n_pts >= set(fdr.N_PTS), (n_objs, n_pts)
    assert kept > 200 and erased > 200 and penalised > 200 and zeroed > 50 and nans >= 1, (kept, erased, penalised, zeroed, nans)


def test_thresholds_exactly_on_values_the_restatement_produced(dctx):
    """min_score == an object's exact score - IS keeps it, nextafter above erases it; the object is one that pays a
    penalty, so a FILTER that compared the projection score would keep it both times."""
    rng = np.random.default_rng(0x7E57)
    hits = 0
    for case in range(60):
        c = fdr.make_depth_case(rng, n_obj=[3, 65, 129, 257][case % 4])
        base = _ref(c, min_points=0, min_score=-1e30)
        cand = np.nonzero((base[4] > 0) & (base[0] > 0) & np.isfinite(base[0]))[0]
        if not len(cand):
            continue
        o = int(cand[-1])
        s = f32(base[0][o])
        assert s < s + base[4][o]                       # (the penalty is visible at the score's precision)
        for ms, stays in ((float(s), True), (float(np.nextafter(s, f32(np.inf))), False)):
            r = _ref(c, min_points=0, min_score=ms)
            assert bool(r[1][o]) == stays
            same(_device(dctx, c, min_points=0, min_score=ms), r, ("min_score", case, stays))
        hits += 1
    assert hits >= 15, hits


def test_calls_on_one_context_do_not_see_each_other():
    """Different points, maps and sizes one after the other on one context: every call equals the same call on a fresh
    context and the restatement."""
    rng = np.random.default_rng(0x415D)
    sizes = [(257, 300), (1, 0), (129, 65), (3, 1), (65, 129), (2, 64)]
    c = capi.Context(0)
    try:
        for j, (n_obj, n_pts) in enumerate(sizes):
            cs = fdr.make_depth_case(rng, n_obj=n_obj, n_pts=n_pts)
            got = _device(c, cs)
            fresh = capi.Context(0)
            try:
                want = _device(fresh, cs)
            finally:
                fresh.close()
            same(got, want, ("fresh context", j))
            same(got, _ref(cs), ("restatement", j))
    finally:
        c.close()


def test_refusals_and_stale_points_after_a_db_edit():
    rng = np.random.default_rng(0x57A1)
    db = synth.make_db(3, 300, seed=11)
    c = capi.Context(0)
    try:
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        cs = fdr.make_depth_case(rng, n_obj=5)
        while len(cs["model_off"]) != 4:                 # three models, like the database
            cs = fdr.make_depth_case(rng, n_obj=5)
        args = (capi.pack_corr(cs["uv"], cs["xyz"]), cs["model_off"], cs["obj_model"], cs["obj_pose"], cs["K"], cs["cam"],
                cs["min_points"], cs["fd"], cs["min_score"], cs["depth_K"], cs["depth_cam"],
                (cs["psd"], cs["depth_fraction"], cs["min_kp_fraction"]))
        c.filter_depth_set_points(cs["pts_xyz"], cs["pts_off"])
        with pytest.raises(capi.MhError, match="no depth map"):
            c.filter_depth(*args)
        c.frame_set_depth_image_host(cs["depth_img"], cs["fill_img"])
        want = _ref(cs)
        same(c.filter_depth(*args), want, "before the edit")
        gen = c.db_generation()
        c.db_splice(capi.DB_REPLACE, 1, db.desc[:50], db.xyz[:50], normalize=True)
        assert c.db_generation() != gen
        with pytest.raises(capi.MhError, match="mh_filter_depth_set_points again"):
            c.filter_depth(*args)
        c.filter_depth_set_points(cs["pts_xyz"], cs["pts_off"])
        same(c.filter_depth(*args), want, "points set again")
        c.filter_depth_set_points(None, None)            # cleared
        with pytest.raises(capi.MhError, match="no test points"):
            c.filter_depth(*args)
        c.filter_depth_set_points(cs["pts_xyz"][:int(cs["pts_off"][2])], cs["pts_off"][:3])   # for two models only
        with pytest.raises(capi.MhError, match="another number of models"):
            c.filter_depth(*args)
    finally:
        c.close()
