"""The frame form of mean shift -- meanshift_models_kernel and layout_cluster_table, the CLUSTER step of the default frame
path -- exactly against the oracle, on frames injected behind MATCH (tests/cluster_frame_cases.py): a row of workgroups
that each cluster several models one after another in the same LDS, more than 1 024 models, n clusters in n points, the
parameters, merged batches, frames with several cameras ((model, image) pairs) and the capacity flags.

Every frame is checked in this order: the fetched match lists equal group_ref.expected; the per-model cluster lists
(mh_frame_debug_fetch_clusters_slot) equal the oracle's table; the flat table POSE walks
(mh_frame_debug_fetch_cluster_table_slot) equals it too; counts[1] is its length.  POSE .. FILTER2 run behind CLUSTER
with parameters under which they report nothing.  tests/test_cluster_frame_cases_cpu.py shows that the cases bite."""
import numpy as np
import pytest

import cluster_frame_cases as cs
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY


def _params(prm):
    p = capi.default_frame_params()
    p.ratio = cs.RATIO
    p.ms_radius, p.ms_merge, p.ms_min_pts, p.ms_max_iter = prm["radius"], prm["merge"], prm["min_pts"], prm["max_iter"]
    for pose in (p.pose1, p.pose2):     # one replica, one round of hypotheses, no cluster large enough for an object
        pose.n_hypotheses, pose.max_objects_per_cluster, pose.min_n_pts_object = 256, 1, 1 << 20
    return p


def _ctx(fr, frames=1, max_clusters=1024):
    """(an object slot per cluster and replica: 4 096 slots for at most 1 024 clusters)"""
    c = capi.Context(0)
    db = fr.db
    c.db_upload(db["desc"], db["model_of"], db["xyz"], db["n_models"])
    if frames > 1:
        c.reserve_batch(fr.Q, frames, max_clusters=max_clusters)
    else:
        c.reserve(fr.Q, max_clusters=max_clusters)
    return c


def _enqueue(c, fr, prm, seed=1):
    import torch
    dev = torch.device("cuda:0")
    w = torch.from_numpy(np.ascontiguousarray(fr.words).reshape(-1)).to(dev)
    u = torch.from_numpy(np.ascontiguousarray(fr.uv, np.float32)).to(dev)
    qi = torch.from_numpy(fr.q_img).to(dev) if fr.n_images > 1 else None
    torch.cuda.synchronize()        # (torch's stream made the copies; the context runs on its own)
    if qi is not None:
        c.frame_set_images(qi.data_ptr(), [K] * fr.n_images, [CAM0] * fr.n_images)
    c.frame_enqueue_rest(u.data_ptr(), fr.Q, w.data_ptr(), 1, K, CAM0, _params(prm), seed)
    return w, u, qi      # (alive until the frame is fetched)


def _check(c, fr, tab, objs, counts, slot=0, what=""):
    e = fr.e
    q, m = c.frame_fetch_matches_slot(slot)
    assert counts[0] == e["n"] and np.array_equal(q, e["q"]) and np.array_equal(m, e["model"]), what
    lists = [(mm, mem.tolist()) for mm, mem in c.frame_debug_fetch_clusters_slot(slot)]
    want = [(r[0], list(r[2])) for r in tab]
    assert len(lists) == len(want), (what, len(lists), len(want))
    for k, (a, b) in enumerate(zip(lists, want)):
        assert a == b, (what, "per-model lists, row", k, a[0], b[0])
    cm, cb, cc, now = c.frame_debug_fetch_cluster_table_slot(slot)
    assert np.array_equal(cm, [r[0] for r in tab]), (what, "cl_model")
    assert np.array_equal(cb, [r[1] for r in tab]), (what, "cl_begin")
    assert np.array_equal(cc, [len(r[2]) for r in tab]), (what, "cl_count")
    assert counts[1] == len(tab), (what, counts)
    # POSE .. FILTER2 reported nothing (and FILTER2, which kept nothing, left the device's row count at zero)
    assert len(objs) == 0 and counts[2] == 0 and counts[3] == 0 and now == 0, (what, counts, now)


def _run(c, fr, prm=cs.DEFAULT, what="", seed=1):
    tab = cs.table(fr, prm)
    keep = _enqueue(c, fr, prm, seed)
    objs, counts = c.frame_fetch()
    _check(c, fr, tab, objs, counts, 0, what)
    del keep
    return tab


def test_a_mixed_sizes_on_every_grid():
    """~60 models, 53 with work, sizes 0 .. 2048: on a fresh context, again (the grid is then sized by the feedback) and
    after a frame with a single busy model (the grid shrinks) -- the same table every time."""
    fr = cs.case_a()
    c = _ctx(fr)
    try:
        _run(c, fr, what="fresh")
        _run(c, fr, what="again")
        _run(c, cs.one_busy(), what="one busy model")
        _run(c, fr, what="after one busy model")
    finally:
        c.close()


def test_b_more_than_1024_models():
    fr = cs.case_b()
    c = _ctx(fr)
    try:
        _run(c, fr, what="2500 models")
        _run(c, fr, what="2500 models, again")
    finally:
        c.close()


def test_c_n_clusters_in_n_points():
    fr = cs.case_c()
    c = _ctx(fr)
    try:
        tab = _run(c, fr, cs.PRM_C, "n singletons")
        assert len(tab) == fr.e["n"] == 120
        _run(c, fr, cs.DEFAULT, "the same frame, default parameters")
    finally:
        c.close()


def test_d_parameters_reach_the_kernel():
    fr = cs.case_d()
    c = _ctx(fr)
    try:
        for name in ("iter1", "iter2", "iter100", "r60", "iter1"):
            _run(c, fr, cs.PRMS_D[name], name)
    finally:
        c.close()


def _batch(c, frames, prm=cs.DEFAULT):
    import torch
    dev = torch.device("cuda:0")
    B, Q = len(frames), frames[0].Q
    plane = B * Q
    words = np.zeros((1, 3, plane), np.int32)
    uv = np.zeros((plane, 2), np.float32)
    for f, fr in enumerate(frames):
        words[:, :, f * Q:(f + 1) * Q] = fr.words
        uv[f * Q:(f + 1) * Q] = fr.uv
    wt, ut = torch.from_numpy(words.reshape(-1)).to(dev), torch.from_numpy(uv).to(dev)
    torch.cuda.synchronize()
    c.frame_enqueue_rest_frames(ut.data_ptr(), Q, wt.data_ptr(), 1, 3 * plane, plane, B, K, CAM0, _params(prm),
                                [5 + f for f in range(B)])
    assert c.frame_route()[:2].tolist() == [B, 1]       # the frames shared their launches
    fetched = [c.frame_fetch_slot(f) for f in range(B)]
    for f, fr in enumerate(frames):
        _check(c, fr, cs.table(fr, prm), *fetched[f], slot=f, what=("slot", f))


def test_e_batch_of_four_frames():
    """No accepted match at all / case a / one busy model / only lists below MinPts in one merged batch: every slot's
    table is the oracle's for that frame alone -- twice, then with the frames in reverse order."""
    frames = cs.batch_e()
    c = _ctx(frames[0], frames=4)
    try:
        _batch(c, frames)
        _batch(c, frames)
        _batch(c, frames[::-1])
        _run(c, frames[1], what="a frame alone after the batches")
    finally:
        c.close()


@pytest.mark.parametrize("n_images", [2, 8])
def test_f_several_cameras(n_images):
    fr = cs.case_f(n_images)
    c = _ctx(fr)
    try:
        tab = _run(c, fr, what=("images", n_images))
        assert {r[0] for r in tab} <= set(range(fr.n_models))       # cl_model is the real model
        _run(c, fr, what=("images", n_images, "again"))
    finally:
        c.frame_set_images(0)
        c.close()


def test_g_cluster_cap_is_exact_at_k_and_an_error_at_k_plus_1():
    k = 3
    c = _ctx(cs.case_g(k), max_clusters=k)
    try:
        _run(c, cs.case_g(k), what="k clusters in k rows")
        keep = _enqueue(c, cs.case_g(k + 1), cs.DEFAULT)
        with pytest.raises(capi.MhError, match="capacity"):
            c.frame_fetch()
        del keep
        _run(c, cs.case_g(k), what="k clusters after the flagged frame")
    finally:
        c.close()


def test_g_a_list_past_the_mean_shift_capacity_is_an_error():
    over, after = cs.case_g_over_cap(), cs.case_g_after_cap()
    c = _ctx(over)
    try:
        keep = _enqueue(c, over, cs.DEFAULT)
        with pytest.raises(capi.MhError, match="capacity"):
            c.frame_fetch()
        del keep
        _run(c, after, what="2048 points after the flagged frame")
    finally:
        c.close()
