"""Resident frames hand MATCH their ratio (csrc/api_frame.hip: frame_accept_ratio), so pass C answers the queries the ratio
test provably rejects without a search: everything behind MATCH must be what it is with the exact triple of every query
(mh_match_set_accept(-1)) -- the accepted match lists, the cluster tables, the objects' poses and scores bit for bit.
A batch of 16 frames x 768 queries (one MATCH launch of 12 288, the counted lists) and a frame alone (the lane-private
slots), on the 20 x 5 000 DB.  A context with a depth-adaptive ratio table keeps the exact triples: nothing pre-rejected."""
import numpy as np
import pytest

from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
Q, B = 768, 16
N_VIS = (2, 2, 5, 1, 2, 3, 0, 2, 4, 2, 0, 1, 2, 2, 3, 2)


@pytest.fixture(scope="module")
def scene():
    import torch
    dev = torch.device("cuda:0")
    db = synth.make_db(20, 5000)
    frs = [synth.make_frame(db, n_vis=n, seed=500 + i, Q=Q, pts_per_obj=120) for i, n in enumerate(N_VIS)]
    c = capi.Context(0)
    c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
    c.reserve_batch(Q, B)
    assert capi.screen_launch_plan(B * Q, len(db.desc))["onesweep"] == 1 and c.match_stats(Q)["two_stage"]
    yield torch, dev, db, frs, c
    c.close()


def _batch(torch, dev, c, frs, accept):
    c.match_set_accept(accept)
    c.match_prerejected(reset=True)
    qd = torch.cat([torch.from_numpy(f.desc) for f in frs]).to(dev)      # (MATCH normalises in place: a fresh copy)
    uv = torch.cat([torch.from_numpy(f.uv) for f in frs]).to(dev)
    c.frame_enqueue_batch(qd.data_ptr(), uv.data_ptr(), Q, len(frs), synth.K_DEFAULT, synth.CAM_IDENTITY, capi.default_frame_params(),
                          [90 + i for i in range(len(frs))])
    out = []
    for f in range(len(frs)):
        objs, counts = c.frame_fetch_slot(f)
        out.append((objs, counts, c.frame_fetch_matches_slot(f), c.frame_debug_fetch_cluster_table_slot(f)[:3]))
    n_pre = c.match_prerejected()
    c.match_set_accept(0.0)
    return out, n_pre


def _alone(torch, dev, c, fr, accept):
    c.match_set_accept(accept)
    c.match_prerejected(reset=True)
    qd, uv = torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev)
    c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), Q, synth.K_DEFAULT, synth.CAM_IDENTITY, capi.default_frame_params(), 7)
    objs, counts = c.frame_fetch()
    out = (objs, counts, c.frame_fetch_matches(), c.frame_debug_fetch_cluster_table_slot(0)[:3])
    n_pre = c.match_prerejected()
    c.match_set_accept(0.0)
    return out, n_pre


def _equal(got, want, tag):
    (o, n, m, t), (a, an, am, at) = got, want
    assert np.array_equal(n, an), ("counts", tag, n, an)
    assert np.array_equal(m[0], am[0]) and np.array_equal(m[1], am[1]), ("match list", tag)
    for x, y in zip(t, at):
        assert np.array_equal(x, y), ("cluster table", tag)
    assert np.array_equal(o["model"], a["model"]), ("models", tag)
    assert np.array_equal(o["pose"].view(np.uint32), a["pose"].view(np.uint32)), ("pose", tag)
    assert np.array_equal(o["score"].view(np.uint32), a["score"].view(np.uint32)), ("score", tag)


def test_batch_of_16_frames(scene):
    torch, dev, db, frs, c = scene
    off, n_off = _batch(torch, dev, c, frs, -1.0)
    on, n_on = _batch(torch, dev, c, frs, 0.0)
    print("batch: pre-rejected", n_on, "of", B * Q, "objects per frame", [len(o[0]) for o in on])
    # switched off, nothing; by default the exit is taken -- by at least half of the queries the ratio test rejects (the
    # host model of tests/accept_model.py proves 0.69 of all queries where 0.12 are accepted, 0.78 of the rejected ones;
    # times the 0.8 the device is held to against the model, rounded down)
    rejected = B * Q - sum(int(o[1][0]) for o in off)
    assert n_off == 0 and n_on >= rejected // 2, (n_on, rejected)
    for f in range(B):
        _equal(on[f], off[f], f)
    assert sum(len(o[0]) for o in on) >= sum(N_VIS) // 2 and sum(len(o[2][0]) for o in on) > 0
    again, _ = _batch(torch, dev, c, frs, -1.0)      # the exact mode after it: slots and counts were left clean
    for f in range(B):
        _equal(again[f], off[f], f)


def test_frame_alone(scene):
    torch, dev, db, frs, c = scene
    assert capi.screen_launch_plan(Q, len(db.desc))["onesweep"] == 0
    off, n_off = _alone(torch, dev, c, frs[2], -1.0)
    on, n_on = _alone(torch, dev, c, frs[2], 0.0)
    print("alone: pre-rejected", n_on, "of", Q, "objects", len(on[0]))
    rejected = Q - int(off[1][0])
    assert n_off == 0 and n_on >= rejected // 2, (n_on, rejected)        # (as in the batch)
    _equal(on, off, "alone")
    assert len(on[0]) >= 1 and len(on[2][0]) > 0


def test_a_ratio_table_keeps_the_exact_triples(scene):
    torch, dev, db, frs, c0 = scene
    from moped_amd import moped3d
    fr = frs[2]
    img, fill = synth.depth_image(db, fr, seed=3)
    t_img, t_fill = torch.from_numpy(img).to(dev), torch.from_numpy(fill).to(dev)
    c = capi.Context(0)
    try:
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        c.reserve(Q)
        c.frame_set_depth_image(t_img.data_ptr(), t_fill.data_ptr(), 640, 480, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        c.frame_set_depth_rules(synth.K_DEFAULT, 64, -1.0, -1.0, moped3d.ratio_table(db.xyz, db.model_of, db.n_models, synth.K_DEFAULT))
        c.match_prerejected(reset=True)
        qd, uv = torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev)
        c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), Q, synth.K_DEFAULT, synth.CAM_IDENTITY, capi.default_frame_params(), 7)
        objs, counts = c.frame_fetch()
        assert c.match_stats()["queries"] >= Q        # the two-stage MATCH ran ...
        assert c.match_prerejected() == 0             # ... and answered every query in full
        assert counts[0] > 0
    finally:
        c.close()
