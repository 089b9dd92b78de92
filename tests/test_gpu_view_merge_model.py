"""mh_db_merge_view / mh_db_keep_rows: a further Kinect view merged into a model of the resident store, and the prune.

Store equality is on bytes, as in tests/test_gpu_view_model.py (whose helpers and `env` these are, copied): after each edit
the store equals a fresh mh_db_upload_raw(normalize = 1) of the host mirror of raw rows -- mirror rows merged_idx
overwritten with merged_desc / merged_xyz, the new rows appended.  Expectations come from Context.sift,
Context.normalize_match (the normalised copy and MATCH's answer) and tests/view_merge_ref.py; the old side of every sum
is the descriptor the store holds, fetched from it.  The scene is the one tests/test_view_merge_cpu.py counts: the
800-row base, frame 0 over the relief under the trap pose, frame 3 as the further view."""
import os

import numpy as np
import pytest

import db_edit_ref as dbref
import view_merge_ref as mref
import view_model_ref as ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K = synth.K_DEFAULT
INSERT, REPLACE = capi.DB_INSERT, capi.DB_REPLACE
ARRAYS = ("desc", "norm", "xyz", "model", "desc_h", "neg_h")
CAP = 2048
H, W = GOLD["gray0"].shape
POSE = ref.trap_pose()
MERGE = dict(merge_ratio=0.8, merge_dist=0.002)
EMPTY_BOX = np.array([10E10] * 3 + [-10E10] * 3, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def env():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x91A2)
    # two models nobody sees: raw (unnormalised) rows, as Update() gets them
    desc = np.abs(rng.normal(size=(800, 128))).astype(np.float32)
    xyz = rng.uniform(-0.1, 0.1, (800, 3)).astype(np.float32)
    base = (desc, xyz, np.repeat(np.arange(2, dtype=np.int32), [300, 500]), 2)
    imgs = {"gray0": GOLD["gray0"], "gray3": GOLD["gray3"]}
    relief = ref.relief_map(W, H, tuple(K))
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in imgs.items()}
    m = torch.from_numpy(relief).to(dev)
    torch.cuda.synchronize()
    a, f, b = capi.Context(0), capi.Context(0), capi.Context(0)
    feats = {}
    for k, v in imgs.items():   # FEAT once per image, through the host
        xy, _, d = f.sift(v)
        feats[k] = (xy, d)
        xy.setflags(write=False)
        d.setflags(write=False)
    relief.setflags(write=False)
    yield dict(torch=torch, dev=dev, base=base, g=g, m=m, relief=relief, a=a, f=f, b=b, feats=feats)
    for c in (a, f, b):
        c.close()


def upload_raw(c, db):
    d, x, m = (np.ascontiguousarray(v) for v in db[:3])
    rc = c.L.mh_db_upload_raw(c.h, capi._ptr(d), capi._ptr(m), capi._ptr(x), len(m), db[3], 0, 1)
    assert rc == 0, c.L.mh_last_error(c.h)


def snapshot(c):
    out = {k: c.db_debug_fetch(k) for k in ARRAYS}
    out["screen"] = c.db_debug_screen()
    out["size"] = c.db_size()
    return out


def same_snapshot(got, want, what=""):
    assert got["size"] == want["size"], what
    assert got["screen"] == want["screen"], (what, got["screen"], want["screen"])
    for k in ARRAYS:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)


def assert_store_is_fresh_upload(a, f, db, what=""):
    upload_raw(f, db)
    got = snapshot(a)
    assert got["size"] == (len(db[2]), db[3]), what
    same_snapshot(got, snapshot(f), what)
    assert np.array_equal(got["model"], db[2]), what
    for m in range(db[3]):
        assert a.db_model_rows(m) == dbref.model_rows(db, m), (what, m)


def patched(db, model, idx, desc, xyz, new_desc, new_xyz):
    """The mirror after a merge: rows idx of `model` overwritten, the new rows behind its last row."""
    b, n = dbref.model_rows(db, model)
    d, x = db[0][b:b + n].copy(), db[1][b:b + n].copy()
    d[idx], x[idx] = desc, xyz
    return dbref.splice(db, REPLACE, model, np.concatenate([d, new_desc]), np.concatenate([x, new_xyz]))


def kept(db, model, mask):
    b, n = dbref.model_rows(db, model)
    return dbref.splice(db, REPLACE, model, db[0][b:b + n][mask], db[1][b:b + n][mask])


def expect_merge(env, c2, a, db, model, image, views_in=None, cap=None):
    """What merging `image` into `model` of a's store (mirror db) must give, from a second context's normalize_match
    and the store's own descriptors -> (why, new-row reference, (merged_idx, s, p', views_out))."""
    xy, d = env["feats"][image]
    if cap is not None:
        xy, d = xy[:cap], d[:cap]
    upload_raw(c2, db)
    qn, acc, raw, d1, d2 = c2.normalize_match(d, 0.8)
    b, n = dbref.model_rows(db, model)
    dup = dict(idx=raw, d1=d1, d2=d2, model_of=db[2], xyz=db[1], model=model, row_begin=b, row_end=b + n)
    store_desc = a.db_debug_fetch("desc").reshape(-1, 128)
    why, xyz, merged = mref.merge_view(xy, len(xy), env["relief"], None, POSE, MERGE, dup, qn, store_desc, views_in)
    rows = ref.rows(d, xy, len(xy), env["relief"], None, POSE, dup=dup, old_xyz=db[1][b:b + n], **MERGE)
    return why, rows, merged


def teach_frame0(env, c, db):
    view = capi.make_view(env["m"].data_ptr(), None, POSE)
    n, bbox, stats, d, x = c.db_splice_view(INSERT, 2, env["g"]["gray0"].data_ptr(), view, W, H, capi.make_view_spec(),
                                            max_keypoints=CAP, want_rows=True)
    assert n == 586
    return dbref.splice(db, INSERT, 2, d, x)


def test_merge_then_merge_again_then_prune_equals_a_fresh_upload(env):
    a, f, b, g = env["a"], env["f"], env["b"], env["g"]
    c3 = capi.Context(0)
    try:
        upload_raw(a, env["base"])
        upload_raw(b, env["base"])
        c3.db_share(a)
        db = teach_frame0(env, a, env["base"])
        assert np.array_equal(bits(teach_frame0(env, b, env["base"])[0]), bits(db[0]))
        assert_store_is_fresh_upload(a, f, db, "frame 0")
        view = capi.make_view(env["m"].data_ptr(), None, POSE)
        spec = capi.make_view_spec(**MERGE)

        # ---- frame 3 merged ----
        why, want_rows, (widx, ws, wp, wviews) = expect_merge(env, f, a, db, 2, "gray3")
        assert len(widx) >= 300 and (why == ref.KEEP).sum() >= 100   # the scene's conditions (tests/test_view_merge_cpu.py)
        launches, gen = sum(a.match_kernel_launches().values()), a.db_generation()
        n, m, bbox, stats, views, midx, md, mx, nd, nx = a.db_merge_view(2, g["gray3"].data_ptr(), view, W, H, spec, max_keypoints=CAP)
        assert not a.planar_truncated and a.db_generation() == gen + 1
        assert sum(a.match_kernel_launches().values()) == launches + 1
        print("merged rows", m, "duplicates", int(stats[ref.DUP]), "new rows", n)
        assert m == len(widx) and np.array_equal(midx, widx)
        assert np.array_equal(bits(md), bits(ws)) and np.array_equal(bits(mx), bits(wp))
        assert np.array_equal(views, np.concatenate([wviews, np.ones(n, np.int32)]))
        # the new rows and the statistics: the reference's, and mh_db_append_view's on a second context from the same start
        assert n == len(want_rows[0]) and np.array_equal(stats, want_rows[3])
        assert np.array_equal(bits(nd), bits(want_rows[0])) and np.array_equal(bits(nx), bits(want_rows[1]))
        n_b, bbox_b, stats_b, d_b, x_b = b.db_append_view(2, g["gray3"].data_ptr(), view, W, H, spec, max_keypoints=CAP, want_rows=True)
        assert n_b == n and np.array_equal(stats_b, stats) and np.array_equal(bits(d_b), bits(nd)) and np.array_equal(bits(x_b), bits(nx))
        db1 = patched(db, 2, midx, md, mx, nd, nx)
        assert_store_is_fresh_upload(a, f, db1, "frame 3 merged")
        # the box is over the final points
        mine = db1[1][db1[2] == 2]
        assert np.array_equal(bits(bbox), bits(np.concatenate([mine.min(0), mine.max(0)])))
        # untouched rows kept their bits (the fresh upload says so too): the appended store has the same rows there
        untouched = np.setdiff1d(np.arange(586), midx)
        assert np.array_equal(bits(a.db_debug_fetch("desc").reshape(-1, 128)[800 + untouched]),
                              bits(b.db_debug_fetch("desc").reshape(-1, 128)[800 + untouched]))
        # the other context adopts
        assert c3.db_generation() == gen - 1
        c3.db_adopt(a)
        assert c3.db_generation() == gen + 1 and c3.db_size() == a.db_size()
        same_snapshot(snapshot(c3), snapshot(a), "adopted")

        # ---- the same view again: counts 3 where they were 2; the old side is the store's renormalised row ----
        why2, want_rows2, (widx2, ws2, wp2, wviews2) = expect_merge(env, f, a, db1, 2, "gray3", views_in=views)
        gen = a.db_generation()
        n2, m2, bbox2, stats2, views2, midx2, md2, mx2, nd2, nx2 = a.db_merge_view(2, g["gray3"].data_ptr(), view, W, H, spec,
                                                                                   max_keypoints=CAP, views_in=views)
        assert a.db_generation() == gen + 1
        assert m2 == len(widx2) and np.array_equal(midx2, widx2) and n2 == len(want_rows2[0])
        assert np.array_equal(bits(md2), bits(ws2)) and np.array_equal(bits(mx2), bits(wp2))
        assert np.array_equal(views2, np.concatenate([wviews2, np.ones(n2, np.int32)]))
        both = np.intersect1d(midx, midx2)
        assert len(both) >= 300 and np.all(views2[both] == 3) and np.all(views[both] == 2)
        assert len(np.setdiff1d(midx2, midx)) >= 100 and np.all(views2[np.setdiff1d(midx2, midx)] == 2)   # the first merge's new rows
        db2 = patched(db1, 2, midx2, md2, mx2, nd2, nx2)
        assert_store_is_fresh_upload(a, f, db2, "frame 3 merged twice")

        # ---- the prune ----
        for what, mask in (("views >= 2", views2 >= 2), ("all", np.ones(len(views2), bool)), ("none", np.zeros(len(views2), bool))):
            upload_raw(a, db2)
            gen = a.db_generation()
            nk, bk = a.db_keep_rows(2, mask)
            assert nk == int(mask.sum()) and a.db_generation() == gen + 1
            dbk = kept(db2, 2, mask)
            assert_store_is_fresh_upload(a, f, dbk, what)
            mine = dbk[1][dbk[2] == 2]
            assert np.array_equal(bits(bk), bits(np.concatenate([mine.min(0), mine.max(0)]) if len(mine) else EMPTY_BOX)), what
        assert a.db_model_rows(2) == (800, 0) and a.db_size() == (800, 3)
        assert 300 <= int((views2 >= 2).sum()) < len(views2)
    finally:
        c3.close()


def test_fewer_slots_than_keypoints_merges_the_first_of_the_list_and_says_so(env):
    import ctypes as C
    a, f, g = env["a"], env["f"], env["g"]
    upload_raw(a, env["base"])
    db = teach_frame0(env, a, env["base"])
    why, want_rows, (widx, ws, wp, wviews) = expect_merge(env, f, a, db, 2, "gray3", cap=256)
    assert len(widx) > 100 and len(want_rows[0]) > 30
    view = capi.make_view(env["m"].data_ptr(), None, POSE)
    spec = capi.make_view_spec(**MERGE)
    na, nm = C.c_int32(0), C.c_int32(0)
    stats = np.zeros(8, np.int32)
    nd, nx = np.zeros((256, 128), np.float32), np.zeros((256, 3), np.float32)
    mi, md, mx = np.zeros(256, np.int32), np.zeros((256, 128), np.float32), np.zeros((256, 3), np.float32)
    vout = np.zeros(586 + 256, np.int32)
    rc = a.L.mh_db_merge_view(a.h, 2, g["gray3"].data_ptr(), C.byref(view), W, H, 1, 256, C.byref(spec), None, 0, C.byref(na),
                              C.byref(nm), None, capi._ptr(stats), capi._ptr(nd), capi._ptr(nx), 256, capi._ptr(mi), capi._ptr(md),
                              capi._ptr(mx), 256, capi._ptr(vout), len(vout))
    assert rc == -3 and "max_keypoints" in a.L.mh_last_error(a.h).decode()   # MH_ERR_CAPACITY: the edit is made
    n, m = na.value, nm.value
    assert stats[0] == 256 and m == len(widx) and n == len(want_rows[0]) and np.array_equal(stats, want_rows[3])
    assert np.array_equal(mi[:m], widx) and np.array_equal(bits(md[:m]), bits(ws)) and np.array_equal(bits(mx[:m]), bits(wp))
    assert np.array_equal(vout[:586 + n], np.concatenate([wviews, np.ones(n, np.int32)]))
    assert_store_is_fresh_upload(a, f, patched(db, 2, mi[:m], md[:m], mx[:m], nd[:n], nx[:n]), "capacity")


def test_the_duplicate_test_off_is_append_view(env):
    a, f, b, g = env["a"], env["f"], env["b"], env["g"]
    view = capi.make_view(env["m"].data_ptr(), None, POSE)
    views_in = (np.arange(586) % 3 + 1).astype(np.int32)
    for off in (dict(merge_ratio=0.0, merge_dist=0.002), dict(merge_ratio=0.8, merge_dist=-1.0)):
        upload_raw(a, env["base"])
        upload_raw(b, env["base"])
        db = teach_frame0(env, a, env["base"])
        teach_frame0(env, b, env["base"])
        spec = capi.make_view_spec(**off)
        launches, gen = a.match_kernel_launches(), a.db_generation()
        n, m, bbox, stats, views, midx, md, mx, nd, nx = a.db_merge_view(2, g["gray3"].data_ptr(), view, W, H, spec,
                                                                         max_keypoints=CAP, views_in=views_in)
        assert a.match_kernel_launches() == launches and a.db_generation() == gen + 1
        n_b, bbox_b, stats_b, d_b, x_b = b.db_append_view(2, g["gray3"].data_ptr(), view, W, H, spec, max_keypoints=CAP, want_rows=True)
        assert m == 0 and len(midx) == 0 and n == n_b == 599 and np.array_equal(stats, stats_b) and np.array_equal(bits(bbox), bits(bbox_b))
        assert np.array_equal(bits(nd), bits(d_b)) and np.array_equal(bits(nx), bits(x_b))
        assert np.array_equal(views, np.concatenate([views_in, np.ones(n, np.int32)]))
        same_snapshot(snapshot(a), snapshot(b), off)
        assert_store_is_fresh_upload(a, f, patched(db, 2, [], np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32), nd, nx), off)


def test_refusals_leave_the_store_as_it_was(env):
    import ctypes as C
    a, g = env["a"], env["g"]
    upload_raw(a, env["base"])
    teach_frame0(env, a, env["base"])
    before, gen = snapshot(a), a.db_generation()
    view = capi.make_view(env["m"].data_ptr(), None, POSE)
    spec = capi.make_view_spec(**MERGE)
    na, nm = C.c_int32(-5), C.c_int32(-5)
    vout = np.full(586 + CAP, -9, np.int32)

    def call(model=2, vin=None, n_vin=0, vcap=586 + CAP, mi=None, mdp=None, mxp=None, mcap=0, image=g["gray3"].data_ptr()):
        return a.L.mh_db_merge_view(a.h, model, image, C.byref(view), W, H, 1, CAP, C.byref(spec), capi._ptr(vin), n_vin,
                                    C.byref(na), C.byref(nm), None, None, None, None, 0, capi._ptr(mi), capi._ptr(mdp),
                                    capi._ptr(mxp), mcap, capi._ptr(vout), vcap)

    ones = np.ones(586, np.int32)
    bad = ones.copy()
    bad[585] = 0
    assert call(model=3) == -1 and "model index out of range" in a.L.mh_last_error(a.h).decode()
    assert call(vin=ones, n_vin=585) == -1 and "row count" in a.L.mh_last_error(a.h).decode()
    assert call(vin=bad, n_vin=586) == -1 and "count < 1" in a.L.mh_last_error(a.h).decode()
    assert call(vin=None, n_vin=586) == -1
    assert call(vcap=586 + CAP - 1) == -1 and "views_out_cap" in a.L.mh_last_error(a.h).decode()
    assert call(mi=np.zeros(4, np.int32), mcap=4) == -1   # the merged rows' arrays come together
    assert call(mcap=-1) == -1
    assert call(image=None) == -1
    keep = np.ones(586, np.uint8)
    nr = C.c_int32(-5)
    assert a.L.mh_db_keep_rows(a.h, 2, capi._ptr(keep), 585, C.byref(nr), None) == -1
    assert "n_flags" in a.L.mh_last_error(a.h).decode()
    assert a.L.mh_db_keep_rows(a.h, 3, capi._ptr(keep), 586, C.byref(nr), None) == -1
    assert a.L.mh_db_keep_rows(a.h, 2, None, 586, C.byref(nr), None) == -1
    same_snapshot(snapshot(a), before, "refused")
    assert a.db_generation() == gen and np.all(vout == -9)
    # a sharded store is refused, like every edit
    d, x, mo, n_models = env["base"]
    dn = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), np.float32)
    a.db_upload(dn, mo, x, n_models, index_base=128)
    assert call(model=1) == -1 and "index_base is not 0" in a.L.mh_last_error(a.h).decode()
    assert a.L.mh_db_keep_rows(a.h, 1, capi._ptr(np.ones(500, np.uint8)), 500, C.byref(nr), None) == -1
