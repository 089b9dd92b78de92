"""mh_db_splice_view[s] / mh_db_append / mh_db_append_view: Kinect views become and grow models of the resident store.

Store equality is on bytes, over everything a fresh upload defines (the arrays of tests/test_gpu_db_edit.py): after each
edit the store equals a fresh mh_db_upload_raw(normalize = 1) of rows composed in numpy from Context.sift and
tests/view_model_ref.py, spliced by tests/db_edit_ref.py.  The frames are the bundled ones
(tests/golden/sift_ref_frames.npz), the maps the relief and the plane of view_model_ref, the base store the one of
tests/test_gpu_planar_model.py."""
import ctypes as C
import os

import numpy as np
import pytest

import db_edit_ref as dbref
import view_model_ref as ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
INSERT, REPLACE, REMOVE = capi.DB_INSERT, capi.DB_REPLACE, capi.DB_REMOVE
ARRAYS = ("desc", "norm", "xyz", "model", "desc_h", "neg_h")
CAP = 2048
H, W = GOLD["gray0"].shape
EMPTY_BOX = np.array([10E10] * 3 + [-10E10] * 3, np.float32)
POSE = ref.trap_pose()
RULES = dict(roi=(60.0, 40.0, 600.0, 440.0), box=(-0.30, -0.22, -0.06, 0.25, 0.30, 0.08), max_rows=300)
MERGE = dict(merge_ratio=0.8, merge_dist=0.002)


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
    imgs = {"gray0": GOLD["gray0"], "gray3": GOLD["gray3"], "blank": np.full((H, W), 128, np.uint8)}
    maps = {"relief": ref.relief_map(W, H, tuple(K)), "plane": ref.plane_map(0.8, W, H, tuple(K))}
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in imgs.items()}
    m = {k: torch.from_numpy(v).to(dev) for k, v in maps.items()}
    torch.cuda.synchronize()
    a, f = capi.Context(0), capi.Context(0)
    feats = {}
    for k, v in imgs.items():   # FEAT once per image, through the host
        xy, _, d = f.sift(v)
        feats[k] = (xy, d)
        xy.setflags(write=False)
        d.setflags(write=False)
    for v in maps.values():
        v.setflags(write=False)
    yield dict(torch=torch, dev=dev, base=base, g=g, m=m, maps=maps, a=a, f=f, feats=feats)
    a.close()
    f.close()


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


def appended(db, model, desc, xyz):
    """db with rows behind the last row of `model`: REPLACE by the model's rows ++ the new ones."""
    b, n = dbref.model_rows(db, model)
    return dbref.splice(db, REPLACE, model, np.concatenate([db[0][b:b + n], desc]), np.concatenate([db[1][b:b + n], xyz]))


def expected(env, image, map_name, pose, kw, cap=None, **more):
    xy, d = env["feats"][image]
    n = len(xy) if cap is None else min(cap, len(xy))
    return ref.rows(d[:n], xy[:n], n, env["maps"][map_name], None, pose, **kw, **more)


def same_rows(got, want, what=""):
    n, bbox, stats, d, x = got
    wd, wx, wb, ws, _ = want
    assert n == len(wd) and np.array_equal(stats, ws), (what, n, len(wd), stats, ws)
    assert np.array_equal(bits(bbox), bits(wb)), (what, bbox, wb)
    assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(x), bits(wx)), what   # FEAT's bits, X_model's bits


def test_single_edits_equal_a_fresh_upload(env):
    a, f, g, m = env["a"], env["f"], env["g"], env["m"]
    want = expected(env, "gray0", "relief", POSE, RULES)
    ws = want[3]
    assert len(want[0]) == 300 and ws[ref.ROI] > 10 and ws[ref.BOX] > 10 and ws[ref.LIMIT] > 10   # every rule cuts
    spec = capi.make_view_spec(**RULES)
    view = capi.make_view(m["relief"].data_ptr(), None, POSE)
    upload_raw(a, env["base"])
    db = env["base"]
    for step, (op, model) in enumerate([(INSERT, 0), (INSERT, 3), (REPLACE, 1)]):   # front, end, replace
        gen = a.db_generation()
        got = a.db_splice_view(op, model, g["gray0"].data_ptr(), view, W, H, spec, max_keypoints=CAP, want_rows=True)
        assert not a.planar_truncated and a.db_generation() == gen + 1
        same_rows(got, want, step)
        db = dbref.splice(db, op, model, want[0], want[1])
        assert_store_is_fresh_upload(a, f, db, step)
    # without the host copy of the rows: the same store
    n, bbox, stats = a.db_splice_view(REPLACE, 0, g["gray0"].data_ptr(), view, W, H, spec, max_keypoints=CAP)
    assert n == 300 and np.array_equal(bits(bbox), bits(want[2])) and np.array_equal(stats, ws)
    assert_store_is_fresh_upload(a, f, db, "no host rows")


def test_fewer_slots_than_keypoints_is_the_first_of_the_list_and_says_so(env):
    a, f, g, m = env["a"], env["f"], env["g"], env["m"]
    want = expected(env, "gray0", "relief", POSE, {}, cap=256)
    upload_raw(a, env["base"])
    n = C.c_int32(0)
    bbox, stats = np.zeros(6, np.float32), np.zeros(8, np.int32)
    spec = capi.make_view_spec()
    view = capi.make_view(m["relief"].data_ptr(), None, POSE)
    rc = a.L.mh_db_splice_view(a.h, INSERT, 1, g["gray0"].data_ptr(), C.byref(view), W, H, 1, 256, C.byref(spec), C.byref(n),
                               capi._ptr(bbox), capi._ptr(stats), None, None, 0)
    assert rc == -3 and n.value == 256 == len(want[0]) and stats[0] == 256   # MH_ERR_CAPACITY, as mh_sift_extract
    assert np.array_equal(bits(bbox), bits(want[2])) and np.array_equal(stats, want[3])
    assert_store_is_fresh_upload(a, f, dbref.splice(env["base"], INSERT, 1, want[0], want[1]), "capacity")


def test_batch_equals_the_views_one_call_at_a_time(env):
    a, f, g, m = env["a"], env["f"], env["g"], env["m"]
    names = [("gray0", "relief", POSE), ("blank", "plane", None), ("gray3", "plane", None)]
    kw = dict(roi=(20.0, 20.0, 620.0, 460.0))
    spec = capi.make_view_spec(**kw)
    views = [capi.make_view(m[mp].data_ptr(), None, pose) for _, mp, pose in names]
    b = capi.Context(0)
    try:
        upload_raw(a, env["base"])
        upload_raw(b, env["base"])
        n, bbox, stats, d, x = a.db_splice_views(1, [g[k].data_ptr() for k, _, _ in names], views, W, H, spec, max_keypoints=CAP,
                                                 want_rows=True)
        db = env["base"]
        for i, (k, mp, pose) in enumerate(names):
            one = b.db_splice_view(INSERT, 1 + i, g[k].data_ptr(), views[i], W, H, spec, max_keypoints=CAP, want_rows=True)
            same_rows((int(n[i]), bbox[i], stats[i], d[i], x[i]), (one[3], one[4], one[1], one[2], None), ("batch", i))
            want = expected(env, k, mp, pose, kw)
            same_rows(one, want, ("single", i))
            db = dbref.splice(db, INSERT, 1 + i, want[0], want[1])
        assert n[1] == 0 and np.array_equal(bits(bbox[1]), bits(EMPTY_BOX)) and n[0] > 100 and n[2] > 100
        assert a.db_generation() == b.db_generation() == 3
        same_snapshot(snapshot(a), snapshot(b), "batch against single calls")
        assert_store_is_fresh_upload(a, f, db, "batch")
    finally:
        b.close()


def test_db_append_is_the_splice_behind_the_models_last_row(env):
    a, f = env["a"], env["f"]
    torch, dev = env["torch"], env["dev"]
    rng = np.random.default_rng(0xA99)
    nd = np.abs(rng.normal(size=(130, 128))).astype(np.float32)
    nx = rng.uniform(-0.2, 0.2, (130, 3)).astype(np.float32)
    upload_raw(a, env["base"])
    db = env["base"]
    for model, lo, hi in ((0, 0, 70), (1, 70, 130), (0, 0, 0)):   # a model in front, the last model, no rows
        gen = a.db_generation()
        a.db_append(model, nd[lo:hi], nx[lo:hi], normalize=True)
        db = appended(db, model, nd[lo:hi], nx[lo:hi])
        assert a.db_generation() == gen + 1
        assert_store_is_fresh_upload(a, f, db, ("append", model))
    assert a.db_model_rows(0) == (0, 370) and a.db_model_rows(1) == (370, 560)
    # from device rows
    dd, dx = torch.from_numpy(nd).to(dev), torch.from_numpy(nx).to(dev)
    torch.cuda.synchronize()
    a.db_append(1, dd.data_ptr(), dx.data_ptr(), normalize=True, on_device=True, n_rows=130)
    db = appended(db, 1, nd, nx)
    assert_store_is_fresh_upload(a, f, db, "append from the device")
    # refusals leave the store as it was
    before, gen = snapshot(a), a.db_generation()
    for model in (-1, 2):
        assert a.L.mh_db_append(a.h, model, capi._ptr(nd), capi._ptr(nx), 5, 1, 0) == -1
        assert "model index out of range" in a.L.mh_last_error(a.h).decode()
    assert a.L.mh_db_append(a.h, 0, None, capi._ptr(nx), 5, 1, 0) == -1 and a.L.mh_db_append(a.h, 0, capi._ptr(nd), capi._ptr(nx), -1, 1, 0) == -1
    same_snapshot(snapshot(a), before, "refused appends")
    assert a.db_generation() == gen


def teach_frame0(env, c, db, model):
    """Frame 0 on the plane under the identity pose as model `model` (INSERT) of c's store -> the db tuple."""
    want = expected(env, "gray0", "plane", None, {})
    view = capi.make_view(env["m"]["plane"].data_ptr(), None, None)
    got = c.db_splice_view(INSERT, model, env["g"]["gray0"].data_ptr(), view, W, H, capi.make_view_spec(), max_keypoints=CAP,
                           want_rows=True)
    same_rows(got, want, "frame 0")
    return dbref.splice(db, INSERT, model, want[0], want[1])


def match_of(env, c2, db, image):
    """MATCH's answer for the image's FEAT descriptors against db, from a second context's mh_normalize_match."""
    upload_raw(c2, db)
    _, acc, raw, d1, d2 = c2.normalize_match(env["feats"][image][1], 0.8)
    assert np.array_equal(acc >= 0, ref.accepted(raw, d1, d2, 0.8))   # the verdict the selection must reach
    return acc, dict(idx=raw, d1=d1, d2=d2, model_of=db[2], xyz=db[1])


def test_append_view_leaves_out_what_the_model_holds(env):
    a, f, g, m = env["a"], env["f"], env["g"], env["m"]
    c2 = capi.Context(0)
    try:
        upload_raw(a, env["base"])
        db = teach_frame0(env, a, env["base"], 2)
        acc, dup = match_of(env, c2, db, "gray3")
        dup["model"] = 2
        b0, n0 = dbref.model_rows(db, 2)
        want = expected(env, "gray3", "plane", None, MERGE, dup=dup, old_xyz=db[1][b0:b0 + n0])
        # all three classes are live, counted from MATCH's own verdicts, before the device is trusted
        why = ref.verdicts(env["feats"]["gray3"][0], len(acc), env["maps"]["plane"], dup=dup, **MERGE)[0]
        in_model = (acc >= 0) & (db[2][np.maximum(acc, 0)] == 2)
        classes = (int((why == ref.DUP).sum()), int((in_model & (why == ref.KEEP)).sum()), int((acc < 0).sum()))
        print("duplicates, accepted but farther than 2 mm, not accepted:", classes)
        assert min(classes) >= 10
        view = capi.make_view(m["plane"].data_ptr(), None, None)
        spec = capi.make_view_spec(**MERGE)
        launches, gen = sum(a.match_kernel_launches().values()), a.db_generation()
        got = a.db_append_view(2, g["gray3"].data_ptr(), view, W, H, spec, max_keypoints=CAP, want_rows=True)
        same_rows(got, want, "append with the duplicate test")
        assert got[2][ref.DUP] == classes[0] and got[0] == len(acc) - classes[0]
        assert sum(a.match_kernel_launches().values()) == launches + 1 and a.db_generation() == gen + 1
        # the box covers old and new rows
        both = np.concatenate([db[1][b0:b0 + n0], want[1]])
        assert np.array_equal(got[1][:3], both.min(0)) and np.array_equal(got[1][3:], both.max(0))
        db2 = appended(db, 2, want[0], want[1])
        assert_store_is_fresh_upload(a, f, db2, "append view")
        assert a.db_model_rows(2) == (800, n0 + got[0])

        # the duplicate test off: every keypoint is appended, and no MATCH is launched
        for off in (dict(merge_ratio=0.0, merge_dist=0.002), dict(merge_ratio=0.8, merge_dist=-1.0)):
            upload_raw(a, db)
            launches = a.match_kernel_launches()
            want_off = expected(env, "gray3", "plane", None, off, old_xyz=db[1][b0:b0 + n0])
            got = a.db_append_view(2, g["gray3"].data_ptr(), view, W, H, capi.make_view_spec(**off), max_keypoints=CAP, want_rows=True)
            same_rows(got, want_off, ("off", off))
            assert got[0] == len(acc) and got[2][ref.DUP] == 0 and a.match_kernel_launches() == launches
            assert_store_is_fresh_upload(a, f, appended(db, 2, want_off[0], want_off[1]), ("off", off))

        # the model's rows also present as another model in front: every nearest row lies there (the lower row wins a
        # tie), so nothing is dropped
        b, n = dbref.model_rows(db, 2)
        twin = dbref.splice(db, INSERT, 0, db[0][b:b + n], db[1][b:b + n])
        upload_raw(a, twin)
        acc_t, dup_t = match_of(env, c2, twin, "gray3")
        dup_t["model"] = 3
        assert np.all(twin[2][dup_t["idx"]] != 3)
        want_t = expected(env, "gray3", "plane", None, MERGE, dup=dup_t, old_xyz=twin[1][twin[2] == 3])
        got = a.db_append_view(3, g["gray3"].data_ptr(), view, W, H, spec, max_keypoints=CAP, want_rows=True)
        same_rows(got, want_t, "twin")
        assert got[0] == len(acc) and got[2][ref.DUP] == 0
        assert_store_is_fresh_upload(a, f, appended(twin, 3, want_t[0], want_t[1]), "twin")
    finally:
        c2.close()


def test_refusals_leave_the_store_as_it_was(env):
    a, g, m = env["a"], env["g"], env["m"]
    d, x, mo, nm = env["base"]
    dn = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), np.float32)
    ok = capi.make_view_spec()
    okv = capi.make_view(m["relief"].data_ptr(), None, POSE)
    img = g["gray0"].data_ptr()
    nan = float("nan")

    def refused(match, op=INSERT, model=1, image=img, view=okv, spec=ok, cap=CAP, w=W, append=True, batch=True):
        before, gen = snapshot(a), a.db_generation()
        n = C.c_int32(-1)
        vp = C.byref(view) if view is not None else None
        sp = C.byref(spec) if spec is not None else None
        rc = a.L.mh_db_splice_view(a.h, op, model, image, vp, w, H, 1, cap, sp, C.byref(n), None, None, None, None, 0)
        assert rc == -1, (match, rc)
        assert match in a.L.mh_last_error(a.h).decode(), (match, a.L.mh_last_error(a.h))
        if append:
            rc = a.L.mh_db_append_view(a.h, min(model, 1), image, vp, w, H, 1, cap, sp, C.byref(n), None, None, None, None, 0)
            assert rc == -1, ("append", match, rc)
        if batch and op == INSERT and view is not None:
            ptrs = (C.c_void_p * 2)(image, image)
            vs = (capi.mh_view * 2)(view, view)
            rc = a.L.mh_db_splice_views(a.h, model, ptrs, vs, 2, w, H, 1, cap, sp, None, None, None, None, None, 0)
            assert rc == -1, ("batch", match, rc)
        same_snapshot(snapshot(a), before, match)
        assert a.db_generation() == gen

    # stores that are not editable
    a.db_upload_blocks(dn, mo, x, nm, [0, 9000], [300, 500])
    refused("uploaded in blocks")
    a.db_upload(dn, mo, x, nm, index_base=128)
    refused("index_base is not 0")
    upload_raw(a, env["base"])
    refused("INSERT or MH_DB_REPLACE", op=REMOVE, append=False)
    refused("model index out of range", model=3, append=False)
    refused("model index out of range", op=REPLACE, model=2, append=False)
    n = C.c_int32(-1)
    assert a.L.mh_db_append_view(a.h, 2, img, C.byref(okv), W, H, 1, CAP, C.byref(ok), C.byref(n), None, None, None, None, 0) == -1
    refused("bad argument", image=None)
    refused("bad argument", cap=0)
    refused("bad argument", w=0)
    refused("no mh_view_spec", spec=None)
    refused("no mh_view", view=None)
    refused("null depth map", view=capi.make_view(None, None, POSE))
    refused("16-byte aligned", view=capi.make_view(m["relief"].data_ptr() + 4, None, POSE))
    for k in (0, 3, 6):
        pose = np.array(POSE)
        pose[k] = nan if k else float("inf")
        refused("non-finite pose", view=capi.make_view(m["relief"].data_ptr(), None, pose))
    for why, bad in (("NaN in roi", dict(roi=(0.0, 0.0, nan, 1.0))), ("non-finite box", dict(box=(0.0, 0.0, 0.0, 1.0, 1.0, nan))),
                     ("non-finite box", dict(box=(0.0, 0.0, 0.0, float("inf"), 1.0, 1.0))), ("max_rows < 0", dict(max_rows=-1)),
                     ("NaN in max_fill_distance", dict(max_fill_distance=nan)), ("NaN in max_fill_distance", dict(merge_ratio=nan)),
                     ("NaN in max_fill_distance", dict(merge_dist=nan))):
        refused(why, spec=capi.make_view_spec(**bad))
    a.frame_set_undistort((0.1, -0.05, 0.001, 0.001))
    try:
        refused("undistortion is on", view=capi.make_view(m["relief"].data_ptr(), None, POSE, K=(0.0, 800.0, 320.0, 240.0)))
    finally:
        a.frame_set_undistort(None)
    # no kept row: what mh_db_splice does with zero rows -- an empty model at that index, one generation on
    b = capi.Context(0)
    try:
        upload_raw(b, env["base"])
        gen = a.db_generation()
        n, bbox, stats = a.db_splice_view(INSERT, 1, g["blank"].data_ptr(), okv, W, H, ok, max_keypoints=CAP)
        assert n == 0 and np.array_equal(bits(bbox), bits(EMPTY_BOX)) and a.db_generation() == gen + 1 and not stats.any()
        b.db_splice(INSERT, 1, np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32), normalize=True)
        assert a.db_size() == b.db_size() == (800, 3) and a.db_model_rows(1) == b.db_model_rows(1) == (300, 0)
        same_snapshot(snapshot(a), snapshot(b), "zero rows")
    finally:
        b.close()


def test_frames_in_flight_finish_on_the_store_they_were_enqueued_against(env):
    from moped_amd.pipeline import FramePipeline, ShardedDB
    d, x, mo, nm = env["base"]
    pipe = FramePipeline(0, ShardedDB(d.copy(), x.copy(), mo.copy(), nm), depth=2, max_queries=CAP, K=K, cam=CAM0)
    g, m = env["g"], env["m"]
    frame = lambda slot, name: pipe.ctxs[slot].frame_enqueue_image(g[name].data_ptr(), W, H, True, CAP, K, CAM0, pipe.params, seed=5)
    best = lambda objs: objs[np.argmax(objs["score"])]
    try:
        # the left half of frame 0 on the plane is the model
        i, n_half, bbox, stats = pipe.add_kinect_model(g["gray0"], m["plane"], name="m", roi=(0.0, 0.0, 320.0, 480.0), max_keypoints=CAP)
        want = expected(env, "gray0", "plane", None, dict(roi=(0.0, 0.0, 320.0, 480.0)))
        assert i == 2 and n_half == len(want[0]) and np.array_equal(stats, want[3]) and np.array_equal(bits(bbox), bits(want[2]))
        assert [c.db_generation() for c in pipe.ctxs] == [1, 1] and pipe.model_names == [None, None, "m"]
        assert np.array_equal(bits(pipe.db.desc[800:]), bits(want[0])) and np.array_equal(bits(pipe.db.xyz[800:]), bits(want[1]))
        frame(1, "gray0")
        before, before_counts = pipe.fetch(1)
        assert best(before)["model"] == 2
        # a frame on slot 1, then -- no wait in between -- the right half is appended on slot 0
        frame(1, "gray0")
        i, n_more, bbox2, stats2 = pipe.extend_kinect_model(2, g["gray0"], m["plane"], max_keypoints=CAP)
        got, got_counts = pipe.fetch(1)
        assert got.tobytes() == before.tobytes() and np.array_equal(got_counts, before_counts)
        # the view is the one the model came from: its left half is all duplicates, its right half is new
        assert i == 2 and stats2[ref.DUP] > 0.9 * n_half and n_more + stats2[ref.DUP] == stats2[0] and n_more > 50
        assert bbox2[3] > bbox[3] and bbox2[0] == bbox[0]
        assert [c.db_generation() for c in pipe.ctxs] == [2, 2]
        assert pipe.ctxs[1].db_size() == (len(pipe.db.model_of), 3) == (800 + n_half + n_more, 3)
        assert np.all(pipe.db.model_of[800:] == 2)
        # the next frame sees the new rows
        frame(1, "gray0")
        after, after_counts = pipe.fetch(1)
        assert best(after)["model"] == 2 and after_counts[0] > before_counts[0]
        # rows by hand behind model 0; a batch of two more models; the mirror stays in step
        rng = np.random.default_rng(5)
        pipe.append_model_rows(0, np.abs(rng.normal(size=(10, 128))).astype(np.float32), np.zeros((10, 3), np.float32))
        assert pipe.ctxs[1].db_model_rows(0) == (0, 310) and pipe.ctxs[1].db_model_rows(2)[0] == 810
        out = pipe.add_kinect_models([g["gray3"], g["blank"]], [m["relief"], m["plane"]], ["three", "nothing"], poses=[POSE, None],
                                     max_keypoints=CAP)
        assert [o[0] for o in out] == [3, 4] and out[1][1] == 0 and out[0][1] > 100
        assert pipe.model_names == [None, None, "m", "three", "nothing"] and pipe.db.n_models == 5
        c1 = pipe.ctxs[1]
        assert c1.db_size() == (len(pipe.db.model_of), 5)
        assert np.array_equal(c1.db_debug_fetch("model"), pipe.db.model_of)
        assert np.array_equal(bits(c1.db_debug_fetch("xyz")), bits(pipe.db.xyz).reshape(-1))
    finally:
        pipe.close()
