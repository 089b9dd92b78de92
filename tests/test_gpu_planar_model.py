"""mh_db_splice_image[s] / FramePipeline.add_planar_model: a device image becomes a model of the resident store
(Moped::createPlanarModelsFromImages, moped2/libmoped/src/moped.cpp:196-236).

Store equality is on bytes, over everything a fresh upload defines (the arrays of tests/test_gpu_db_edit.py): after each
edit the store equals a fresh mh_db_upload_raw(normalize = 1) of rows composed in numpy from Context.sift and
tests/planar_ref.py, spliced by tests/db_edit_ref.py.  The frames are the bundled ones (tests/golden/sift_ref_frames.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import db_edit_ref as dbref
import planar_ref as ref
import undistort_ref as ur
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
LAUNCH_K, LAUNCH_D = ur.cameras()["launch"]
INSERT, REPLACE, REMOVE = capi.DB_INSERT, capi.DB_REPLACE, capi.DB_REMOVE
ARRAYS = ("desc", "norm", "xyz", "model", "desc_h", "neg_h")
CAP = 2048
H, W = GOLD["gray0"].shape
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
    imgs = {"gray0": GOLD["gray0"], "gray3": GOLD["gray3"], "blank": np.full((H, W), 128, np.uint8)}
    g = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in imgs.items()}
    torch.cuda.synchronize()
    a, f = capi.Context(0), capi.Context(0)
    feats = {}
    for k, v in imgs.items():   # FEAT once per image, through the host
        xy, _, d = f.sift(v)
        feats[k] = (xy, d)
    und = f.undistort(imgs["gray0"], LAUNCH_K, LAUNCH_D)
    xy, _, d = f.sift(und)
    feats["gray0-undistorted"] = (xy, d)
    for v in feats.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    yield dict(torch=torch, dev=dev, base=base, g=g, a=a, f=f, feats=feats)
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


def expected_rows(feats, kw):
    xy, d = feats
    form = 0 if kw.get("z") is None else 1
    wd, wx, wb, _ = ref.rows(d, xy, len(xy), form, kw.get("scale") or 1.0, kw.get("K") or (1, 1, 0, 0), kw.get("z") or 0.0,
                             kw.get("roi"), kw.get("max_rows", 0))
    return wd, wx, wb


VARIANTS = {
    "form1": (dict(z=0.8, K=tuple(K)), None),
    "form0-roi-max_rows": (dict(scale=0.001, roi=(100.0, 50.0, 500.0, 400.0), max_rows=200), None),
    "undistort": (dict(z=0.8, K=tuple(LAUNCH_K)), LAUNCH_D),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_single_edits_equal_a_fresh_upload(env, variant):
    a, f, g = env["a"], env["f"], env["g"]
    kw, dist = VARIANTS[variant]
    wd, wx, wb = expected_rows(env["feats"]["gray0-undistorted" if dist is not None else "gray0"], kw)
    assert len(wd) > 100 and (variant != "form0-roi-max_rows" or len(wd) == 200)
    spec = capi.make_planar_spec(**kw)
    upload_raw(a, env["base"])
    db = env["base"]
    a.frame_set_undistort(dist)
    try:
        for step, (op, model) in enumerate([(INSERT, 2), (INSERT, 0), (REPLACE, 1)]):
            gen = a.db_generation()
            n, bbox, d, x = a.db_splice_image(op, model, g["gray0"].data_ptr(), W, H, spec, max_keypoints=CAP, want_rows=True)
            assert not a.planar_truncated and a.db_generation() == gen + 1
            assert n == len(wd) and np.array_equal(bits(bbox), bits(wb))
            assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(x), bits(wx))   # the selected rows, FEAT's bits
            db = dbref.splice(db, op, model, wd, wx)
            assert_store_is_fresh_upload(a, f, db, (variant, step))
        # without the host copy of the rows: the same store
        n, bbox = a.db_splice_image(REPLACE, 0, g["gray0"].data_ptr(), W, H, spec, max_keypoints=CAP)
        assert n == len(wd) and np.array_equal(bits(bbox), bits(wb))
        assert_store_is_fresh_upload(a, f, db, (variant, "no host rows"))
    finally:
        a.frame_set_undistort(None)


def test_fewer_slots_than_keypoints_is_the_first_of_the_list_and_says_so(env):
    a, f, g = env["a"], env["f"], env["g"]
    xy, d = env["feats"]["gray0"]
    kw = dict(z=0.8, K=tuple(K))
    wd, wx, wb, _ = ref.rows(d[:256], xy[:256], 256, 1, K=tuple(K), z=0.8)
    upload_raw(a, env["base"])
    n = C.c_int32(0)
    bbox = np.zeros(6, np.float32)
    spec = capi.make_planar_spec(**kw)
    rc = a.L.mh_db_splice_image(a.h, INSERT, 1, g["gray0"].data_ptr(), W, H, 1, 256, C.byref(spec), C.byref(n), capi._ptr(bbox),
                                None, None, 0)
    assert rc == -3 and n.value == 256 and np.array_equal(bits(bbox), bits(wb))   # MH_ERR_CAPACITY, as mh_sift_extract
    assert_store_is_fresh_upload(a, f, dbref.splice(env["base"], INSERT, 1, wd, wx), "capacity")


def test_batch_equals_the_images_one_call_at_a_time(env):
    a, f, g = env["a"], env["f"], env["g"]
    names = ["gray0", "blank", "gray3"]
    kw = dict(z=0.8, K=tuple(K), roi=(20.0, 20.0, 620.0, 460.0))
    spec = capi.make_planar_spec(**kw)
    b = capi.Context(0)
    try:
        upload_raw(a, env["base"])
        upload_raw(b, env["base"])
        n, bbox, d, x = a.db_splice_images(1, [g[k].data_ptr() for k in names], W, H, spec, max_keypoints=CAP, want_rows=True)
        db = env["base"]
        for i, k in enumerate(names):
            n1, bbox1, d1, x1 = b.db_splice_image(INSERT, 1 + i, g[k].data_ptr(), W, H, spec, max_keypoints=CAP, want_rows=True)
            assert n[i] == n1 and np.array_equal(bits(bbox[i]), bits(bbox1))
            assert np.array_equal(bits(d[i]), bits(d1)) and np.array_equal(bits(x[i]), bits(x1))
            wd, wx, wb = expected_rows(env["feats"][k], kw)
            assert n1 == len(wd) and np.array_equal(bits(d1), bits(wd)) and np.array_equal(bits(x1), bits(wx))
            assert np.array_equal(bits(bbox1), bits(wb))
            db = dbref.splice(db, INSERT, 1 + i, wd, wx)
        assert n[1] == 0 and np.array_equal(bits(bbox[1]), bits(EMPTY_BOX)) and n[0] > 100 and n[2] > 100
        assert a.db_generation() == b.db_generation() == 3
        same_snapshot(snapshot(a), snapshot(b), "batch against single calls")
        assert_store_is_fresh_upload(a, f, db, "batch")
    finally:
        b.close()


def best(objs):
    assert len(objs) >= 1
    return objs[np.argmax(objs["score"])]


def make_pipe(env, depth=2):
    from moped_amd.pipeline import FramePipeline, ShardedDB
    d, x, m, nm = env["base"]
    return FramePipeline(0, ShardedDB(d.copy(), x.copy(), m.copy(), nm), depth=depth, max_queries=CAP, K=K, cam=CAM0)


def frame(pipe, env, slot, name, seed=5):
    pipe.ctxs[slot].frame_enqueue_image(env["g"][name].data_ptr(), W, H, True, CAP, K, CAM0, pipe.params, seed=seed)


def test_taught_model_is_found_in_every_frame_form1(env):
    pipe = make_pipe(env)
    try:
        i, n, bbox = pipe.add_planar_model(env["g"]["gray0"], name="frame 0", z=0.8, max_keypoints=CAP)
        wd, wx, wb = expected_rows(env["feats"]["gray0"], dict(z=0.8, K=tuple(K)))
        assert i == 2 and n == len(wd) and np.array_equal(bits(bbox), bits(wb))
        assert pipe.db.n_models == 3 and pipe.model_names == [None, None, "frame 0"]
        assert np.array_equal(bits(pipe.db.desc[800:]), bits(wd)) and np.array_equal(bits(pipe.db.xyz[800:]), bits(wx))
        for slot, name in enumerate(("gray0", "gray3")):
            frame(pipe, env, slot, name)
        for slot in range(2):
            objs, counts = pipe.fetch(slot)
            o = best(objs)
            assert o["model"] == 2 and counts[0] > 50
            # the pose bounds of tests/test_gpu_image_frame.py: model frame = camera frame of frame 0
            assert np.abs(o["pose"][4:7]).max() < 0.05 and abs(abs(o["pose"][3]) - 1) < 0.01
    finally:
        pipe.close()


def test_taught_model_is_found_form0(env):
    """The reference's form: model point (u s, v s, 0).  With s = 0.8 / fx and fx = fy the point the camera of frame 0
    sees at pixel (u, v) on the plane z = 0.8 is ((u - cx) / fx 0.8, (v - cy) / fy 0.8, 0.8) = (u s, v s, 0) + t with
    t = (-cx s, -cy s, 0.8): the two parametrisations of the plane differ by that translation and no rotation, so the
    object's pose (model frame -> world = camera frame) is (identity, t)."""
    assert K[0] == K[1]
    s = np.float32(0.8) / np.float32(K[0])
    t = np.array([-K[2] * s, -K[3] * s, 0.8], np.float64)
    pipe = make_pipe(env, depth=1)
    try:
        i, n, bbox = pipe.add_planar_model(env["g"]["gray0"], scale=float(s), max_keypoints=CAP)
        wd, wx, wb = expected_rows(env["feats"]["gray0"], dict(scale=float(s)))
        assert i == 2 and n == len(wd) and np.array_equal(bits(bbox), bits(wb)) and bbox[2] == 0 and bbox[5] == 0
        frame(pipe, env, 0, "gray0")
        objs, counts = pipe.fetch(0)
        o = best(objs)
        assert o["model"] == 2 and counts[0] > 50
        assert np.abs(o["pose"][4:7] - t).max() < 0.05 and abs(abs(o["pose"][3]) - 1) < 0.01
        # fewer slots than the image has keypoints: the model is the first of the list, and the caller is told
        with pytest.warns(RuntimeWarning, match="more keypoints than max_keypoints=256"):
            i, n, _ = pipe.add_planar_model(env["g"]["gray0"], name="first 256", scale=float(s), max_keypoints=256)
        assert (i, n) == (3, 256) and np.array_equal(bits(pipe.db.desc[-256:]), bits(wd[:256]))
    finally:
        pipe.close()


def test_frames_in_flight_finish_on_the_store_they_were_enqueued_against(env):
    pipe = make_pipe(env)
    g0 = env["g"]["gray0"]
    try:
        # the left half of frame 0 is the model
        i, n_half, _ = pipe.add_planar_model(g0, name="m", z=0.8, roi=(0.0, 0.0, 320.0, 480.0), max_keypoints=CAP)
        assert i == 2 and [c.db_generation() for c in pipe.ctxs] == [1, 1]
        frame(pipe, env, 1, "gray0")
        want, want_counts = pipe.fetch(1)
        assert best(want)["model"] == 2
        # a frame on slot 1, then -- no wait in between -- the whole image replaces the model on slot 0
        frame(pipe, env, 1, "gray0")
        i, n_full, _ = pipe.add_planar_model(g0, name="m", z=0.8, max_keypoints=CAP)
        got, got_counts = pipe.fetch(1)
        assert i == 2 and n_full > n_half > 50
        assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts)
        assert [c.db_generation() for c in pipe.ctxs] == [2, 2]
        # the next frame sees the new rows
        frame(pipe, env, 1, "gray0")
        after, after_counts = pipe.fetch(1)
        assert best(after)["model"] == 2 and after_counts[0] > want_counts[0]
        # two more models in one call: one generation per taught model
        out = pipe.add_planar_models([env["g"]["gray3"], env["g"]["blank"]], ["three", "nothing"], z=0.8, max_keypoints=CAP)
        assert [o[0] for o in out] == [3, 4] and out[1][1] == 0 and out[0][1] > 100
        assert [c.db_generation() for c in pipe.ctxs] == [4, 4] and pipe.db.n_models == 5
        assert pipe.model_names == [None, None, "m", "three", "nothing"]
        assert pipe.ctxs[1].db_size() == (len(pipe.db.model_of), 5)
        with pytest.raises(ValueError):
            pipe.add_planar_model(g0, name="x", max_keypoints=CAP)                 # neither scale nor z
        with pytest.raises(ValueError):
            pipe.add_planar_model(g0, name="x", scale=1.0, z=1.0, max_keypoints=CAP)   # both
    finally:
        pipe.close()


def test_refusals_leave_the_store_as_it_was_and_zero_rows_is_an_empty_model(env):
    a, f, g = env["a"], env["f"], env["g"]
    d, x, m, nm = env["base"]
    dn = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), np.float32)
    ok = capi.make_planar_spec(z=0.8, K=tuple(K))
    img = g["gray0"].data_ptr()

    def refused(match, op=INSERT, model=1, image=img, spec=ok, cap=CAP, w=W):
        before, gen = snapshot(a), a.db_generation()
        n = C.c_int32(-1)
        rc = a.L.mh_db_splice_image(a.h, op, model, image, w, H, 1, cap, C.byref(spec) if spec is not None else None,
                                    C.byref(n), None, None, None, 0)
        assert rc == -1, (match, rc)
        assert match in a.L.mh_last_error(a.h).decode(), (match, a.L.mh_last_error(a.h))
        same_snapshot(snapshot(a), before, match)
        assert a.db_generation() == gen
        if op == INSERT:   # the batch form refuses the same
            ptrs = (C.c_void_p * 2)(image, image)
            rc = a.L.mh_db_splice_images(a.h, model, ptrs, 2, w, H, 1, cap, C.byref(spec) if spec is not None else None,
                                         None, None, None, None, 0)
            assert rc == -1, ("batch", match, rc)
            same_snapshot(snapshot(a), before, match)
            assert a.db_generation() == gen

    # stores that are not editable
    a.db_upload_blocks(dn, m, x, nm, [0, 9000], [300, 500])
    refused("uploaded in blocks")
    a.db_upload(dn, m, x, nm, index_base=128)
    refused("index_base is not 0")
    upload_raw(a, env["base"])
    refused("INSERT or MH_DB_REPLACE", op=REMOVE)
    refused("model index out of range", model=3)
    refused("model index out of range", op=REPLACE, model=2)
    refused("bad argument", image=None)
    refused("bad argument", cap=0)
    refused("bad argument", w=0)
    refused("no mh_planar_spec", spec=None)
    for why, bad in (("form is 0", dict(form=2)), ("form is 0", dict(form=-1)), ("non-finite", dict(scale=float("inf"))),
                     ("non-finite", dict(z=float("nan"))), ("max_rows < 0", dict(max_rows=-1))):
        sp = capi.make_planar_spec(z=0.8, K=tuple(K))
        for k, v in bad.items():
            setattr(sp, k, v)
        refused(why, spec=sp)
    refused("non-finite", spec=capi.make_planar_spec(z=0.8, K=(800.0, float("inf"), 320.0, 240.0)))
    refused("fx or fy is 0", spec=capi.make_planar_spec(z=0.8, K=(800.0, 0.0, 320.0, 240.0)))
    refused("NaN in roi", spec=capi.make_planar_spec(z=0.8, K=tuple(K), roi=(0.0, 0.0, float("nan"), 1.0)))
    a.frame_set_undistort(LAUNCH_D)
    try:
        refused("undistortion is on", spec=capi.make_planar_spec(scale=0.001, K=(0.0, 800.0, 320.0, 240.0)))
    finally:
        a.frame_set_undistort(None)
    # no kept row: what mh_db_splice does with zero rows -- an empty model at that index, one generation on
    b = capi.Context(0)
    try:
        upload_raw(b, env["base"])
        gen = a.db_generation()
        n, bbox = a.db_splice_image(INSERT, 1, g["blank"].data_ptr(), W, H, ok, max_keypoints=CAP)
        assert n == 0 and np.array_equal(bits(bbox), bits(EMPTY_BOX)) and a.db_generation() == gen + 1
        b.db_splice(INSERT, 1, np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32), normalize=True)
        assert a.db_size() == b.db_size() == (800, 3) and a.db_model_rows(1) == b.db_model_rows(1) == (300, 0)
        same_snapshot(snapshot(a), snapshot(b), "zero rows")
        # ... and an image whose keypoints all lie outside the region of interest
        n, bbox = a.db_splice_image(REPLACE, 0, g["gray0"].data_ptr(), W, H,
                                    capi.make_planar_spec(z=0.8, K=tuple(K), roi=(-9.0, -9.0, -1.0, -1.0)), max_keypoints=CAP)
        b.db_splice(REPLACE, 0, np.zeros((0, 128), np.float32), np.zeros((0, 3), np.float32), normalize=True)
        assert n == 0 and a.db_model_rows(0) == (0, 0)
        same_snapshot(snapshot(a), snapshot(b), "zero rows, replace")
    finally:
        b.close()
