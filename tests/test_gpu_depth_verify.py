"""mh_depth_verify (csrc/depth_verify.hip) against the restatement of moped3d's DEPTH_VERIFY_CPU::process
(tests/depth_verify_ref.py, itself held to the recorded class by test_depth_verify_ref_cpu.py): all nine words of every
object's record as uint32, over generated cases (a 40 x 30 map with measured, filled, NaN and far pixels, a depth camera
that is not the identity, poses on, in front of and behind the surface, off the map, behind the camera, NaN), models of
0 .. 1 025 rows around the kernel's chunk, match lists of 0 .. 300, object counts up to one past the grid stride; both
device forms; the recorded cases through the device; thresholds placed exactly on produced values; calls on one context
that must not see each other; the refusals.

A NaN has no defined bit pattern across the two machines: NaN words are compared as "NaN on both sides", everything else
at the bits."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_verify_ref as dvr
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
CHUNK = capi.DEPTH_VERIFY_CHUNK
GRID = 128                                   # DV_GRID: the grid stride over the objects
SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 1025, 2 * CHUNK + 7]
MATCH_SIZES = [0, 1, 64, 65, 300, CHUNK, CHUNK + 1, 63, 130, 2]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_verify_ref.npz")


def _bits(a):
    a = np.array(a, f32)
    a[np.isnan(a)] = np.nan                  # one pattern for every NaN
    return a.view(np.uint32)


def same(got, want, tag=None):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k in dvr.WORDS:
        g, w = (got[k], want[k]) if got[k].dtype.kind == "i" else (_bits(got[k]), _bits(want[k]))
        bad = np.nonzero(g != w)[0]
        assert not len(bad), (tag, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def upload(ctx, kp_xyz, kp_off, seed=7):
    rng = np.random.default_rng(seed)
    n = np.diff(kp_off)
    model_of = np.repeat(np.arange(len(n), dtype=np.int32), n)
    desc = synth.l2_normalize(rng.normal(size=(len(kp_xyz), 128)).astype(f32))
    ctx.db_upload(desc, model_of, kp_xyz, len(n))


def device(ctx, c, **over):
    a = dict(c, **over)
    ctx.frame_set_depth_image_host(a["depth_img"], a["fill_img"])
    return ctx.depth_verify(capi.pack_corr(a["uv"], a["xyz"]), a["model_off"], a["obj_model"], a["obj_pose"], a["K"], a["cam"],
                            a["depth_K"], a["depth_cam"], a["params"])


@pytest.fixture(scope="module")
def models():
    return dvr.make_models(np.random.default_rng(0xD0), SIZES)


@pytest.fixture(scope="module")
def vctx(models):
    """A context of this module's own with the models resident."""
    c = capi.Context(0)
    upload(c, *models)
    yield c
    c.close()


def _cases(models, n, seed):
    """n cases over the module's models: every model size and match count comes round, the object counts 1, 65 and one
    past the grid stride among them, a map without distances in one case of eight"""
    rng = np.random.default_rng(seed)
    kp, kp_off = models
    out = []
    for i in range(n):
        n_obj = {0: 65, 1: GRID + 1, 2: 1}.get(i, None)
        ms = np.roll(MATCH_SIZES, i)
        if n_obj is None:
            obj_model = np.roll(np.arange(len(SIZES)), i)[:int(rng.integers(2, 8))]
        else:
            obj_model = np.arange(n_obj) % len(SIZES)
        c = dvr.make_verify_case(rng, kp, kp_off, match_sizes=ms, obj_model=obj_model)
        if i % 8 == 5:
            c["fill_img"] = None
        if i % 4 == 3:                        # NaN in a pose: every coordinate NaN, off the map by the rule
            c["obj_pose"][0, int(rng.integers(0, 7))] = np.nan
        if i % 4 == 1:
            dvr.plant_equal_depth(c, 0)
        out.append(c)
    return out


@pytest.fixture(scope="module")
def cases(models):
    cs = _cases(models, 24, 0xD1)
    return cs, [dvr.run_ref(c) for c in cs]


@pytest.mark.parametrize("form", [0, 1])
def test_depth_verify_equals_the_restatement(vctx, cases, form):
    cs, want = cases
    vctx.depth_verify_debug_form(form)
    try:
        got = [device(vctx, c) for c in cs]
    finally:
        vctx.depth_verify_debug_form(0)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, (form, i))
    w = np.concatenate(want)
    # what the cases reach: both verdicts, off-map keypoints (used + skipped < keypoints is not it: count directly)
    assert (w["keep"] == 1).sum() > 30 and (w["keep"] == 0).sum() > 30, np.bincount(w["keep"])
    assert set(SIZES) <= set(w["keypoints"].tolist())
    assert np.isnan(w["is_raw"]).any() and np.isnan(w["multiplier"]).any() and (w["used"] == 0).any() and (w["plausible"] == 0).any()
    assert {len(x) for x in want} >= {1, 65, GRID + 1}


def test_cases_reach_off_map_and_behind_camera_points(cases):
    cs, _ = cases
    off = behind = nan = 0
    for c in cs:
        detail = []
        dvr.run_ref(c, detail=detail)
        for out, _, _, pix, _, putative in detail:
            off += int((pix[:, 0] < 0).sum())
            behind += int(((pix[:, 0] >= 0) & (putative < 0)).sum())
            nan += int(np.isnan(putative).sum())
    assert off > 1000 and behind > 100 and nan > 100, (off, behind, nan)


def test_both_forms_equal_each_other(vctx, models):
    for i, c in enumerate(_cases(models, 6, 0xD2)):
        vctx.depth_verify_debug_form(1)
        try:
            wave = device(vctx, c).copy()
        finally:
            vctx.depth_verify_debug_form(0)
        same(device(vctx, c), wave, i)


def test_no_objects(vctx, cases):
    c = cases[0][0]
    assert len(device(vctx, c, obj_model=np.zeros(0, np.int32), obj_pose=np.zeros((0, 7), f32))) == 0


def test_golden_cases_through_the_device():
    """What the reference's own class printed and kept (tests/golden/depth_verify_ref.npz), from the device."""
    golden = dvr.load_golden(GOLDEN)
    c = capi.Context(0)
    try:
        store = None
        for i, g in enumerate(golden):
            if store != g["set"]:
                upload(c, g["kp_xyz"], g["kp_off"])
                store = g["set"]
            got, want = device(c, g), g["want"]
            for k in ("qs_raw", "is_raw", "qs", "is"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (i, k, got[k], want[k])
            for k in ("plausible", "used", "keep"):
                assert np.array_equal(got[k], want[k]), (i, k)
            cap = f32(g["params"][1])
            with np.errstate(invalid="ignore"):
                capped = np.where(want["multiplier_raw"] > cap, cap, want["multiplier_raw"])
            assert np.array_equal(_bits(got["multiplier"]), _bits(capped)), (i, "multiplier")
    finally:
        c.close()


def test_thresholds_exactly_on_produced_values(vctx, cases):
    """MaxMultiplier exactly on a produced multiplier is no cap (`>`), one ulp below it caps."""
    cs, want = cases
    hits = 0
    for c, w in zip(cs, want):
        cand = np.nonzero(np.isfinite(w["multiplier"]) & (w["used"] > 0) & (w["used"] < w["keypoints"]) & (w["is_raw"] > 0))[0]
        if not len(cand):
            continue
        o = int(cand[0])
        sub = dict(obj_model=c["obj_model"][o:o + 1], obj_pose=c["obj_pose"][o:o + 1])
        mult = f32(w["keypoints"][o]) / f32(w["used"][o])
        for cap, capped in ((mult, False), (np.nextafter(mult, f32(0)), True)):
            prm = (c["params"][0], float(cap), c["params"][2], c["params"][3])
            r = dvr.run_ref(c, params=prm, **sub)
            assert (r["multiplier"][0] == cap) and (r["multiplier"][0] < mult) == capped
            same(device(vctx, c, params=prm, **sub), r, ("cap", capped))
        hits += 1
    assert hits >= 8, hits


def test_is_equal_to_qs_keeps_the_object(vctx, models):
    """IS == QS exactly: the object stays (`IS > QS`).  One keypoint with term 1 (IS = 1/2) and one match with error 1
    (QS = 1/2), by construction in the class's own float32 arithmetic; listed twice, both stay; a match with error 9
    (QS = 1/10) erases both."""
    ID = np.array([0, 0, 0, 1, 0, 0, 0], f32)
    K1 = np.array([1, 1, 0, 0], f32)
    c = capi.Context(0)
    try:
        upload(c, np.array([[0.25, 0.25, 1.0]], f32), np.array([0, 1], np.int32))
        img = np.zeros((1, 1, 4), f32)
        img[0, 0, 2] = 2.0
        c.frame_set_depth_image_host(img, np.zeros((1, 1), f32))
        for uv, qs, keep in (([2.0, 1.0], f32(0.5), 1), ([1.0, 4.0], f32(0.1), 0)):
            r = c.depth_verify(capi.pack_corr(np.array([uv], f32), np.array([[1, 1, 1]], f32)), [0, 1], [0, 0], [ID, ID], K1, ID,
                               K1, ID, (100.0, 8.0, 2.0, 0.5))
            assert r["qs"].tolist() == [qs, qs] and r["is"].tolist() == [0.5, 0.5] and r["keep"].tolist() == [keep, keep]
            assert r["plausible"].tolist() == [1, 1] and r["used"].tolist() == [1, 1] and r["keypoints"].tolist() == [1, 1]
    finally:
        c.close()


def test_calls_on_one_context_do_not_see_each_other(vctx, models):
    """Different maps, match lists and object counts one after the other on one context, large after small and small
    after large: every call equals the restatement."""
    kp, kp_off = models
    rng = np.random.default_rng(0xD3)
    for j, n_obj in enumerate([GRID + 1, 1, 65, 2, 7]):
        c = dvr.make_verify_case(rng, kp, kp_off, match_sizes=np.roll(MATCH_SIZES, j), obj_model=(np.arange(n_obj) + j) % len(SIZES))
        same(device(vctx, c), dvr.run_ref(c), j)


def test_refusals_leave_the_records_untouched(vctx, cases):
    c = cases[0][0]
    L, h = vctx.L, vctx.h
    vctx.frame_set_depth_image_host(c["depth_img"], c["fill_img"])
    corr = capi.pack_corr(c["uv"], c["xyz"])
    off = np.ascontiguousarray(c["model_off"], np.int32)
    om = np.ascontiguousarray(c["obj_model"], np.int32)
    op = np.ascontiguousarray(c["obj_pose"], f32)
    cam, dcam = capi.make_cam(c["K"], c["cam"]), capi.make_cam(c["depth_K"], c["depth_cam"])
    prm = capi.make_depth_verify_params(c["params"])
    rec = np.zeros(len(om), capi.VERIFY_DTYPE)
    rec.view(np.uint8)[:] = 0x5A
    ptr = capi._ptr

    def call(handle=None, **kw):
        a = dict(corr=ptr(corr), off=ptr(off), n_models=len(off) - 1, om=ptr(om), op=ptr(op), n=len(om), cam=C.byref(cam),
                 dcam=C.byref(dcam), prm=C.byref(prm), rec=ptr(rec))
        a.update(kw)
        return L.mh_depth_verify(handle or h, a["corr"], a["off"], a["n_models"], a["om"], a["op"], a["n"], a["cam"], a["dcam"],
                                 a["prm"], a["rec"])

    bad_model = om.copy()
    bad_model[-1] = len(off) - 1
    neg_model = om.copy()
    neg_model[0] = -1
    for kw in (dict(corr=None), dict(off=None), dict(om=None), dict(op=None), dict(cam=None), dict(dcam=None), dict(prm=None),
               dict(rec=None), dict(n=-1), dict(n_models=len(off) - 2), dict(n_models=len(off)), dict(om=ptr(bad_model)),
               dict(om=ptr(neg_model))):
        assert call(**kw) == capi.MH_ERR_ARG, kw
        assert L.mh_last_error(h).decode().startswith("mh_depth_verify"), kw
    assert L.mh_depth_verify_debug_form(h, 2) == capi.MH_ERR_ARG
    # no map
    vctx.frame_set_depth_image_host(None, None)
    assert call() == capi.MH_ERR_ARG and "no depth map" in L.mh_last_error(h).decode()
    # no database; a store that is not grouped; one uploaded in blocks
    rng = np.random.default_rng(3)
    desc = synth.l2_normalize(rng.normal(size=(256, 128)).astype(f32))
    xyz = rng.uniform(-0.1, 0.1, (256, 3)).astype(f32)
    two = np.array([0, 0, 0], np.int32)
    other = capi.Context(0)
    try:
        other.frame_set_depth_image_host(c["depth_img"], c["fill_img"])
        kw = dict(off=ptr(two), n_models=2, om=ptr(np.zeros(len(om), np.int32)), corr=None)
        assert call(other.h, **kw) == capi.MH_ERR_ARG and "no model database" in L.mh_last_error(other.h).decode()
        other.db_upload(desc, np.array([1] * 128 + [0] * 128, np.int32), xyz, 2)
        assert call(other.h, **kw) == capi.MH_ERR_ARG and "not grouped" in L.mh_last_error(other.h).decode()
        other.db_upload_blocks(desc, np.array([0] * 128 + [1] * 128, np.int32), xyz, 2, [0, 512], [128, 128])
        assert call(other.h, **kw) == capi.MH_ERR_ARG and "blocks" in L.mh_last_error(other.h).decode()
    finally:
        other.close()
    assert (rec.view(np.uint8) == 0x5A).all()
    # n_obj = 0: MH_OK, nothing done; and the context is as it was
    vctx.frame_set_depth_image_host(c["depth_img"], c["fill_img"])
    assert call(n=0) == capi.MH_OK and (rec.view(np.uint8) == 0x5A).all()
    same(device(vctx, c), cases[1][0], "after the refusals")
