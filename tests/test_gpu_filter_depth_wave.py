"""The two device forms of the depth FILTER's F1 (csrc/filter_depth_dev.h) under the stage-level entry, without POSE in
between: form 0, the workgroup form of the stand-alone launch (filter_depth_score), and form 1, filter_depth_score_wave
-- one wavefront per object, no LDS, the form the POSE tails of a fused frame run (mh_filter_depth_debug_form).  Both
must equal the restatement of FILTER_PROJECTION_DEPTH_CPU::process (tests/filter_depth_ref.py) bit for bit: scores, IS,
used and plausible per slot, survivors, their order and the rewritten clusters.

The cases are the smallest that can break the wave form (64 lanes per step, four wavefronts per workgroup, in-cluster
flags cached for 32 steps), on maps of 64 x 48:
  points     test points per model 0, 1, 63, 64, 65, 130 -- the empty chain, ragged tails, a chain over three steps
  objects    1, 4, 5 and 9 slots, two objects of one model among them
  matches    1, 64, 65 and 2 100 per model -- the last is 33 steps: the claims' flags are recomputed
  map        NaN (under a used point: a NaN score), zero and negative depths, fill > 0 patches, no fill map at all, points off the image and one whose
             projected coordinate is finite but beyond int's range
  branches   a surface in front of a point (occlusion: nothing added) and one behind it (the Cauchy term)
  threshold  MinKeypointFraction placed so that `used` is exactly (int)(fraction * n): IS = 0, one point fewer: IS > 0
  generated  one case of filter_cases.make_case (random poses per model, duplicate keys) with a map added
Every case first asserts on the restatement's own output that it reaches what it names."""
import functools

import numpy as np
import pytest

import filter_cases
import filter_depth_ref as fdr
import orclib
import test_gpu_filter_depth as tfd
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = 64, 48
DEPTH_K = np.array([48.0, 45.0, 32.0, 24.0], f32)
DEPTH_CAM = fdr.DEPTH_CAM                                        # not the identity
CAM_SHIFT = np.array([0, 0, 0, 1, 0.03, -0.02, 0.01], f32)      # exact rotations: coordinates beyond int stay finite
TWO31 = 2147483648.0


def _map(rng, zc, fill):
    """A 64 x 48 map about depth zc: per pixel a few per mille behind, far behind, in front, a hole (negative), zero,
    filled."""
    cat = rng.choice(6, (H, W), p=[0.3, 0.22, 0.18, 0.05, 0.05, 0.2])
    factor = np.select([cat == 0, cat == 1, cat == 2], [rng.uniform(1.003, 1.006, (H, W)), rng.uniform(1.5, 10.0, (H, W)),
                                                         rng.uniform(0.3, 0.9, (H, W))], 1.0)
    z = (zc * factor).astype(f32)
    z[cat == 3] = f32(-1.0)
    z[cat == 4] = f32(0.0)
    img = np.zeros((H, W, 4), f32)
    img[..., 0] = rng.normal(0, 1, (H, W))                       # (x, y, norm: never read by the class)
    img[..., 1] = rng.normal(0, 1, (H, W))
    img[..., 2] = z
    img[..., 3] = np.abs(z)
    fill_img = np.where(cat == 5, rng.uniform(0.5, 6.0, (H, W)), 0.0).astype(f32) if fill else None
    return img, fill_img


def _build(seed, sizes, counts, obj_model, exact=False, fill=True, nan_under=None):
    """Models with `sizes` matches and `counts` test points each, all at one true pose; objects at the truth, near it,
    in front of the surface and behind the cameras.  exact: identity rotations everywhere and one test point far out
    along x, so that its projected coordinate is finite and beyond int's range."""
    rng = np.random.default_rng([0x3A7E, seed])
    K, cam0 = synth.K_DEFAULT, synth.CAM_IDENTITY
    model_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = int(model_off[-1])
    if exact:
        q = np.array([0.0, 0.0, 0.0, 1.0])
    else:
        q = np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.3), 1.0])
    truth = np.concatenate([q / np.linalg.norm(q), [0.02, -0.03, 0.8]]).astype(f32)
    xyz = np.concatenate([rng.uniform(-0.08, 0.08, (M, 2)), rng.uniform(-0.01, 0.01, (M, 1))], 1).astype(f32)
    uv = (orclib.project(truth, xyz, K, cam0) + rng.normal(0, 0.3, (M, 2))).astype(f32)
    for _ in range(3):                                           # one keypoint in two lists: ownership by the projection score
        a, b = rng.integers(0, M, 2)
        uv[a] = uv[b]
    pts_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    P = int(pts_off[-1])
    pts = np.concatenate([rng.uniform(-0.7, 0.7, (P, 2)), rng.uniform(-0.001, 0.001, (P, 1))], 1).astype(f32)   # some leave the map
    depth_cam = CAM_SHIFT if exact else DEPTH_CAM
    if exact:
        m = int(np.argmax(counts))
        pts[int(pts_off[m]) + 2] = (1e12, 0.01, 0.0)
    img, fill_img = _map(rng, 0.8, fill)
    obj_model = np.asarray(obj_model, np.int32)
    obj_pose = np.zeros((len(obj_model), 7), f32)
    for o in range(len(obj_model)):
        kind = o % 5
        if kind in (0, 3):
            obj_pose[o] = truth
        elif kind == 1:
            obj_pose[o] = truth + np.concatenate([np.zeros(4), rng.normal(0, 0.003, 3)]).astype(f32)
        elif kind == 2:
            obj_pose[o] = np.concatenate([truth[:6], [truth[6] - 0.35]])   # in front of the surface: every reading lies behind it
        else:
            obj_pose[o] = np.concatenate([truth[:6], [-truth[6]]])          # behind both cameras
    c = dict(uv=uv, xyz=xyz, model_off=model_off, obj_model=obj_model, obj_pose=obj_pose, K=K, cam=cam0, min_points=2,
             fd=4096.0, min_score=0.5, pts_xyz=pts, pts_off=pts_off, depth_img=img, fill_img=fill_img, depth_K=DEPTH_K,
             depth_cam=depth_cam, psd=16.0, depth_fraction=0.25, min_kp_fraction=0.1)
    if nan_under is not None:                                    # a NaN reading where a point of that object is used
        on, ix, iy, _ = _pixels(c, nan_under)
        hit = np.nonzero(on & ((fill_img[iy, ix] == 0) if fill_img is not None else True))[0]
        img[iy[hit[0]], ix[hit[0]], 2] = np.nan
    return c


def _generated():
    """filter_cases.make_case (poses per model, duplicate and signed-zero keys, its own thresholds) + test points and a map."""
    rng = np.random.default_rng(0x9E4)
    c = filter_cases.make_case(rng, n_obj=9, work=30_000)
    n_models = len(c["model_off"]) - 1
    counts = np.array([130, 0, 65, 1, 64][:n_models])
    pts_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pts = rng.uniform(-0.08, 0.08, (int(pts_off[-1]), 3)).astype(f32)
    img, fill_img = _map(rng, 0.75, True)
    # the map's camera looks at the objects with a short focal length: their points land on the 64 x 48 pixels
    return dict(uv=c["uv"], xyz=c["xyz"], model_off=c["model_off"], obj_model=c["obj_model"], obj_pose=c["obj_pose"],
                K=c["Ks"][0], cam=c["cams"][0], min_points=c["min_points"], fd=c["fd"], min_score=c["min_score"], pts_xyz=pts,
                pts_off=pts_off, depth_img=img, fill_img=fill_img, depth_K=np.array([60.0, 60.0, 32.0, 24.0], f32),
                depth_cam=synth.CAM_IDENTITY, psd=4096.0, depth_fraction=0.25, min_kp_fraction=0.1)


CASES = {
    # name: (builder, what the case must reach)
    "four_objects_short_lists": (lambda: _build(1, [1, 64, 65], [0, 1, 63], [0, 1, 2, 2]),
                                 dict(kept=True, erased=True, same_model=True)),
    "five_objects_33_steps": (lambda: _build(2, [65, 2100, 64], [64, 65, 130], [0, 1, 1, 2, 2], nan_under=4),
                              dict(kept=True, erased=True, same_model=True, map=True)),
    "one_object_no_fill_map": (lambda: _build(3, [2100], [130], [0], fill=False), dict(kept=True)),
    "nine_objects_beyond_int": (lambda: _build(4, [64, 1, 65], [65, 130, 0], [0, 0, 0, 1, 1, 1, 2, 2, 2], exact=True),
                                dict(kept=True, erased=True, same_model=True, beyond_int=True)),
    "generated": (_generated, dict(kept=True, erased=True)),
}


def _restate(c):
    detail = []
    r = fdr.filter_projection_depth(c["uv"], c["xyz"], c["model_off"], c["obj_model"], c["obj_pose"], c["K"], c["cam"],
                                    c["min_points"], c["fd"], c["min_score"], c["pts_xyz"], c["pts_off"], c["depth_img"],
                                    c["fill_img"], c["depth_K"], c["depth_cam"], c["psd"], c["depth_fraction"],
                                    c["min_kp_fraction"], detail=detail)
    return r, detail


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (case, restatement's answer, per-object outcome arrays): built once, shared by both forms, never changed."""
    if name.startswith("threshold"):
        base, want, detail = _case("five_objects_33_steps")
        # an object whose IS counts: `used` exactly on (int)(fraction * n) zeroes it, one point fewer does not
        o = int(np.nonzero((want[4] > 0) & (want[5] > 1))[0][0])
        n = int(np.diff(base["pts_off"])[base["obj_model"][o]])
        used = int(want[5][o])
        frac = float(f32((used + (0.5 if name == "threshold_on" else -0.5)) / n))
        assert fdr._int_of(f32(frac) * f32(n)) == (used if name == "threshold_on" else used - 1)
        c = dict(base, min_kp_fraction=frac)
        r, detail = _restate(c)
        assert r[5][o] == used
        assert (r[4][o] == 0) == (name == "threshold_on"), (name, r[4][o])
        return c, r, detail
    c = CASES[name][0]()
    r, detail = _restate(c)
    return c, r, detail


def _pixels(c, o):
    """Where object o's test points land, in the class's own arithmetic -> (on the image [n], ix, iy, pu)."""
    m = int(c["obj_model"][o])
    k = np.asarray(c["pts_xyz"], f32)[int(c["pts_off"][m]):int(c["pts_off"][m + 1])]
    if not len(k):
        z = np.zeros(0, np.int64)
        return z.astype(bool), z, z, np.zeros(0, f32)
    with np.errstate(all="ignore"):
        p3 = fdr.inverse_transform(fdr.transform_matrix(c["depth_cam"]), fdr.transform(fdr.transform_matrix(c["obj_pose"][o]), k))
        pu = p3[:, 0] / p3[:, 2] * c["depth_K"][0] + c["depth_K"][2]
        pv = p3[:, 1] / p3[:, 2] * c["depth_K"][1] + c["depth_K"][3]
        ok = (np.abs(pu) < f32(TWO31)) & (np.abs(pv) < f32(TWO31))
        ix, iy = np.where(ok, pu, 0).astype(np.int64), np.where(ok, pv, 0).astype(np.int64)
    on = ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    return on, np.where(on, ix, 0), np.where(on, iy, 0), pu


def _covers(name, c, r, detail):
    """What the case names, read off the restatement's output (the threshold cases have asserted theirs in _case)."""
    if name.startswith("threshold"):
        return
    score, keep, order, clusters, inc, used, plaus = r
    need = CASES[name][1]
    out = np.concatenate(detail)
    assert (out == 3).any() and (out == 2).any(), "a surface behind a point and one in front of it"
    assert (out == 0).any(), "points off the image"
    assert (out == 1).any() == (c["fill_img"] is not None), "filled pixels, or no fill map"
    assert (inc > 0).any() and (used > 0).any() and (plaus > 0).any(), "an IS that counts"
    assert (used < np.diff(c["pts_off"])[c["obj_model"]]).any(), "some points skipped"
    if need.get("kept"):
        assert keep.any() and len(clusters) == int(keep.sum())
    if need.get("erased"):
        assert (~keep).any()
    if need.get("same_model"):
        assert len(set(c["obj_model"].tolist())) < len(c["obj_model"])
    if need.get("map"):     # used points on a zero and on a negative reading; a NaN reading under a used point: a NaN score
        z_at = np.concatenate([c["depth_img"][iy, ix, 2][on & (d >= 2)] for o, d in enumerate(detail)
                               for on, ix, iy, _ in [_pixels(c, o)]])
        assert (z_at == 0).any() and (z_at < 0).any() and np.isnan(z_at).any(), "zero, negative and NaN depths under used points"
        assert np.isnan(score).any()
    if need.get("beyond_int"):
        pu = np.concatenate([_pixels(c, o)[3] for o in range(len(c["obj_model"]))])
        assert (np.isfinite(pu) & (np.abs(pu) >= f32(TWO31))).any(), "a finite coordinate beyond int's range"


@pytest.fixture(scope="module")
def wctx():
    c = capi.Context(0)
    yield c
    c.filter_depth_debug_form(0)
    c.close()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", list(CASES) + ["threshold_on", "threshold_below"])
def test_both_forms_equal_the_restatement(wctx, name, form):
    c, want, detail = _case(name)
    _covers(name, c, want, detail)
    wctx.filter_depth_debug_form(form)
    got = tfd._device(wctx, c)
    print(name, "form", form, "objects", len(c["obj_model"]), "kept", int(want[1].sum()), "IS", want[4][:9], "used", want[5][:9],
          "plausible", want[6][:9])
    tfd.same(got, want, (name, form))
    assert np.array_equal(tfd._bits(got[0]), tfd._bits(want[0]))   # scores as uint32 (same() has said so; kept explicit)


def test_form_setter_refuses_other_values(wctx):
    with pytest.raises(capi.MhError, match="mh_filter_depth_debug_form"):
        wctx.filter_depth_debug_form(2)
    wctx.filter_depth_debug_form(1)
    wctx.filter_depth_debug_form(0)
