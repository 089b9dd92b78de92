"""The restatement of moped3d's DEPTH_VERIFY_CPU::process (tests/depth_verify_ref.py) against the class itself:
tests/golden/depth_verify_ref.npz holds what the reference's own header printed and kept for 54 cases whose keypoints all
land on the map (tests/tools/make_depth_verify_golden.py).  Bit for bit: raw and adjusted QS and IS, the multiplier before
the cap, both counts, the verdict; NaN is compared as "NaN on both sides".  Then: the per-point outcomes against the depth
FILTER's restatement where the two classes coincide, hand-worked values for every branch of :164-205, and seven one-token
mutants of the text that the golden must each notice."""
import os

import numpy as np
import pytest

import depth_verify_ref as dvr
import filter_depth_ref as fdr

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_verify_ref.npz")
PRINTED = ("qs_raw", "is_raw", "multiplier_raw", "qs", "is", "plausible", "used", "keep")


@pytest.fixture(scope="module")
def golden():
    return dvr.load_golden(GOLDEN)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        both_nan = np.isnan(a) & np.isnan(b)
        return both_nan | (a.view(np.uint32) == b.view(np.uint32))
    return a == b


def _differs(got, want):
    return any(not _same(got[k], want[k]).all() for k in PRINTED)


def test_restatement_equals_the_recorded_class(golden):
    kept = erased = 0
    for i, c in enumerate(golden):
        got, want = dvr.run_ref(c), c["want"]
        for k in PRINTED:
            bad = np.nonzero(~_same(got[k], want[k]))[0]
            assert not len(bad), (i, k, bad[:4], got[k][bad[:4]], want[k][bad[:4]])
        assert np.array_equal(got["keypoints"], np.diff(c["kp_off"])[c["obj_model"]])
        kept += int(want["keep"].sum())
        erased += int((want["keep"] == 0).sum())
    n = kept + erased
    assert kept >= 0.2 * n and erased >= 0.2 * n, (kept, erased)


def test_the_golden_covers_what_it_claims(golden):
    w = np.concatenate([c["want"] for c in golden])
    cap = np.concatenate([np.full(len(c["want"]), c["params"][1], f32) for c in golden])
    assert (w["multiplier_raw"] > cap).any() and (w["multiplier_raw"] < cap).any()
    assert (w["used"] == 0).any() and (w["plausible"] == 0).any() and np.isnan(w["is_raw"]).any()
    assert np.isinf(w["multiplier_raw"]).any() and np.isnan(w["multiplier_raw"]).any()     # x/0 and 0/0
    assert any(c["model_off"][m + 1] == c["model_off"][m] for c in golden for m in c["obj_model"])
    at = above = equal = 0
    for c in golden:
        detail = []
        dvr.run_ref(c, detail=detail)
        md = f32(c["params"][2])
        for out, _, _, pix, dist, putative in detail:
            assert (pix >= 0).all()                     # every keypoint on the map: the reference read inside its buffers
            at += int(((out >= 2) & (dist == md) & (md > 0)).sum())
            above += int(((out == 1) & (dist == np.nextafter(md, f32(np.inf)))).sum())
            equal += int(((out == 3) & (c["depth_img"][pix[:, 1], pix[:, 0], 2] == putative)).sum())
    assert at and above and equal, (at, above, equal)


@pytest.mark.parametrize("mutant", dvr.MUTANTS)
def test_one_token_mutants_differ_from_the_golden(golden, mutant):
    hits = sum(_differs(dvr.run_ref(c, mutant=mutant), c["want"]) for c in golden)
    assert hits >= 1, mutant


def test_point_outcomes_equal_the_depth_filter_where_the_classes_coincide():
    """On-map or not, MaxDistance = 0 and no negative (or NaN) distances: `distance > MaxDistance` is the FILTER's
    `distance > 0`, and both classes then take the same branch and form the same term for every point."""
    rng = np.random.default_rng(0xC01C)
    seen = np.zeros(4, int)
    for case in range(40):
        kp, kp_off = dvr.make_models(rng, [int(rng.choice([1, 64, 65, 129, 300]))])
        c = dvr.make_verify_case(rng, kp, kp_off, n_obj=3)
        fill = np.nan_to_num(c["fill_img"], nan=0.0) if case % 5 else None
        for pose in c["obj_pose"]:
            a = dvr.point_outcomes(pose, kp, c["depth_img"], fill, c["depth_K"], c["depth_cam"], 0.0, c["params"][3])
            b = fdr.point_outcomes(pose, kp, c["depth_img"], fill, c["depth_K"], c["depth_cam"], c["params"][3])
            assert np.array_equal(a[0], b[0])
            assert _same(a[1], b[1]).all()
            assert np.array_equal(a[2].view(np.uint64)[~np.isnan(a[2])], b[2].view(np.uint64)[~np.isnan(b[2])])
            assert np.array_equal(np.isnan(a[2]), np.isnan(b[2]))
            seen += np.bincount(a[0], minlength=4)
    assert (seen > 100).all(), seen


# ---- hand-worked values: one keypoint, identity pose and cameras, K = (1, 1, 0, 0): the pixel is (x/z, y/z) --------
ID = np.array([0, 0, 0, 1, 0, 0, 0], f32)
UNIT_K = np.array([1, 1, 0, 0], f32)


def _one(points, depth, fill, params, matches=None, pose=ID):
    """records of one object over `points` [n, 3] on a map with depth [h, w] and fill [h, w] (or None)"""
    depth = np.asarray(depth, f32)
    img = np.zeros(depth.shape + (4,), f32)
    img[..., 2] = depth
    img[..., 3] = 77.0
    uv, xyz = (np.zeros((0, 2), f32), np.zeros((0, 3), f32)) if matches is None else matches
    pts = np.asarray(points, f32).reshape(-1, 3)
    return dvr.depth_verify(uv, xyz, [0, len(uv)], pts, [0, len(pts)], [0], pose[None], UNIT_K, ID, img,
                            None if fill is None else np.asarray(fill, f32), UNIT_K, ID, params)[0]


def test_hand_worked_branches():
    z2 = [[2.0, 4.0], [1.0, np.nan]]                    # depth at pixels (0,0) (1,0) / (0,1) (1,1)
    fill = [[0.0, 3.0], [2.0, 0.0]]
    P = (100.0, 8.0, 2.0, 0.5)
    # :168 distance 3 > 2: skipped -- counted, not used; multiplier 1/0 = inf capped to 8; IS = 0 * 8 / 1 = 0
    r = _one([[2.5, 0.5, 2.0]], z2, fill, P)            # pixel (1, 0)
    assert (r["keypoints"], r["used"], r["is_raw"], r["multiplier_raw"], r["multiplier"], r["is"]) == (1, 0, 0, np.inf, 8, 0)
    assert np.isnan(r["qs"]) and r["keep"] == 1         # no match: QS = 0/0, IS > NaN is false
    # :168 distance exactly MaxDistance: used; :178 kinect 1 < putative 2: an occlusion, nothing added
    r = _one([[0.5, 2.5, 2.0]], z2, fill, P)            # pixel (0, 1)
    assert (r["used"], r["is_raw"], r["multiplier"]) == (1, 0, 1)
    # :182-188 kinect 2 behind putative 1: cauchy = 0.5 * 2 = 1, term = ((1 - 2) / 1)^2 = 1, IS = 1 - 1/2
    r = _one([[0.25, 0.25, 1.0]], z2, fill, P)          # pixel (0, 0)
    assert (r["used"], r["is_raw"], r["is"]) == (1, 0.5, 0.5)
    # kinect == putative: not an occlusion (`<`), term 0
    r = _one([[0.5, 0.5, 2.0]], z2, fill, P)
    assert (r["used"], r["is_raw"]) == (1, 0)
    # a NaN depth: `<` is false, the term and IS are NaN; IS > QS false: kept
    r = _one([[1.5, 1.5, 1.0]], z2, fill, P)            # pixel (1, 1)
    assert r["used"] == 1 and np.isnan(r["is_raw"]) and np.isnan(r["is"]) and r["keep"] == 1
    # a NaN distance is used; no distance map: the filled pixel is used
    r = _one([[2.5, 0.5, 2.0]], z2, [[0, np.nan], [0, 0]], P)
    assert r["used"] == 1 and r["is_raw"] == 0.5        # kinect 4 behind putative 2: ((2 - 4) / (0.5 * 4))^2 = 1
    r = _one([[2.5, 0.5, 2.0]], z2, None, P)
    assert r["used"] == 1
    # off the map (pixel (2, 0)), a coordinate in (-1, 0) (pixel (0, 0)), behind the camera, z = 0 (NaN / inf coordinates)
    assert _one([[4.5, 0.5, 2.0]], z2, fill, P)["used"] == 0
    assert _one([[-0.25, 0.25, 1.0]], z2, fill, P)["used"] == 1
    r = _one([[-0.25, -0.25, -1.0]], z2, fill, P)       # x/z = 0.25: pixel (0, 0); kinect 2 < putative -1 is false
    assert r["used"] == 1 and r["is_raw"] == f32(1.0 - 1.0 / (1.0 + 9.0))          # ((-1 - 2) / 1)^2 = 9
    assert _one([[0.0, 0.0, 0.0]], z2, fill, P)["used"] == 0 and _one([[1.0, 1.0, 0.0]], z2, fill, P)["used"] == 0
    # two keypoints, one used: multiplier 2 (below the cap 8), IS = 0.5 * 2 / 2; with the cap at 1.5: 0.5 * 1.5 / 2
    two = [[0.25, 0.25, 1.0], [2.5, 0.5, 2.0]]
    r = _one(two, z2, fill, P)
    assert (r["keypoints"], r["used"], r["multiplier_raw"], r["multiplier"], r["is"]) == (2, 1, 2, 2, 0.5)
    r = _one(two, z2, fill, (100.0, 1.5, 2.0, 0.5))
    assert (r["multiplier_raw"], r["multiplier"], r["is"]) == (2, 1.5, 0.375)
    # a model without keypoints: 0/0 = NaN passes the cap, IS = NaN: kept
    r = _one(np.zeros((0, 3)), z2, fill, P)
    assert r["keypoints"] == 0 and np.isnan(r["multiplier"]) and np.isnan(r["is"]) and r["keep"] == 1


def test_hand_worked_quality_score_and_verdict():
    z2, fill = [[2.0]], [[0.0]]
    kp = [[0.25, 0.25, 1.0]]                            # IS = 0.5 (above)
    # matches: errors 0 (quotient 1), 1 (1/2), 9 (1/10), behind the camera (FLT_MAX: infinite error, quotient 0)
    xyz = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, -1]], f32)
    uv = np.array([[1, 1], [2, 1], [1, 4], [0, 0]], f32)
    r = _one(kp, z2, fill, (4.0, 8.0, 2.0, 0.5), (uv, xyz))
    assert r["qs_raw"] == f32(1.5 + 1.0 / 10.0) and r["plausible"] == 2   # errors 0 and 1 are < 4
    assert r["qs"] == r["qs_raw"] / f32(2) and r["keep"] == 1                      # IS 0.5 <= QS 0.8
    # FeatureDistance 0: nothing plausible, QS = 1.6 / 0 = inf: kept
    r = _one(kp, z2, fill, (0.0, 8.0, 2.0, 0.5), (uv, xyz))
    assert r["plausible"] == 0 and r["qs"] == np.inf and r["keep"] == 1
    # one match with error 1: QS = 0.5 = IS: `>` keeps; error 9: QS = 0.1 < IS: erased
    r = _one(kp, z2, fill, (4.0, 8.0, 2.0, 0.5), (uv[1:2], xyz[1:2]))
    assert (r["qs"], r["is"], r["keep"]) == (0.5, 0.5, 1)
    r = _one(kp, z2, fill, (100.0, 8.0, 2.0, 0.5), (uv[2:3], xyz[2:3]))
    assert (r["qs"], r["is"], r["keep"]) == (f32(0.1), 0.5, 0)


def test_chain_is_ordered_float_plus_double():
    """Three terms whose float32 chain depends on the order and differs from the float64 sum rounded once."""
    terms = [1.0, 2.0 ** -24, 2.0 ** -24]
    assert dvr._chain(0.0, terms) == f32(1.0)                                       # each half-ulp rounds to even: lost
    assert dvr._chain(0.0, terms[::-1]) == np.nextafter(f32(1.0), f32(2.0))         # added first, they count
    assert f32(sum(terms)) == np.nextafter(f32(1.0), f32(2.0))
