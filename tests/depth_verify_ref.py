"""DEPTH_VERIFY_CPU::process restated line by line (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp:86-208, `VERIFY.hpp`
below), and the generator of the cases the device is compared on.

The class itself is recorded in tests/golden/depth_verify_ref.npz (tests/tools/make_depth_verify_golden.py) for cases whose
keypoints all land on the map; test_depth_verify_ref_cpu.py holds this restatement to that record bit for bit, and the
device's mh_depth_verify is held to the restatement everywhere else.  Float is float (moped.hpp:76): every value the
reference holds in a Float is an np.float32 here, every expression with a double literal (`1.0 / (1.0 + e)`,
`1.0 - (1.0 / (1.0 + term))`) an np.float64; the ordered `Float += double` chains are Python loops (filter_depth_ref._chain).
The transform helpers and the (int) conventions are filter_depth_ref's; the projection error comes from orclib.project (the
pinned project()).

Readings: a keypoint that projects off the map -- the reference reads outside the buffer there -- or to a
coordinate that is NaN, infinite or outside int is counted in keypointCount and not used; without a distance map there is
no distance test; everything else as written."""
import numpy as np

import orclib
from filter_depth_ref import (DEPTH_CAM, DEPTH_K, H, W, _chain, _surface, inverse_transform, transform, transform_matrix)
from moped_amd import synth

f32, f64 = np.float32, np.float64

# mh_verify_record (moped_amd.capi.VERIFY_DTYPE) + the multiplier as the class prints it, before the cap
RECORD = np.dtype([("qs_raw", "<f4"), ("is_raw", "<f4"), ("multiplier", "<f4"), ("qs", "<f4"), ("is", "<f4"),
                   ("plausible", "<i4"), ("used", "<i4"), ("keypoints", "<i4"), ("keep", "<i4"), ("multiplier_raw", "<f4")])
WORDS = ("qs_raw", "is_raw", "multiplier", "qs", "is", "plausible", "used", "keypoints", "keep")

# one-token changes of the text, for test_depth_verify_ref_cpu's check that the golden would notice each of them
MUTANTS = ("ge_168", "occlusion_reversed", "word3", "uncapped", "is_by_used", "float32_quotient", "pairwise")


def point_outcomes(pose7, pts, depth_img, fill_img, depth_K, depth_cam, max_distance, depth_fraction, mutant=None):
    """VERIFY.hpp:156-188 for one object over its model's keypoints `pts` [n, 3] in order -> (outcome [n]: 0 off the map,
    1 skipped at :168, 2 the sensor in front (:178), 3 a term was added; term [n] float32 (outcome 3), contribution [n]
    float64, pixel [n, 2] (x, y; -1 off the map), distance [n] float32, putative [n] float32)."""
    n = len(pts)
    out = np.zeros(n, np.int32)
    term = np.zeros(n, f32)
    contrib = np.zeros(n, f64)
    if n == 0:
        return out, term, contrib, np.zeros((0, 2), np.int64), np.zeros(0, f32), np.zeros(0, f32)
    h, w = depth_img.shape[:2]
    K = np.asarray(depth_K, f32)
    with np.errstate(all="ignore"):
        p3 = transform(transform_matrix(pose7), np.asarray(pts, f32))              # :161
        p3 = inverse_transform(transform_matrix(depth_cam), p3)                      # :162
        pu = p3[:, 0] / p3[:, 2] * K[0] + K[2]                                       # :164
        pv = p3[:, 1] / p3[:, 2] * K[1] + K[3]                                       # :165
        ok = (pu >= f32(-2147483648.0)) & (pu < f32(2147483648.0)) & (pv >= f32(-2147483648.0)) & (pv < f32(2147483648.0))
        ix = np.where(ok, pu, 0).astype(np.int64)                                    # :167 (int): toward zero
        iy = np.where(ok, pv, 0).astype(np.int64)
        on = ok & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)                        # (the reference reads outside)
        ix, iy = np.where(on, ix, 0), np.where(on, iy, 0)
        distance = fill_img[iy, ix].astype(f32) if fill_img is not None else np.zeros(n, f32)   # :167
        md = f32(max_distance)
        if fill_img is None:
            skip = np.zeros(n, bool)                                                 # no distance map: no test
        elif mutant == "ge_168":
            skip = on & (distance >= md)
        else:
            skip = on & (distance > md)                                              # :168 (a NaN distance is used)
        used = on & ~skip                                                            # :171
        kinect = depth_img[iy, ix, 3 if mutant == "word3" else 2].astype(f32)        # :173
        putative = p3[:, 2]                                                          # :174
        if mutant == "occlusion_reversed":
            front = used & (kinect > putative)
        else:
            front = used & (kinect < putative)                                       # :178
        add = used & ~front
        cauchy = f32(depth_fraction) * kinect                                        # :182
        t = (putative - kinect) / cauchy                                             # :184
        t = t * t                                                                    # :185
        if mutant == "float32_quotient":
            c = (f32(1) - (f32(1) / (f32(1) + t))).astype(f64)
        else:
            c = 1.0 - (1.0 / (1.0 + t.astype(f64)))                                  # :188
    out[skip] = 1
    out[front] = 2
    out[add] = 3
    term[add] = t[add]
    contrib[add] = c[add]
    pix = np.stack([np.where(on, ix, -1), np.where(on, iy, -1)], 1)
    return out, term, contrib, pix, np.where(on, distance, 0).astype(f32), putative


def _pairwise(terms):
    """(a mutant's sum) float32 pairwise instead of the ordered chain"""
    v = [f32(t) for t in terms]
    if not v:
        return f32(0)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return f32(v[0])


def depth_verify(uv, xyz, model_off, kp_xyz, kp_off, obj_model, obj_pose, K, cam, depth_img, fill_img, depth_K, depth_cam,
                 params, mutant=None, detail=None):
    """VERIFY.hpp:86-208.  uv / xyz / model_off: matches[m] (one image, camera K / cam); kp_xyz / kp_off: the models'
    keypoints in order; params: (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction) -> records [n_obj] (RECORD),
    in list order, nothing erased: `keep` is the verdict of :204.  detail (a list): gets every object's point_outcomes."""
    fd, max_mult, max_dist, frac = (f32(v) for v in params)
    n_obj = len(obj_model)
    rec = np.zeros(n_obj, RECORD)
    kp_xyz = np.asarray(kp_xyz, f32).reshape(-1, 3)
    chain = (lambda acc, terms: _pairwise(terms)) if mutant == "pairwise" else _chain
    for o in range(n_obj):                                                           # :118
        m = int(obj_model[o])                                                        # :121-127 modelNum
        lo, hi = int(model_off[m]), int(model_off[m + 1])
        with np.errstate(all="ignore"):
            if hi > lo:
                p = orclib.project(obj_pose[o], np.asarray(xyz, f32)[lo:hi], K, cam) - np.asarray(uv, f32)[lo:hi]   # :129-130
            else:
                p = np.zeros((0, 2), f32)
            e = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]                                # :131
            plausible = int((e < fd).sum())                                          # :132-134
            if mutant == "float32_quotient":
                q = (f32(1) / (f32(1) + e)).astype(f64)
            else:
                q = 1.0 / (1.0 + e.astype(f64))                                      # :135
            QS = chain(0.0, q.tolist())
        pts = kp_xyz[int(kp_off[m]):int(kp_off[m + 1])]                              # :142-150
        po = point_outcomes(obj_pose[o], pts, depth_img, fill_img, depth_K, depth_cam, max_dist, frac, mutant)
        if detail is not None:
            detail.append(po)
        keypoints = len(pts)                                                         # :156
        used = int((po[0] >= 2).sum())                                               # :171
        IS = chain(0.0, po[2].tolist())                                              # :188
        with np.errstate(all="ignore"):
            mult = f32(keypoints) / f32(used)                                        # :191
            r = rec[o]
            r["qs_raw"], r["is_raw"], r["multiplier_raw"] = QS, IS, mult             # :192-193
            if mult > max_mult and mutant != "uncapped":                             # :194-196
                mult = max_mult
            IS = IS * mult                                                           # :197
            QS = QS / f32(plausible)                                                 # :200
            IS = IS / (f32(used) if mutant == "is_by_used" else f32(keypoints))
        r["multiplier"], r["qs"], r["is"] = mult, QS, IS
        r["plausible"], r["used"], r["keypoints"] = plausible, used, keypoints
        r["keep"] = 0 if IS > QS else 1                                              # :204
    return rec


# ------------------------------------------------------------------------------------------------- generated cases
IMAGE_CAM = synth.camera_pose(-0.015, (0.01, 0.0, -0.02)).astype(f32)                # the matches' image: not the identity either
# fill distances of filled pixels: the MaxDistance values the cases use (1, 2) exactly and one ulp above among them
FILLS = np.array([0.5, 1.0, np.nextafter(f32(1.0), f32(2)), 1.5, 2.0, np.nextafter(f32(2.0), f32(3)), 3.0, 6.0], f32)


def quant(a, q=4096.0):
    return (np.round(np.asarray(a, f64) * q) / q).astype(f32)


def make_models(rng, sizes, spread=(0.55, 0.55)):
    """Keypoints of len(sizes) models on the model plane z = 0 (a millimetre of relief) -> (kp_xyz [total, 3], kp_off).
    spread: half extents in x and y; (0.55, 0.55) sends some keypoints off the 40 x 30 map, (0.2, 0.14) none."""
    kp_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    P = int(kp_off[-1])
    kp = np.concatenate([rng.uniform(-spread[0], spread[0], (P, 1)), rng.uniform(-spread[1], spread[1], (P, 1)),
                         rng.uniform(-0.001, 0.001, (P, 1))], 1)
    return quant(kp, 65536.0), kp_off


def make_map(rng, truth, mode=None):
    """A 40 x 30 map of the model plane under `truth` seen through DEPTH_CAM: per pixel measured on the surface (a few
    per mille behind), measured far behind, measured in front, or filled (distance from FILLS), with a NaN reading or two -> (depth_img [H, W, 4], fill_img [H, W])."""
    surf = _surface(truth)
    mode = mode or rng.choice(["agree", "refute", "mixed"], p=[0.4, 0.35, 0.25])
    pr = dict(agree=[0.6, 0.04, 0.1], refute=[0.1, 0.5, 0.1], mixed=[0.32, 0.24, 0.14])[mode]   # surface, far, in front
    cat = rng.choice(4, (H, W), p=pr + [1.0 - sum(pr)])                              # 3: filled
    factor = np.select([cat == 0, cat == 1, cat == 2, cat == 3],
                       [rng.uniform(1.002, 1.006, (H, W)), rng.uniform(1.5, 8.0, (H, W)), rng.uniform(0.3, 0.9, (H, W)),
                        rng.uniform(0.98, 1.3, (H, W))], 1.0)
    z = quant(surf * factor, 16384.0)
    for _ in range(int(rng.integers(0, 3))):
        z[int(rng.integers(0, H)), int(rng.integers(0, W))] = np.nan
    depth_img = np.zeros((H, W, 4), f32)
    depth_img[..., 0] = rng.integers(-8, 9, (H, W)) / 8.0                            # (x, y: never read by the class)
    depth_img[..., 1] = rng.integers(-8, 9, (H, W)) / 8.0
    depth_img[..., 2] = z
    depth_img[..., 3] = quant(np.abs(np.nan_to_num(z, nan=1.0)) * 1.25, 16384.0)     # (norm: never read; not z)
    fill_img = np.where(cat == 3, FILLS[rng.integers(0, len(FILLS), (H, W))], f32(0)).astype(f32)
    if rng.random() < 0.3:
        fill_img[int(rng.integers(0, H)), int(rng.integers(0, W))] = np.nan         # a NaN distance is used
    return depth_img, fill_img


def make_truth(rng):
    q = np.array([rng.normal(0, 0.04), rng.normal(0, 0.04), rng.normal(0, 0.3), 1.0])
    return np.concatenate([q / np.linalg.norm(q), [rng.uniform(-0.04, 0.04), rng.uniform(-0.04, 0.04), rng.uniform(0.8, 0.95)]]).astype(f32)


POSE_KINDS = ("truth", "near", "front", "behind", "mirror", "random")


def make_pose(rng, truth, kind):
    """An object's pose: on the surface (truth, or millimetres off), in front of it, behind it, behind both cameras
    (finite coordinates), or anywhere."""
    if kind == "truth":
        return truth.copy()
    if kind == "near":
        return (truth + np.concatenate([np.zeros(4), rng.normal(0, 0.003, 3)])).astype(f32)
    if kind == "front":
        return np.concatenate([truth[:6], [truth[6] - rng.uniform(0.15, 0.3)]]).astype(f32)
    if kind == "behind":
        return np.concatenate([truth[:6], [truth[6] + rng.uniform(0.15, 0.5)]]).astype(f32)
    if kind == "mirror":
        return np.concatenate([truth[:6], [-truth[6]]]).astype(f32)
    return np.concatenate([synth.random_quat(rng), [0, 0, rng.uniform(0.4, 1.2)]]).astype(f32)


def make_matches(rng, truth, sizes, noise=None):
    """matches[m] of len(sizes) models: points of the model plane and where IMAGE_CAM sees them under `truth`, plus pixel
    noise -> (uv, xyz, model_off)."""
    model_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = int(model_off[-1])
    xyz = quant(np.concatenate([rng.uniform(-0.08, 0.08, (M, 2)), rng.uniform(-0.01, 0.01, (M, 1))], 1), 65536.0)
    if M:
        sigma = noise if noise is not None else rng.choice([0.3, 1.0, 3.0])
        uv = quant(orclib.project(truth, xyz, synth.K_DEFAULT, IMAGE_CAM) + rng.normal(0, sigma, (M, 2)), 64.0)
    else:
        uv = np.zeros((0, 2), f32)
    return uv, xyz, model_off


def make_verify_case(rng, kp_xyz, kp_off, n_obj=None, match_sizes=None, kinds=None, params=None, mode=None, truth=None,
                     obj_model=None, maps=None):
    """-> dict for depth_verify / Context.depth_verify over the given models' keypoints: uv, xyz, model_off, obj_model,
    obj_pose, K, cam, depth_img, fill_img, depth_K, depth_cam, params, kp_xyz, kp_off."""
    n_models = len(kp_off) - 1
    truth = make_truth(rng) if truth is None else truth
    if match_sizes is None:
        match_sizes = rng.choice([0, 1, 63, 64, 65, 130], n_models, p=[0.1, 0.1, 0.2, 0.2, 0.2, 0.2])
    uv, xyz, model_off = make_matches(rng, truth, match_sizes)
    if params is None:
        params = (float(rng.choice([4096.0, 64.0, 4.0])), float(rng.choice([1.5, 3.0, 10.0])), float(rng.choice([2.0, 0.0, 1.0])),
                  float(rng.choice([0.1, 0.25, 0.5])))
    depth_img, fill_img = make_map(rng, truth, mode) if maps is None else maps
    if obj_model is None:
        if n_obj is None:
            n_obj = int(rng.integers(1, 7))
        obj_model = rng.integers(0, n_models, n_obj)
    obj_model = np.asarray(obj_model, np.int32)
    n_obj = len(obj_model)
    if kinds is None:
        kinds = rng.choice(POSE_KINDS, n_obj, p=[0.35, 0.25, 0.12, 0.12, 0.08, 0.08])
    obj_pose = np.stack([make_pose(rng, truth, k) for k in kinds]).astype(f32) if n_obj else np.zeros((0, 7), f32)
    return dict(uv=uv, xyz=xyz, model_off=model_off, obj_model=obj_model, obj_pose=obj_pose, K=synth.K_DEFAULT, cam=IMAGE_CAM,
                depth_img=depth_img, fill_img=fill_img, depth_K=DEPTH_K, depth_cam=DEPTH_CAM, params=tuple(params),
                kp_xyz=kp_xyz, kp_off=kp_off, truth=truth)


def run_ref(c, mutant=None, detail=None, **over):
    a = dict(c, **over)
    return depth_verify(a["uv"], a["xyz"], a["model_off"], a["kp_xyz"], a["kp_off"], a["obj_model"], a["obj_pose"], a["K"],
                        a["cam"], a["depth_img"], a["fill_img"], a["depth_K"], a["depth_cam"], a["params"], mutant, detail)


def plant_equal_depth(c, o=0):
    """The pixel under one keypoint of object o's model gets exactly that keypoint's putative depth (:178 is false, the
    term is 0.): the first keypoint that is used and alone on its pixel.  -> its index inside the model, or None."""
    detail = []
    run_ref(c, detail=detail, obj_model=c["obj_model"][o:o + 1], obj_pose=c["obj_pose"][o:o + 1])
    out, _, _, pix, _, putative = detail[0]
    for j in np.nonzero(out >= 2)[0]:
        if ((pix == pix[j]).all(1)).sum() == 1 and np.isfinite(putative[j]):
            c["depth_img"][pix[j, 1], pix[j, 0], 2] = putative[j]
            return int(j)
    return None


# ------------------------------------------------------------------------------------------------- the golden
def load_golden(path):
    """tests/golden/depth_verify_ref.npz -> a list of cases (make_verify_case's dict + `want`: what the class printed and
    kept, as RECORD without the capped multiplier and the counts' keypoints -- see make_depth_verify_golden.py)."""
    g = dict(np.load(path))
    cases = []
    for i in range(len(g["case_set"])):
        s, mp = int(g["case_set"][i]), int(g["case_map"][i])
        ko = g["kp_off_all"][g["set_off"][s]:g["set_off"][s + 1]]
        kp = g["kp_xyz_all"][g["set_kp"][s]:g["set_kp"][s + 1]]
        n_models = len(ko) - 1
        mo = g["model_off_all"][g["case_moff"][i]:g["case_moff"][i] + n_models + 1]
        mlo = int(g["case_match"][i])
        M = int(mo[-1])
        olo, ohi = int(g["case_obj"][i]), int(g["case_obj"][i + 1])
        cases.append(dict(uv=g["match_all"][mlo:mlo + M, :2].copy(), xyz=g["match_all"][mlo:mlo + M, 2:].copy(), model_off=mo,
                          obj_model=g["obj_model_all"][olo:ohi], obj_pose=g["obj_pose_all"][olo:ohi], K=g["K"], cam=g["cam"],
                          depth_img=g["depth_all"][mp].copy(), fill_img=g["fill_all"][mp].copy(), depth_K=g["depth_K"],
                          depth_cam=g["depth_cam"], params=tuple(float(v) for v in g["params"][i]), kp_xyz=kp, kp_off=ko, set=s,
                          want=g["want"][olo:ohi]))
    return cases
