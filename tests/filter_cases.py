"""FILTER cases at the sizes the device treats differently (filter_dev.h): object slots around FILTER_GRID = 128
workgroups and FL_SLOTS = 256 LDS slots, models around 32 x 64 = 2 048 matches (the in-cluster bit cache), equal
scores on both sides of slots 128 and 256, duplicate image coordinates inside and across models with (0.0, y) against
(-0.0, y), poses behind the camera or near z = 0.  Shared by the GPU differential fuzz (test_gpu_filter.py) and the
oracle-against-witness check at those sizes (test_witness_cpu.py)."""
import numpy as np

import orclib
from moped_amd import synth

K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
f32 = np.float32
N_OBJ = (0, 1, 4, 127, 128, 129, 255, 256, 257, 600)
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 5000)
SMALL = (0, 1, 63, 64, 65)


def _cams(rng, n_images):
    if n_images == 1:
        return np.array([K]), np.array([CAM0])
    Ks = np.array([K * f32(rng.uniform(0.9, 1.1)) for _ in range(n_images)], f32)
    cams = np.array([CAM0] + [synth.camera_pose(rng.uniform(-0.15, 0.15), (rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), 0))
                              for _ in range(n_images - 1)], f32)
    return Ks, cams


def make_case(rng, n_images=1, work=400_000, n_obj=None):
    """-> dict(uv, xyz, img, model_off, obj_model (sorted by model: the (model, list) order the reference sweeps),
    obj_pose, Ks, cams, min_points, fd, min_score).  `work` bounds sum over objects of their model's match count."""
    n_models = int(rng.integers(1, 6))
    sizes = np.array([rng.choice(SIZES if rng.random() < 0.5 else SMALL) for _ in range(n_models)], np.int64)
    while sizes.sum() > 12_000:
        sizes[int(np.argmax(sizes))] = rng.choice(SMALL)
    model_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = int(model_off[-1])
    Ks, cams = _cams(rng, n_images)
    img = rng.integers(0, n_images, M).astype(np.int32) if n_images > 1 else np.zeros(M, np.int32)
    xyz = rng.uniform(-0.08, 0.08, size=(M, 3)).astype(f32)
    truth = np.zeros((n_models, 7), f32)
    uv = np.zeros((M, 2), f32)
    for m in range(n_models):
        tz = rng.uniform(0.5, 1.0)
        tx = -0.4 * tz if rng.random() < 0.3 else rng.uniform(-0.2, 0.2)      # about u = 0: room for (+-0.0, y) keys
        truth[m] = np.concatenate([synth.random_quat(rng), [tx, rng.uniform(-0.15, 0.15), tz]])
        if m and rng.random() < 0.3:                                          # two models at one pose: shared keys compete
            truth[m] = truth[m - 1]
        lo, hi = model_off[m], model_off[m + 1]
        if hi > lo:
            p = orclib.project_images(truth[m], xyz[lo:hi], img[lo:hi], Ks, cams)
            uv[lo:hi] = p + rng.normal(0, rng.choice([0.3, 3.0, 30.0]), size=(hi - lo, 2))
    if M and rng.random() < 0.7:     # the same coordinate twice, inside a model and across models
        for _ in range(int(rng.integers(1, 12))):
            a, b = rng.integers(0, M, 2)
            uv[a] = uv[b]
            if rng.random() < 0.5:
                img[a] = img[b]      # (several images: the same key; otherwise the same uv in another image)
    if M and rng.random() < 0.5:     # (0.0, y) and (-0.0, y): one key (std::map compares floats)
        for _ in range(int(rng.integers(1, 6))):
            a, b = rng.integers(0, M, 2)
            if rng.random() < 0.5:   # a copied point: the same projection, so both in or both out of the cluster
                xyz[b] = xyz[a]
                img[b] = img[a]
            uv[a, 0], uv[b, 0] = f32(0.0), f32(-0.0)
            uv[b, 1] = uv[a, 1]
    if n_obj is None:
        n_obj = int(rng.choice(N_OBJ))
    obj_model = rng.integers(0, n_models, n_obj).astype(np.int32)
    small = np.nonzero(sizes <= 65)[0]
    big = [o for o in range(n_obj) if sizes[obj_model[o]] > 65]
    rng.shuffle(big)
    while big and int(sizes[obj_model[obj_model >= 0]].sum()) > work:   # most objects on small models, a few on big ones
        obj_model[big.pop()] = rng.choice(small) if len(small) else -1
    obj_model = np.sort(obj_model[obj_model >= 0]).astype(np.int32)
    n_obj = len(obj_model)
    obj_pose = np.zeros((n_obj, 7), f32)
    for o in range(n_obj):
        t = truth[obj_model[o]]
        r = rng.random()
        if r < 0.4:
            obj_pose[o] = t                                                        # equal scores: the first object wins
        elif r < 0.7:
            obj_pose[o] = t + np.concatenate([np.zeros(4), rng.normal(0, 0.01, 3)])
        elif r < 0.8:
            obj_pose[o] = np.concatenate([t[:4], t[4:6], [-t[6]]])                 # behind the camera
        elif r < 0.9:
            obj_pose[o] = np.concatenate([t[:6], [rng.choice([0.0, 1e-3, -1e-3, 0.05])]])   # points about z = 0
        else:
            obj_pose[o] = np.concatenate([synth.random_quat(rng), [0, 0, rng.uniform(0.4, 1.2)]])
    for edge in (128, 256):          # one model's objects on both sides of the slot edge: the same pose on both sides
        if n_obj > edge and obj_model[edge - 1] == obj_model[edge]:
            first = int(np.searchsorted(obj_model, obj_model[edge]))
            obj_pose[edge + int(rng.integers(0, min(8, n_obj - edge)))] = obj_pose[first] = truth[obj_model[edge]]
    return dict(uv=uv, xyz=xyz, img=img, model_off=model_off, obj_model=obj_model, obj_pose=obj_pose, Ks=Ks, cams=cams,
                min_points=int(rng.integers(0, 9)), fd=float(rng.choice([4096.0, 64.0, 8192.0, 1e6])),
                min_score=float(rng.choice([2.0, 3.0, 0.0, 1e-4])))


def oracle(c, **over):
    a = dict(c, **over)
    if len(a["Ks"]) == 1:
        return orclib.filter_projection(a["uv"], a["xyz"], a["model_off"], a["obj_model"], a["obj_pose"], a["Ks"][0],
                                        a["cams"][0], a["min_points"], a["fd"], a["min_score"])
    return orclib.filter_images(a["uv"], a["img"], a["xyz"], a["model_off"], a["obj_model"], a["obj_pose"], a["Ks"], a["cams"],
                                a["min_points"], a["fd"], a["min_score"])


def err2(c, o):
    """Squared reprojection errors of object o over its model's matches, as FILTER computes them (p -= coord2D;
    p0*p0 + p1*p1)."""
    m = c["obj_model"][o]
    lo, hi = c["model_off"][m], c["model_off"][m + 1]
    d = orclib.project_images(c["obj_pose"][o], c["xyz"][lo:hi], c["img"][lo:hi], c["Ks"], c["cams"]) - c["uv"][lo:hi]
    with np.errstate(over="ignore", invalid="ignore"):     # (points about z = 0)
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


class Regimes:
    """What a block of cases reached, from the oracle's answers: a run that misses a regime fails its block."""

    def __init__(self):
        self.kept_past_256 = self.big_cluster = self.tie_256 = self.tie_128 = self.signed_zero = 0
        self.empty_model_obj = self.kept = self.erased = self.signed_zero_owned = 0

    def add(self, c, res):
        score, keep, order, clusters = res
        om, off, uv = c["obj_model"], c["model_off"], c["uv"]
        n_obj = len(om)
        self.kept += int(keep.sum())
        self.erased += n_obj - int(keep.sum())
        self.kept_past_256 += n_obj > 256 and bool((order >= 256).any())
        self.big_cluster += any(len(cl) > 2048 for cl in clusters)
        self.empty_model_obj += any(off[m + 1] == off[m] for m in om)
        for edge in (128, 256):      # an exact tie across the edge decided for the lower slot
            if n_obj > edge:
                lo = np.nonzero(om[:edge] == om[edge])[0]
                hi = np.nonzero(om[edge:] == om[edge])[0] + edge
                tied = any(score[a] > 0 and score[a] == score[b] and keep[a] for a in lo[:1] for b in hi)
                if edge == 128:
                    self.tie_128 += tied
                else:
                    self.tie_256 += tied
        z = uv[:, 0] == 0
        self.signed_zero += bool(np.signbit(uv[z, 0]).any() and (~np.signbit(uv[z, 0])).any())
        owned = [off[om[o]] + cl for o, cl in zip(order, clusters)]
        self.signed_zero_owned += bool(self.signed_zero) and any(np.signbit(uv[g, 0][uv[g, 0] == 0]).any() for g in owned)


def same(g, o, tag=None):
    """A device FILTER answer equals the oracle's: every score at the bits, keep flags, out order, every cluster."""
    assert np.array_equal(g[0].view(np.uint32), o[0].view(np.uint32)), ("score", tag)
    assert np.array_equal(g[1], o[1]), ("keep", tag)
    assert np.array_equal(g[2], o[2]), ("order", tag)
    assert len(g[3]) == len(o[3]), ("kept", tag)
    for k, (a, b) in enumerate(zip(g[3], o[3])):
        assert np.array_equal(a, b), ("members", k, tag)


def assert_delivered_scores(objs, uv, xyz, model_off, feature_distance, Ks=(K,), cams=(CAM0,), img=None):
    """A delivered object's FILTER2 score depends on its own pose and its model's match list alone: FILTER of that one
    object at the DEVICE's pose gives the device's score bit for bit.  uv / xyz / model_off: the accepted matches
    (orclib.match_accept's lists, index-exact with the device's), img: their images (several cameras)."""
    for j, g in enumerate(objs):
        om, op = np.array([g["model"]], np.int32), g["pose"][None].astype(np.float32)
        if img is None:
            s = orclib.filter_projection(uv, xyz, model_off, om, op, Ks[0], cams[0], 0, feature_distance, 0.0)[0]
        else:
            s = orclib.filter_images(uv, img, xyz, model_off, om, op, Ks, cams, 0, feature_distance, 0.0)[0]
        assert s.view(np.uint32)[0] == np.float32(g["score"]).view(np.uint32), (j, int(g["model"]), float(s[0]), float(g["score"]))


# ------------------------------------------------------------------------------------------- frames for the frame paths
def plant_duplicates(db, fr, rng, n_pairs=8, reach=40.0):
    """Keypoints of two visible objects at one image coordinate: the closest planted points of two different objects
    (< `reach` px apart) both moved to their midpoint -- in both objects' FILTER clusters, one key of the ownership map.
    Then the image is shifted so that one such pair sits at u = 0, as (0.0, y) and (-0.0, y), with the principal point
    shifted by as much.  -> (uv, K, number of pairs planted)."""
    uv = fr.uv.copy()
    rows = np.nonzero((fr.src_point >= 0) & ~fr.is_outlier)[0]
    owner = db.model_of[fr.src_point[rows]]
    pairs = []
    for a_i, a in enumerate(fr.visible):
        for b in fr.visible[a_i + 1:]:
            ra, rb = rows[owner == a], rows[owner == b]
            if not len(ra) or not len(rb):
                continue
            d = np.linalg.norm(uv[ra][:, None, :] - uv[rb][None, :, :], axis=2)
            i, j = np.unravel_index(np.argmin(d), d.shape)
            if d[i, j] < reach:
                pairs.append((float(d[i, j]), int(ra[i]), int(rb[j])))
    pairs = sorted(pairs)[:n_pairs]
    for _, i, j in pairs:
        uv[i] = uv[j] = ((uv[i].astype(np.float64) + uv[j]) / 2).astype(f32)
    Kx = K.copy()
    if pairs:
        _, i, j = pairs[int(rng.integers(0, len(pairs)))]
        u0 = uv[i, 0]
        uv[:, 0] -= u0
        Kx[2] -= u0
        uv[i, 0], uv[j, 0] = f32(0.0), f32(-0.0)
    return uv, Kx, len(pairs)


def frame_scene(name):
    """-> (db, frame, uv, K): the frames the FILTER tests run through the frame paths."""
    rng = np.random.default_rng([ord(ch) for ch in name])
    if name == "duplicates":          # <= 2 048 accepted matches: group_kernel's LDS hash of the representatives
        db = synth.make_db(12, 2000, seed=61)
        fr = synth.make_frame(db, n_vis=8, seed=62, Q=2500, pts_per_obj=90)
    elif name == "duplicates_big":    # > 2 048 accepted matches: the representative scan past the LDS copies
        db = synth.make_db(12, 3000)
        fr = synth.make_frame(db, n_vis=10, seed=63, Q=9000, pts_per_obj=300)
    elif name == "slots":             # > 256 object slots after POSE (FL_SLOTS)
        db = synth.make_db(80, 400, seed=5)
        fr = synth.make_frame(db, n_vis=72, seed=64, Q=6000, pts_per_obj=60)
    elif name == "pose2_none":        # 8 clean matches per object: POSE finds them, POSE2 (needs more than 8) nothing
        db = synth.make_db(12, 2000, seed=65)
        fr = synth.make_frame(db, n_vis=3, seed=66, pts_per_obj=8, outlier_frac=0.0, pix_noise=0.2)
    else:
        raise KeyError(name)
    if name.startswith("duplicates"):
        uv, Kx, n = plant_duplicates(db, fr, rng)
        assert n >= 2, n
        return db, fr, uv, Kx
    return db, fr, fr.uv, K.copy()
