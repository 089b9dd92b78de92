"""FILTER_PROJECTION_DEPTH_CPU::process restated line by line
(moped3d/libmoped/src/filter/FILTER_PROJECTION_DEPTH_CPU.hpp:140-329, `DEPTH.hpp` below), and the generator of the cases
the device is compared on.

The class cannot be built against the oracle's stand-ins yet (it needs util.hpp), so this restatement is what the
device's mh_filter_depth is held to; test_filter_depth_ref_cpu.py ties it to the pinned FILTER_PROJECTION_CPU
(filter_cases.oracle) wherever the two classes coincide.  Float is float (moped.hpp:76): every value the reference
holds in a Float is an np.float32 here, every expression with a double literal (`1./(e + 1.)`, `1.0 - 1.0/(1.0 + term)`)
an np.float64.  numpy does not fuse multiply-adds and evaluates elementwise float32 expressions like the scalar ones, so
an array expression below IS the reference's scalar expression for every element; the ordered `Float += double` chains
are Python loops.  The projection error comes from orclib.project (the pinned project())."""
import ctypes

import numpy as np

import orclib
from moped_amd import synth

f32, f64 = np.float32, np.float64
_ONE, _TWO = f32(1), f32(2)


def _round32(x):
    """(Float) of a double."""
    return ctypes.c_float(x).value


def transform_matrix(pose7):
    """TransformMatrix::init (moped3d/libmoped/include/moped.hpp:180-187): p[r][c] rows, translation."""
    q0, q1, q2, q3 = (f32(v) for v in pose7[:4])
    r = np.array([[_ONE - _TWO * q1 * q1 - _TWO * q2 * q2, _TWO * q0 * q1 - _TWO * q3 * q2, _TWO * q0 * q2 + _TWO * q3 * q1],
                  [_TWO * q0 * q1 + _TWO * q3 * q2, _ONE - _TWO * q0 * q0 - _TWO * q2 * q2, _TWO * q1 * q2 - _TWO * q3 * q0],
                  [_TWO * q0 * q2 - _TWO * q3 * q1, _TWO * q1 * q2 + _TWO * q3 * q0, _ONE - _TWO * q0 * q0 - _TWO * q1 * q1]], f32)
    return r, np.asarray(pose7[4:7], f32)


def transform(tm, p):
    """TransformMatrix::transform (moped.hpp:188-193) of the rows of p."""
    r, t = tm
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([x * r[i, 0] + y * r[i, 1] + z * r[i, 2] + t[i] for i in range(3)], 1)


def inverse_transform(tm, p):
    """TransformMatrix::inverseTransform (moped.hpp:195-205) of the rows of p."""
    r, t = tm
    d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
    return np.stack([d0 * r[0, i] + d1 * r[1, i] + d2 * r[2, i] for i in range(3)], 1)


def _int_of(v):
    """(int) of a Float where the reference defines it; outside int (undefined there): the nearest int, NaN: 0 -- as the
    device has it."""
    v = float(v)
    if v != v:
        return 0
    return int(min(max(v, -2147483648.0), 2147483647.0))


def _chain(acc, terms):
    """`Float acc; acc += double` over terms in order; adding 0. leaves a float unchanged, so zeros are skipped."""
    acc = float(acc)
    for t in terms:
        if t != 0.0:            # (a NaN term is not 0.0)
            acc = _round32(acc + t)
    return f32(acc)


def point_outcomes(pose7, pts, depth_img, fill_img, depth_K, depth_cam, depth_fraction):
    """DEPTH.hpp:213-255 for one object over its model's test points `pts` [n, 3] in list order ->
    (outcome [n]: 0 off the image, 1 filled, 2 the sensor in front, 3 a term was added; term [n] float32 (outcome 3),
    contribution [n] float64).  The (int) of a coordinate that is NaN, infinite or outside int's range is undefined in
    the reference: such a point is off the image."""
    n = len(pts)
    out = np.zeros(n, np.int32)
    term = np.zeros(n, f32)
    contrib = np.zeros(n, f64)
    if n == 0:
        return out, term, contrib
    h, w = depth_img.shape[:2]
    K = np.asarray(depth_K, f32)
    with np.errstate(all="ignore"):
        p3 = transform(transform_matrix(pose7), np.asarray(pts, f32))            # :220
        p3 = inverse_transform(transform_matrix(depth_cam), p3)                    # :221
        pu = p3[:, 0] / p3[:, 2] * K[0] + K[2]                                     # :223
        pv = p3[:, 1] / p3[:, 2] * K[1] + K[3]                                     # :224
        ok = (pu >= f32(-2147483648.0)) & (pu < f32(2147483648.0)) & (pv >= f32(-2147483648.0)) & (pv < f32(2147483648.0))
        ix = np.where(ok, pu, 0).astype(np.int64)                                  # :226 (int): toward zero
        iy = np.where(ok, pv, 0).astype(np.int64)
        on = ok & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)                      # :229
        ix, iy = np.where(on, ix, 0), np.where(on, iy, 0)
        distance = fill_img[iy, ix] if fill_img is not None else np.zeros(n, f32)  # :233 (no map: every pixel measured)
        filled = on & (distance > 0)                                               # :234
        used = on & ~filled                                                        # :237
        kinect = depth_img[iy, ix, 2].astype(f32)                                  # :239
        putative = p3[:, 2]                                                        # :240
        front = used & (kinect < putative)                                         # :244
        add = used & ~front
        cauchy = f32(depth_fraction) * kinect                                      # :248
        t = (putative - kinect) / cauchy                                           # :250
        t = t * t                                                                  # :251
        c = 1.0 - (1.0 / (1.0 + t.astype(f64)))                                    # :254
    out[filled] = 1
    out[front] = 2
    out[add] = 3
    term[add] = t[add]
    contrib[add] = c[add]
    return out, term, contrib


def filter_projection_depth(uv, xyz, model_off, obj_model, obj_pose, K, cam, min_points, feature_distance, min_score,
                            pts_xyz, pts_off, depth_img, fill_img, depth_K, depth_cam, plausible_sq_distance, depth_fraction,
                            min_keypoint_fraction, detail=None):
    """DEPTH.hpp:140-329.  uv / xyz / model_off: matches[m] (one image); obj_model sorted ascending = the (model, list)
    order of :182-183; pts_xyz / pts_off: TestPoints.  -> (score [n_obj] = object->score, keep, order, clusters,
    incorrect_score [n_obj], used [n_obj], plausible [n_obj]) as Context.filter_depth returns them.  detail (a list):
    gets every object's outcome array."""
    n_models, n_obj = len(model_off) - 1, len(obj_model)
    fd, psd = f32(feature_distance), f32(plausible_sq_distance)
    score_out = np.zeros(n_obj, f32)
    inc = np.zeros(n_obj, f32)
    used_out = np.zeros(n_obj, np.int32)
    plaus = np.zeros(n_obj, np.int32)
    best = {}                                        # :175 bestPoints: key -> [score, object]
    keys = [(float(u) + 0.0, float(v) + 0.0) for u, v in np.asarray(uv, f32)]   # (std::map compares floats: -0.0 is 0.0)
    for m in range(n_models):                        # :182
        lo, hi = int(model_off[m]), int(model_off[m + 1])
        pts = np.asarray(pts_xyz, f32).reshape(-1, 3)[int(pts_off[m]):int(pts_off[m + 1])]
        for o in range(n_obj):                       # :183
            if obj_model[o] != m:
                continue
            with np.errstate(all="ignore"):
                p = orclib.project(obj_pose[o], xyz[lo:hi], K, cam) - np.asarray(uv[lo:hi], f32)    # :195-196
                e = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]                                       # :197
                inl = e < fd                                                                    # :198
                score = _chain(0.0, (1. / (e[inl].astype(f64) + 1.)).tolist())                  # :200
            cluster_size = int((e < psd).sum())                                                 # :202-204
            out, _, contrib = point_outcomes(obj_pose[o], pts, depth_img, fill_img, depth_K, depth_cam,
                                                  depth_fraction) if len(pts) else (np.zeros(0, np.int32), None, np.zeros(0))
            IS = _chain(0.0, contrib.tolist())                                                  # :208, :254
            used = int((out >= 2).sum())                                                        # :237
            lim = f32(min_keypoint_fraction) * f32(len(pts))                                    # :260
            if used <= _int_of(lim):
                IS = f32(0)                                                                     # :261
            else:
                with np.errstate(all="ignore"):
                    IS = IS * (f32(cluster_size) / f32(used))                                   # :266
            with np.errstate(all="ignore"):
                score_out[o] = score - IS                                                       # :270
            inc[o], used_out[o], plaus[o] = IS, used, cluster_size
            if detail is not None:
                detail.append(out)
            for i in np.nonzero(inl)[0]:                                                        # :274-286
                pt = best.setdefault(keys[lo + i], [f32(0), None])
                if pt[0] < score:
                    pt[0], pt[1] = score, o
    new = {o: [] for o in range(n_obj)}              # :292-300
    for m in range(n_models):
        for i in range(int(model_off[m]), int(model_off[m + 1])):
            pt = best.get(keys[i])
            if pt is not None and pt[1] is not None and obj_model[pt[1]] == m:
                new[pt[1]].append(i - int(model_off[m]))
    keep = np.zeros(n_obj, bool)
    order, clusters = [], []
    ms = f32(min_score)
    for m in range(n_models):                        # :305-326
        for o in range(n_obj):
            if obj_model[o] != m:
                continue
            if len(new[o]) < min_points or score_out[o] < ms:                                   # :309
                continue
            keep[o] = True
            order.append(o)
            clusters.append(np.array(new[o], np.int32))
    return score_out, keep, np.array(order, np.int32), clusters, inc, used_out, plaus


# ------------------------------------------------------------------------------------------------- generated cases
W, H = 40, 30                                        # non-square: a swapped stride shows
DEPTH_K = np.array([30.0, 28.0, 20.0, 15.0], f32)
DEPTH_CAM = np.concatenate([[0.0, np.sin(0.02), 0.0, np.cos(0.02)], [0.03, -0.02, 0.01]]).astype(f32)   # not the identity
N_PTS = (0, 1, 63, 64, 65, 129, 300)                 # the chunk boundaries of the chain
N_OBJ = (1, 65, 129, 257)                            # a second wavefront, the FILTER_GRID stride, FL_SLOTS
N_MATCH = (0, 1, 63, 64, 65, 130)


def _surface(truth):
    """Depth (in the depth camera) of the model plane z = 0 under `truth`, per pixel (float64 geometry: it only places
    the map's values); pixels the plane does not reach: the pose's own depth."""
    g = np.linspace(-0.9, 0.9, 241)
    p = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    p = np.concatenate([p, np.zeros((len(p), 1))], 1)
    w = p @ synth.quat_to_R(truth[:4]).T + truth[4:].astype(f64)
    c = (w - DEPTH_CAM[4:].astype(f64)) @ synth.quat_to_R(DEPTH_CAM[:4])
    surf = np.full((H, W), float(c[:, 2].mean()))
    ok = c[:, 2] > 0.05
    u = (c[ok, 0] / c[ok, 2] * DEPTH_K[0] + DEPTH_K[2]).astype(int)
    v = (c[ok, 1] / c[ok, 2] * DEPTH_K[1] + DEPTH_K[3]).astype(int)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    surf[v[inside], u[inside]] = c[ok, 2][inside]
    return surf


def make_depth_case(rng, n_obj=None, n_pts=None):
    """-> dict for filter_projection_depth / Context.filter_depth: the fields of filter_cases.make_case (one image) plus
    pts_xyz, pts_off, depth_img [H, W, 4], fill_img [H, W], depth_K, depth_cam, psd, depth_fraction, min_kp_fraction.
    All models share one true pose; the map is that pose's surface, per pixel consistent (a few per cent behind), far
    behind, in front, a hole (z < 0) or filled, with a NaN reading or two in some maps.  n_obj / n_pts: the object count / one model's test-point count."""
    K, cam0 = synth.K_DEFAULT, synth.CAM_IDENTITY
    n_models = int(rng.integers(1, 5))
    sizes = rng.choice(N_MATCH, n_models, p=[0.1, 0.1, 0.2, 0.2, 0.2, 0.2])
    model_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    M = int(model_off[-1])
    q = np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.3), 1.0])
    truth = np.concatenate([q / np.linalg.norm(q), [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.0)]]).astype(f32)
    xyz = np.concatenate([rng.uniform(-0.08, 0.08, (M, 2)), rng.uniform(-0.01, 0.01, (M, 1))], 1).astype(f32)
    uv = (orclib.project(truth, xyz, K, cam0) + rng.normal(0, rng.choice([0.3, 3.0]), (M, 2))).astype(f32) if M else np.zeros((0, 2), f32)
    if M > 1 and rng.random() < 0.5:                 # one keypoint in two lists: ownership by the projection score
        for _ in range(int(rng.integers(1, 6))):
            a, b = rng.integers(0, M, 2)
            uv[a] = uv[b]
    # test points: on the model plane, wide enough that some leave the 40 x 30 map; coordinates in (-1, 0) and exactly
    # on width / height are planted below through the depth camera's own arithmetic
    counts = rng.choice(N_PTS, n_models)
    if n_pts is not None:
        counts[int(rng.integers(0, n_models))] = n_pts
    pts_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    P = int(pts_off[-1])
    pts = np.concatenate([rng.uniform(-0.55, 0.55, (P, 2)), rng.uniform(-0.001, 0.001, (P, 1))], 1).astype(f32)
    # the map
    surf = _surface(truth)
    mode = rng.choice(["agree", "refute", "mixed"], p=[0.35, 0.4, 0.25])
    pr = dict(agree=[0.55, 0.06, 0.1], refute=[0.1, 0.46, 0.14], mixed=[0.3, 0.24, 0.16])[mode]   # consistent, behind, in front
    cat = rng.choice(5, (H, W), p=pr + [0.04, 1.0 - sum(pr) - 0.04])   # 3: hole, 4: filled
    factor = np.select([cat == 0, cat == 1, cat == 2], [rng.uniform(1.003, 1.006, (H, W)), rng.uniform(1.5, 10.0, (H, W)),
                                                         rng.uniform(0.3, 0.9, (H, W))], 1.0)
    z = (surf * factor).astype(f32)
    z[cat == 3] = f32(-1.0)
    if rng.random() < 0.2:                           # a NaN reading or two (a used point on one makes the score NaN)
        for _ in range(int(rng.integers(1, 3))):
            z[int(rng.integers(0, H)), int(rng.integers(0, W))] = np.nan
    depth_img = np.zeros((H, W, 4), f32)
    depth_img[..., 0] = rng.normal(0, 1, (H, W))     # (x, y, norm: never read by the class)
    depth_img[..., 1] = rng.normal(0, 1, (H, W))
    depth_img[..., 2] = z
    depth_img[..., 3] = np.abs(z)
    fill_img = np.where(cat == 4, rng.uniform(0.5, 6.0, (H, W)), 0.0).astype(f32)
    if rng.random() < 0.1:
        fill_img = None                              # every pixel measured
    # objects, sorted by model
    if n_obj is None:
        n_obj = int(rng.choice(N_OBJ)) if rng.random() < 0.1 else int(rng.integers(1, 7))
    obj_model = np.sort(rng.integers(0, n_models, n_obj)).astype(np.int32)
    obj_pose = np.zeros((n_obj, 7), f32)
    for o in range(n_obj):
        r = rng.random()
        if r < 0.45:
            obj_pose[o] = truth
        elif r < 0.75:
            obj_pose[o] = truth + np.concatenate([np.zeros(4), rng.normal(0, 0.003, 3)]).astype(f32)
        elif r < 0.85:
            obj_pose[o] = np.concatenate([truth[:6], [-truth[6]]])                  # behind both cameras: finite coordinates
        elif r < 0.93:
            obj_pose[o] = np.concatenate([truth[:6], [truth[6] - rng.uniform(0.3, 0.5)]])   # in front of the surface
        else:
            obj_pose[o] = np.concatenate([synth.random_quat(rng), [0, 0, rng.uniform(0.4, 1.2)]])
    c = dict(uv=uv, xyz=xyz, model_off=model_off, obj_model=obj_model, obj_pose=obj_pose, K=K, cam=cam0,
             min_points=int(rng.integers(0, 4)), fd=float(rng.choice([4096.0, 64.0])),
             min_score=float(rng.choice([2.0, 3.0, 10.0, 0.0])), pts_xyz=pts, pts_off=pts_off, depth_img=depth_img,
             fill_img=fill_img, depth_K=DEPTH_K, depth_cam=DEPTH_CAM, psd=float(rng.choice([4096.0, 16.0, 1e6])),
             depth_fraction=float(rng.choice([0.5, 0.25, 0.1])), min_kp_fraction=float(rng.choice([0.0, 0.1, 0.5, 0.8, 2.0])))
    _plant_edges(rng, c)
    return c


def _plant_edges(rng, c):
    """Four test points of the first object's model moved so that, under that object's pose, a projected coordinate
    falls in (-1, 0) (inside: (int) truncates toward zero) or exactly on width / height (outside).  The place is found
    on a grid of steps along the model-space direction that moves the coordinate, evaluated in the class's own float32
    arithmetic; a target that no step meets leaves the point where it was."""
    if not len(c["obj_model"]):
        return
    m = int(c["obj_model"][0])
    lo, hi = int(c["pts_off"][m]), int(c["pts_off"][m + 1])
    if hi - lo < 4:
        return
    pose = c["obj_pose"][0]
    R, t = synth.quat_to_R(pose[:4]).astype(f64), pose[4:].astype(f64)
    Rd, td = synth.quat_to_R(DEPTH_CAM[:4]).astype(f64), DEPTH_CAM[4:].astype(f64)
    tmo, tmd = transform_matrix(pose), transform_matrix(DEPTH_CAM)
    rows = rng.choice(np.arange(lo, hi), 4, replace=False)
    for j, (axis, want) in zip(rows, [(0, -0.5), (1, -0.5), (0, float(W)), (1, float(H))]):
        other = rng.uniform(3, 25) if axis == 0 else rng.uniform(3, 35)
        px = (want, other) if axis == 0 else (other, want)
        zc = 0.8
        cpt = np.array([(px[0] - DEPTH_K[2]) / DEPTH_K[0] * zc, (px[1] - DEPTH_K[3]) / DEPTH_K[1] * zc, zc])
        model = ((cpt @ Rd.T + td) - t) @ R          # depth camera -> world -> model
        d = (np.eye(3)[axis] @ Rd.T) @ R

        def got(sv):                                 # the coordinate for every step in sv, in the class's arithmetic
            k = (model[None] + np.asarray(sv, f64)[:, None] * d[None]).astype(f32)
            with np.errstate(all="ignore"):
                p3 = inverse_transform(tmd, transform(tmo, k))
                return p3[:, axis] / p3[:, 2] * DEPTH_K[axis] + DEPTH_K[2 + axis], k

        sv = np.linspace(-0.05, 0.05, 2001)
        g, k = got(sv)
        if want < 0:
            hit = np.nonzero((g > -0.9) & (g < -0.1))[0]
        else:                                        # exactly on the edge: every float32 result about the crossing
            cross = np.nonzero((g[:-1] < want) & (g[1:] >= want))[0]
            if not len(cross):
                continue
            g, k = got(np.linspace(sv[cross[0]], sv[cross[0] + 1], 10001))
            hit = np.nonzero(g == f32(want))[0]
        if len(hit):
            c["pts_xyz"][j] = k[hit[0]]
