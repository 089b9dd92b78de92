"""Model rows from a Kinect view, in numpy float32: what mh_view_rows_dev must write (the rules above mh_view_spec in
include/moped_hip.h; DEPTHMAP_PROP_CPU.hpp:103-131, DEPTH_VERIFY_CPU.hpp:167-170, TransformMatrix in moped.hpp:175-194,
MATCH_ANN_CPU.hpp:165).

Per keypoint of the list, in list order, the first failing test decides: 1 pixel, 2 depth valid, 3 fill distance, 4 roi,
(5 model coordinates), 6 box, 7 duplicate, 8 limit.  stats = [seen, dropped by 1, 2, 3, 4, 6, 7, 8].  Every operation is
one float32 rounding, in the order written."""
import numpy as np

import planar_ref

F = np.float32
KEEP, PIXEL, DEPTH, FILL, ROI, BOX, DUP, LIMIT = range(8)   # a keypoint's verdict = its stats word (KEEP: none)


def tm_from_pose(pose):
    """TransformMatrix::init (moped.hpp:175-182): -> (r [9] row-major, t [3]) float32."""
    q0, q1, q2, q3 = (F(v) for v in pose[:4])
    two, one = F(2), F(1)
    r = np.array([
        (one - (two * q1) * q1) - (two * q2) * q2, (two * q0) * q1 - (two * q3) * q2, (two * q0) * q2 + (two * q3) * q1,
        (two * q0) * q1 + (two * q3) * q2, (one - (two * q0) * q0) - (two * q2) * q2, (two * q1) * q2 - (two * q3) * q0,
        (two * q0) * q2 - (two * q3) * q1, (two * q1) * q2 + (two * q3) * q0, (one - (two * q0) * q0) - (two * q1) * q1],
        np.float32)
    assert r.dtype == np.float32
    return r, np.asarray(pose[4:7], np.float32)


def apply_inv(r, t, p):
    """TransformMatrix::inverseTransform: R^T (p - t), [n,3] float32 -> [n,3] float32."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
        out = np.stack([(d0 * r[0] + d1 * r[3]) + d2 * r[6], (d0 * r[1] + d1 * r[4]) + d2 * r[7],
                        (d0 * r[2] + d1 * r[5]) + d2 * r[8]], 1)
    assert out.dtype == np.float32
    return out


def apply_inv_fused(r, t, p):
    """The same with its multiply-adds fused, fma(d2, r6, fma(d1, r3, d0 r0)): what a build that contracts would
    compute.  (float64 holds a float32 product exactly; the one extra rounding of the sum to 53 bits is far below the
    float32 bit this is compared on.)"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    d = [(p[:, k] - t[k]).astype(np.float64) for k in range(3)]
    R = r.astype(np.float64)
    cols = []
    for c in range(3):
        acc = (d[0] * R[c]).astype(np.float32).astype(np.float64)
        acc = (d[1] * R[3 + c] + acc).astype(np.float32).astype(np.float64)
        cols.append((d[2] * R[6 + c] + acc).astype(np.float32))
    return np.stack(cols, 1)


def accepted(idx, d1, d2, ratio):
    """MATCH's verdict: idx >= 0 and d1 / d2 < ratio on float32 squared distances (MATCH_ANN_CPU.hpp:165)."""
    with np.errstate(all="ignore"):
        return (np.asarray(idx) >= 0) & (np.asarray(d1, np.float32) / np.asarray(d2, np.float32) < F(ratio))


def verdicts(xy, n, depth, fill=None, pose=None, roi=None, box=None, max_fill_distance=-1.0, merge_ratio=0.0,
             merge_dist=-1.0, dup=None):
    """-> (why [n] in KEEP .. DUP, xyz [n,3] model coordinates where they were computed, else 0).  depth [h,w,4],
    fill [h,w] or None.  dup: dict(idx, d1, d2, model_of, xyz, model) -- MATCH's answer per keypoint and the store."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    n = max(0, min(int(n), len(xy)))
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape[:2]
    r, t = tm_from_pose(pose if pose is not None else (0, 0, 0, 1, 0, 0, 0))
    roi = None if roi is None or not np.any(np.asarray(roi, np.float32)) else np.asarray(roi, np.float32)
    box = None if box is None or not np.any(np.asarray(box, np.float32)) else np.asarray(box, np.float32)
    dup_on = dup is not None and F(merge_ratio) > 0 and F(merge_dist) >= 0
    far2 = F(merge_dist) * F(merge_dist)
    why = np.zeros(n, np.int32)
    xyz = np.zeros((n, 3), np.float32)
    for i in range(n):
        u, v = xy[i]
        if not (u > F(-1) and u < F(w) and v > F(-1) and v < F(h)):   # NaN and +-inf fail
            why[i] = PIXEL
            continue
        ix, iy = int(u), int(v)   # truncation: -0.5 -> 0
        m = depth[iy, ix]
        if not m[3] >= 0:
            why[i] = DEPTH
            continue
        if fill is not None and F(max_fill_distance) >= 0 and not fill[iy, ix] <= F(max_fill_distance):
            why[i] = FILL
            continue
        if roi is not None and not (u >= roi[0] and u < roi[2] and v >= roi[1] and v < roi[3]):
            why[i] = ROI
            continue
        X = apply_inv(r, t, m[:3])[0]
        xyz[i] = X
        if box is not None and not (np.all(X >= box[:3]) and np.all(X <= box[3:])):
            why[i] = BOX
            continue
        if dup_on:
            j = int(dup["idx"][i])
            if accepted(j, dup["d1"][i], dup["d2"][i], merge_ratio) and j < len(dup["model_of"]) and dup["model_of"][j] == dup["model"]:
                with np.errstate(all="ignore"):
                    dx, dy, dz = X - np.asarray(dup["xyz"][j], np.float32)
                    d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == np.float32
                if d2 <= far2:
                    why[i] = DUP
    return why, xyz


def rows(desc, xy, n, depth, fill=None, pose=None, roi=None, box=None, max_fill_distance=-1.0, max_rows=0, out_cap=None,
         merge_ratio=0.0, merge_dist=-1.0, dup=None, old_xyz=None):
    """-> (desc [k,128], xyz [k,3], bbox [6], stats [8], kept indices).  old_xyz: the rows the model has already (an
    append): the box is the whole model's."""
    desc = np.asarray(desc, np.float32).reshape(-1, 128)
    why, xyz = verdicts(xy, n, depth, fill, pose, roi, box, max_fill_distance, merge_ratio, merge_dist, dup)
    idx = np.nonzero(why == KEEP)[0]
    limit = len(idx)
    if max_rows > 0:
        limit = min(limit, max_rows)
    if out_cap is not None:
        limit = min(limit, out_cap)
    stats = np.zeros(8, np.int32)
    stats[0] = len(why)
    for k in range(PIXEL, DUP + 1):
        stats[k] = np.count_nonzero(why == k)
    stats[LIMIT] = len(idx) - limit
    idx = idx[:limit]
    out = xyz[idx]
    assert limit + stats[1:].sum() == stats[0]
    whole = out if old_xyz is None else np.concatenate([np.asarray(old_xyz, np.float32).reshape(-1, 3), out])
    return desc[idx].copy(), out, planar_ref.bbox(whole), stats, idx


def relief_map(w=640, h=480, K=(800.0, 800.0, 320.0, 240.0)):
    """The relief the tests teach from (K: synth.K_DEFAULT): z = 0.8 + 0.1 sin(u / 40) cos(v / 55) at every pixel (u, v) = (column, row),
    x = (u - cx) / fx z, y = (v - cy) / fy z, valid = 1; float32 [h,w,4]."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = 0.8 + 0.1 * np.sin(u / 40.0) * np.cos(v / 55.0)
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z, np.ones_like(z)], 2).astype(np.float32)


def plane_map(z=0.8, w=640, h=480, K=(800.0, 800.0, 320.0, 240.0)):
    """The plane at depth z, as planar_ref.coords(form 1) at the integer pixels."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    xyz = planar_ref.coords(np.stack([u.ravel(), v.ravel()], 1), 1, K=K, z=z).reshape(h, w, 3)
    return np.concatenate([xyz, np.ones((h, w, 1), np.float32)], 2)


def trap_pose():
    """The pose of the rounding trap: q = normalise(0.12, -0.2, 0.31, 0.92), t = (0.03, -0.02, 0.8)."""
    q = np.array([0.12, -0.2, 0.31, 0.92], np.float64)
    q /= np.linalg.norm(q)
    return np.concatenate([q, [0.03, -0.02, 0.8]]).astype(np.float32)
