"""tests/view_model_ref.py on hand-worked cases: every rule of a Kinect view's selection at its boundary, and the
liveness of what the GPU tests lean on -- that a fused inverse transform would show, and that the bundled frames
populate all three classes of the duplicate test.  No GPU."""
import os

import numpy as np
import pytest

import planar_ref
import view_model_ref as ref
from moped_amd import synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
W, H = 8, 6
f = np.float32
nxt = lambda v, to: np.nextafter(f(v), f(to))


def small_map():
    """8 x 6: the point of pixel (ix, iy) is (ix, iy, 1) -- a keypoint's x, y say which pixel it read."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.stack([u, v, np.ones_like(u), np.ones_like(u)], 2)


def why_of(xy, depth, **kw):
    return list(ref.verdicts(np.array(xy, np.float32), len(xy), depth, **kw)[0])


def test_pixel_rule_truncates_and_never_clamps():
    depth = small_map()
    xy = [(-0.5, 0.0), (-1.0, 0.0), (W - 0.5, 0.0), (W, 0.0), (np.nan, 0.0), (np.inf, 0.0), (-np.inf, 0.0),
          (0.0, -0.5), (0.0, -1.0), (0.0, H - 0.5), (0.0, H), (0.0, np.nan), (nxt(-1.0, 0), nxt(H, 0)), (nxt(W, 0), 2.9)]
    why, xyz = ref.verdicts(np.array(xy, np.float32), len(xy), depth)
    P, K = ref.PIXEL, ref.KEEP
    assert list(why) == [K, P, K, P, P, P, P, K, P, K, P, P, K, K]
    # which pixel was read: -0.5 -> 0, w - 0.5 -> w - 1, just above -1 -> 0, just below h -> h - 1
    assert xyz[0].tolist() == [0, 0, 1] and xyz[2].tolist() == [W - 1, 0, 1] and xyz[7].tolist() == [0, 0, 1]
    assert xyz[9].tolist() == [0, H - 1, 1] and xyz[12].tolist() == [0, H - 1, 1] and xyz[13].tolist() == [W - 1, 2, 1]


def test_depth_valid_word_and_fill_distance_at_the_limit():
    depth = small_map()
    depth[0, 0, 3] = -0.0      # >= 0 holds
    depth[0, 1, 3] = 0.0
    depth[0, 2, 3] = np.nan
    depth[0, 3, 3] = -1.0
    depth[0, 4, 3] = nxt(0.0, -1)   # the largest negative denormal
    xy = [(0.5, 0.5), (1.5, 0.5), (2.5, 0.5), (3.5, 0.5), (4.5, 0.5), (5.5, 0.5)]
    D, K, FL = ref.DEPTH, ref.KEEP, ref.FILL
    assert why_of(xy, depth) == [K, K, D, D, D, K]
    fill = np.zeros((H, W), np.float32)
    fill[0, 0], fill[0, 1], fill[0, 5] = 3.0, nxt(3.0, 4), np.nan
    fill[0, 2] = 100.0   # (its depth is invalid: rule 2 decides first)
    assert why_of(xy, depth, fill=fill, max_fill_distance=3.0) == [K, FL, D, D, D, FL]
    assert why_of(xy, depth, fill=fill, max_fill_distance=-1.0) == [K, K, D, D, D, K]   # < 0: off, NaN and all
    assert why_of(xy, depth, fill=fill, max_fill_distance=0.0) == [FL, FL, D, D, D, FL]


def test_roi_and_box_edges_and_their_order():
    depth = small_map()
    roi = (1.25, 1.5, 4.75, 3.0)
    xy = [(1.25, 1.5), (4.75, 2.0), (nxt(4.75, 0), 2.0), (nxt(1.25, 0), 2.0), (2.0, 3.0), (2.0, nxt(3.0, 0)), (2.0, 1.5)]
    R, K, B = ref.ROI, ref.KEEP, ref.BOX
    assert why_of(xy, depth, roi=roi) == [K, R, K, R, R, K, K]
    assert why_of(xy, depth, roi=(0, 0, 0, 0)) == [K] * 7
    # box on X_model = the pixel's point under the identity pose: closed on both sides
    box = (1.0, 1.0, 1.0, 4.0, 2.0, 1.0)
    pts = [(1.0, 1.0), (4.9, 2.9), (0.9, 1.0), (5.0, 1.0), (2.0, 0.5), (2.0, 3.0)]
    assert why_of(pts, depth, box=box) == [K, K, B, B, B, B]
    assert why_of(pts, depth, box=(0,) * 6) == [K] * 6
    # a NaN coordinate: kept without a box, dropped with one; roi decides before the box
    depth[1, 1, 0] = np.nan
    assert why_of([(1.0, 1.0)], depth) == [K] and why_of([(1.0, 1.0)], depth, box=box) == [B]
    assert why_of([(0.9, 1.0)], depth, box=box, roi=(1.0, 0.0, 9.0, 9.0)) == [R]
    # the box is taken in the model frame: t moves the point out of it
    assert why_of([(1.0, 1.0)], small_map(), box=box, pose=(0, 0, 0, 1, 0.5, 0, 0)) == [B]


def test_duplicate_needs_all_three_and_the_distance_is_closed():
    depth = small_map()
    xy = [(2.0, 2.0)] * 6
    md = f(0.25)
    edge = f(2.0) - md   # (2 - 0.25 and 0.25^2 are exact: the squared distance is exactly merge_dist^2)
    store_xyz = np.array([[edge, 2, 1], [nxt(edge, 0), 2, 1], [2, 2, 1], [2, 2, 1]], np.float32)
    dup = dict(idx=[0, 1, 2, 3, -1, 2], d1=[0.1, 0.1, 0.1, 0.1, 0.1, 0.8], d2=[1.0] * 6, model_of=[5, 5, 5, 4], xyz=store_xyz,
               model=5)
    K, D = ref.KEEP, ref.DUP
    #                 on the edge  beyond  same point  other model  no neighbour  ratio fails (0.8 < 0.8 is false)
    assert why_of(xy, depth, dup=dup, merge_ratio=0.8, merge_dist=float(md)) == [D, K, D, K, K, K]
    assert why_of(xy, depth, dup=dup, merge_ratio=0.0, merge_dist=float(md)) == [K] * 6    # off
    assert why_of(xy, depth, dup=dup, merge_ratio=0.8, merge_dist=-1.0) == [K] * 6         # off
    assert why_of(xy, depth, dup=dup, merge_ratio=0.8, merge_dist=0.0) == [K, K, D, K, K, K]
    assert bool(ref.accepted(2, nxt(0.8, 0), 1.0, 0.8)) and not bool(ref.accepted(2, 0.8, 1.0, 0.8))
    assert not bool(ref.accepted(2, 0.0, 0.0, 0.8))   # 0 / 0


def test_limit_statistics_and_the_box_of_an_append():
    depth = small_map()
    depth[5, :, 3] = -1.0
    rng = np.random.default_rng(3)
    xy = rng.uniform(-1.5, 8.5, (200, 2)).astype(np.float32)
    desc = rng.normal(size=(200, 128)).astype(np.float32)
    d, x, bb, st, idx = ref.rows(desc, xy, 200, depth, roi=(0.0, 0.0, 7.0, 6.0), max_rows=40)
    assert len(idx) == 40 and st[0] == 200 and st[ref.LIMIT] > 0 and st[ref.PIXEL] > 0 and st[ref.DEPTH] > 0 and st[ref.ROI] > 0
    assert 40 + st[1:].sum() == 200 and np.array_equal(d, desc[idx]) and list(idx) == sorted(idx)
    d2, x2, bb2, st2, idx2 = ref.rows(desc, xy, 200, depth, roi=(0.0, 0.0, 7.0, 6.0), max_rows=40, out_cap=25)
    assert list(idx2) == list(idx[:25]) and st2[ref.LIMIT] == st[ref.LIMIT] + 15
    old = np.array([[-3.0, 0.5, 1.0], [2.0, 9.0, 0.25]], np.float32)
    _, x3, bb3, _, _ = ref.rows(desc, xy, 200, depth, roi=(0.0, 0.0, 7.0, 6.0), max_rows=40, old_xyz=old)
    assert np.array_equal(x3, x) and np.array_equal(bb3, planar_ref.bbox(np.concatenate([old, x])))
    assert bb3[0] == -3.0 and bb3[4] == 9.0 and bb3[2] == 0.25 and bb3[3] == bb[3] and bb3[5] == 1.0
    assert np.array_equal(ref.rows(desc, xy, 0, depth)[2], np.array([10E10] * 3 + [-10E10] * 3, np.float32))


def truncated_points(xy, depth):
    ix, iy = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    return depth[iy, ix, :3]


def test_rounding_trap_is_live():
    """The inverse transform with its multiply-adds fused differs in at least one bit for hundreds of frame 0's 586
    keypoints over the relief under the trap pose: a build that contracts cannot pass the bit comparison."""
    xy = GOLD["xy0"]
    assert len(xy) == 586 and xy.min() >= 0
    pts = truncated_points(xy, ref.relief_map(K=tuple(synth.K_DEFAULT)))
    r, t = ref.tm_from_pose(ref.trap_pose())
    exact, fused = ref.apply_inv(r, t, pts), ref.apply_inv_fused(r, t, pts)
    differ = np.any(exact.view(np.uint32) != fused.view(np.uint32), axis=1)
    print("keypoints whose fused inverse transform differs:", int(differ.sum()), "of", len(xy))
    assert differ.sum() >= 100
    assert np.abs(exact.astype(np.float64) - fused).max() < 1e-6   # ... in the last bits only
    # the rotation is one: R R^T = 1 to float32
    R = r.reshape(3, 3).astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6


def test_duplicate_classes_are_live_on_the_bundled_frames():
    """desc3 against desc0 at ratio 0.8, both frames on the plane z = 0.8 at their truncated pixels, merge_dist 2 mm: in
    float64 all three classes -- duplicate, accepted but farther, not accepted -- hold well over 10 keypoints."""
    d0 = GOLD["desc0"].astype(np.float64)
    d3 = GOLD["desc3"].astype(np.float64)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    d3 /= np.linalg.norm(d3, axis=1, keepdims=True)
    dist = ((d3 * d3).sum(1)[:, None] - 2.0 * d3 @ d0.T) + (d0 * d0).sum(1)[None, :]
    order = np.argsort(dist, axis=1)[:, :2]
    b1 = dist[np.arange(len(d3)), order[:, 0]]
    b2 = dist[np.arange(len(d3)), order[:, 1]]
    acc = b1 / b2 < 0.8
    plane = ref.plane_map(0.8, K=tuple(synth.K_DEFAULT))
    p3 = truncated_points(GOLD["xy3"], plane).astype(np.float64)
    p0 = truncated_points(GOLD["xy0"], plane).astype(np.float64)
    near = ((p3 - p0[order[:, 0]]) ** 2).sum(1) <= 0.002 ** 2
    classes = (int((acc & near).sum()), int((acc & ~near).sum()), int((~acc).sum()))
    print("duplicates, accepted but farther than 2 mm, not accepted:", classes)
    assert min(classes) >= 10 and sum(classes) == 599
