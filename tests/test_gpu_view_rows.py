"""mh_view_rows_dev / mh_view_rows_batch_dev: the selection kernel of the Kinect-view models on synthetic device arrays
against tests/view_model_ref.py.  Everything is compared on bits: the kept descriptors, the model coordinates, the count,
the bounding box, the statistics, and the sentinel in every row at and beyond the count.

The map is 64 x 48 with a block of holes, a row whose valid word is NaN and a fill-distance ramp.  The kernel walks a list
in chunks of 1024 keypoints, 16 wavefronts of 64 lanes: the list lengths sit on those seams.  Keypoints behind a list's
count would all be kept if they were read."""
import ctypes as C

import numpy as np
import pytest

import view_model_ref as ref
from moped_amd import capi

pytestmark = pytest.mark.gpu
CAP = 2304
W, H = 64, 48
SENT_BITS = 0x7FC0BEEF   # a NaN no computation here makes
POSE = ref.trap_pose()
f = np.float32
nxt = lambda v, to: np.nextafter(f(v), f(to))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_map(seed):
    rng = np.random.default_rng(seed)
    depth = np.concatenate([rng.uniform(-0.5, 1.5, (H, W, 3)), np.ones((H, W, 1))], 2).astype(np.float32)
    depth[10:20, 12:24, 3] = -1.0       # holes
    depth[30, :, 3] = np.nan            # a row that is neither valid nor invalid
    depth[40, 5, 3] = -0.0              # valid
    depth[41, 7, :3] = np.nan           # a measured pixel without coordinates
    fill = np.tile(np.arange(W, dtype=np.float32) * f(0.125), (H, 1))   # the ramp: 0 .. 7.875
    fill[3, :] = np.nan
    return depth, fill


@pytest.fixture(scope="module")
def dev():
    import torch
    c = capi.Context(0)
    rng = np.random.default_rng(0x71E)
    desc = rng.normal(size=(CAP, 128)).astype(np.float32)
    # keypoints over and around the map: some outside, some in the holes; behind any count: pixels that would be kept
    xy = rng.uniform(-2.0, 66.0, (CAP, 2)).astype(np.float32)
    xy[:, 1] = rng.uniform(-2.0, 50.0, CAP).astype(np.float32)
    depth, fill = make_map(0x3A9)
    d = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    env = dict(c=c, torch=torch, d=d, t=t, desc=desc, desc_d=t(desc), xy=xy, depth=depth, fill=fill, depth_d=t(depth), fill_d=t(fill))
    for a in (desc, xy, depth, fill):
        a.setflags(write=False)
    yield env
    c.close()


def poisoned(xy, n):
    """The list with every row behind the count replaced by a keypoint every rule would keep."""
    out = np.array(xy, np.float32)
    out[n:] = (33.5, 25.5)
    return out


def run(dev, xy, n, kw, cap=CAP, out_cap=CAP, desc_d=None, depth_d=None, fill_d=None, use_fill=True, pose=POSE, dup=None,
        w=W, h=H):
    """One launch -> (desc_out, xyz_out, n_out, bbox, stats) as numpy, outputs pre-filled with the sentinel."""
    c, torch, d, t = dev["c"], dev["torch"], dev["d"], dev["t"]
    xy_d = t(np.asarray(xy, np.float32))
    n_d = torch.tensor([n], dtype=torch.int32, device=d)
    od = torch.full((CAP, 128), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    ox = torch.full((CAP, 3), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    no = torch.full((1,), -7, dtype=torch.int32, device=d)
    bb = torch.zeros(6, dtype=torch.float32, device=d)
    st = torch.full((8,), -7, dtype=torch.int32, device=d)
    depth_d = dev["depth_d"] if depth_d is None else depth_d
    fill_d = dev["fill_d"] if fill_d is None else fill_d
    view = capi.make_view(depth_d.data_ptr(), fill_d.data_ptr() if use_fill else None, pose)
    keep = []
    dd = None
    if dup is not None:
        arrs = [t(np.asarray(dup[k], ty)) for k, ty in (("idx", np.int32), ("d1", np.float32), ("d2", np.float32),
                                                         ("model_of", np.int32), ("xyz", np.float32))]
        keep.append(arrs)
        dd = capi.mh_view_dup(*[a.data_ptr() for a in arrs], len(dup["model_of"]), dup["model"], dup["row_begin"], dup["row_end"])
    torch.cuda.synchronize()
    c.view_rows_dev((dev["desc_d"] if desc_d is None else desc_d).data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, view, w, h,
                    capi.make_view_spec(**kw), od.data_ptr(), ox.data_ptr(), out_cap, no.data_ptr(), bb.data_ptr(), st.data_ptr(),
                    dup=dd)
    c.synchronize()
    return od.cpu().numpy(), ox.cpu().numpy(), int(no.cpu()[0]), bb.cpu().numpy(), st.cpu().numpy()


def check(got, desc, xy, n, kw, depth, fill, cap=CAP, out_cap=CAP, pose=POSE, dup=None, what=""):
    od, ox, k, bb, st = got
    old = None if dup is None else np.asarray(dup["xyz"], np.float32)[dup["row_begin"]:dup["row_end"]]
    wd, wx, wb, ws, idx = ref.rows(desc[:cap], np.asarray(xy, np.float32)[:cap], min(n, cap), depth, fill, pose, out_cap=out_cap,
                                   dup=dup, old_xyz=old, **kw)
    assert k == len(idx), (what, k, len(idx))
    assert np.array_equal(st, ws), (what, st, ws)
    assert k + st[1:].sum() == st[0]
    assert np.array_equal(bits(od[:k]), bits(wd)), what
    assert np.array_equal(bits(ox[:k]), bits(wx)), what
    assert np.array_equal(bits(bb), bits(wb)), (what, bb, wb)
    assert np.all(bits(od[k:]) == SENT_BITS) and np.all(bits(ox[k:]) == SENT_BITS), what   # nothing written past the count
    return idx, ws


RULES = dict(roi=(4.0, 3.0, 60.0, 45.0), box=(-1.2, -1.0, -1.4, 1.0, 1.2, 0.9), max_fill_distance=6.5)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_every_rule_at_the_seams_of_the_compaction(dev, n):
    xy = poisoned(dev["xy"], n)
    idx, st = check(run(dev, xy, n, RULES), dev["desc"], xy, n, RULES, dev["depth"], dev["fill"], what=("rules", n))
    if n >= 1023:   # every counter is live
        assert len(idx) > 100 and all(st[k] > 5 for k in (ref.PIXEL, ref.DEPTH, ref.FILL, ref.ROI, ref.BOX))
    # no rule but the map's own: pixel and depth
    check(run(dev, xy, n, {}, use_fill=False), dev["desc"], xy, n, {}, dev["depth"], None, what=("bare", n))
    # a distance map without a limit is not read
    kw = dict(max_fill_distance=-1.0)
    check(run(dev, xy, n, kw), dev["desc"], xy, n, kw, dev["depth"], dev["fill"], what=("fill off", n))


def test_rule_boundaries(dev):
    depth, fill = dev["depth"], dev["fill"]
    pts = [(-0.5, 0.0), (-1.0, 0.0), (W - 0.5, 0.0), (W, 0.0), (np.nan, 1.0), (np.inf, 1.0), (-np.inf, 1.0), (1.0, np.nan),
           (0.0, -0.5), (0.0, -1.0), (0.0, H - 0.5), (0.0, H), (nxt(-1.0, 0), nxt(H, 0)), (nxt(W, 0), 2.9),
           (5.5, 40.5), (7.5, 41.5), (12.0, 10.0), (nxt(12.0, 0), 10.0), (24.0, 19.9), (5.0, 30.5), (5.0, 3.5)]
    xy = np.array(pts, np.float32)
    n = len(xy)
    idx, st = check(run(dev, xy, n, {}, cap=n, use_fill=False), dev["desc"], xy, n, {}, depth, None, cap=n, what="pixel + depth")
    # pixel: -1, w, h, NaN and +-inf in either coordinate; depth: (12, 10) in the holes, (5, 30.5) in the NaN row
    assert st[ref.PIXEL] == 8 and st[ref.DEPTH] == 2 and len(idx) == n - 10
    # the NaN point: kept without a box, dropped with one
    kw = dict(box=(-9.0, -9.0, -9.0, 9.0, 9.0, 9.0))
    idx2, st2 = check(run(dev, xy, n, kw, cap=n, use_fill=False, pose=None), dev["desc"], xy, n, kw, depth, None, cap=n, pose=None,
                      what="box + NaN")
    assert st2[ref.BOX] == 1 and len(idx2) == len(idx) - 1
    # fill distance exactly at the limit: the ramp holds x / 8, so 2.5 at x = 20; the NaN row of the distance map
    fx = np.array([(20.5, 5.5), (21.5, 5.5), (19.5, 5.5), (2.5, 3.5), (20.5, 3.5)], np.float32)
    kw = dict(max_fill_distance=2.5)
    idx, st = check(run(dev, fx, 5, kw, cap=5), dev["desc"], fx, 5, kw, depth, fill, cap=5, what="fill edge")
    assert list(idx) == [0, 2] and st[ref.FILL] == 3
    # roi half-open on the float coordinates
    roi = (10.25, 20.5, 30.75, 29.0)
    rx = np.array([(10.25, 20.5), (30.75, 25.0), (nxt(30.75, 0), 25.0), (nxt(10.25, 0), 25.0), (15.0, 29.0), (15.0, nxt(29.0, 0)),
                   (15.0, 20.5)], np.float32)
    kw = dict(roi=roi)
    idx, st = check(run(dev, rx, 7, kw, cap=7, use_fill=False), dev["desc"], rx, 7, kw, depth, None, cap=7, what="roi edges")
    assert list(idx) == [0, 2, 5, 6] and st[ref.ROI] == 3
    # box closed on both sides, on the very coordinates the kernel computes: the box is the point of keypoint 0
    X = ref.rows(dev["desc"], rx, 7, depth, None, POSE)[1]
    for k, want in ((0, True), (1, False)):
        b = np.concatenate([X[0], X[0]]).astype(np.float32)
        if not want:
            b[3] = nxt(b[3], -9)   # max x just below the point
        kw = dict(box=tuple(float(v) for v in b))
        idx, st = check(run(dev, rx, 7, kw, cap=7, use_fill=False), dev["desc"], rx, 7, kw, depth, None, cap=7, what=("box edge", k))
        assert (0 in idx) == want
    # nothing kept: the box is the reference's initial one (moped.cpp:107-108)
    kw = dict(roi=(1000.0, 1000.0, 1001.0, 1001.0))
    od, ox, k, bb, st = run(dev, rx, 7, kw, cap=7)
    assert k == 0 and st[ref.ROI] == 7 and np.array_equal(bits(bb), bits(np.array([10E10] * 3 + [-10E10] * 3, np.float32)))


def valid_list():
    """CAP keypoints every rule keeps (pixels with a measured point outside the holes)."""
    i = np.arange(CAP)
    return np.stack([f(0.25) + (i % 10).astype(np.float32), f(0.5) + ((i // 10) % 8).astype(np.float32)], 1).astype(np.float32)


def test_limits_cut_inside_a_chunk_and_at_its_end(dev):
    xy = valid_list()
    depth = dev["depth"]
    for max_rows in (1, 700, 1024, 1025, 2048, 2049, 5000):
        kw = dict(max_rows=max_rows)
        idx, st = check(run(dev, xy, 2049, kw, use_fill=False), dev["desc"], xy, 2049, kw, depth, None, what=("max_rows", max_rows))
        assert len(idx) == min(max_rows, 2049) and st[ref.LIMIT] == 2049 - len(idx)
    for out_cap in (1, 100, 1024, 1030):
        idx, st = check(run(dev, xy, 2049, {}, out_cap=out_cap, use_fill=False), dev["desc"], xy, 2049, {}, depth, None,
                        out_cap=out_cap, what=("out_cap", out_cap))
        assert len(idx) == out_cap and st[ref.LIMIT] == 2049 - out_cap
    kw = dict(max_rows=50)
    assert len(check(run(dev, xy, 2049, kw, out_cap=100, use_fill=False), dev["desc"], xy, 2049, kw, depth, None, out_cap=100)[0]) == 50
    # every second keypoint dropped (outside the map): the cut falls between kept rows of different wavefronts
    alt = xy.copy()
    alt[1::2, 0] = f(70.0)
    for max_rows in (512, 513, 1000):
        kw = dict(max_rows=max_rows)
        idx, st = check(run(dev, alt, 2049, kw, use_fill=False), dev["desc"], alt, 2049, kw, depth, None, what=("alternate", max_rows))
        assert len(idx) == max_rows and st[ref.PIXEL] == 1024 and st[ref.LIMIT] == 1025 - max_rows
    # a count beyond cap, a negative count
    idx, st = check(run(dev, xy, 800, {}, cap=300, use_fill=False), dev["desc"], xy, 800, {}, depth, None, cap=300, what="n > cap")
    assert len(idx) == 300 and st[0] == 300
    idx, st = check(run(dev, xy, -5, {}, use_fill=False), dev["desc"], xy, 0, {}, depth, None, what="n < 0")
    assert len(idx) == 0 and st[0] == 0


def test_duplicates_need_match_model_and_distance(dev):
    depth = dev["depth"]
    n = 1500
    xy = poisoned(valid_list(), n)
    rng = np.random.default_rng(0xD0B)
    X = ref.rows(dev["desc"], xy, n, depth, None, POSE)[1]   # every keypoint is kept: its model coordinates
    assert len(X) == n
    n_db = 4000
    store = rng.uniform(-1.0, 1.0, (n_db, 3)).astype(np.float32)
    model_of = np.repeat(np.arange(4, dtype=np.int32), 1000)
    idx = rng.integers(0, n_db, n).astype(np.int32)
    idx[::7] = -1
    md = f(0.25)
    # rows near the keypoint's own point: inside, outside, and exactly merge_dist away along x where the arithmetic is exact
    close = np.nonzero(idx >= 0)[0]
    step = rng.choice([0.0, 0.1, 0.3], len(close)).astype(np.float32)
    store[idx[close]] = X[close] + np.stack([step, np.zeros_like(step), np.zeros_like(step)], 1)
    d2 = np.ones(n, np.float32)
    d1 = rng.choice(np.array([0.3, nxt(0.8, 0), 0.8, 0.9], np.float32), n)
    dup = dict(idx=idx, d1=d1, d2=d2, model_of=model_of, xyz=store, model=2, row_begin=2000, row_end=3000)
    kw = dict(merge_ratio=0.8, merge_dist=float(md))
    why = ref.verdicts(xy, n, depth, None, POSE, dup=dup, **kw)[0]
    acc = ref.accepted(idx, d1, d2, 0.8)
    same = acc & (model_of[np.maximum(idx, 0)] == 2)
    assert (why == ref.DUP).sum() > 20 and (same & (why == ref.KEEP)).sum() > 20 and (acc & ~same).sum() > 100 and (~acc).sum() > 300
    got = run(dev, xy, n, kw, use_fill=False, dup=dup)
    kept, st = check(got, dev["desc"], xy, n, kw, depth, None, dup=dup, what="dup")
    assert st[ref.DUP] == (why == ref.DUP).sum()
    # the box covers the model's old rows [2000, 3000) and nothing else of the store
    assert got[3][0] <= store[2000:3000, 0].min() and got[3][3] >= store[2000:3000, 0].max()
    # a squared distance exactly merge_dist^2 is a duplicate, the next float above is not
    # (identity pose, the point (2, 2, 1): 2 - 1.75 and 0.25^2 are exact)
    flat = np.array(depth)
    flat[2, 2] = (2.0, 2.0, 1.0, 1.0)
    e = np.full((2, 2), 2.5, np.float32)
    st2 = np.array([[1.75, 2.0, 1.0], [nxt(1.75, 0), 2.0, 1.0]], np.float32)
    edge = dict(idx=[0, 1], d1=[0.1, 0.1], d2=[1.0, 1.0], model_of=[0, 0], xyz=st2, model=0, row_begin=0, row_end=0)
    kept, st = check(run(dev, e, 2, kw, cap=2, use_fill=False, dup=edge, depth_d=dev["t"](flat), pose=None), dev["desc"], e, 2, kw,
                     flat, None, cap=2, pose=None, dup=edge, what="dup edge")
    assert list(kept) == [1] and st[ref.DUP] == 1
    # off: by ratio, by distance, without the inputs
    for off in (dict(merge_ratio=0.0, merge_dist=0.25), dict(merge_ratio=0.8, merge_dist=-1.0)):
        kept, st = check(run(dev, xy, n, off, use_fill=False, dup=dup), dev["desc"], xy, n, off, depth, None, dup=dup, what=off)
        assert st[ref.DUP] == 0 and len(kept) == n
    kept, st = check(run(dev, xy, n, kw, use_fill=False), dev["desc"], xy, n, kw, depth, None, what="no dup inputs")
    assert st[ref.DUP] == 0 and len(kept) == n


def test_one_rounding_per_operation_on_the_relief(dev):
    """Frame 0's keypoints over the 640 x 480 relief under the trap pose: tests/test_view_model_cpu.py shows that a fused
    inverse transform changes a bit of hundreds of these rows."""
    import os
    from moped_amd import synth
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))
    xy, desc = gold["xy0"], gold["desc0"]
    relief = ref.relief_map(K=tuple(synth.K_DEFAULT))
    n = len(xy)
    got = run(dev, xy, n, {}, cap=n, desc_d=dev["t"](desc), depth_d=dev["t"](relief), use_fill=False, w=640, h=480)
    idx, st = check(got, desc, xy, n, {}, relief, None, cap=n, what="relief")
    assert len(idx) == n == 586
    r, t = ref.tm_from_pose(POSE)
    fused = ref.apply_inv_fused(r, t, relief[xy[:, 1].astype(int), xy[:, 0].astype(int), :3])
    assert np.any(bits(got[1][:n]) != bits(fused), axis=1).sum() >= 100


def test_batch_of_three_views_equals_the_single_calls(dev):
    c, torch, d, t = dev["c"], dev["torch"], dev["d"], dev["t"]
    counts = [65, 0, 1025]
    cap, out_cap = 1100, 1050
    rng = np.random.default_rng(0xBA8)
    dd = rng.normal(size=(3, cap, 128)).astype(np.float32)
    xy = rng.uniform(-1.5, 65.0, (3, cap, 2)).astype(np.float32)
    xy[:, :, 1] = rng.uniform(-1.5, 49.0, (3, cap)).astype(np.float32)
    maps = [make_map(s) for s in (11, 12, 13)]
    q = rng.normal(size=(3, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([q, rng.uniform(-0.3, 0.3, (3, 3))], 1).astype(np.float32)
    kw = dict(roi=(2.0, 2.0, 62.0, 46.0), max_fill_distance=7.0, max_rows=700)
    dd_d, xy_d = t(dd), t(xy)
    n_d = torch.tensor(counts, dtype=torch.int32, device=d)
    depth_d = [t(m[0]) for m in maps]
    fill_d = [t(m[1]) for m in maps]
    od = torch.full((3, out_cap, 128), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    ox = torch.full((3, out_cap, 3), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    no = torch.full((3,), -7, dtype=torch.int32, device=d)
    bb = torch.zeros((3, 6), dtype=torch.float32, device=d)
    st = torch.full((3, 8), -7, dtype=torch.int32, device=d)
    views = [capi.make_view(depth_d[i].data_ptr(), fill_d[i].data_ptr(), poses[i]) for i in range(3)]
    torch.cuda.synchronize()
    c.view_rows_batch_dev(dd_d.data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, views, W, H, capi.make_view_spec(**kw),
                          od.data_ptr(), ox.data_ptr(), out_cap, no.data_ptr(), bb.data_ptr(), st.data_ptr())
    c.synchronize()
    od, ox, no, bb, st = od.cpu().numpy(), ox.cpu().numpy(), no.cpu().numpy(), bb.cpu().numpy(), st.cpu().numpy()
    for i in range(3):
        one = run(dev, xy[i], counts[i], kw, cap=cap, out_cap=out_cap, desc_d=t(dd[i]), depth_d=depth_d[i], fill_d=fill_d[i],
                  pose=poses[i])
        sd, sx, sk, sb, ss = one
        assert no[i] == sk and np.array_equal(st[i], ss)
        assert np.array_equal(bits(od[i]), bits(sd[:out_cap])) and np.array_equal(bits(ox[i]), bits(sx[:out_cap]))
        assert np.array_equal(bits(bb[i]), bits(sb))
        check(one, dd[i], xy[i], counts[i], kw, maps[i][0], maps[i][1], cap=cap, out_cap=out_cap, pose=poses[i], what=("batch", i))
        # a view that read its neighbour's map or pose would differ
        j = (i + 1) % 3
        if counts[i] > 0:
            other = ref.rows(dd[i], xy[i], counts[i], maps[j][0], maps[j][1], poses[i], out_cap=out_cap, **kw)
            assert not np.array_equal(bits(other[1]), bits(sx[:sk]))
            other = ref.rows(dd[i], xy[i], counts[i], maps[i][0], maps[i][1], poses[j], out_cap=out_cap, **kw)
            assert not np.array_equal(bits(other[1]), bits(sx[:sk]))
    assert no[0] > 10 and no[1] == 0 and no[2] > 300


def test_bad_arguments_launch_nothing(dev):
    c, torch, d = dev["c"], dev["torch"], dev["d"]
    L = c.L
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=d)
    p = buf.data_ptr()
    ok_spec = capi.make_view_spec()
    ok_view = capi.make_view(dev["depth_d"].data_ptr(), dev["fill_d"].data_ptr(), POSE)

    def call(spec=ok_spec, view=ok_view, desc_ptr=p, cap=4, out_cap=4, w=W, h=H, dup=None):
        return L.mh_view_rows_dev(c.h, desc_ptr, p + 2048, p + 4096 - 64, cap, C.byref(view) if view is not None else None, w, h,
                                  C.byref(spec) if spec is not None else None, C.byref(dup) if dup is not None else None,
                                  p + 8192, p + 12288, out_cap, p + 4096 - 32, p + 4096 - 128, p + 4096 - 256)

    assert call() == 0
    c.synchronize()
    assert call(spec=None) == -1 and call(view=None) == -1 and call(cap=0) == -1 and call(out_cap=0) == -1
    assert call(w=0) == -1 and call(h=-1) == -1
    assert call(desc_ptr=p + 4) == -1   # descriptors are read 16 bytes at a time
    assert call(view=capi.make_view(None, None, POSE)) == -1
    assert call(view=capi.make_view(dev["depth_d"].data_ptr() + 4, None, POSE)) == -1   # the map is read 16 bytes at a time
    for k in range(7):
        for bad in (np.nan, np.inf):
            pose = np.array(POSE)
            pose[k] = bad
            assert call(view=capi.make_view(dev["depth_d"].data_ptr(), None, pose)) == -1
    nan, inf = float("nan"), float("inf")
    for bad in (dict(roi=(0.0, nan, 1.0, 1.0)), dict(box=(0.0, 0.0, 0.0, 1.0, nan, 1.0)), dict(box=(-inf, 0.0, 0.0, 1.0, 1.0, 1.0)),
                dict(max_rows=-1), dict(max_fill_distance=nan), dict(merge_ratio=nan), dict(merge_dist=nan)):
        assert call(spec=capi.make_view_spec(**bad)) == -1, bad
    assert "mh_view_rows_dev" in L.mh_last_error(c.h).decode()
    assert call(dup=capi.mh_view_dup(p, p, p, p, None, 4, 0, 0, 0)) == -1
    assert call(dup=capi.mh_view_dup(p, p, p, p, p, 4, 0, 0, 5)) == -1
    c.synchronize()
