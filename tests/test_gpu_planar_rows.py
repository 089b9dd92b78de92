"""mh_planar_rows_dev: the selection kernel of createPlanarModelsFromImages (moped2/libmoped/src/moped.cpp:220-232) on
synthetic device arrays against tests/planar_ref.py.  Everything is compared on bits: the kept descriptors, the model
coordinates, the count, the bounding box, and the sentinel in every row at and beyond the count.

The kernel walks a list in chunks of 1024 keypoints, 16 wavefronts of 64 lanes: the counts below sit on the wavefront,
workgroup and chunk edges of that compaction."""
import numpy as np
import pytest

import planar_ref as ref
from moped_amd import capi

pytestmark = pytest.mark.gpu
CAP = 2304
SENT_BITS = 0x7FC0BEEF   # a NaN no computation here makes
K1 = (525.0, 519.0, 319.5, 239.5)
V_HI = 1.0e6


@pytest.fixture(scope="module")
def dev():
    import torch
    c = capi.Context(0)
    rng = np.random.default_rng(0x91A)
    desc = rng.normal(size=(CAP, 128)).astype(np.float32)
    d = torch.device("cuda:0")
    desc_d = torch.from_numpy(desc).to(d)
    desc.setflags(write=False)
    yield c, torch, d, desc, desc_d
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(dev, xy, n, spec_kw, cap=CAP, out_cap=CAP, desc=None):
    """One launch on (desc, xy, n) -> (desc_out, xyz_out, n_out, bbox) as numpy, outputs pre-filled with the sentinel."""
    c, torch, d, desc_h, desc_d = dev
    if desc is not None:
        desc_d = torch.from_numpy(np.ascontiguousarray(desc, np.float32)).to(d)
    xy_d = torch.from_numpy(np.ascontiguousarray(xy, np.float32)).to(d)
    n_d = torch.tensor([n], dtype=torch.int32, device=d)
    od = torch.full((CAP, 128), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    ox = torch.full((CAP, 3), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    no = torch.full((1,), -7, dtype=torch.int32, device=d)
    bb = torch.zeros(6, dtype=torch.float32, device=d)
    torch.cuda.synchronize()
    spec = capi.make_planar_spec(**spec_kw)
    c.planar_rows_dev(desc_d.data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, spec, od.data_ptr(), ox.data_ptr(), out_cap,
                      no.data_ptr(), bb.data_ptr())
    c.synchronize()
    return od.cpu().numpy(), ox.cpu().numpy(), int(no.cpu()[0]), bb.cpu().numpy()


def check(got, desc, xy, n, spec_kw, cap=CAP, out_cap=CAP, what=""):
    od, ox, k, bb = got
    form = 0 if spec_kw.get("z") is None else 1
    wd, wx, wb, idx = ref.rows(desc[:cap], np.asarray(xy, np.float32)[:cap], min(n, cap), form, spec_kw.get("scale") or 1.0,
                               spec_kw.get("K") or (1, 1, 0, 0), spec_kw.get("z") or 0.0, spec_kw.get("roi"),
                               spec_kw.get("max_rows", 0), out_cap)
    assert k == len(idx), (what, k, len(idx))
    assert np.array_equal(bits(od[:k]), bits(wd)), what
    assert np.array_equal(bits(ox[:k]), bits(wx)), what
    assert np.array_equal(bits(bb), bits(wb)), (what, bb, wb)
    assert np.all(bits(od[k:]) == SENT_BITS) and np.all(bits(ox[k:]) == SENT_BITS), what   # nothing written past the count
    return idx


def planted(n, pattern):
    """xy [CAP,2] and the roi that makes `pattern` of the first n keypoints: u = i + 0.5 unless said otherwise."""
    i = np.arange(CAP, dtype=np.float32)
    xy = np.stack([i + np.float32(0.5), np.float32(1.0) + i * np.float32(0.25)], 1).astype(np.float32)
    if pattern == "all":
        return xy, None, np.arange(n)
    if pattern == "none":
        return xy, (-10.0, -10.0, -5.0, -5.0), np.zeros(0, int)
    if pattern == "alternate":
        xy[1::2, 0] = np.float32(5000.5)
        return xy, (0.0, 0.0, 4000.0, V_HI), np.arange(0, n, 2)
    if pattern == "first":
        return xy, (0.0, 0.0, 1.0, V_HI), np.arange(min(n, 1))
    if pattern == "last":
        return xy, (float(n - 1), 0.0, float(n), V_HI), np.arange(max(n - 1, 0), n)
    assert pattern == "run"   # one run across a chunk edge (1024) where the list has one, else across a wavefront edge (64)
    lo, hi = (1000, 1050) if n > 1024 else (60, 70)
    return xy, (float(lo), 0.0, float(hi), V_HI), np.arange(min(lo, n), min(hi, n))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_every_keep_pattern_at_the_edges_of_the_compaction(dev, n):
    desc = dev[3]
    for j, pattern in enumerate(("all", "none", "alternate", "first", "last", "run")):
        xy, roi, want_idx = planted(n, pattern)
        for form in (0, 1):
            kw = dict(scale=0.0015, roi=roi) if form == 0 else dict(z=0.8, K=K1, roi=roi)
            idx = check(run(dev, xy, n, kw), desc, xy, n, kw, what=(n, pattern, form))
            assert np.array_equal(idx, want_idx), (n, pattern)   # the reference selects what the pattern plants


def test_count_above_capacity_and_limits(dev):
    desc = dev[3]
    xy, _, _ = planted(CAP, "all")
    # a count beyond cap: only cap keypoints are read (the rows behind them would be kept too)
    kw = dict(z=0.8, K=K1)
    idx = check(run(dev, xy, 300 + 500, kw, cap=300), desc, xy, 800, kw, cap=300, what="n > cap")
    assert len(idx) == 300
    idx = check(run(dev, xy, -5, kw), desc, xy, 0, kw, what="n < 0")
    assert len(idx) == 0
    # max_rows inside a chunk, exactly on chunk edges, beyond the kept count; with every keypoint kept and with every second
    for roi, step in ((None, 1), ((0.0, 0.0, 4000.0, V_HI), 2)):
        pts = xy.copy()
        if step == 2:
            pts[1::2, 0] = np.float32(5000.5)
        for max_rows in (1, 700, 1024, 1025, 1500, 2048, 2049, 5000):
            kw = dict(scale=0.002, roi=roi, max_rows=max_rows)
            idx = check(run(dev, pts, 2049, kw), desc, pts, 2049, kw, what=("max_rows", max_rows, step))
            assert len(idx) == min(max_rows, len(range(0, 2049, step)))
    # out_cap smaller than the kept count: the first out_cap, n_out = out_cap, nothing behind them
    for out_cap in (1, 100, 1024, 1030):
        kw = dict(z=0.8, K=K1)
        idx = check(run(dev, xy, 2049, kw, out_cap=out_cap), desc, xy, 2049, kw, out_cap=out_cap, what=("out_cap", out_cap))
        assert len(idx) == out_cap
    kw = dict(z=0.8, K=K1, max_rows=50)
    assert len(check(run(dev, xy, 2049, kw, out_cap=100), desc, xy, 2049, kw, out_cap=100)) == 50


def test_roi_is_half_open_on_the_float_coordinates_and_drops_nan(dev):
    desc = dev[3]
    f = np.float32
    roi = (10.25, 20.5, 30.75, 40.0)
    nxt = lambda v, to: np.nextafter(f(v), f(to))
    pts = [(10.25, 20.5), (30.75, 25.0), (nxt(30.75, 0), 25.0), (nxt(10.25, 0), 25.0), (15.0, 40.0), (15.0, nxt(40.0, 0)),
           (np.nan, 25.0), (15.0, np.nan), (np.nan, np.nan), (15.0, 20.5), (np.inf, 25.0), (-np.inf, 25.0), (30.0, 39.0)]
    xy = np.array(pts, np.float32)
    want = [0, 2, 5, 9, 12]
    for kw in (dict(scale=0.01, roi=roi), dict(z=1.25, K=K1, roi=roi)):
        idx = check(run(dev, xy, len(xy), kw, cap=len(xy)), desc, xy, len(xy), kw, cap=len(xy), what="roi edges")
        assert list(idx) == want
    # nothing kept: the box is the reference's initial one (moped.cpp:107-108)
    kw = dict(z=1.25, K=K1, roi=(1000.0, 1000.0, 1001.0, 1001.0))
    od, ox, k, bb = run(dev, xy, len(xy), kw, cap=len(xy))
    assert k == 0 and np.array_equal(bits(bb), bits(np.array([1e11, 1e11, 1e11, -1e11, -1e11, -1e11], np.float32)))
    assert np.array_equal(bits(bb), bits(np.array([10E10] * 3 + [-10E10] * 3, np.float32)))


def test_one_rounding_per_operation(dev):
    """Keypoints planar_ref chose on the CPU because a reciprocal-multiply division (form 1) or a scale folded into the
    product (form 0) changes the last bit of x there."""
    desc = dev[3]
    uv, K, z = ref.form1_cases()
    kw = dict(z=float(z), K=tuple(float(k) for k in K))
    check(run(dev, uv, len(uv), kw, cap=len(uv)), desc, uv, len(uv), kw, cap=len(uv), what="form 1")
    kw = dict(z=float(z), K=(float(K[1]), float(K[0]), float(K[3]), float(K[2])))   # the same through y
    check(run(dev, uv[:, ::-1].copy(), len(uv), kw, cap=len(uv)), desc, uv[:, ::-1].copy(), len(uv), kw, cap=len(uv), what="form 1 y")
    uv0, scale = ref.form0_cases()
    kw = dict(scale=float(scale))
    check(run(dev, uv0, len(uv0), kw, cap=len(uv0)), desc, uv0, len(uv0), kw, cap=len(uv0), what="form 0")
    # denormal and huge products keep their bits too
    odd = np.array([[1e-30, 3e-39], [3.0e38, 1e-45], [0.0, 639.99994]], np.float32)
    for kw in (dict(scale=1e-9), dict(scale=float(scale)), dict(z=0.8, K=K1)):
        check(run(dev, odd, 3, kw, cap=3), desc, odd, 3, kw, cap=3, what=("odd", kw))


def test_batch_launch_equals_the_single_launches(dev):
    c, torch, d, desc, desc_d = dev
    counts = [0, 65, 1025]
    cap = 1100
    rng = np.random.default_rng(0xBA7)
    dd = rng.normal(size=(3, cap, 128)).astype(np.float32)
    xy = rng.uniform(0, 640, (3, cap, 2)).astype(np.float32)
    roi = (100.0, 50.0, 600.0, 400.0)
    out_cap = 1050
    for kw in (dict(z=0.8, K=K1, roi=roi, max_rows=700), dict(scale=0.0015)):
        spec = capi.make_planar_spec(**kw)
        dd_d, xy_d = torch.from_numpy(dd).to(d), torch.from_numpy(xy).to(d)
        n_d = torch.tensor(counts, dtype=torch.int32, device=d)
        od = torch.full((3, out_cap, 128), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
        ox = torch.full((3, out_cap, 3), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
        no = torch.full((3,), -7, dtype=torch.int32, device=d)
        bb = torch.zeros((3, 6), dtype=torch.float32, device=d)
        torch.cuda.synchronize()
        c.planar_rows_dev(dd_d.data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, spec, od.data_ptr(), ox.data_ptr(), out_cap,
                          no.data_ptr(), bb.data_ptr(), n_images=3)
        c.synchronize()
        od, ox, no, bb = od.cpu().numpy(), ox.cpu().numpy(), no.cpu().numpy(), bb.cpu().numpy()
        for i in range(3):
            sd, sx, sk, sb = run(dev, xy[i], counts[i], kw, cap=cap, out_cap=out_cap, desc=dd[i])
            assert no[i] == sk
            assert np.array_equal(bits(od[i]), bits(sd[:out_cap])) and np.array_equal(bits(ox[i]), bits(sx[:out_cap]))
            assert np.array_equal(bits(bb[i]), bits(sb))
            check((sd, sx, sk, sb), dd[i], xy[i], counts[i], kw, cap=cap, out_cap=out_cap, what=("batch", i))
        assert no[0] == 0 and no[1] > 10 and no[2] > 300


def test_bad_arguments_launch_nothing(dev):
    c, torch, d, desc, desc_d = dev
    L = c.L
    buf = torch.zeros(4096, dtype=torch.float32, device=d)
    p = buf.data_ptr()
    ok = capi.make_planar_spec(scale=1.0)
    call = lambda spec, desc_ptr=p, cap=4, out_cap=4: L.mh_planar_rows_dev(
        c.h, desc_ptr, p + 2048, p + 4096 - 64, cap, spec, p + 8192, p + 12288, out_cap, p + 4096 - 32, p + 4096 - 128)
    import ctypes as C
    assert call(C.byref(ok)) == 0
    c.synchronize()
    assert call(None) == -1 and call(C.byref(ok), cap=0) == -1 and call(C.byref(ok), out_cap=0) == -1
    assert call(C.byref(ok), desc_ptr=p + 4) == -1   # descriptors are read 16 bytes at a time
    for bad in (dict(form=2), dict(form=-1), dict(scale=float("nan")), dict(z=float("inf")), dict(max_rows=-1)):
        sp = capi.make_planar_spec(scale=1.0)
        for k, v in bad.items():
            setattr(sp, k, v)
        assert call(C.byref(sp)) == -1, bad
    sp = capi.make_planar_spec(z=1.0, K=(0.0, 1.0, 0.0, 0.0))
    assert call(C.byref(sp)) == -1
    sp = capi.make_planar_spec(z=1.0, K=(1.0, float("nan"), 0.0, 0.0))
    assert call(C.byref(sp)) == -1
    sp = capi.make_planar_spec(scale=1.0, roi=(0.0, float("nan"), 1.0, 1.0))
    assert call(C.byref(sp)) == -1
    c.synchronize()
