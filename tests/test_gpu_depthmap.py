"""mh_depth_map_from_raw_*: the Kinect depth map from raw sensor depth on the device (moped_amd/csrc/depthmap.hip) against
the numpy float32 restatement tests/depthmap_ref.py, as uint32 views with array_equal -- no tolerance: both sides perform
the same sequence of single IEEE operations.

Shapes where the indexing can go wrong: odd sizes, sizes that are no multiple of the 256-thread block, more than one
block, the same size / exactly twice / a pad of invalid pixels / a crop; every case under synth.K_DEFAULT and a
non-square K; all three input layouts; missing readings in the corners, on the borders and alone in the interior."""
import ctypes as C

import numpy as np
import pytest

import depthmap_ref as ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
KS = (synth.K_DEFAULT, np.array([612.5, 431.25, 17.75, 9.5], f32))
# (raw width, raw height, map width, map height)
SHAPES = [(7, 5, 7, 5), (33, 17, 33, 17), (64, 48, 64, 48), (7, 5, 14, 10), (33, 17, 66, 34), (64, 48, 128, 96),
          (32, 16, 70, 40), (32, 16, 60, 30)]
LAYOUTS = ["f32", "u16", "cloud16", "cloud32"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def defects(rw, rh, which=None):
    """Missing readings: the four corners, one on every border, one alone in the interior."""
    d = [(0, 0), (rw - 1, 0), (0, rh - 1), (rw - 1, rh - 1), (rw // 2, 0), (0, rh // 2), (rw - 1, rh // 2 - 1),
         (rw // 2 - 1, rh - 1), (rw // 2 + 1, rh // 2)]
    return d if which is None else [d[i] for i in which]


def raw_input(layout, rw, rh, seed=0, which=None):
    """-> (buffer uint8, the arguments of ref.depth_map between the buffer and K)."""
    rng = np.random.default_rng(100 + seed)
    if layout == "u16":
        mm = rng.integers(400, 9000, (rh, rw)).astype(np.uint16)
        for x, y in defects(rw, rh, which):
            mm[y, x] = 0
        a = ref.plain(mm)
    else:
        z = rng.uniform(0.4, 4.0, (rh, rw)).astype(f32)
        z[rh // 2, rw // 2 - 1] = 0.0                 # a valid reading of depth zero
        for x, y in defects(rw, rh, which):
            z[y, x] = np.nan
        a = ref.plain(z) if layout == "f32" else \
            ref.cloud(z, 16, 8, 48, seed) if layout == "cloud16" else ref.cloud(z, 32, 8, 64, seed)
    return np.ascontiguousarray(a[0]), a[1:]


def desc(a):
    fmt, rw, rh, es, rs, off = a
    return capi.make_raw_depth(fmt, rw, rh, es, rs, off)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch, torch.device("cuda:0")


def to_dev(dev, buf):
    torch, d = dev
    t = torch.from_numpy(buf).to(d)
    torch.cuda.synchronize()
    return t


def stale(dev, *shape):
    torch, d = dev
    t = torch.full(shape, 7.25, dtype=torch.float32, device=d)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_device_map_equals_the_restatement(ctx, dev, shape, layout):
    rw, rh, w, h = shape
    buf, a = raw_input(layout, rw, rh)
    t_raw = to_dev(dev, buf)
    for K in KS:
        want = ref.depth_map(buf, *a, K, w, h)
        t_out = stale(dev, h, w, 4)
        ctx.depth_map_from_raw_dev(t_raw.data_ptr(), desc(a), K, t_out.data_ptr(), w, h)
        ctx.synchronize()
        got = t_out.cpu().numpy()
        valid = want[..., 2] >= 0
        print(shape, layout, "valid", int(valid.sum()), "of", w * h, "differing words", int((bits(got) != bits(want)).sum()))
        assert 0 < valid.sum() < w * h
        assert np.array_equal(bits(got), bits(want))


def test_pad_and_crop_are_what_they_claim(ctx, dev):
    """Raw 32 x 16: into 70 x 40 the columns from 64 and the rows from 32 are invalid; 60 x 30 is the 2x map cropped."""
    buf, a = raw_input("f32", 32, 16)
    t_raw = to_dev(dev, buf)
    K = KS[0]
    maps = {}
    for w, h in ((64, 32), (70, 40), (60, 30)):
        t_out = stale(dev, h, w, 4)
        ctx.depth_map_from_raw_dev(t_raw.data_ptr(), desc(a), K, t_out.data_ptr(), w, h)
        ctx.synchronize()
        maps[(w, h)] = t_out.cpu().numpy()
    full, pad, crop = maps[(64, 32)], maps[(70, 40)], maps[(60, 30)]
    assert np.array_equal(bits(pad[:32, :64]), bits(full))
    assert np.array_equal(bits(pad[32:]), bits(np.full((8, 70, 4), -1, f32)))
    assert np.array_equal(bits(pad[:, 64:]), bits(np.full((40, 6, 4), -1, f32)))
    assert np.array_equal(bits(crop), bits(full[:30, :60]))


@pytest.mark.parametrize("layout", ["f32", "u16", "cloud32"])
def test_batch_of_five_equals_the_five_single_calls(ctx, dev, layout):
    """Five frames with different defects in ONE launch, into a stale non-zero buffer, against the single calls byte for
    byte (and the restatement)."""
    torch, d = dev
    rw, rh, w, h = 33, 17, 66, 34
    K = KS[1]
    which = [(0, 8), (1, 4, 6), (2, 5), (3, 7, 8), (8,)]
    ins = [raw_input(layout, rw, rh, seed=f, which=which[f]) for f in range(5)]
    a = ins[0][1]
    assert all(i[1] == a for i in ins)
    t_raw = [to_dev(dev, b) for b, _ in ins]
    t_batch = stale(dev, 5, h, w, 4)
    ctx.depth_map_from_raw_batch_dev([t.data_ptr() for t in t_raw], desc(a), K, [t_batch[f].data_ptr() for f in range(5)], w, h)
    ctx.synchronize()
    got = t_batch.cpu().numpy()
    singles = []
    for f in range(5):
        t_out = stale(dev, h, w, 4)
        ctx.depth_map_from_raw_dev(t_raw[f].data_ptr(), desc(a), K, t_out.data_ptr(), w, h)
        ctx.synchronize()
        singles.append(t_out.cpu().numpy())
    for f in range(5):
        assert got[f].tobytes() == singles[f].tobytes(), f
        assert np.array_equal(bits(got[f]), bits(ref.depth_map(ins[f][0], *a, K, w, h))), f
    assert len({g.tobytes() for g in got}) == 5


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_entry_equals_the_device_entry(ctx, dev, layout):
    for rw, rh, w, h in ((33, 17, 33, 17), (33, 17, 66, 34), (32, 16, 70, 40)):
        buf, a = raw_input(layout, rw, rh, seed=3)
        t_raw = to_dev(dev, buf)
        t_out = stale(dev, h, w, 4)
        ctx.depth_map_from_raw_dev(t_raw.data_ptr(), desc(a), KS[0], t_out.data_ptr(), w, h)
        ctx.synchronize()
        # the host copies exactly the bytes the description spans: hand it no more than those
        fmt, _, _, es, rs, off = a
        span = off + (rh - 1) * rs + (rw - 1) * es + (4 if fmt == ref.F32_M else 2)
        got = ctx.depth_map_from_raw(buf[:span].copy(), desc(a), KS[0], w, h)
        assert got.tobytes() == t_out.cpu().numpy().tobytes(), (layout, rw, rh, w, h)


def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx, dev):
    torch, d = dev
    rw, rh, w, h = 33, 17, 66, 34
    buf, a = raw_input("f32", rw, rh)
    t_raw = to_dev(dev, buf)
    t_out = stale(dev, 2, h, w, 4)
    k = np.ascontiguousarray(KS[0], f32)
    kp = k.ctypes.data_as(C.c_void_p)
    L, H = ctx.L, ctx.h
    raw_p, out_p = C.c_void_p(t_raw.data_ptr()), C.c_void_p(t_out.data_ptr())
    good = desc(a)

    def single(raw=raw_p, r=good, K=kp, out=out_p, ww=w, hh=h):
        return L.mh_depth_map_from_raw_dev(H, raw, C.byref(r) if r is not None else None, K, out, ww, hh)

    def rd(**kw):
        v = dict(fmt=capi.RAW_DEPTH_F32_M, width=rw, height=rh, elem_stride=4, row_stride=4 * rw, offset=0)
        v.update(kw)
        return capi.mh_raw_depth(v["fmt"], v["width"], v["height"], v["elem_stride"], v["row_stride"], v["offset"])

    # null pointers
    assert single(raw=None) == -1 and single(r=None) == -1 and single(K=None) == -1 and single(out=None) == -1
    # non-positive sizes
    assert single(ww=0) == -1 and single(hh=-1) == -1 and single(r=rd(width=0)) == -1 and single(r=rd(height=-3)) == -1
    # an unknown format
    assert single(r=rd(fmt=2)) == -1 and single(r=rd(fmt=-1)) == -1
    # strides or offset that are no multiple of the element size; an element stride below it
    assert single(r=rd(elem_stride=6)) == -1 and single(r=rd(row_stride=4 * rw + 2)) == -1 and single(r=rd(offset=2)) == -1
    assert single(r=rd(elem_stride=2)) == -1 and single(r=rd(elem_stride=0)) == -1
    assert single(r=rd(fmt=capi.RAW_DEPTH_U16_MM, elem_stride=3, row_stride=2 * rw)) == -1
    assert single(r=rd(fmt=capi.RAW_DEPTH_U16_MM, elem_stride=2, row_stride=2 * rw, offset=1)) == -1
    assert single(r=rd(fmt=capi.RAW_DEPTH_U16_MM, elem_stride=1, row_stride=2 * rw)) == -1
    # the batch: n_frames outside 1 .. MH_MAX_BATCH, null arrays and entries, two frames writing the same map
    raws = (C.c_void_p * 33)(*([t_raw.data_ptr()] * 33))
    outs = (C.c_void_p * 33)(*([t_out[0].data_ptr(), t_out[1].data_ptr()] + [t_out[0].data_ptr()] * 31))

    def batch(n, rr=raws, oo=outs):
        return L.mh_depth_map_from_raw_batch_dev(H, rr, C.byref(good), kp, oo, n, w, h)

    assert batch(0) == -1 and batch(-2) == -1 and batch(capi.MAX_BATCH + 1) == -1
    assert batch(2, rr=None) == -1 and batch(2, oo=None) == -1
    assert batch(2, rr=(C.c_void_p * 2)(t_raw.data_ptr(), None)) == -1
    assert batch(2, oo=(C.c_void_p * 2)(t_out[0].data_ptr(), None)) == -1
    assert batch(3) == -1                                   # frame 2 writes frame 0's map
    with pytest.raises(capi.MhError) as e:
        ctx.depth_map_from_raw_batch_dev([t_raw.data_ptr()] * 2, good, KS[0], [t_out[0].data_ptr()] * 2, w, h)
    assert "-> -1:" in str(e.value) and "same map" in str(e.value)
    # the host entry
    hb = np.ascontiguousarray(buf)
    ho = np.zeros((h, w, 4), f32)
    hbp, hop = hb.ctypes.data_as(C.c_void_p), ho.ctypes.data_as(C.c_void_p)
    assert L.mh_depth_map_from_raw_host(H, None, C.byref(good), kp, hop, w, h) == -1
    assert L.mh_depth_map_from_raw_host(H, hbp, None, kp, hop, w, h) == -1
    assert L.mh_depth_map_from_raw_host(H, hbp, C.byref(rd(fmt=5)), kp, hop, w, h) == -1
    assert L.mh_depth_map_from_raw_host(H, hbp, C.byref(rd(offset=3)), kp, hop, 0, h) == -1
    # nothing was written by any of them
    torch.cuda.synchronize()
    assert bool((t_out == 7.25).all()) and not ho.any()
    # ... and the context is as it was: two frames, one launch, the restatement's bytes
    assert batch(2) == 0
    ctx.synchronize()
    want = ref.depth_map(buf, *a, KS[0], w, h)
    got = t_out.cpu().numpy()
    assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[1]), bits(want))
