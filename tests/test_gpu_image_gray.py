"""mh_image_gray_* and mh_frame_set_image_format: the gray image from what a camera delivers (moped_amd/csrc/image_gray.hip,
moped3d/moped3d.cpp:249) against the integer restatement tests/image_gray_ref.py -- bytes, no tolerance.

Shapes where the kernel can go wrong: it cuts every output row at the 8-byte boundaries of its own output address and
moves aligned dwords in between, so widths below, at and around one and many runs, rows whose alignment changes from row
to row (odd widths, padded strides), raw pointers, offsets and output pointers at every byte alignment, and both sizes a
camera really has.  Every output lies between 64 guard bytes inside a larger tensor, and every raw buffer between spare
bytes of its tensor: a read outside the extent is excluded by the kernel's construction (every dword is checked against
the extent), not provoked here."""
import numpy as np
import pytest

import image_gray_ref as ref
from moped_amd import capi, synth
from test_gpu_undistort import CAM0, CAP, GOLD, LAUNCH_D, LAUNCH_K, _scene_db

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257]
HEIGHTS = [1, 2, 3, 5]
BAYER_HEIGHTS = [3, 4, 5]
GUARD = 64
LEAD = 64   # spare bytes in front of a raw buffer inside its tensor


@pytest.fixture(scope="module")
def gpu():
    import torch
    return torch, torch.device("cuda:0")


def strides(fmt, w):
    tight = w * ref.bpp(fmt)
    return [tight, tight + 1, tight + 13, 2 * tight]


class Out:
    """n packed outputs of w x h, each moved by `shift` bytes and between guards of 0xA5, inside one tensor."""

    def __init__(self, gpu, w, h, shift, n=1):
        torch, dev = gpu
        self.px, self.shift, self.n = w * h, shift, n
        self.step = GUARD + 3 + self.px + GUARD
        self.t = torch.full((n * self.step,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptrs = [self.t.data_ptr() + i * self.step + GUARD + shift for i in range(n)]
        self.w, self.h = w, h

    def read(self):
        """-> the n images; asserts that every byte around them is still 0xA5."""
        a = self.t.cpu().numpy().reshape(self.n, self.step)
        lo = GUARD + self.shift
        assert (a[:, :lo] == 0xA5).all() and (a[:, lo + self.px:] == 0xA5).all(), "bytes outside the output were written"
        return [a[i, lo:lo + self.px].reshape(self.h, self.w) for i in range(self.n)]


def upload(gpu, raw, move):
    """The raw buffer at LEAD + move bytes inside a larger tensor -> (tensor, device pointer)."""
    torch, dev = gpu
    host = np.full(LEAD + move + raw.size + 64, 0x3C, np.uint8)
    host[LEAD + move:LEAD + move + raw.size] = raw
    t = torch.from_numpy(host).to(dev)
    return t, t.data_ptr() + LEAD + move


def check_case(ctx, gpu, fmt, w, h, row_stride, offset, move, shift, rng, what="random"):
    n = ref.extent(fmt, w, h, row_stride, offset)
    if what == "random":
        raws = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(2)]
    else:
        raws = [np.full(n, what, np.uint8)] * 2
    want = [ref.gray(r, fmt, w, h, row_stride, offset) for r in raws]
    d = capi.make_raw_image(fmt, w, h, row_stride, offset)
    ups = [upload(gpu, r, move) for r in raws]
    tag = (ref.NAMES[fmt], w, h, row_stride, offset, move, shift)
    one, two = Out(gpu, w, h, shift), Out(gpu, w, h, shift, 2)
    gpu[0].cuda.synchronize()   # (the tensors are filled on torch's stream, the context has one of its own)
    ctx.image_gray_dev(ups[0][1], d, one.ptrs[0])
    ctx.image_gray_batch_dev([u[1] for u in ups], d, two.ptrs)
    ctx.synchronize()
    assert np.array_equal(one.read()[0], want[0]), ("dev",) + tag
    got = two.read()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("batch",) + tag
    assert np.array_equal(ctx.image_gray(raws[1], d), want[1]), ("host",) + tag


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
def test_bytes_equal_the_restatement(ctx, gpu, fmt):
    """Device, batch and host call at every width and height; raw offset, raw pointer, row stride and output pointer go
    round their values so that every value of each meets every width, and all four strides meet every (width, height)."""
    rng = np.random.default_rng(1000 + fmt)
    bayer = fmt in ref.BAYER
    for wi, w in enumerate(w for w in WIDTHS if not bayer or w >= 3):
        for hi, h in enumerate(BAYER_HEIGHTS if bayer else HEIGHTS):
            for k in range(4):
                check_case(ctx, gpu, fmt, w, h, strides(fmt, w)[k], (k + wi) % 4, (k + hi + wi) % 4, (2 * k + hi + wi // 4) % 4, rng)


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
def test_every_offset_meets_every_output_alignment(ctx, gpu, fmt):
    """offset 0 .. 3 x output moved by 0 .. 3, at one width around a run and one of many runs."""
    rng = np.random.default_rng(2000 + fmt)
    for w in (9, 65):
        for offset in range(4):
            for shift in range(4):
                check_case(ctx, gpu, fmt, w, 3, strides(fmt, w)[(offset + shift) % 4], offset, (offset * 3 + shift) % 4, shift, rng)


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
def test_camera_sizes_and_constant_images(ctx, gpu, fmt):
    rng = np.random.default_rng(3000 + fmt)
    tight = 640 * ref.bpp(fmt)
    check_case(ctx, gpu, fmt, 640, 480, tight + 13, 3, 1, 2, rng)
    check_case(ctx, gpu, fmt, 1280, 960, 2 * tight, 0, 0, 0, rng)
    for v in (0, 255):
        check_case(ctx, gpu, fmt, 65, 5, strides(fmt, 65)[1], 1, 2, 3, rng, what=v)


@pytest.mark.parametrize("n", [3, capi.MAX_BATCH])
def test_batch_equals_the_single_calls(ctx, gpu, n):
    rng = np.random.default_rng(40 + n)
    for fmt, w, h in ((ref.BGR8, 67, 9), (ref.RGBA8, 33, 5), (ref.BAYER_GRBG8, 67, 9), (ref.GRAY8, 21, 4)):
        rs, off = strides(fmt, w)[2], 3
        d = capi.make_raw_image(fmt, w, h, rs, off)
        raws = [rng.integers(0, 256, ref.extent(fmt, w, h, rs, off), dtype=np.uint8) for _ in range(n)]
        ups = [upload(gpu, r, i % 4) for i, r in enumerate(raws)]
        single, batch = Out(gpu, w, h, 1, n), Out(gpu, w, h, 3, n)
        gpu[0].cuda.synchronize()
        for i in range(n):
            ctx.image_gray_dev(ups[i][1], d, single.ptrs[i])
        ctx.image_gray_batch_dev([u[1] for u in ups], d, batch.ptrs)
        ctx.synchronize()
        a, b = single.read(), batch.read()
        assert len({x.tobytes() for x in a}) == n                  # distinct images
        for i in range(n):
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], ref.gray(raws[i], fmt, w, h, rs, off)), (fmt, i)


def test_more_rows_than_one_grid_holds(ctx, gpu):
    """One pixel per row and 2^31 - 100 rows: two runs per row are 2^32 - 200 threads, more than a grid holds with its
    last block rounded up, so the call goes in two launches, the second from a row offset -- a path no camera-sized image
    reaches.  gray8 with packed rows is a copy, so the device compares its 2 GiB itself."""
    torch, dev = gpu
    h = 2 ** 31 - 100
    src = torch.randint(0, 256, (h,), dtype=torch.uint8, device=dev)
    out = torch.full((h + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # (the context has a stream of its own)
    ctx.image_gray_dev(src.data_ptr(), capi.make_raw_image(capi.IMAGE_GRAY8, 1, h), out.data_ptr() + GUARD)
    ctx.synchronize()
    assert torch.equal(out[GUARD:GUARD + h], src)
    assert bool((out[:GUARD] == 0xA5).all()) and bool((out[GUARD + h:] == 0xA5).all())
    del src, out
    torch.cuda.empty_cache()


# ---- frames ----------------------------------------------------------------------------------------------------------
def colour_of(gray, k=0):
    """R = clip(g + a smooth field), G = g, B = clip(g - another): an image whose gray is close to `gray`."""
    h, w = gray.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = 30.0 * np.sin(x / (50.0 + 7 * k)) * np.cos(y / 70.0)
    b = 25.0 * np.cos(x / 90.0 + k) * np.sin(y / (40.0 + 3 * k))
    g = gray.astype(np.float64)
    return np.stack([np.clip(np.rint(g + a), 0, 255), g, np.clip(np.rint(g - b), 0, 255)], 2).astype(np.uint8)


def raw_of(rgb, fmt, row_stride=None, offset=0):
    """-> (raw buffer, description, the restatement's gray)."""
    h, w, _ = rgb.shape
    raw = ref.pack(ref.from_rgb(rgb, fmt), fmt, row_stride, offset)
    return raw, capi.make_raw_image(fmt, w, h, row_stride, offset), ref.gray(raw, fmt, w, h, row_stride, offset)


def same(a, b):
    return np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()


def test_frames_from_camera_images(gpu):
    torch, dev = gpu
    K = np.float32(LAUNCH_K)
    W, H = 640, 480
    prm = capi.default_frame_params()
    rgb = colour_of(GOLD["gray0"])
    bgr = raw_of(rgb, ref.BGR8, 3 * W + 20, 2)                      # a padded stride and an offset
    rggb, grbg = raw_of(rgb, ref.BAYER_RGGB8), raw_of(rgb, ref.BAYER_GRBG8)
    assert np.abs(bgr[2].astype(int) - GOLD["gray0"].astype(int)).max() > 3     # the colour does change the gray
    others = [raw_of(colour_of(GOLD["gray3"], 1), ref.BGR8, 3 * W + 20, 2), raw_of(colour_of(GOLD["gray0"], 2), ref.BGR8, 3 * W + 20, 2)]

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    c = capi.Context(0)
    try:
        db = _scene_db(c, bgr[2], K)
        # one image, each format: the frame from the restatement's gray, no format set, against the raw buffer with it
        for raw, d, g in (bgr, rggb, grbg):
            t_g, t_r = dev_of(g), dev_of(raw)
            torch.cuda.synchronize()
            c.frame_set_image_format(None)
            c.frame_enqueue_image(t_g.data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=20)
            want, want_kp = c.frame_fetch(), c.frame_keypoints()
            assert len(want[0]) >= 1, d.format
            c.frame_set_image_format(d)
            c.frame_enqueue_image(t_r.data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=20)
            got = c.frame_fetch()
            assert c.frame_keypoints() == want_kp and same(got, want), d.format
        # a batch of 3 bgr8 images with a padded stride
        three = [bgr] + others
        t_g, t_r = [dev_of(x[2]) for x in three], [dev_of(x[0]) for x in three]
        torch.cuda.synchronize()
        seeds = [31, 32, 33]
        for und in (None, LAUNCH_D):
            c.frame_set_undistort(und)
            c.frame_set_image_format(None)
            c.frame_enqueue_image_batch([t.data_ptr() for t in t_g], W, H, True, CAP, K, CAM0, prm, seeds)
            want = [c.frame_fetch_slot(f) for f in range(3)]
            c.frame_set_image_format(bgr[1])
            c.frame_enqueue_image_batch([t.data_ptr() for t in t_r], W, H, True, CAP, K, CAM0, prm, seeds)
            for f in range(3):
                assert same(c.frame_fetch_slot(f), want[f]), (und, f)
            assert len(want[0][0]) >= 1 and want[0][0].tobytes() != want[1][0].tobytes()
            # one image and a rig of 2 cameras the same way (undistortion, when on, behind the conversion)
            Ks, cams = np.stack([K, K]), np.stack([CAM0, CAM0])
            c.frame_set_image_format(None)
            c.frame_enqueue_image(t_g[0].data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=41)
            want1, kp1 = c.frame_fetch(), c.frame_keypoints()
            c.frame_enqueue_images([t_g[0].data_ptr(), t_g[2].data_ptr()], W, H, True, CAP, Ks, cams, prm, seed=42)
            want2, kp2 = c.frame_fetch(), c.frame_keypoints()
            c.frame_set_image_format(bgr[1])
            c.frame_enqueue_image(t_r[0].data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=41)
            assert same(c.frame_fetch(), want1) and c.frame_keypoints() == kp1, und
            c.frame_enqueue_images([t_r[0].data_ptr(), t_r[2].data_ptr()], W, H, True, CAP, Ks, cams, prm, seed=42)
            assert same(c.frame_fetch(), want2) and c.frame_keypoints() == kp2 and kp2 > kp1, und
            assert len(want1[0]) >= 1 and len(want2[0]) >= 1
        # a size other than the format's is refused, and the frame after it is right
        with pytest.raises(capi.MhError, match="mh_frame_set_image_format"):
            c.frame_enqueue_image(t_r[0].data_ptr(), W, H - 1, True, CAP, K, CAM0, prm, seed=41)
        c.frame_enqueue_image(t_r[0].data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=41)
        assert same(c.frame_fetch(), want1)
        # off again: the gray image gives what a fresh context gives
        c.frame_set_undistort(None)
        c.frame_set_image_format(None)
        c.frame_enqueue_image(t_g[1].data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=50)
        got = c.frame_fetch()
    finally:
        c.close()
    fresh = capi.Context(0)
    try:
        fresh.db_upload(*db[:2], db[2], 2)
        fresh.reserve(4 * CAP)
        fresh.frame_enqueue_image(t_g[1].data_ptr(), W, H, True, CAP, K, CAM0, prm, seed=50)
        assert same(got, fresh.frame_fetch())
    finally:
        fresh.close()


def test_kinect_raw_batch_from_bgr8_images(gpu):
    """FramePipeline.enqueue_kinect_raw_batch, B = 2, with bgr8 images and the format set, against the same call fed the
    converted gray images: image and depth as the sensor delivers them."""
    torch, dev = gpu
    from moped_amd.pipeline import FramePipeline, ShardedDB
    W, H, cap = 640, 480, 2048
    K = synth.K_DEFAULT
    two = [raw_of(colour_of(GOLD["gray0"]), ref.BGR8), raw_of(colour_of(GOLD["gray0"], 2), ref.BGR8, 3 * W + 4, 1)]
    probe = capi.Context(0)
    xy, _, desc = probe.sift(two[0][2])
    probe.close()
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    rng = np.random.default_rng(7)
    db = ShardedDB(np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(np.float32)]),
                   np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)]),
                   np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)]), 2)
    pipe = FramePipeline(0, db, depth=1, max_queries=2 * cap, batch=2)
    try:
        depth = np.full((H, W), 0.8, np.float32)
        depth[:30] = np.nan
        t_z = [torch.from_numpy(depth).to(dev) for _ in range(2)]
        zfmt = capi.make_raw_depth(capi.RAW_DEPTH_F32_M, W, H)
        seeds = [5, 6]
        results = []
        # (the two images have different strides: one description per call, so the second is repacked like the first)
        packed = [two[0], raw_of(colour_of(GOLD["gray0"], 2), ref.BGR8)]
        assert np.array_equal(packed[1][2], two[1][2])
        for fmt, imgs in ((None, [x[2] for x in packed]), (packed[0][1], [x[0] for x in packed])):
            t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in imgs]
            torch.cuda.synchronize()
            pipe.set_image_format(fmt)
            pipe.enqueue_kinect_raw_batch(0, [x.data_ptr() for x in t], [x.data_ptr() for x in t_z], zfmt, W, H, seeds,
                                          fill_scale=8, max_keypoints=cap, keep=(t, t_z))
            results.append([pipe.ctxs[0].frame_fetch_slot(f) for f in range(2)])
            pipe.ctxs[0].depth_fill_status()
        for f in range(2):
            assert same(results[0][f], results[1][f]), f
        assert len(results[0][0][0]) >= 1
        # ... and from host memory in one call: mh_frame_run_kinect_raw_host with the camera's buffer
        c = pipe.ctxs[0]
        c.frame_set_image_format(None)
        want = c.frame_run_kinect_raw_host(two[1][2], depth, zfmt, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap)
        c.frame_set_image_format(two[1][1])
        got = c.frame_run_kinect_raw_host(two[1][0], depth, zfmt, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap,
                                          size=(W, H))
        assert same(got, want) and got[2].tobytes() == want[2].tobytes() and len(want[0]) >= 1
        m = c.depth_map_from_raw(depth, zfmt, K, W, H)
        c.frame_set_image_format(None)
        want = c.frame_run_kinect_host(two[1][2], m, None, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap)
        c.frame_set_image_format(two[1][1])
        got = c.frame_run_kinect_host(two[1][0], m, None, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap)   # (size: the format's)
        assert same(got, want) and len(want[0]) >= 1
        with pytest.raises(ValueError, match="shorter than the extent"):
            c.frame_run_kinect_host(two[1][0][:-1], m, None, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap)
        with pytest.raises(capi.MhError, match="mh_frame_set_image_format"):
            c.frame_run_kinect_host(two[1][0], m[:-1], None, K, synth.CAM_IDENTITY, pipe.params, 9, max_keypoints=cap,
                                    size=(W, H - 1))
    finally:
        pipe.set_image_format(None)
        pipe.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(ctx, gpu):
    torch, dev = gpu
    rng = np.random.default_rng(8)
    w, h = 37, 6
    raw = rng.integers(0, 256, ref.extent(ref.BGR8, w, h), dtype=np.uint8)
    t_raw, p_raw = upload(gpu, raw, 1)
    out = Out(gpu, w, h, 1, 2)
    torch.cuda.synchronize()
    good = capi.make_raw_image(capi.IMAGE_BGR8, w, h)
    INT_MAX = 2 ** 31 - 1

    def refused(what, call):
        with pytest.raises(capi.MhError, match=r"-> -1: mh_image_gray\w*: .*" + what):
            call()

    def fmt(f=capi.IMAGE_BGR8, ww=w, hh=h, rs=None, off=0):
        return capi.make_raw_image(f, ww, hh, rs, off)

    def one(d, raw_ptr=p_raw, out_ptr=out.ptrs[0]):
        return lambda: ctx.image_gray_dev(raw_ptr, d, out_ptr)

    refused("null", one(good, raw_ptr=0))
    refused("null", one(good, out_ptr=0))
    refused("no mh_raw_image", one(None))
    refused("unknown format", one(fmt(9)))
    refused("unknown format", one(fmt(-1)))
    refused("not positive", one(fmt(ww=0, rs=3 * w)))
    refused("not positive", one(fmt(hh=-1)))
    refused("Bayer", one(fmt(capi.IMAGE_BAYER_RGGB8, 2, 3)))
    refused("Bayer", one(fmt(capi.IMAGE_BAYER_GRBG8, 3, 2)))
    refused("negative offset", one(fmt(off=-1)))
    refused("row_stride", one(fmt(rs=3 * w - 1)))
    refused("INT_MAX", one(fmt(rs=2 ** 30, hh=4)))                                     # the extent
    refused("INT_MAX", one(fmt(capi.IMAGE_GRAY8, 65536, 32768)))                        # width times height
    assert capi.raw_image_bytes(fmt(rs=(INT_MAX - 3 * w) // (h - 1))) <= INT_MAX       # (the largest extent is a description)
    refused("MH_MAX_BATCH", lambda: ctx.image_gray_batch_dev([], good, []))
    many = capi.MAX_BATCH + 1
    refused("MH_MAX_BATCH", lambda: ctx.image_gray_batch_dev([p_raw] * many, good, [out.ptrs[0]] * many))
    refused("same output", lambda: ctx.image_gray_batch_dev([p_raw, p_raw], good, [out.ptrs[0], out.ptrs[0]]))
    refused("same output", lambda: ctx.image_gray_batch_dev([p_raw, p_raw], good, [out.ptrs[0], out.ptrs[0] + w * h - 1]))
    refused("overlaps its own raw", one(good, out_ptr=p_raw))
    refused("overlaps its own raw", one(good, out_ptr=p_raw + raw.size - 1))
    refused("overlaps its own raw", one(good, out_ptr=p_raw - w * h + 1))
    buf = raw.copy()
    with pytest.raises(capi.MhError, match="-> -1: mh_image_gray_host: .*overlaps its own raw"):
        ctx._ck(ctx.L.mh_image_gray_host(ctx.h, capi._ptr(buf), good, capi._ptr(buf[8:])), "mh_image_gray_host")
    with pytest.raises(capi.MhError, match="-> -1: mh_frame_set_image_format: .*unknown format"):
        ctx.frame_set_image_format(fmt(12))
    # nothing was launched, nothing written; the valid calls that follow give the right bytes
    ctx.synchronize()
    out.read()
    ctx.image_gray_batch_dev([p_raw, p_raw], good, out.ptrs)
    ctx.synchronize()
    want = ref.gray(raw, ref.BGR8, w, h)
    got = out.read()
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    assert np.array_equal(ctx.image_gray(raw, good), want)
