"""tests/image_gray_ref.py, the project's definition of the sensor image conversion (mh_image_gray_*), held against
itself and against what its constants mean: the vectorised and the per-pixel form agree, gray stays gray, a Bayer mosaic
of a constant image is that constant, nothing wraps, and the interleaved formats are the luma 0.299 R + 0.587 G + 0.114 B
to within the rounding of the 14-bit coefficients.  No device."""
import os
import subprocess

import numpy as np
import pytest

import image_gray_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(3, 3), (4, 5), (13, 7), (64, 9)]   # (w, h)


def random_raw(fmt, w, h, seed, row_stride=None, offset=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, ref.extent(fmt, w, h, row_stride, offset), dtype=np.uint8)


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_two_forms_agree(fmt, size):
    w, h = size
    b = ref.bpp(fmt)
    for k, (rs, off) in enumerate([(None, 0), (w * b + 5, 3)]):
        raw = random_raw(fmt, w, h, 10 * fmt + k, rs, off)
        fast, slow = ref.gray(raw, fmt, w, h, rs, off), ref.gray_slow(raw, fmt, w, h, rs, off)
        assert fast.dtype == np.uint8 and fast.shape == (h, w)
        assert np.array_equal(fast, slow)


def test_pack_and_pixels_are_inverse():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    raw = ref.pack(px, ref.BGR8, 13 * 3 + 13, 2)
    assert raw.size == ref.extent(ref.BGR8, 13, 7, 13 * 3 + 13, 2)
    assert np.array_equal(ref.pixels(raw, ref.BGR8, 13, 7, 13 * 3 + 13, 2), px)


@pytest.mark.parametrize("fmt", ref.INTERLEAVED, ids=[ref.NAMES[f] for f in ref.INTERLEAVED])
def test_gray_stays_gray(fmt):
    """R = G = B = v gives v for every v: the coefficients sum to 2^14."""
    assert ref.R2Y + ref.G2Y + ref.B2Y == 1 << 14
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rgb = np.stack([v, v, v], axis=2)
    raw = ref.pack(ref.from_rgb(rgb, fmt), fmt)
    assert np.array_equal(ref.gray(raw, fmt, 16, 16), v)


@pytest.mark.parametrize("fmt", ref.BAYER, ids=[ref.NAMES[f] for f in ref.BAYER])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_mosaic_of_a_constant_is_that_constant(fmt, size):
    w, h = size
    for v in (0, 1, 2, 17, 127, 128, 200, 254, 255):
        raw = np.full(w * h, v, np.uint8)
        assert np.array_equal(ref.gray(raw, fmt, w, h), np.full((h, w), v, np.uint8)), v


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
def test_all_255_gives_255(fmt):
    """The largest sums still fit: no wrap-around."""
    w, h = 13, 7
    raw = np.full(ref.extent(fmt, w, h), 255, np.uint8)
    assert np.array_equal(ref.gray(raw, fmt, w, h), np.full((h, w), 255, np.uint8))
    assert np.array_equal(ref.gray_slow(raw, fmt, w, h), np.full((h, w), 255, np.uint8))


@pytest.mark.parametrize("fmt", ref.INTERLEAVED, ids=[ref.NAMES[f] for f in ref.INTERLEAVED])
def test_interleaved_is_the_luma(fmt):
    """|gray - (0.299 R + 0.587 G + 0.114 B)| <= 0.52: 0.5 from the rounding, and 255 times the coefficients' errors
    (|4899 / 2^14 - 0.299| + |9617 / 2^14 - 0.587| + |1868 / 2^14 - 0.114| < 5.1e-5) = 0.013.  Derived, not measured."""
    err = abs(ref.R2Y / 16384 - 0.299) + abs(ref.G2Y / 16384 - 0.587) + abs(ref.B2Y / 16384 - 0.114)
    assert err < 5.1e-5
    rng = np.random.default_rng(77)
    rgb = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    rgb[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    raw = ref.pack(ref.from_rgb(rgb, fmt), fmt)
    luma = 0.299 * rgb[:, :, 0].astype(np.float64) + 0.587 * rgb[:, :, 1] + 0.114 * rgb[:, :, 2]
    assert np.abs(ref.gray(raw, fmt, 64, 64).astype(np.float64) - luma).max() <= 0.52


def test_bayer_formats_differ_by_a_shift():
    """rggb read from (1, 0) on is grbg, from (0, 1) on gbrg, from (1, 1) on bggr: the interiors agree where both are
    interior."""
    rng = np.random.default_rng(9)
    m = rng.integers(0, 256, (12, 14), dtype=np.uint8)
    full = ref.gray(m.reshape(-1), ref.BAYER_RGGB8, 14, 12)
    for fmt, dx, dy in ((ref.BAYER_GRBG8, 1, 0), (ref.BAYER_GBRG8, 0, 1), (ref.BAYER_BGGR8, 1, 1)):
        sub = np.ascontiguousarray(m[dy:, dx:])
        g = ref.gray(sub.reshape(-1), fmt, sub.shape[1], sub.shape[0])
        assert np.array_equal(g[1:-1, 1:-1], full[dy + 1:-1, dx + 1:-1])


def test_bayer_below_3x3_is_refused():
    with pytest.raises(ValueError):
        ref.gray(np.zeros(6, np.uint8), ref.BAYER_RGGB8, 3, 2)
    with pytest.raises(ValueError):
        ref.gray_slow(np.zeros(6, np.uint8), ref.BAYER_GRBG8, 2, 3)


@pytest.mark.parametrize("fmt", ref.FORMATS, ids=ref.NAMES)
@pytest.mark.parametrize("size,pad", [((33, 17), 0), ((33, 17), 7), ((640, 480), 0)], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "pad%d" % v)
def test_host_loop_of_sensor_image_test_equals_the_restatement(tmp_path, fmt, size, pad):
    """The plain C++ loop the host program measures the device against (moped_amd/host/sensor_image_test.cpp --dump: no
    device needed) gives the restatement's bytes, so the program's 0 differing bytes mean the same thing."""
    exe = os.path.join(ROOT, "moped_amd", "host", "sensor_image_test")
    out = str(tmp_path / "dump.bin")
    subprocess.run([exe, "--encoding", ref.NAMES[fmt], "--size", str(size[0]), str(size[1]), "--pad", str(pad), "--dump", out],
                   check=True, timeout=60)
    blob = open(out, "rb").read()
    head = [int(v) for v in np.frombuffer(blob, np.int32, 8)]
    assert head[:3] == [fmt, size[0], size[1]] and head[3] == size[0] * ref.bpp(fmt) + pad
    buf = np.frombuffer(blob, np.uint8, head[5], 32)
    got = np.frombuffer(blob, np.uint8, size[0] * size[1], 32 + head[5]).reshape(size[1], size[0])
    want = ref.gray(buf, *head[:5])
    assert len(np.unique(want)) > 16
    assert np.array_equal(got, want)
