"""The project's definition of the sensor image conversion (mh_image_gray_*, csrc/image_gray.hip) in numpy: what
cv_bridge's "mono8" (moped3d/moped3d.cpp:249) gives for 8-bit gray, interleaved colour and Bayer images, restated from
knowledge of OpenCV 2.x cvtColor WITHOUT OpenCV at hand -- unpinned, and integers only, hence bit for bit.

  gray8        the byte
  interleaved  (R2Y R + G2Y G + B2Y B + 8192) >> 14, alpha ignored
  Bayer        the four letters of the name are the top-left 2 x 2 row by row: the colour of (x, y) is c[y & 1][x & 1].
               Interior (1 <= x <= w - 2, 1 <= y <= h - 2), p the site's byte:
                 R / B site, own colour o, opposite q:
                   (C(q) (4 diagonal) + G2Y (4 edge) + 4 C(o) p + 32768) >> 16
                 G site, ch the colour of (x + 1, y), cv that of (x, y + 1):
                   (C(ch) (left + right) + C(cv) (up + down) + 2 G2Y p + 16384) >> 15
               gray(0, y) = gray(1, y), gray(w - 1, y) = gray(w - 2, y) for the interior rows; then row 0 = row 1 and
               row h - 1 = row h - 2, whole rows.

gray() is the vectorised form, gray_slow() the per-pixel one in Python integers; tests/test_image_gray_cpu.py holds them
against each other.  A raw buffer is a flat uint8 array read at offset + y row_stride + x bpp.
"""
import numpy as np

R2Y, G2Y, B2Y = 4899, 9617, 1868

GRAY8, BGR8, RGB8, BGRA8, RGBA8, BAYER_RGGB8, BAYER_BGGR8, BAYER_GBRG8, BAYER_GRBG8 = range(9)   # MH_IMAGE_*
FORMATS = list(range(9))
INTERLEAVED = [BGR8, RGB8, BGRA8, RGBA8]
BAYER = [BAYER_RGGB8, BAYER_BGGR8, BAYER_GBRG8, BAYER_GRBG8]
NAMES = ["mono8", "bgr8", "rgb8", "bgra8", "rgba8", "bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8"]

_BPP = {GRAY8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
_R_AT = {BGR8: 2, RGB8: 0, BGRA8: 2, RGBA8: 0}            # byte of R inside a pixel; G is byte 1, B is byte 2 - that
_LETTERS = {BAYER_RGGB8: "rggb", BAYER_BGGR8: "bggr", BAYER_GBRG8: "gbrg", BAYER_GRBG8: "grbg"}
_COEF = {"r": R2Y, "g": G2Y, "b": B2Y}


def bpp(fmt):
    return _BPP.get(fmt, 1)


def extent(fmt, w, h, row_stride=None, offset=0):
    """Bytes of the raw buffer a description speaks of."""
    rs = w * bpp(fmt) if row_stride is None else row_stride
    return offset + (h - 1) * rs + w * bpp(fmt)


def site_colour(fmt, x, y):
    """'r', 'g' or 'b': the colour of site (x, y) of a Bayer format."""
    return _LETTERS[fmt][2 * (y & 1) + (x & 1)]


def pixels(raw, fmt, w, h, row_stride=None, offset=0):
    """The [h, w, bpp] bytes a description addresses inside the flat uint8 buffer `raw` (a copy)."""
    b = bpp(fmt)
    rs = w * b if row_stride is None else row_stride
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    assert extent(fmt, w, h, rs, offset) <= raw.size
    idx = offset + np.arange(h)[:, None, None] * rs + np.arange(w)[None, :, None] * b + np.arange(b)[None, None, :]
    return raw[idx]


def pack(px, fmt, row_stride=None, offset=0, fill=0x5A, tail=0):
    """The inverse: px [h, w, bpp] (or [h, w]) -> a flat raw buffer of extent + tail bytes, `fill` between the pixels."""
    px = np.asarray(px, np.uint8)
    if px.ndim == 2:
        px = px[:, :, None]
    h, w, b = px.shape
    assert b == bpp(fmt)
    rs = w * b if row_stride is None else row_stride
    raw = np.full(extent(fmt, w, h, rs, offset) + tail, fill, np.uint8)
    idx = offset + np.arange(h)[:, None, None] * rs + np.arange(w)[None, :, None] * b + np.arange(b)[None, None, :]
    raw[idx] = px
    return raw


def from_rgb(rgb, fmt, alpha=0xC3):
    """An [h, w, 3] R, G, B image as the pixels of `fmt`: reordered, with alpha, or sampled as that Bayer mosaic."""
    rgb = np.asarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    if fmt == GRAY8:
        raise ValueError("gray8 has no colour")
    if fmt in INTERLEAVED:
        out = np.full((h, w, _BPP[fmt]), alpha, np.uint8)
        out[:, :, _R_AT[fmt]] = rgb[:, :, 0]
        out[:, :, 1] = rgb[:, :, 1]
        out[:, :, 2 - _R_AT[fmt]] = rgb[:, :, 2]
        return out
    out = np.zeros((h, w, 1), np.uint8)
    for py in range(2):
        for px in range(2):
            ch = "rgb".index(site_colour(fmt, px, py))
            out[py::2, px::2, 0] = rgb[py::2, px::2, ch]
    return out


def _bayer(p, fmt):
    h, w = p.shape
    if w < 3 or h < 3:
        raise ValueError("Bayer needs w >= 3 and h >= 3")
    p = p.astype(np.uint32)
    # coefficient of every site's own colour, and whether it is a G site
    coef = np.zeros((h + 1, w + 1), np.uint32)
    is_g = np.zeros((h + 1, w + 1), bool)
    for py in range(2):
        for px in range(2):
            c = site_colour(fmt, px, py)
            coef[py::2, px::2] = _COEF[c]
            is_g[py::2, px::2] = c == "g"
    c = p[1:-1, 1:-1]
    up, down, left, right = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    diag = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    own = coef[1:h - 1, 1:w - 1]
    ch = coef[1:h - 1, 2:w]          # the colour of (x + 1, y)
    cv = coef[2:h, 1:w - 1]          # the colour of (x, y + 1)
    opposite = np.uint32(R2Y + B2Y) - own   # at an R or B site
    at_c = (opposite * diag + np.uint32(G2Y) * (up + down + left + right) + np.uint32(4) * own * c + np.uint32(32768)) >> 16
    at_g = (ch * (left + right) + cv * (up + down) + np.uint32(2 * G2Y) * c + np.uint32(16384)) >> 15
    g = np.zeros((h, w), np.uint32)
    g[1:-1, 1:-1] = np.where(is_g[1:h - 1, 1:w - 1], at_g, at_c)
    g[1:-1, 0] = g[1:-1, 1]
    g[1:-1, -1] = g[1:-1, -2]
    g[0] = g[1]
    g[-1] = g[-2]
    assert g.max() <= 255
    return g.astype(np.uint8)


def gray(raw, fmt, w, h, row_stride=None, offset=0):
    """The gray image [h, w] uint8 of a raw buffer: the vectorised form."""
    px = pixels(raw, fmt, w, h, row_stride, offset)
    if fmt == GRAY8:
        return px[:, :, 0].copy()
    if fmt in INTERLEAVED:
        p = px.astype(np.uint32)
        r, g, b = p[:, :, _R_AT[fmt]], p[:, :, 1], p[:, :, 2 - _R_AT[fmt]]
        return ((np.uint32(R2Y) * r + np.uint32(G2Y) * g + np.uint32(B2Y) * b + np.uint32(8192)) >> 14).astype(np.uint8)
    if fmt in BAYER:
        return _bayer(px[:, :, 0], fmt)
    raise ValueError("unknown format")


def gray_slow(raw, fmt, w, h, row_stride=None, offset=0):
    """The same pixel by pixel in Python integers, straight from the text above."""
    b = bpp(fmt)
    rs = w * b if row_stride is None else row_stride
    raw = [int(v) for v in np.ascontiguousarray(raw, np.uint8).reshape(-1)]

    def at(x, y, k=0):
        return raw[offset + y * rs + x * b + k]

    out = np.zeros((h, w), np.uint8)
    if fmt == GRAY8:
        for y in range(h):
            for x in range(w):
                out[y, x] = at(x, y)
        return out
    if fmt in INTERLEAVED:
        for y in range(h):
            for x in range(w):
                r, g, bl = at(x, y, _R_AT[fmt]), at(x, y, 1), at(x, y, 2 - _R_AT[fmt])
                out[y, x] = (R2Y * r + G2Y * g + B2Y * bl + 8192) >> 14
        return out
    if fmt not in BAYER:
        raise ValueError("unknown format")
    if w < 3 or h < 3:
        raise ValueError("Bayer needs w >= 3 and h >= 3")
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            o = site_colour(fmt, x, y)
            p = at(x, y)
            if o == "g":
                ch, cv = _COEF[site_colour(fmt, x + 1, y)], _COEF[site_colour(fmt, x, y + 1)]
                v = (ch * (at(x - 1, y) + at(x + 1, y)) + cv * (at(x, y - 1) + at(x, y + 1)) + 2 * G2Y * p + 16384) >> 15
            else:
                q = "b" if o == "r" else "r"
                diag = at(x - 1, y - 1) + at(x + 1, y - 1) + at(x - 1, y + 1) + at(x + 1, y + 1)
                edge = at(x, y - 1) + at(x, y + 1) + at(x - 1, y) + at(x + 1, y)
                v = (_COEF[q] * diag + G2Y * edge + 4 * _COEF[o] * p + 32768) >> 16
            assert 0 <= v <= 255
            out[y, x] = v
    for y in range(1, h - 1):
        out[y, 0] = out[y, 1]
        out[y, w - 1] = out[y, w - 2]
    out[0, :] = out[1, :]
    out[h - 1, :] = out[h - 2, :]
    return out
