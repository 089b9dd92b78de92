"""Plain numpy restatement of UTIL_UNDISTORT (src/util/UTIL_UNDISTORT.hpp), the reference of
moped_amd/csrc/undistort.hip.

The step builds one pair of float maps per camera with cvInitUndistortMap (:68-98): OpenCV 2.x
initUndistortRectifyMap with R = I, the new camera = K and k3 = 0, in double, with a running sum along each row.
It then resamples the 8-bit image with cvRemap(CV_INTER_LINEAR + CV_WARP_FILL_OUTLIERS) (:127): the map in 5-bit
fixed point, bilinear weights that sum to 2^15, taps outside the image read 0.

OpenCV is not part of this project, so nothing here is pinned to an oracle: tests/test_undistort_ref_cpu.py checks
this restatement against an independent float64 witness instead."""
from __future__ import annotations

import json
import os

import numpy as np

F32 = np.float32
CAMERAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort_cameras.json")


def cameras() -> dict:
    """The calibrations the reference ships (name -> (K, dist)), from tests/golden/undistort_cameras.json."""
    with open(CAMERAS) as f:
        d = json.load(f)
    return {k: (v["K"], v["dist"]) for k, v in d.items() if not k.startswith("_")}


# ---- cvInitUndistortMap (:94) -----------------------------------------------------------------------------------
def maps(w, h, K, dist, running=True):
    """-> (mapx, mapy) float32 [h, w].  K and dist are the Image's float calibration (:77-87), widened to double.
    running=False evaluates _x as ir2 + j ir0 instead of the reference's running sum (to size what the last bits of
    the chain can move)."""
    fx, fy, cx, cy = np.asarray(K, F32).astype(np.float64)
    k1, k2, p1, p2 = np.asarray(dist, F32).astype(np.float64)
    k3 = 0.0
    # iR: the inverse of K through its determinant
    d = 1.0 / (fx * fy)
    ir0, ir2, ir4, ir5, ir8 = fy * d, -(cx * fy) * d, fx * d, -(fx * cy) * d, (fx * fy) * d
    i = np.arange(h, dtype=np.float64)[:, None]
    x0 = i * 0.0 + ir2
    if running:   # _x += ir0 after every pixel; np.add.accumulate is sequential
        steps = np.empty((h, w))
        steps[:, :1] = x0
        steps[:, 1:] = ir0
        _x = np.add.accumulate(steps, axis=1)
    else:
        _x = x0 + np.arange(w, dtype=np.float64) * ir0
    _y = i * ir4 + ir5
    _w = i * 0.0 + ir8
    iw = 1.0 / _w
    x, y = _x * iw, _y * iw
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    xy2 = 2 * x * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = fx * (x * kr + p1 * xy2 + p2 * (r2 + 2 * x2)) + cx
    v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * xy2) + cy
    return u.astype(F32), np.broadcast_to(v, (h, w)).astype(F32)


# ---- cvRemap (:127) ---------------------------------------------------------------------------------------------
def fixed(mapx, mapy):
    """-> (sx, sy, ax, ay): X = round-half-even(map 32), sx = X >> 5 saturated to int16, ax = X & 31.  A value that
    does not fit int32, or NaN, becomes INT_MIN, i.e. lands outside the image."""
    def fix5(m):
        v = np.asarray(m, F32) * F32(32)
        ok = (v >= -2.0 ** 31) & (v < 2.0 ** 31)
        return np.where(ok, np.rint(np.where(ok, v, 0)), -2.0 ** 31).astype(np.int64)
    X, Y = fix5(mapx), fix5(mapy)
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31


def remap(img, sx, sy, ax, ay):
    """Bilinear in integers: out = (sum tap w + 2^14) >> 15, taps outside the image read 0."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    src = img.astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)

    s = (tap(sx, sy) * ((32 - ax) * (32 - ay) * 32) + tap(sx + 1, sy) * (ax * (32 - ay) * 32) +
         tap(sx, sy + 1) * ((32 - ax) * ay * 32) + tap(sx + 1, sy + 1) * (ax * ay * 32))
    return ((s + (1 << 14)) >> 15).astype(np.uint8)


def undistort(img, K, dist):
    """UTIL_UNDISTORT::process on one 8-bit image (:121-131)."""
    h, w = np.shape(img)
    return remap(img, *fixed(*maps(w, h, K, dist)))
