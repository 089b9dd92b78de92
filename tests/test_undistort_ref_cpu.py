"""tests/undistort_ref.py, the reference of tests/test_gpu_undistort.py, against what can be known without OpenCV:
the identity for zero coefficients, a half-pixel shift by hand, the zero border, an independent float64 witness
(the distortion model evaluated per pixel, plain float64 bilinear sampling), and the size of what the last bits of
the double chain can move."""
import numpy as np

import undistort_ref as ur

LAUNCH = ur.cameras()["launch"]


def _witness_maps(w, h, K, dist):
    """The distortion model per pixel, directly: (x, y) = ((j - cx) / fx, (i - cy) / fy)."""
    fx, fy, cx, cy = np.asarray(K, np.float32).astype(np.float64)
    k1, k2, p1, p2 = np.asarray(dist, np.float32).astype(np.float64)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (j - cx) / fx, (i - cy) / fy
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2
    u = fx * (x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
    v = fy * (y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
    return u, v


def _witness_sample(img, u, v):
    """Plain float64 bilinear sampling, zero outside the image, rounded to u8."""
    h, w = img.shape
    src = img.astype(np.float64)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0.0)

    s = (tap(x0, y0) * (1 - fx) * (1 - fy) + tap(x0 + 1, y0) * fx * (1 - fy) + tap(x0, y0 + 1) * (1 - fx) * fy +
         tap(x0 + 1, y0 + 1) * fx * fy)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def _smooth_image(w, h, seed):
    """A texture whose gradient stays below 20 levels per pixel: the 1/32-pixel grid of the fixed-point positions
    then moves a byte by less than one level."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    img = 128.0
    for _ in range(4):
        a, b, ph = rng.uniform(-0.06, 0.06, 2).tolist() + [rng.uniform(0, 6.3)]
        img = img + 30 * np.sin(a * j + b * i + ph)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _random_cameras(n, w, h, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        f = rng.uniform(400, 1200)
        K = [f, f * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20)]
        dist = [rng.uniform(-0.3, 0.2), rng.uniform(-0.1, 0.2), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3)]
        out.append((K, dist))
    return out


def test_zero_and_node_default_coefficients_are_the_identity():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    cams = ur.cameras()
    for K, dist in [(LAUNCH[0], [0, 0, 0, 0]), cams["node_default"], cams["kinect_rgb"], cams["kinect_depth"]]:
        sx, sy, ax, ay = ur.fixed(*ur.maps(640, 480, K, dist))
        j, i = np.meshgrid(np.arange(640), np.arange(480))
        assert np.array_equal(sx, j) and np.array_equal(sy, i) and not ax.any() and not ay.any()
        assert np.array_equal(ur.undistort(img, K, dist), img)


def test_half_pixel_shift_by_hand():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    j, i = np.meshgrid(np.arange(8, dtype=np.float32), np.arange(6, dtype=np.float32))
    out = ur.remap(img[:, :8], *ur.fixed(j + 0.5, i))
    a, b = img[:, :8].astype(int), np.concatenate([img[:, 1:8], np.zeros((6, 1), np.uint8)], 1).astype(int)
    assert np.array_equal(out, ((a + b + 1) >> 1).astype(np.uint8))
    # the weights (16 32 32) each: 2^14 a + 2^14 b + 2^14 >> 15 = (a + b + 1) >> 1, by hand for one pixel
    assert ur.remap(np.array([[7, 10]], np.uint8), *ur.fixed(np.float32([[0.5]]), np.float32([[0]])))[0, 0] == 9


def test_border_taps_read_zero():
    img = np.full((4, 5), 200, np.uint8)
    mx = np.float32([[-0.5, 4.5, 2.0, 2.0, -1.0, 5.0, -40.0, np.nan, 3e9]])
    my = np.float32([[1.0, 1.0, -0.5, 3.5, 1.0, 1.0, 1.0, 1.0, 1.0]])
    out = ur.remap(img, *ur.fixed(mx, my))[0]
    # half a pixel beyond the left / right / top / bottom edge: half the weight on taps that read 0
    assert out[:4].tolist() == [100, 100, 100, 100]
    # all four taps outside, NaN, a value beyond int32: 0
    assert out[4:].tolist() == [0, 0, 0, 0, 0]


def test_float64_witness_agrees():
    w, h = 640, 480
    img = _smooth_image(w, h, 3)
    for K, dist in [LAUNCH] + _random_cameras(3, w, h):
        mx, my = ur.maps(w, h, K, dist)
        u, v = _witness_maps(w, h, K, dist)
        assert np.abs(mx - u).max() < 1e-3 and np.abs(my - v).max() < 1e-3
        out, wit = ur.undistort(img, K, dist), _witness_sample(img, u, v)
        inner = (u >= 1) & (u <= w - 2) & (v >= 1) & (v <= h - 2)
        diff = np.abs(out.astype(int) - wit.astype(int))
        assert inner.mean() > 0.5 and diff[inner].max() <= 1
        outside = (u < -1) | (u > w) | (v < -1) | (v > h)
        assert not out[outside].any() and not wit[outside].any()


def test_running_sum_moves_no_fixed_point_entry_of_the_launch_camera():
    """What the unpinned last bits of the double chain can move: 0 entries for the launch camera at 640x480."""
    run = ur.fixed(*ur.maps(640, 480, *LAUNCH, running=True))
    direct = ur.fixed(*ur.maps(640, 480, *LAUNCH, running=False))
    changed = np.zeros((480, 640), bool)
    for a, b in zip(run, direct):
        changed |= a != b
    assert int(changed.sum()) == 0
    # ... and the launch camera does move pixels: up to 14 px, by more than POSE's sqrt(10) px on a good part
    mx, my = ur.maps(640, 480, *LAUNCH)
    j, i = np.meshgrid(np.arange(640), np.arange(480))
    shift = np.hypot(mx - j, my - i)
    assert 12 < shift.max() < 15 and (shift > np.sqrt(10)).mean() > 0.4
