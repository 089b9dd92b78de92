"""The scene of the stand-alone depth steps' tests (test_gpu_depth_steps.py; its oracle-only part runs in
test_moped3d_host_cpu.py): a 320x240 depth map of a tilted plane with a NaN band, a corner beyond MaximumDepth (4 m) and
a block of invalid pixels, and 600 points in 3 groups of unequal size, one of them empty, some of them on the map's last
row and last column and outside it.  PatchSize 32 does not divide the height: the last patch row is half a patch."""
import numpy as np

W, H, PATCH = 320, 240, 32
K = np.array([262.5, 262.5, 160.0, 120.0], np.float32)
GROUP_OFF = np.array([0, 380, 380, 600], np.int32)
# Density: DEPTHFILTER_CPU compares the dilated density with Density * 100 * 100.  The two non-empty groups' point
# densities differ by about their sizes' ratio; 0.03 (filter 300 per square metre) lies between the thin background's
# densities (the oracle's 20th percentiles: 241 and 215) and the blobs' (medians 3166 and 1642), so the oracle keeps the
# blobs and the patches next to them and drops most of the background of both: 85 % of all points as one group, 74 % and
# 69 % of the two groups (oracle_window() asserts between 20 % and 95 % in each).
DENSITY = 0.03


def depth_map():
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    z = (np.float32(0.8) + np.float32(0.002) * xs + np.float32(0.001) * ys).astype(np.float32)
    z[100:110, :] = np.nan                       # a band of NaN depths
    z[200:, :60] = 5.0                           # a corner beyond 4 m
    img = np.zeros((H, W, 4), np.float32)
    img[:, :, 0] = (xs - K[2]) / K[0] * z
    img[:, :, 1] = (ys - K[3]) / K[1] * z
    img[:, :, 2] = z
    with np.errstate(all="ignore"):
        img[:, :, 3] = np.sqrt(img[:, :, 0] ** 2 + img[:, :, 1] ** 2 + z ** 2)
    img[50:60, 100:140, 3] = -1.0                # invalid pixels (negative norm)
    rng = np.random.default_rng(11)
    fill = (rng.random((H, W)) * 0.3).astype(np.float32)
    fill[img[:, :, 3] >= 0] *= (rng.random((H, W)) < 0.5)[img[:, :, 3] >= 0]   # measured pixels: distance 0
    return img, fill.astype(np.float32)


def points():
    """uv [600, 2] in group order: per non-empty group two dense blobs, a thin background over the whole map, and the
    edge cases -- last row, last column, outside the map on every side."""
    rng = np.random.default_rng(7)
    out = []
    for g, n in enumerate(np.diff(GROUP_OFF)):
        if n == 0:
            continue
        edge = np.array([[5.5, H - 0.5], [W - 0.25, 17.0], [W - 0.5, H - 0.5], [W + 10.0, 40.0], [30.0, -5.0],
                         [-3.0, H + 10.0], [W - 1.0, H - 1.0], [200.25, H - 0.75]], np.float32)
        n_blob = int(0.55 * n)
        c0 = np.array([[70.0, 60.0], [250.0, 170.0]][g % 2], np.float32)
        c1 = np.array([[180.0, 215.0], [40.0, 30.0]][g % 2], np.float32)
        blob = np.concatenate([c0 + rng.normal(0, 14, (n_blob // 2, 2)), c1 + rng.normal(0, 10, (n_blob - n_blob // 2, 2))])
        back = rng.random((n - n_blob - len(edge), 2)) * [W, H]
        pts = np.concatenate([blob, back, edge]).astype(np.float32)
        out.append(pts[rng.permutation(len(pts))])
    uv = np.concatenate(out).astype(np.float32)
    assert len(uv) == GROUP_OFF[-1]
    return uv


def inside(uv):
    return (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)


def oracle_window(orclib, img, uv):
    """The oracle's keep flags with one group and with the three, after asserting that they keep between 20 % and 95 %
    of every non-empty group: a filter that keeps or drops everything cannot equal them."""
    one = orclib.depthfilter_keep(img, K, PATCH, DENSITY, uv)
    three = orclib.depthfilter_keep(img, K, PATCH, DENSITY, uv, GROUP_OFF)
    assert 0.20 <= one.mean() <= 0.95, one.mean()
    for g in range(len(GROUP_OFF) - 1):
        a, b = GROUP_OFF[g], GROUP_OFF[g + 1]
        if b > a:
            assert 0.20 <= three[a:b].mean() <= 0.95, (g, three[a:b].mean())
    return one, three
