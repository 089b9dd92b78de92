"""The UNDISTORTED_IMAGE STEP plugin (moped_amd/host/UTIL_UNDISTORT_HIP.hpp) in a pipeline with FEAT_SIFT_HIP, driven by
moped_amd/host/undistort_step_test.cpp: one frame with two images under different cameras, then a second frame with the
cameras swapped (the context's map cache hit).  The plugin's bytes are the restatement's (tests/undistort_ref.py) and
the SIFT step's keypoints are capi.sift's on those bytes."""
import os
import subprocess

import numpy as np
import pytest

import undistort_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
pytestmark = pytest.mark.gpu


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5 %d %d 255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def _parse(text):
    frames = []
    lines = iter(text.splitlines())
    for line in lines:
        if line.startswith("FRAME"):
            frames.append([])
        elif line.startswith("IMAGE"):
            _, _, w, h = line.split()
            data = bytes.fromhex(next(lines).split()[1])
            n = int(next(lines).split()[1])
            kps = np.array([[float(x) for x in next(lines).split()[2:]] for _ in range(n)]).reshape(n, 3)
            frames[-1].append((np.frombuffer(data, np.uint8).reshape(int(h), int(w)), kps))
    return frames


def _checksum(desc):
    """moped_hip_test's sum of descriptor[k] (k + 1): float products, summed in double in order."""
    prod = (desc.astype(np.float32) * np.arange(1, 129, dtype=np.float32)).astype(np.float64)
    return np.add.accumulate(prod, axis=1)[:, -1] if len(prod) else np.zeros(0)


def test_plugin_bytes_and_keypoints(ctx, tmp_path):
    subprocess.check_call(["make", "-s", "-C", HOST, "undistort_step_test"])
    cams = ur.cameras()
    cam_a = cams["launch"]
    cam_b = ([520.0, 515.0, 170.0, 115.0], [0.12, -0.05, 1e-3, -5e-4])
    imgs = [GOLD["gray0"][:240, :320], GOLD["gray3"][100:340, 200:520]]
    paths = []
    for i, img in enumerate(imgs):
        paths.append(str(tmp_path / f"img{i}.pgm"))
        _write_pgm(paths[-1], img)

    def arg(path, cam):
        return [path] + [repr(float(x)) for x in list(cam[0]) + list(cam[1])]

    plan = [[(0, cam_a), (1, cam_b)], [(0, cam_b), (1, cam_a)]]
    argv = [os.path.join(HOST, "undistort_step_test")]
    for f, frame in enumerate(plan):
        if f:
            argv.append("--frame")
        for i, cam in frame:
            argv += arg(paths[i], cam)
    out = subprocess.run(argv, capture_output=True, text=True, timeout=120, check=True).stdout
    frames = _parse(out)
    assert len(frames) == 2 and all(len(fr) == 2 for fr in frames)
    for f, frame in enumerate(plan):
        for k, (i, cam) in enumerate(frame):
            got, kps = frames[f][k]
            want = ur.undistort(imgs[i], *cam)
            assert np.array_equal(got, want), (f, k)
            xy, _, desc = ctx.sift(want)
            assert len(kps) == len(xy) > 0, (f, k)
            assert np.array_equal(kps[:, :2].astype(np.float32), xy), (f, k)
            assert np.array_equal(kps[:, 2], _checksum(desc)), (f, k)
