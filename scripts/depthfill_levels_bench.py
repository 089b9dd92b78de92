#!/usr/bin/env python3
"""mh_depth_fill in its two modes (mh_depth_fill_set_mode: REPLAY, the one-wavefront replay of the FIFO queue, against
LEVELS, the queue generation by generation) on device-resident maps, the hole patterns of tests/test_gpu_depthfill.py:

  * ms per call at 640x480 factor 8 ('blobs', 'sparse', 'one_valid', and the holed plane of scene B below) in both
    modes, alternating, three rounds;
  * mh_depth_fill_batch of 16 'blobs' maps in both modes;
  * LEVELS alone where the replay refuses the map: (480, 640, 4), (480, 640, 2), (960, 1280, 8), (240, 320, 1) 'blobs';
  * moped3d_hip_test --loop N on scene B of tests/test_gpu_host_moped3d.py: frames/s of the eleven-step and the one-step
    wiring, with and without --level-fill.

Every timed call restores the raw map by a device copy first, on the stream the context fills on (the fill rewrites the
map in place: a copy on another stream would not be ordered before it, and all fills of a window but the first would find
a map without holes); the copy alone is timed too and subtracted.  Host clock around a window that ends in a device
synchronise.

    python scripts/depthfill_levels_bench.py [--loop N] [--no-plugins] [out.txt]"""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
from moped_amd import capi, synth  # noqa: E402
from test_gpu_depthfill import K, holes  # noqa: E402

BIN = os.path.join(ROOT, "moped_amd", "host", "moped3d_hip_test")
MODES = (("REPLAY", capi.DEPTH_FILL_REPLAY), ("LEVELS", capi.DEPTH_FILL_LEVELS))


def window(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fills(c, lines, maps, scale, modes, label, reps):
    """ms per call of the fill of `maps` (one: mh_depth_fill, more: mh_depth_fill_batch), copy of the raw maps excluded."""
    import torch
    dev = torch.device("cuda:0")
    h, w = maps[0].shape[:2]
    src = [torch.from_numpy(m).to(dev) for m in maps]
    work = [torch.empty_like(s) for s in src]
    fill = [torch.empty((h, w), dtype=torch.float32, device=dev) for _ in maps]

    def copy():
        for a, b in zip(work, src):
            a.copy_(b)

    def once():
        copy()
        if len(maps) == 1:
            c.depth_fill_dev(work[0].data_ptr(), w, h, K, fill[0].data_ptr(), scale)
        else:
            c.depth_fill_batch_dev([t.data_ptr() for t in work], [t.data_ptr() for t in fill], w, h, K, scale)

    t_copy = window(copy, reps)
    res = {name: [] for name, _ in modes}
    for _ in range(3):
        for name, mode in modes:
            c.depth_fill_set_mode(mode)
            res[name].append(window(once, reps) - t_copy)
    c.depth_fill_status()
    c.depth_fill_set_mode(capi.DEPTH_FILL_LEVELS)
    once()
    st = c.depth_fill_stats(0)
    c.depth_fill_set_mode(capi.DEPTH_FILL_REPLAY)
    txt = "   ".join("%s %s ms" % (name, " / ".join("%.3f" % v for v in res[name])) for name, _ in modes)
    lines.append("%-34s %s   (copy %.3f ms excluded; frame 0: %d generations, largest %d, %d elements)"
                 % (label, txt, t_copy, st[0], st[1], st[2]))
    print(lines[-1], flush=True)


def kinect_map():
    """Scene B's raw map: the z = 0.8 plane under synth.K_DEFAULT with the 'blobs' holes of seed 3."""
    H, W, Ks = 480, 640, synth.K_DEFAULT
    zmap = np.full((H, W), 0.8, np.float32)
    zmap[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = -1.0
    raw = np.zeros((H, W, 4), np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    raw[..., 2] = zmap
    raw[..., 0] = (u - Ks[2]) / Ks[0] * zmap
    raw[..., 1] = (v - Ks[3]) / Ks[1] * zmap
    raw[..., 3] = np.sqrt((raw[..., :3] ** 2).sum(-1))
    return raw


def plugins(lines, n):
    import dump_scene
    H, W, CAP, Ks, CAM0 = 480, 640, 1024, synth.K_DEFAULT, synth.CAM_IDENTITY
    gray = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))["gray0"])
    c = capi.Context(0)
    xy, _, desc = c.sift(gray)
    c.close()
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - Ks[2]) / Ks[0] * z, (xy[:, 1] - Ks[3]) / Ks[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    rng = np.random.default_rng(7)
    db_desc = np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(np.float32)])
    db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)])
    model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
    raw = kinect_map()
    lines.append("moped3d_hip_test --loop %d: bundled frame 0 (%d keypoints) + 500 clutter rows, 640x480 'blobs' map unfilled, "
                 "fill_scale 8, one synchronous frame at a time" % (n, len(xy)))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene_b.bin")
        dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, Ks, CAM0, gray=gray, patch_size=64, feature_density=0.8,
                               match_density=0.01, fill_scale=8, max_keypoints=CAP)
        for name, args in (("step wiring (11 steps)", []), ("step wiring, --level-fill", ["--level-fill"]),
                           ("FRAME_RESIDENT_3D_HIP (--resident)", ["--resident"]),
                           ("--resident --level-fill", ["--resident", "--level-fill"])):
            r = subprocess.run([BIN] + args + ["--loop", str(n), path], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit("%s: status %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
            fps = re.search(r"^FPS (\S+)", r.stdout, re.M).group(1)
            objs = len(re.findall(r"^OBJ ", r.stdout.split("STEP")[-1], re.M))
            lines.append("%-40s %10s frames/s   (%d objects)" % (name, fps, objs))
            print(lines[-1], flush=True)


def main():
    args = sys.argv[1:]
    n, with_plugins, out = 200, True, None
    while args:
        a = args.pop(0)
        if a == "--loop":
            n = int(args.pop(0))
        elif a == "--no-plugins":
            with_plugins = False
        else:
            out = a
    lines = ["mh_depth_fill, ms per call on device maps (three rounds, the modes alternating)"]
    import torch
    c = capi.Context(0)
    st = torch.cuda.Stream()                 # (not torch's default stream: its handle is 0, which mh_set_stream reads as "your own")
    c.set_stream(st.cuda_stream)             # the restoring copy and the fill on ONE stream, in order
    torch.cuda.set_stream(st)
    rng = lambda: np.random.default_rng(0)  # noqa: E731
    for kind in ("blobs", "sparse", "one_valid"):
        fills(c, lines, [holes(kind, 480, 640, rng())], 8, MODES, "640x480 / 8 %s" % kind, 500)
    fills(c, lines, [kinect_map()], 8, MODES, "640x480 / 8 scene B's map", 100)
    fills(c, lines, [holes("blobs", 480, 640, np.random.default_rng(i)) for i in range(16)], 8, MODES,
          "batch of 16, 640x480 / 8 blobs", 100)
    for h, w, scale in ((480, 640, 4), (480, 640, 2), (960, 1280, 8), (240, 320, 1)):
        fills(c, lines, [holes("blobs", h, w, rng())], scale, MODES[1:], "%dx%d / %d blobs" % (w, h, scale), 50)
    c.close()
    if with_plugins:
        plugins(lines, n)
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
