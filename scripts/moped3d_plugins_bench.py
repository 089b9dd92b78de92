#!/usr/bin/env python3
"""Frames/s of moped3d's pipeline through its STEP plugins (moped_amd/host/moped3d_hip_test --loop N), on scene B of
tests/test_gpu_host_moped3d.py: bundled frame 0 over the 640x480 "blobs" map, unfilled, fill_scale 8, one synchronous
frame at a time.  Three figures: the step wiring (config.hpp:38-49 with the HIP classes, SIFT on the device too), the one
step FRAME_RESIDENT_3D_HIP (--resident), and the same frame composed through capi from device buffers (mh_depth_fill ->
mh_frame_set_depth_image -> mh_frame_enqueue_image -> mh_frame_fetch; the raw map restored by a device copy per frame).

    python scripts/moped3d_plugins_bench.py [N] [out.txt] [--linkage-rowmax]

--linkage-rowmax: CLUSTER in MH_LINKAGE_ROWMAX mode in all three (the harness's flag of that name, linkage_set_mode)."""
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
import dump_scene  # noqa: E402
from moped_amd import capi, moped3d, synth  # noqa: E402
from test_gpu_depthfill import holes  # noqa: E402
from test_gpu_host_moped3d import moped3d_params  # noqa: E402

BIN = os.path.join(ROOT, "moped_amd", "host", "moped3d_hip_test")
K, CAM0, H, W, CAP = synth.K_DEFAULT, synth.CAM_IDENTITY, 480, 640, 1024


def main():
    import torch
    rowmax = "--linkage-rowmax" in sys.argv
    argv = [a for a in sys.argv if a != "--linkage-rowmax"]
    n = int(argv[1]) if len(argv) > 1 else 200
    out = argv[2] if len(argv) > 2 else None
    gray = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))["gray0"])
    c = capi.Context(0)
    xy, _, desc = c.sift(gray)
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    rng = np.random.default_rng(7)
    db_desc = np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(np.float32)])
    db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)])
    model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
    zmap = np.full((H, W), 0.8, np.float32)
    zmap[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = -1.0
    raw = np.zeros((H, W, 4), np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    raw[..., 2] = zmap
    raw[..., 0] = (u - K[2]) / K[0] * zmap
    raw[..., 1] = (v - K[3]) / K[1] * zmap
    raw[..., 3] = np.sqrt((raw[..., :3] ** 2).sum(-1))
    lines = ["scene: bundled frame 0 (%d keypoints) + 500 clutter rows, 640x480 'blobs' map unfilled, fill_scale 8; "
             "%d synchronous frames each, the first not timed%s" % (len(xy), n, "; CLUSTER in MH_LINKAGE_ROWMAX mode" if rowmax else "")]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene_b.bin")
        dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, K, CAM0, gray=gray, patch_size=64, feature_density=0.8,
                               match_density=0.01, fill_scale=8, max_keypoints=CAP)
        for name, args in (("step wiring (11 steps)", []), ("FRAME_RESIDENT_3D_HIP (--resident)", ["--resident"])):
            r = subprocess.run([BIN] + args + (["--linkage-rowmax"] if rowmax else []) + ["--loop", str(n), path], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit("%s: status %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
            fps = re.search(r"^FPS (\S+)", r.stdout, re.M).group(1)
            objs = len(re.findall(r"^OBJ ", r.stdout.split("STEP")[-1], re.M))
            lines.append("%-40s %10s frames/s   (%d objects)" % (name, fps, objs))
    c.db_upload(c.normalize(db_desc), model_of, db_xyz, 2)
    c.reserve(CAP)
    c.frame_set_depth_rules(K, 64, 0.8, 0.01, moped3d.ratio_table(db_xyz, model_of, 2, K))
    c.frame_set_cluster_linkage(capi.default_linkage_params())
    if rowmax:
        c.linkage_set_mode(capi.LINKAGE_ROWMAX)
    dev = torch.device("cuda:0")
    t_gray, t_raw = torch.from_numpy(gray).to(dev), torch.from_numpy(raw).to(dev)
    t_map, t_fill = torch.empty_like(t_raw), torch.zeros((H, W), dtype=torch.float32, device=dev)
    prm = moped3d_params()
    objs = []
    for f in range(n):
        if f == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        t_map.copy_(t_raw)
        torch.cuda.synchronize()
        c.depth_fill_dev(t_map.data_ptr(), W, H, K, t_fill.data_ptr(), 8, False)
        c.frame_set_depth_image(t_map.data_ptr(), t_fill.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        c.frame_enqueue_image(t_gray.data_ptr(), W, H, True, CAP, K, CAM0, prm, 2654435761 * (f + 1))
        objs, _ = c.frame_fetch()
    dt = time.perf_counter() - t0
    lines.append("%-40s %10.2f frames/s   (%d objects)" % ("capi, device buffers (no PCIe copies)", (n - 1) / dt, len(objs)))
    c.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
