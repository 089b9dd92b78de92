#!/usr/bin/env python3
"""Frames/s of moped3d's step wiring and of the one step FRAME_RESIDENT_3D_HIP (moped_amd/host/moped3d_hip_test [--resident]
--loop N) on the scene of
scripts/moped3d_plugins_bench.py -- bundled frame 0 over the 640x480 "blobs" map, one planar model of 586 keypoints -- with
each clusterer in the CLUSTER slot: CLUSTER_LINKAGE_HIP as shipped, the same in MH_LINKAGE_ROWMAX mode, and
CLUSTER_WEIGHTED_MEAN_SHIFT_HIP (--cluster-wms) with a Radius that holds the whole object and with a small one.

    python scripts/wms_steps_bench.py [N] [out.txt]

Two rounds, the configurations alternating; per configuration the objects of the last frame and the model's clusters."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import dump_scene  # noqa: E402
from moped_amd import capi, synth  # noqa: E402
from test_gpu_depthfill import holes  # noqa: E402

BIN = os.path.join(ROOT, "moped_amd", "host", "moped3d_hip_test")
K, CAM0, H, W, CAP = synth.K_DEFAULT, synth.CAM_IDENTITY, 480, 640, 1024
CONFIGS = (("CLUSTER_LINKAGE_HIP (default)", []),
           ("CLUSTER_LINKAGE_HIP, row maxima", ["--linkage-rowmax"]),
           ("CLUSTER_WEIGHTED_MEAN_SHIFT_HIP R 0.7 M 0.05", ["--cluster-wms", "0.7", "0.05", "7", "100", "10"]),
           ("CLUSTER_WEIGHTED_MEAN_SHIFT_HIP R 0.1 M 0.02", ["--cluster-wms", "0.1", "0.02", "7", "100", "10"]))


WIRED = tuple((name, args) for name, args in CONFIGS) + tuple(("one step: " + name.replace("_HIP", ""), ["--resident"] + args)
                                                             for name, args in CONFIGS)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    out = sys.argv[2] if len(sys.argv) > 2 else None
    gray = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))["gray0"])
    c = capi.Context(0)
    xy, _, desc = c.sift(gray)
    c.close()
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
    lines = ["scene: bundled frame 0 (%d keypoints) + 500 clutter rows, 640x480 'blobs' map unfilled, fill_scale 8; step wiring "
             "(11 steps), %d synchronous frames each, the first not timed; two rounds, the configurations alternating" % (len(xy), n)]
    fps = {name: [] for name, _ in WIRED}
    info = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene_b.bin")
        dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, K, CAM0, gray=gray, patch_size=64, feature_density=0.8,
                               match_density=0.01, fill_scale=8, max_keypoints=CAP)
        for _ in range(2):
            for name, args in WIRED:
                r = subprocess.run([BIN] + args + ["--loop", str(n), path], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("%s: status %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
                fps[name].append(float(re.search(r"^FPS (\S+)", r.stdout, re.M).group(1)))
                last = r.stdout.split("STEP")[-1]
                cl = r.stdout.split("STEP DEPTHFILL" if "--resident" in args else "STEP CLUSTER")[-1].split("STEP")[0]
                sizes = [len(line.split()) - 3 for line in cl.splitlines() if line.startswith("CLUSTER 0 ")]
                info[name] = (len(re.findall(r"^OBJ ", last, re.M)), len(re.findall(r"^MATCH 0 ", cl, re.M)), sizes)
    for name, _ in WIRED:
        objs, matches, sizes = info[name]
        lines.append("%-56s %8.2f / %8.2f frames/s   (%d objects; model 0: %d matches, clusters of %s)"
                     % (name, fps[name][0], fps[name][1], objs, matches, sizes))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
