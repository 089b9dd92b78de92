"""UNDISTORTED_IMAGE: what undistortion costs the image -> objects path.

  undistort_bench.py [rounds=6] [batches=40]
      frames/s of mh_frame_enqueue_image_batch (16 images per call, the reference's bundled 640x480 frames, the launch
      camera of moped2/startmoped.launch) with mh_frame_set_undistort on, off, and on with zero coefficients,
      alternated round by round in one process; prints one JSON line (median of the rounds of each setting).
  undistort_bench.py --kernel B
      launches for a kernel-time run of its own under `rocprofv3 --kernel-trace --stats`: B = 1 -> 200 mh_undistort_dev
      calls on one 640x480 image; B = 16 -> 50 batch frames of 16 images with undistortion on (remap_kernel with
      blockIdx.z = 16)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import undistort_ref as ur  # noqa: E402
from moped_amd import capi, synth  # noqa: E402

B, CAP, MODELS = 16, 1024, 20
K, DIST = (np.float32(v) for v in ur.cameras()["launch"])
CAM0 = synth.CAM_IDENTITY
dev = torch.device("cuda:0")
gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
imgs = [torch.from_numpy(gold[f"gray{int(f)}"]).to(dev) for f in gold["frames"]]
h, w = gold["gray0"].shape


def context():
    """The planar model of frame 0 (as scripts/image_frame_bench.py) next to a synthetic 20-model DB."""
    c = capi.Context(0)
    db = synth.make_db(MODELS, 5000)
    xy, _, desc = c.sift(gold["gray0"])
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1)
    c.db_upload(c.normalize(np.concatenate([db.desc, desc])), np.concatenate([db.model_of, np.full(len(xy), MODELS, np.int32)]),
                np.concatenate([db.xyz, xyz]).astype(np.float32), MODELS + 1)
    c.reserve_batch(CAP, B)
    return c


def run(c, n_batches, prm, cam):
    ptrs = [imgs[j % len(imgs)].data_ptr() for j in range(B)]
    for g in range(n_batches):
        c.frame_enqueue_image_batch(ptrs, w, h, True, CAP, K, CAM0, prm, [g * B + j + 1 for j in range(B)], _cam_struct=cam)
    c.frame_fetch_slot(B - 1)


def main():
    prm = capi.default_frame_params()
    cam = capi.make_cam(K, CAM0)
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel":
        c = context()
        torch.cuda.synchronize()
        if int(sys.argv[2]) == 1:
            out = torch.empty_like(imgs[0])
            for _ in range(200):
                c.undistort_dev(imgs[0].data_ptr(), out.data_ptr(), w, h, K, DIST)
            c.synchronize()
        else:
            c.frame_set_undistort(DIST)
            run(c, 50, prm, cam)
        c.close()
        return
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    c = context()
    torch.cuda.synchronize()
    # "zero": undistortion on with zero coefficients -- the identity map, so FEAT .. FILTER2 see the very images of
    # "off" and the difference is the remap's own cost
    dists = {"on": DIST, "off": None, "zero": np.zeros(4, np.float32)}
    fps = {k: [] for k in dists}
    for setting in dists:   # warm-up: maps, staging, the kernels' first launches
        c.frame_set_undistort(dists[setting])
        run(c, 4, prm, cam)
    orders = [("on", "off", "zero"), ("zero", "off", "on"), ("off", "zero", "on")]
    for r in range(rounds):
        for setting in orders[r % 3]:   # alternated: no setting always goes first
            c.frame_set_undistort(dists[setting])
            t0 = time.perf_counter()
            run(c, n, prm, cam)
            fps[setting].append(n * B / (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in fps.items()}
    on, off = med["on"], med["off"]
    # what FEAT finds in the bundled frames as they are and undistorted (the work downstream of the remap differs)
    kp_off = [len(c.sift(gold[f"gray{int(f)}"])[0]) for f in gold["frames"]]
    kp_on = [len(c.sift(c.undistort(gold[f"gray{int(f)}"], K, DIST))[0]) for f in gold["frames"]]
    print(json.dumps({"metric": "image_to_objects_frames_per_s", "batch": B, "batches_per_round": n, "n_rounds": rounds,
                      "undistort_on": round(on, 1), "undistort_off": round(off, 1),
                      "undistort_zero": round(med["zero"], 1), "on_vs_off": round(on / off - 1, 4),
                      "zero_vs_off": round(med["zero"] / off - 1, 4), "keypoints_on": kp_on, "keypoints_off": kp_off,
                      "rounds": {k: [round(x, 1) for x in v] for k, v in fps.items()}}))
    c.close()


if __name__ == "__main__":
    main()
