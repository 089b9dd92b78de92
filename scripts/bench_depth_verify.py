"""What DEPTH_VERIFY costs: writes profiles/depth_verify.txt.

    python scripts/bench_depth_verify.py [--runs 2] [--parent-lib libmoped_hip_parent.so] [--out profiles/depth_verify.txt]

1  mh_depth_verify alone: 1 / 10 / 64 objects of 5 000-row models (150 matches a model, a 640 x 480 map), device time
   between two events on the context's stream (upload of matches, objects and offsets, the launch, the copy back), both
   device forms, `runs` alternating runs of 10 calls each; the records of the two forms must be equal.  The chain cannot
   be timed apart from the terms inside one launch; form 1 (one wavefront does both) against form 0 (three wavefronts
   produce, one chains) is what the forms allow.  Beside it the same objects by the one-thread numpy restatement
   (tests/depth_verify_ref.py) on the same box, whose records must equal the device's.
2  Kinect batches of 16 (the scene of tests/test_gpu_depth_verify_frame.py: one planted object a frame, SIFT on the
   device, a map per frame) with the step on and off, alternating, host clock around enqueue .. fetch of all 16 frames.
3  bench.py against the parent's library (scripts/ab_lib.sh, alternating rounds), where --parent-lib names a build of the
   parent commit under moped_amd/: with the feature off the new library's rounds must lie inside the parent's spread.
A difference is a claim only where it exceeds three times the spread of the sides compared."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
PRM = (4096.0, 3.0, 2.0, 0.1)
W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_verify.txt"))
    args = ap.parse_args()
    import torch
    import depth_verify_ref as dvr
    from moped_amd import capi, synth
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # ---- 1: the launch alone ----
    K, CAM = synth.K_DEFAULT, synth.CAM_IDENTITY
    rng = np.random.default_rng(5)
    n_models, rows = 20, 5000
    xyz = np.concatenate([rng.uniform(-0.12, 0.12, (n_models * rows, 2)), rng.uniform(-0.002, 0.002, (n_models * rows, 1))], 1).astype(np.float32)
    model_of = np.repeat(np.arange(n_models, dtype=np.int32), rows)
    desc = synth.l2_normalize(rng.normal(size=(len(xyz), 128)).astype(np.float32))
    kp_off = np.arange(n_models + 1, dtype=np.int32) * rows
    truth = np.array([0, 0, 0, 1, 0.0, 0.0, 0.8], np.float32)
    z = np.full((H, W), 0.8, np.float32) * rng.choice([1.004, 3.0, 0.7], (H, W), p=[0.7, 0.15, 0.15]).astype(np.float32)
    depth_img = np.zeros((H, W, 4), np.float32)
    depth_img[..., 2] = z
    fill_img = np.where(rng.random((H, W)) < 0.1, 3.0, 0.0).astype(np.float32)
    m_sizes = np.full(n_models, 150)
    model_off = np.concatenate([[0], np.cumsum(m_sizes)]).astype(np.int32)
    mx = xyz.reshape(n_models, rows, 3)[:, :150].reshape(-1, 3)
    import orclib
    muv = (orclib.project(truth, mx, K, CAM) + rng.normal(0, 0.7, (len(mx), 2))).astype(np.float32)
    c = capi.Context(0)
    c.db_upload(desc, model_of, xyz, n_models)
    c.frame_set_depth_image_host(depth_img, fill_img)
    corr = capi.pack_corr(muv, mx)
    stream = torch.cuda.Stream()
    c.set_stream(stream.cuda_stream)
    say(f"1  mh_depth_verify, {rows}-row models, 150 matches a model, {W} x {H} map: device time between stream events "
        f"(upload + launch + copy back), 10 calls a run, {args.runs} alternating runs")
    for n_obj in (1, 10, 64):
        om = (np.arange(n_obj) % n_models).astype(np.int32)
        op = np.stack([truth + np.concatenate([np.zeros(4), rng.normal(0, 0.003, 3)]).astype(np.float32) for _ in range(n_obj)])
        rec = {}
        times = {0: [], 1: []}
        for run in range(args.runs + 1):          # (run 0: warm-up)
            for form in (0, 1):
                c.depth_verify_debug_form(form)
                ms = []
                for _ in range(10):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    rec[form] = c.depth_verify(corr, model_off, om, op, K, CAM, K, CAM, PRM)
                    e1.record(stream)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                if run:
                    times[form].append(float(np.median(ms)))
        c.depth_verify_debug_form(0)
        assert rec[0].tobytes() == rec[1].tobytes(), "the two forms differ"
        t0 = time.perf_counter()
        want = dvr.depth_verify(muv, mx, model_off, xyz, kp_off, om, op, K, CAM, depth_img, fill_img, K, CAM, PRM)
        host = time.perf_counter() - t0
        same = all(np.array_equal(np.nan_to_num(rec[0][k], nan=-7), np.nan_to_num(want[k], nan=-7)) for k in dvr.WORDS)
        for form in (0, 1):
            v = times[form]
            say(f"   {n_obj:2d} objects, form {form}: call ms (median of 10) per run " + " ".join(f"{x:.3f}" for x in v)
                + f"   us/object {1e3 * float(np.median(v)) / n_obj:8.1f}")
        say(f"   {n_obj:2d} objects, numpy restatement, one thread: {1e3 * host:.1f} ms = {1e6 * host / n_obj:.0f} us/object; "
            f"records equal to the device's: {same}; kept {int(rec[0]['keep'].sum())} of {n_obj}, used {int(rec[0]['used'].mean())} of {rows}")
    c.close()

    # ---- 2: Kinect batches of 16 ----
    import test_gpu_depth_verify_frame as tf
    from moped_amd.pipeline import FramePipeline, ShardedDB

    class World16(tf.World):
        def pipeline(self):
            return FramePipeline(0, ShardedDB(self.db[0], self.db[1], self.db[2], 2), depth=1, max_queries=16 * tf.CAP, batch=16)

    w = World16()
    names, seeds = ["a", "b"] * 8, list(range(61, 77))
    sides = {"off": [], "on": []}
    delivered = {}
    for run in range(args.runs + 2):              # (run 0: warm-up)
        for side in ("off", "on"):
            (w.on if side == "on" else w.off)()
            t0 = time.perf_counter()
            for _ in range(5):
                got = w.batch(names, seeds)
            dt = (time.perf_counter() - t0) / 5
            if run:
                sides[side].append(dt)
            delivered[side] = sum(len(g[0]) for g in got)
    w.close()
    say(f"2  Kinect batches of 16 (image -> SIFT -> MATCH .. FILTER2, a map per frame), enqueue .. fetch of all frames, host clock, "
        f"mean of 5 batches a run, {args.runs + 1} alternating runs")
    for side in ("off", "on"):
        v = sides[side]
        say(f"   step {side:3s}: ms/batch " + " ".join(f"{1e3 * x:.3f}" for x in v) + f"   median {1e3 * float(np.median(v)):.3f}"
            f"   ({delivered[side]} objects delivered in the batch's 16 frames)")
    spread = max(max(v) - min(v) for v in sides.values())
    say(f"   cost of the step per batch: {1e3 * (float(np.median(sides['on'])) - float(np.median(sides['off']))):+.3f} ms (medians); "
        f"largest spread of a side {1e3 * spread:.3f} ms")

    # ---- 3: bench.py against the parent's library ----
    if args.parent_lib and os.path.exists(os.path.join(ROOT, "moped_amd", args.parent_lib)):
        say("3  bench.py, the feature off, the parent's library against this one (scripts/ab_lib.sh, 3 alternating rounds)")
        out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "ab_lib.sh"), "3", args.parent_lib, "libmoped_hip.so"], cwd=ROOT,
                             capture_output=True, text=True, timeout=900)
        for ln in out.stdout.splitlines():
            say("   " + ln)
        if out.returncode:
            say(f"   ab_lib.sh failed ({out.returncode})")
    else:
        say("3  bench.py against the parent's library: not run (no --parent-lib)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
