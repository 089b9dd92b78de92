"""What object hulls cost: writes profiles/object_hulls.txt.

    python scripts/bench_object_hulls.py [--rounds 3] [--steps 12] [--out profiles/object_hulls.txt]

1  Config 1 (20 models x 5 000 points, two visible objects, 3 000 keypoints) in batches of 16 over 16 slots, objects
   delivered into pinned memory: frames/s with hulls off, on, and on with the hull block delivered too -- the three
   sides alternate, `rounds` rounds each, after a warm-up of every side; the range of each side is its spread.
2  mh_object_hulls alone: 160 objects (a batch of 16 frames x 10) of 5 000-point models, device time between two
   events on the context's stream (upload of models and poses, the launch, the copy back), both forms; the share of
   points that survive the prefilter and the vertices per hull.
3  The same hulls by a plain host loop on one thread (moped_amd/host/object_hulls_test, `loops` argument), in us/hull,
   and the device through getObjectHulls_HIP (a synchronous round trip per call) beside it.
A difference is a claim only where it exceeds three times the spread of the sides compared."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

Q, B, SLOTS, MAXV = 3000, 16, 16, 64


def frames_side(pipe, torch, qd, uv, work, steps, hulls, deliver_hulls):
    """steps x SLOTS batches through the slots; -> frames/s (host clock around work that ends in the last delivery)."""
    pipe.set_hulls(MAXV if hulls else 0)
    pending = set()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(steps):
        for s in range(SLOTS):
            if s in pending:
                pipe.take_delivery(s)
            with torch.cuda.stream(pipe.streams[s]):
                work[s].copy_(qd, non_blocking=True)
            pipe.enqueue_batch(s, work[s], uv, B, [1000 * r + 16 * s + f + 1 for f in range(B)])
            pipe.deliver(s, tag=s, hulls=deliver_hulls)
            pending.add(s)
    for s in pending:
        pipe.take_delivery(s)
    dt = time.perf_counter() - t0
    return steps * SLOTS * B / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_hulls.txt"))
    args = ap.parse_args()
    import torch
    import hull_ref
    from moped_amd import capi, synth
    from moped_amd.pipeline import FramePipeline, ShardedDB
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    db = synth.make_db(20, 5000)
    frames = [synth.make_frame(db, n_vis=2, seed=100 + i, Q=Q) for i in range(B)]
    qd = torch.cat([torch.from_numpy(f.desc) for f in frames]).to(dev)
    uv = torch.cat([torch.from_numpy(f.uv) for f in frames]).to(dev)
    pipe = FramePipeline(0, ShardedDB(db.desc, db.xyz, db.model_of, db.n_models), depth=SLOTS, max_queries=B * Q, batch=B)
    pipe.attach_delivery(max_objects=16, B=B)
    work = [torch.empty_like(qd) for _ in range(SLOTS)]
    sides = [("hulls off", False, False), ("hulls on", True, False), ("hulls on + hull block delivered", True, True)]
    for name, h, d in sides:                      # warm-up of every side
        frames_side(pipe, torch, qd, uv, work, 2, h, d)
    got = {name: [] for name, _, _ in sides}
    for _ in range(args.rounds):
        for name, h, d in sides:
            got[name].append(frames_side(pipe, torch, qd, uv, work, args.steps, h, d))
    say(f"1  config 1, batches of {B} over {SLOTS} slots, {args.steps * SLOTS * B} frames per figure, {args.rounds} alternating rounds")
    for name, _, _ in sides:
        v = got[name]
        say(f"   {name:34s} frames/s  min {min(v):9.1f}  median {float(np.median(v)):9.1f}  max {max(v):9.1f}   us/frame {1e6 / float(np.median(v)):7.2f}")
    off, on = float(np.median(got["hulls off"])), float(np.median(got["hulls on"]))
    spread = max(max(v) - min(v) for v in got.values())
    say(f"   cost of hulls per frame: {1e6 / on - 1e6 / off:+.2f} us (medians); largest spread of a side {spread:.1f} frames/s "
        f"= {1e6 / off - 1e6 / (off + spread):.2f} us/frame at the off side's rate")
    pipe.set_hulls(0)

    # 2: the launch alone
    c = pipe.ctxs[0]
    stream = pipe.streams[0]
    rng = np.random.default_rng(3)
    n_obj = 160
    model = rng.integers(0, db.n_models, n_obj).astype(np.int32)
    pose = np.stack([np.concatenate([synth.random_quat(rng), [rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(0.6, 1.2)]])
                     for _ in range(n_obj)]).astype(np.float32)
    say(f"2  mh_object_hulls, {n_obj} objects of 5 000-point models, device time between stream events (upload + launch + copy back)")
    for form in (0, 1):
        c.hull_debug_form(form)
        for _ in range(3):
            res = c.object_hulls(model, pose, synth.K_DEFAULT, synth.CAM_IDENTITY, MAXV)
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            res = c.object_hulls(model, pose, synth.K_DEFAULT, synth.CAM_IDENTITY, MAXV)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        say(f"   form {form}: us/object  min {1e3 * min(ms) / n_obj:7.2f}  median {1e3 * float(np.median(ms)) / n_obj:7.2f}  max {1e3 * max(ms) / n_obj:7.2f}"
            f"   (call: {float(np.median(ms)):.3f} ms)   vertices/hull {float(np.mean(res[1])):.1f} (max {int(max(res[1]))})")
    c.hull_debug_form(0)
    share = []
    for o in range(0, n_obj, 8):
        uvp, _ = hull_ref.project_front(pose[o], db.xyz[db.model_of == model[o]], synth.K_DEFAULT, synth.CAM_IDENTITY)
        share.append(len(hull_ref.prefilter(uvp)) / max(len(uvp), 1))
    say(f"   prefilter survivors (the restatement's, 20 objects): mean {100 * np.mean(share):.1f} %  max {100 * max(share):.1f} %")

    # 3: the host loop
    exe = os.path.join(ROOT, "moped_amd", "host", "object_hulls_test")
    scene = os.path.join(os.environ.get("TMPDIR", "/tmp"), "object_hulls_scene.txt")
    with open(scene, "w") as f:
        f.write("K " + " ".join("%.9g" % v for v in synth.K_DEFAULT) + "\nCAM " + " ".join("%.9g" % v for v in synth.CAM_IDENTITY) + "\n")
        for m in range(db.n_models):
            xyz = db.xyz[db.model_of == m]
            f.write(f"MODEL m{m} {len(xyz)}\n" + "\n".join(" ".join("%.9g" % v for v in row) for row in xyz) + "\n")
        for o in range(n_obj):
            f.write(f"OBJECT {model[o]} " + " ".join("%.9g" % v for v in pose[o]) + "\n")
    pipe.close()
    say("3  the same 160 hulls by a plain host loop on one thread, and through getObjectHulls_HIP (one round trip per call)")
    for _ in range(args.rounds):
        out = subprocess.run([exe, scene, "6", "20"], capture_output=True, text=True, timeout=600)
        t = [ln for ln in out.stderr.splitlines() if ln.startswith("TIMING")]
        say("   " + (t[0] if t else f"object_hulls_test failed ({out.returncode}): {out.stderr[-300:]}"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
