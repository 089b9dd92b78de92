"""What a change of the model set costs: mh_db_splice against starting over (normalize + db_upload + db_share x 15).

At the 20-model and the 200-model DB of BASELINE.json (5 000 rows per model), on one GPU, in one process:
  (a) wall time of appending, and of removing, one 5 000-row model with mh_db_splice inside reserved capacity + the 15
      mh_db_adopt calls of a depth-16 pipeline, against the same change made the old way;
  (b) the device time of the edit's pass over the rows (HIP events), fused pass against device copies + the upload's
      preparation;
  (c) frames per second of a depth-16 pipeline over 256 batches with one edit every 16 batches, against the same
      pipeline with no edits and with the edits made the old way.

    python scripts/db_edit_bench.py [--models 20,200] [--out profiles/db_edit_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from moped_amd import capi, synth  # noqa: E402
from moped_amd.pipeline import FramePipeline, ShardedDB  # noqa: E402

ROWS, DEPTH, B, Q = 5000, 16, 16, 3000
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def ms(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def old_way(ctxs, desc, model_of, xyz, n_models):
    """The parent commit's model change: every row through normalize and upload, every other context drained."""
    c0 = ctxs[0]
    c0.db_upload(c0.normalize(desc), model_of, xyz, n_models)
    for c in ctxs[1:]:
        c.db_share(c0)


def measure_edit_calls(db, extra):
    n = db.n_models
    ctxs = [capi.Context(0) for _ in range(DEPTH)]
    try:
        old_way(ctxs, db.desc, db.model_of, db.xyz, n)
        ctxs[0].db_reserve(db.n + 2 * ROWS, n + 2)
        for c in ctxs[1:]:
            c.db_adopt(ctxs[0])

        def splice_pair(times):
            t0 = time.perf_counter()
            ctxs[0].db_splice(capi.DB_INSERT, n, extra.desc, extra.xyz, normalize=True)
            for c in ctxs[1:]:
                c.db_adopt(ctxs[0])
            t1 = time.perf_counter()
            ctxs[0].db_splice(capi.DB_REMOVE, n)
            for c in ctxs[1:]:
                c.db_adopt(ctxs[0])
            t2 = time.perf_counter()
            times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))

        t = []
        for _ in range(4):
            splice_pair(t)
        t = t[1:]   # the first pair warms the staging buffer
        say(f"(a) {n} models: splice + 15 adopts   append {statistics.median(x[0] for x in t):8.2f} ms   "
            f"remove {statistics.median(x[1] for x in t):8.2f} ms   (median of 3)")
        # (b) the pass over the rows, by route
        ctxs[0].enable_timing(True)
        for route, name in ((0, "fused pass"), (1, "copies + preparation")):
            ctxs[0].db_debug_route(route)
            app, rem = [], []
            for _ in range(4):
                ctxs[0].db_splice(capi.DB_INSERT, n, extra.desc, extra.xyz, normalize=True)
                app.append(ctxs[0].db_edit_ms())
                ctxs[0].db_splice(capi.DB_REMOVE, n)
                rem.append(ctxs[0].db_edit_ms())
            say(f"(b) {n} models: {name:22s} append {statistics.median(app[1:]):8.3f} ms   remove "
                f"{statistics.median(rem[1:]):8.3f} ms   (HIP events, median of 3)")
        ctxs[0].db_debug_route(0)
        ctxs[0].enable_timing(False)
        grown_desc = np.concatenate([db.desc, extra.desc])
        grown_of = np.concatenate([db.model_of, np.full(ROWS, n, np.int32)])
        grown_xyz = np.concatenate([db.xyz, extra.xyz])
        a = ms(lambda: old_way(ctxs, grown_desc, grown_of, grown_xyz, n + 1))
        r = ms(lambda: old_way(ctxs, db.desc, db.model_of, db.xyz, n))
        say(f"(a) {n} models: normalize + db_upload + 15 db_share   append {a[0]:8.2f} ms   remove {r[0]:8.2f} ms   (median of 3)")
    finally:
        for c in ctxs:
            c.close()


def measure_pipeline(db, extra, mode, batches=256, every=16):
    """mode: 'none', 'splice' or 'old'.  Frames per second over `batches` batches of B frames."""
    n = db.n_models
    pipe = FramePipeline(0, ShardedDB(db.desc, db.xyz, db.model_of, n), depth=DEPTH, max_queries=Q * B, batch=B,
                         db_capacity=(db.n + 2 * ROWS, n + 2))
    dev = torch.device("cuda:0")
    try:
        frames = [synth.make_frame(db, n_vis=2, seed=s, Q=Q) for s in range(B)]
        raw = torch.from_numpy(np.concatenate([f.desc for f in frames])).to(dev)
        uv = torch.from_numpy(np.concatenate([f.uv for f in frames])).to(dev)
        work = [torch.empty_like(raw) for _ in range(DEPTH)]
        pipe.attach_delivery(16, B)
        grown = (np.concatenate([db.desc, extra.desc]), np.concatenate([db.model_of, np.full(ROWS, n, np.int32)]),
                 np.concatenate([db.xyz, extra.xyz]))
        have_extra = False

        def run(count, edits):
            nonlocal have_extra
            for i in range(count):
                slot = i % DEPTH
                pipe.take_delivery(slot)   # the slot's previous batch has been delivered: its buffers are free
                if edits and i and i % every == 0:
                    if mode == "splice":
                        pipe.remove_model(n) if have_extra else pipe.add_model(extra.desc, extra.xyz)
                    elif have_extra:
                        old_way(pipe.ctxs, db.desc, db.model_of, db.xyz, n)
                    else:
                        old_way(pipe.ctxs, grown[0], grown[1], grown[2], n + 1)
                    have_extra = not have_extra
                with torch.cuda.stream(pipe.streams[slot]):
                    work[slot].copy_(raw, non_blocking=True)   # the frames' descriptors are normalised in place
                pipe.enqueue_batch(slot, work[slot], uv, B, [i * B + f + 1 for f in range(B)])
                pipe.deliver(slot, i)
            for slot in range(DEPTH):
                pipe.take_delivery(slot)

        run(2 * DEPTH, False)   # warm-up: buffers, launch plans
        t0 = time.perf_counter()
        run(batches, mode != "none")
        dt = time.perf_counter() - t0
        if have_extra and mode == "splice":
            pipe.remove_model(n)
        return batches * B / dt
    finally:
        pipe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="20,200")
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; depth {DEPTH}, batches of {B} frames, {Q} queries per frame, "
        f"{ROWS} rows per model")
    for n in (int(x) for x in args.models.split(",")):
        db = synth.make_db(n, ROWS)
        extra = synth.make_db(1, ROWS, seed=0xADD)
        measure_edit_calls(db, extra)
        if args.skip_pipeline:
            continue
        fps = {mode: measure_pipeline(db, extra, mode) for mode in ("none", "splice", "old")}
        say(f"(c) {n} models: depth-16 pipeline, 256 batches, an edit every 16:   no edits {fps['none']:9.0f} frames/s   "
            f"mh_db_splice {fps['splice']:9.0f} frames/s   normalize + upload + share {fps['old']:9.0f} frames/s")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
