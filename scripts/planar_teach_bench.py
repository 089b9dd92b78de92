"""Teaching a planar model from an image: FramePipeline.add_planar_model against the route through the host.

  python scripts/planar_teach_bench.py [--calls 25] [--warmup 5] [--out profiles/planar_teach.txt]

Per image (the reference's bundled 640x480 frame 0; synth.textured_image(0), ~3 240 keypoints):
  (a) add_planar_model(image on the device): FEAT, selection and splice on the device, one added host wait;
  (b) the route without it: Context.sift (image from host memory, rows to the host), the model coordinates in numpy,
      FramePipeline.add_model (rows back up, normalised on the device);
  (c) 16 images: one add_planar_models call against 16 add_planar_model calls.
Every timed call replaces (a, b) or appends (c) into a pipeline of 5 x 5 000 synthetic rows with reserved capacity, and is
timed between host synchronisations of the device; the median of the calls is reported."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_teach.txt"))
    args = ap.parse_args()
    import torch
    from moped_amd import capi, synth
    from moped_amd.pipeline import FramePipeline, ShardedDB
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    K = synth.K_DEFAULT
    dev = torch.device("cuda:0")
    z = np.float32(0.8)
    cap = 4096
    images = {"bundled frame 0": np.ascontiguousarray(gold["gray0"]), "textured": np.ascontiguousarray(synth.textured_image(0))}
    results = {}

    def timed(fn, undo=None):
        out = []
        for k in range(args.warmup + args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if undo:
                undo()
            if k >= args.warmup:
                out.append(dt)
        return out

    for label, img in images.items():
        db = synth.make_db(5, 5000)
        pipe = FramePipeline(0, ShardedDB(db.desc, db.xyz, db.model_of, db.n_models), depth=2, max_queries=cap,
                             db_capacity=(131072, 64))
        try:
            g = torch.from_numpy(img).to(dev)
            h, w = img.shape
            _, n_rows, _ = pipe.add_planar_model(g, name="taught", z=float(z), max_keypoints=cap)   # the model both routes replace

            def device_route():
                pipe.add_planar_model(g, name="taught", z=float(z), max_keypoints=cap)

            def host_route():
                xy, _, desc = pipe.ctxs[0].sift(img, cap=cap)
                xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
                pipe.add_model(desc, xyz, name="taught")

            ms_a = timed(device_route)
            ms_b = timed(host_route)
            ms_a2 = timed(device_route)   # (again, after the other route: the order does not decide it)
            # the same two routes on slot 0's context alone: no host mirror of the database, no host copy of the rows in (a)
            c0 = pipe.ctxs[0]
            spec = capi.make_planar_spec(z=float(z), K=K)

            def device_route_ctx():
                c0.db_splice_image(capi.DB_REPLACE, 5, g.data_ptr(), w, h, spec, max_keypoints=cap)

            def host_route_ctx():
                xy, _, desc = c0.sift(img, cap=cap)
                xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
                c0.db_splice(capi.DB_REPLACE, 5, desc, xyz, normalize=True)

            ms_a0 = timed(device_route_ctx)
            ms_b0 = timed(host_route_ctx)
            d_, xy_, cnt = (torch.empty((cap, 128), device=dev), torch.empty((cap, 2), device=dev),
                            torch.zeros(1, dtype=torch.int32, device=dev))
            ms_feat = timed(lambda: c0.sift_dev(g.data_ptr(), w, h, True, d_.data_ptr(), xy_.data_ptr(), 0, cap, cnt.data_ptr()))
            assert 0 < n_rows <= cap
            xyz_ = torch.zeros((cap, 3), device=dev)   # [cap, 3]: mh_db_splice reads n_rows x 3 floats of it
            ms_splice = timed(lambda: c0.db_splice(capi.DB_REPLACE, 5, d_.data_ptr(), xyz_.data_ptr(), normalize=True,
                                                   on_device=True, n_rows=n_rows))
            c0.db_splice_image(capi.DB_REPLACE, 5, g.data_ptr(), w, h, spec, max_keypoints=cap)   # (the model as it was)
            for c in pipe.ctxs[1:]:
                c.db_adopt(c0)
            batch = [g] * 16
            first = pipe.db.n_models

            def remove16():
                for _ in range(16):
                    pipe.remove_model(first)

            ms_c1 = timed(lambda: pipe.add_planar_models(batch, [None] * 16, z=float(z), max_keypoints=cap), remove16)
            ms_c16 = timed(lambda: [pipe.add_planar_model(x, z=float(z), max_keypoints=cap) for x in batch], remove16)
            med = statistics.median
            results[label] = {
                "rows_of_the_model": int(n_rows), "calls": args.calls, "warmup": args.warmup,
                "a_add_planar_model_ms": round(med(ms_a), 4), "a_again_ms": round(med(ms_a2), 4),
                "b_sift_numpy_add_model_ms": round(med(ms_b), 4),
                "a_min_max_ms": [round(min(ms_a), 4), round(max(ms_a), 4)], "b_min_max_ms": [round(min(ms_b), 4), round(max(ms_b), 4)],
                "context_alone_a_db_splice_image_ms": round(med(ms_a0), 4), "context_alone_b_sift_numpy_db_splice_ms": round(med(ms_b0), 4),
                "context_alone_b_over_a": round(med(ms_b0) / med(ms_a0), 3),
                "feat_alone_ms": round(med(ms_feat), 4), "splice_alone_rows_on_the_device_ms": round(med(ms_splice), 4),
                "c_one_call_16_images_ms": round(med(ms_c1), 4), "c_16_calls_ms": round(med(ms_c16), 4),
                "b_over_a": round(med(ms_b) / med(ms_a), 3), "c_16_calls_over_one_call": round(med(ms_c16) / med(ms_c1), 3),
            }
        finally:
            pipe.close()
    lines = ["Teaching a planar model from a 640x480 image on one MI355X (gfx950): scripts/planar_teach_bench.py, one process.",
             "Store: 5 x 5 000 synthetic rows + the taught model(s), capacity reserved (mh_db_reserve), 2 slots.",
             "Each call timed between host synchronisations of the device (time.perf_counter); medians in ms.",
             "(a) FramePipeline.add_planar_model(image on the device); (b) Context.sift -> numpy -> FramePipeline.add_model;",
             "(c) 16 images: one add_planar_models call against 16 add_planar_model calls (the removals between calls untimed).",
             "Both (a) and (b) include the host copy of the rows and the numpy splice that keep FramePipeline.db in step;",
             "context_alone_*: the same two routes on the context (mh_db_splice_image without a host copy of the rows against",
             "mh_sift_extract -> numpy -> mh_db_splice); feat_alone: mh_sift_extract_dev; splice_alone: mh_db_splice of as many",
             "rows already on the device.", ""]
    for label, r in results.items():
        lines.append("== %s ==" % label)
        lines.append(json.dumps(r))
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
