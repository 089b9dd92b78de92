"""Teaching 3-D models from Kinect views: what the selection launch, mh_db_splice_view and mh_db_append_view cost.

  python scripts/kinect_models_bench.py [--calls 25] [--warmup 5] [--runs 2] [--out profiles/kinect_models.txt]

All times are device events on the context's stream (a stream of torch's, handed over with mh_set_stream); every figure
is the median of --calls after --warmup, and every comparison is taken --runs times with its two sides alternating.
  (1) the selection launch alone (mh_view_rows_dev): the bundled 640x480 frame 0 over the relief map, and 16 views in one
      launch (mh_view_rows_batch_dev); 200 launches per event pair;
  (2) mh_db_splice_view against mh_db_splice_image on the same image (REPLACE of one model of a 20-model store);
  (3) mh_db_append_view of frame 3 to the model of frame 0, with and without the duplicate test, against stores of 20 and
      200 models of 1 000 rows (the model is put back, untimed, before every call)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinect_models.txt"))
    args = ap.parse_args()
    import torch
    import view_model_ref as ref
    from moped_amd import capi, synth
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    K = synth.K_DEFAULT
    dev = torch.device("cuda:0")
    cap = 4096
    h, w = gold["gray0"].shape
    g0 = torch.from_numpy(np.ascontiguousarray(gold["gray0"])).to(dev)
    g3 = torch.from_numpy(np.ascontiguousarray(gold["gray3"])).to(dev)
    relief = torch.from_numpy(ref.relief_map(w, h, tuple(K))).to(dev)
    plane = torch.from_numpy(ref.plane_map(0.8, w, h, tuple(K))).to(dev)
    pose = ref.trap_pose()
    stream = torch.cuda.Stream(device=dev)
    med = statistics.median

    def timed(c, fn, before=None, inner=1):
        """Median ms of fn() between two events on the context's stream (inner: launches per event pair)."""
        out = []
        with torch.cuda.stream(stream):
            for k in range(args.warmup + args.calls):
                if before:
                    before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(inner):
                    fn()
                e1.record(stream)
                e1.synchronize()
                if k >= args.warmup:
                    out.append(e0.elapsed_time(e1) / inner)
        return round(med(out), 5)

    results = {}
    # ---- (1) the selection alone ----
    c = capi.Context(0)
    c.set_stream(stream.cuda_stream)
    B = 16
    desc = torch.zeros((B, cap, 128), device=dev)
    xy = torch.zeros((B, cap, 2), device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c.sift_batch_dev([g0.data_ptr()] * B, w, h, True, desc.data_ptr(), xy.data_ptr(), cap, cnt.data_ptr())
    c.synchronize()
    od = torch.zeros((B, cap, 128), device=dev)
    ox = torch.zeros((B, cap, 3), device=dev)
    no = torch.zeros(B, dtype=torch.int32, device=dev)
    bb = torch.zeros((B, 6), device=dev)
    st = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    view = capi.make_view(relief.data_ptr(), None, pose)
    spec = capi.make_view_spec()
    one = lambda: c.view_rows_dev(desc.data_ptr(), xy.data_ptr(), cnt.data_ptr(), cap, view, w, h, spec, od.data_ptr(), ox.data_ptr(),
                                  cap, no.data_ptr(), bb.data_ptr(), st.data_ptr())
    many = lambda: c.view_rows_batch_dev(desc.data_ptr(), xy.data_ptr(), cnt.data_ptr(), cap, [view] * B, w, h, spec, od.data_ptr(),
                                         ox.data_ptr(), cap, no.data_ptr(), bb.data_ptr(), st.data_ptr())
    sel = {"keypoints_per_view": int(cnt[0]), "one_view_ms": [], "batch_of_16_ms": []}
    for _ in range(args.runs):
        sel["one_view_ms"].append(timed(c, one, inner=200))
        sel["batch_of_16_ms"].append(timed(c, many, inner=200))
    results["selection_launch"] = sel
    c.close()

    # ---- (2), (3): edits of stores of 20 and 200 models ----
    for n_models in (20, 200):
        db = synth.make_db(n_models, 1000)
        c = capi.Context(0)
        c.set_stream(stream.cuda_stream)
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        c.db_reserve(len(db.model_of) + 4 * cap, n_models + 4)
        pview = capi.make_view(plane.data_ptr(), None, None)
        pspec = capi.make_planar_spec(z=0.8, K=K)
        n0, _, _ = c.db_splice_view(capi.DB_INSERT, n_models, g0.data_ptr(), pview, w, h, spec, max_keypoints=cap)
        r = {"rows_of_the_store": int(len(db.model_of)), "rows_of_the_model": int(n0)}
        if n_models == 20:
            r["splice_view_ms"], r["splice_image_ms"] = [], []
            for _ in range(args.runs):
                r["splice_view_ms"].append(timed(c, lambda: c.db_splice_view(capi.DB_REPLACE, n_models, g0.data_ptr(), pview, w, h, spec,
                                                                             max_keypoints=cap)))
                r["splice_image_ms"].append(timed(c, lambda: c.db_splice_image(capi.DB_REPLACE, n_models, g0.data_ptr(), w, h, pspec,
                                                                               max_keypoints=cap)))
        back = lambda: c.db_splice_view(capi.DB_REPLACE, n_models, g0.data_ptr(), pview, w, h, spec, max_keypoints=cap)
        on = capi.make_view_spec(merge_ratio=0.8, merge_dist=0.002)
        off = capi.make_view_spec(merge_ratio=0.0, merge_dist=0.002)
        r["append_view_duplicate_test_ms"], r["append_view_no_test_ms"] = [], []
        for _ in range(args.runs):
            r["append_view_duplicate_test_ms"].append(timed(c, lambda: c.db_append_view(n_models, g3.data_ptr(), pview, w, h, on,
                                                                                        max_keypoints=cap), before=back))
            r["append_view_no_test_ms"].append(timed(c, lambda: c.db_append_view(n_models, g3.data_ptr(), pview, w, h, off,
                                                                                 max_keypoints=cap), before=back))
        back()
        n1, _, s1 = c.db_append_view(n_models, g3.data_ptr(), pview, w, h, on, max_keypoints=cap)
        r["appended_rows"], r["duplicates_left_out"], r["match_launches"] = int(n1), int(s1[6]), c.match_kernel_launches()
        results["store_of_%d_models" % n_models] = r
        c.close()

    lines = ["Teaching 3-D models from Kinect views on one MI355X (gfx950): scripts/kinect_models_bench.py, one process.",
             "Device events on the context's stream; medians of %d calls after %d, in ms; every list holds the --runs = %d"
             % (args.calls, args.warmup, args.runs),
             "repetitions of a figure, the sides of a comparison alternating.  The bundled 640x480 frames 0 and 3.",
             "selection_launch: mh_view_rows_dev / mh_view_rows_batch_dev alone (200 launches per event pair, time per launch).",
             "splice_view / splice_image: mh_db_splice_view against mh_db_splice_image, REPLACE of the same model by the same image.",
             "append_view_*: mh_db_append_view of frame 3 to the model of frame 0 with the duplicate test (normalise + MATCH of",
             "the view's keypoints against the store + the test) and without it (no MATCH launched).", ""]
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
