"""Merging re-seen points into Kinect-view models: what the merge launches, mh_db_merge_view and mh_db_keep_rows cost.

  python scripts/kinect_view_merge_bench.py --parent-lib <the parent commit's libmoped_hip.so>
                                            [--calls 25] [--warmup 5] [--runs 2] [--out profiles/kinect_view_merge.txt]

The method is scripts/kinect_models_bench.py's: device events on the context's stream (a stream of torch's, handed over
with mh_set_stream), every figure the median of --calls after --warmup, every comparison taken --runs times with its two
sides alternating.  Each side runs in a child process of its own (`--child`), because the sides of (2) are two libraries:
  (1) the merge launches alone (mh_view_merge_dev: verdicts + marks + compaction, then one wavefront per merged row) for
      frame 3 against the model of frame 0, next to the selection launch (mh_view_rows_dev) on the same arrays; 200
      launches per event pair;
  (2) mh_db_merge_view of this library against mh_db_append_view of the PARENT commit's library, frame 3 to the model of
      frame 0 with the duplicate test on, against stores of 20 and 200 models of 1 000 rows (the model is put back,
      untimed, before every call);
  (3) mh_db_keep_rows against mh_db_splice(REPLACE) of the same rows from the host (normalised on the device), the model
      of frame 0 keeping three rows of four."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(args):
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
    plane = torch.from_numpy(ref.plane_map(0.8, w, h, tuple(K))).to(dev)
    stream = torch.cuda.Stream(device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def timed(fn, before=None, inner=1):
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
        return round(statistics.median(out), 5)

    pview = capi.make_view(plane.data_ptr(), None, None)
    spec = capi.make_view_spec()
    on = capi.make_view_spec(merge_ratio=0.8, merge_dist=0.002)
    n_models = args.models
    db = synth.make_db(n_models, 1000)
    c = capi.Context(0)
    c.set_stream(stream.cuda_stream)
    c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
    c.db_reserve(len(db.model_of) + 4 * cap, n_models + 4)
    n0, _, _, d0, x0 = c.db_splice_view(capi.DB_INSERT, n_models, g0.data_ptr(), pview, w, h, spec, max_keypoints=cap, want_rows=True)
    back = lambda: c.db_splice_view(capi.DB_REPLACE, n_models, g0.data_ptr(), pview, w, h, spec, max_keypoints=cap)
    r = {"rows_of_the_store": int(len(db.model_of)), "rows_of_the_model": int(n0)}
    if args.child == "append":
        r["append_view_ms"] = timed(lambda: c.db_append_view(n_models, g3.data_ptr(), pview, w, h, on, max_keypoints=cap), before=back)
    elif args.child == "merge":
        r["merge_view_ms"] = timed(lambda: c.db_merge_view(n_models, g3.data_ptr(), pview, w, h, on, max_keypoints=cap, want_rows=False),
                                   before=back)
        back()
        n1, nm, _, st, views = c.db_merge_view(n_models, g3.data_ptr(), pview, w, h, on, max_keypoints=cap, want_rows=False)[:5]
        r["added_rows"], r["merged_rows"], r["duplicates"] = int(n1), int(nm), int(st[6])
    elif args.child == "keep":
        mask = np.arange(n0) % 4 != 0
        r["rows_kept"] = int(mask.sum())
        r["keep_rows_ms"] = timed(lambda: c.db_keep_rows(n_models, mask), before=back)
    elif args.child == "splice":
        mask = np.arange(n0) % 4 != 0
        kd, kx = np.ascontiguousarray(d0[mask]), np.ascontiguousarray(x0[mask])
        r["rows_kept"] = int(mask.sum())
        r["splice_replace_from_host_ms"] = timed(lambda: c.db_splice(capi.DB_REPLACE, n_models, kd, kx, normalize=True), before=back)
    elif args.child == "launch":
        # frame 3's list, its normalised copy and MATCH's answer against the store that holds frame 0's model
        xy3, _, d3 = c.sift(gold["gray3"])
        qn, acc, raw, d1, d2 = c.normalize_match(d3, 0.8)
        b, rows = c.db_model_rows(n_models)
        store_desc = c.db_debug_fetch("desc")
        store_xyz = c.db_debug_fetch("xyz")
        store_model = c.db_debug_fetch("model")
        n = len(xy3)
        pad = lambda a: np.concatenate([a, np.zeros((cap - n,) + a.shape[1:], a.dtype)])
        arrs = [t(pad(raw)), t(pad(d1)), t(pad(d2)), t(store_model), t(store_xyz)]
        dup = capi.mh_view_dup(*[a.data_ptr() for a in arrs], len(store_model), n_models, b, b + rows)
        desc_d, qn_d, xy_d, old_d = t(pad(d3)), t(pad(qn)), t(pad(xy3)), t(store_desc)
        n_d = torch.tensor([n], dtype=torch.int32, device=dev)
        mi = torch.zeros(rows, dtype=torch.int32, device=dev)
        md = torch.zeros((rows, 128), device=dev)
        mx = torch.zeros((rows, 3), device=dev)
        nm = torch.zeros(1, dtype=torch.int32, device=dev)
        vo = torch.zeros(rows, dtype=torch.int32, device=dev)
        od = torch.zeros((cap, 128), device=dev)
        ox = torch.zeros((cap, 3), device=dev)
        no = torch.zeros(1, dtype=torch.int32, device=dev)
        bb = torch.zeros(6, device=dev)
        st = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        merge = lambda: c.view_merge_dev(desc_d.data_ptr(), qn_d.data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, pview, w, h, on, dup,
                                         old_d.data_ptr(), None, mi.data_ptr(), md.data_ptr(), mx.data_ptr(), rows, nm.data_ptr(),
                                         vo.data_ptr())
        select = lambda: c.view_rows_dev(desc_d.data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, pview, w, h, on, od.data_ptr(),
                                         ox.data_ptr(), cap, no.data_ptr(), bb.data_ptr(), st.data_ptr(), dup=dup)
        r["merge_launches_ms"], r["selection_launch_ms"] = [], []
        for _ in range(args.runs):
            r["merge_launches_ms"].append(timed(merge, inner=200))
            r["selection_launch_ms"].append(timed(select, inner=200))
        c.synchronize()
        r["keypoints"], r["merged_rows"], r["new_rows"] = n, int(nm.cpu()[0]), int(no.cpu()[0])
    c.close()
    print("RESULT " + json.dumps(r))


def run_child(args, side, models, lib=None):
    env = dict(os.environ)
    if lib:
        env["MH_LIB_PATH"] = os.path.abspath(lib)
    else:
        env.pop("MH_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--models", str(models), "--calls", str(args.calls),
           "--warmup", str(args.warmup), "--runs", str(args.runs)]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    if out.returncode != 0:   # a child that failed ends the measurement: nothing more is started on the device
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("child %s (%d models) exited with %d" % (side, models, out.returncode))
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--models", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinect_view_merge.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libmoped_hip.so (mh_db_append_view's side of the comparison)")
    results = {"merge_launches_alone": run_child(args, "launch", 20)}
    for models in (20, 200):
        r = {"append_view_parent_ms": [], "merge_view_ms": []}
        for _ in range(args.runs):
            a = run_child(args, "append", models, args.parent_lib)
            m = run_child(args, "merge", models)
            r["append_view_parent_ms"].append(a.pop("append_view_ms"))
            r["merge_view_ms"].append(m.pop("merge_view_ms"))
            r.update(m)
        results["store_of_%d_models" % models] = r
    r = {"keep_rows_ms": [], "splice_replace_from_host_ms": []}
    for _ in range(args.runs):
        k = run_child(args, "keep", 20)
        s = run_child(args, "splice", 20)
        r["keep_rows_ms"].append(k.pop("keep_rows_ms"))
        r["splice_replace_from_host_ms"].append(s.pop("splice_replace_from_host_ms"))
        r.update(k)
    results["prune_store_of_20_models"] = r
    lines = ["Merging re-seen points into Kinect-view models on one MI355X (gfx950): scripts/kinect_view_merge_bench.py.",
             "Device events on the context's stream; medians of %d calls after %d, in ms; every list holds the --runs = %d"
             % (args.calls, args.warmup, args.runs),
             "repetitions of a figure, the sides of a comparison alternating, each in a process of its own.  The bundled",
             "640x480 frames 0 and 3 on the plane z = 0.8.",
             "merge_launches_alone: mh_view_merge_dev (both launches) for frame 3 against the model of frame 0, next to the",
             "selection launch mh_view_rows_dev on the same arrays (200 launches per event pair, time per launch).",
             "merge_view / append_view_parent: mh_db_merge_view of this library against mh_db_append_view of the parent",
             "commit's library, the same image against the same store, the duplicate test on.",
             "keep_rows / splice_replace_from_host: mh_db_keep_rows against mh_db_splice(REPLACE, normalize) of the same rows", "from host arrays.", ""]
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
