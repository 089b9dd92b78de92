"""Kinect frames (a gray image and a depth map per frame, both on the device): frame by frame against batches of 16.

(a) image + map -> objects, 16 slots in flight, the two forms alternately, every round printed:
      frame by frame   mh_depth_fill + mh_frame_set_depth_image + mh_frame_enqueue_image per frame
      batches of 16    FramePipeline.enqueue_kinect_batch (mh_depth_fill_batch + mh_frame_set_depth_image_batch +
                       mh_frame_enqueue_image_batch)
    Scene and images as bench.image_to_objects_leg (the bundled frames; the synthetic DB + frame 0's keypoints as a planar
    model 0.8 m in front of the camera), the plane's depth map with sensor-like holes, moped3d's configuration
    (config.hpp:38-49: DEPTHFILL(8, false), DEPTHFILTER 0.05 / 0.01, the adaptive ratio, linkage, back-projection).
    DEPTHFILL works in place, so every slot restores its 16 raw maps with ONE device copy per 16 frames in both forms
    (the sensor's delivery).
(b) DEPTHFILL alone: device events around sixteen mh_depth_fill calls of 640 x 480 maps against one mh_depth_fill_batch
    of the same maps.

(c) --filter-depth (instead of (a) and (b)): batches of 16 with moped3d's depth-verified FILTER in both slots
    (FramePipeline.set_filter_depth, 300 test points per model) against the same batches with it off, alternating rounds,
    on maps that arrive filled, with the route the last batch took (mh_frame_route); then the FILTER and FILTER2 stage
    times of one frame alone with stage timing on (device events around filter_depth_kernel against filter_kernel).
    MH_LIB_PATH names another build of the library for an A/B run.  > profiles/filter_depth.txt

usage: python scripts/kinect_image_bench.py [--models 5] [--rounds 5] [--seconds 1.2] > profiles/kinect_image_batch.txt
One process on an otherwise idle device; every shape is warmed before it is timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS, B, CAP, W, H = 16, 16, 1024, 640, 480


def holed_plane(K, seed):
    """The z = 0.8 plane [H, W, 4] with sensor-like holes: shadows beside objects, a dead border, speckle."""
    rng = np.random.default_rng(seed)
    z = np.full((H, W), 0.8, np.float32)
    yy, xx = np.ogrid[:H, :W]
    for _ in range(25):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 70)
        z[(yy - cy) ** 2 + ((xx - cx) * rng.uniform(0.3, 1.0)) ** 2 < r * r] = -1.0
    z[:, :12] = -1.0
    z[-9:, :] = -1.0
    z[rng.random((H, W)) < 0.01] = -1.0
    d = np.zeros((H, W, 4), np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    d[..., 2] = z
    d[..., 0] = (u - K[2]) / K[0] * z
    d[..., 1] = (v - K[3]) / K[1] * z
    d[..., 3] = np.sqrt((d[..., :3] ** 2).sum(-1))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--filter-depth", action="store_true", help="(c): what the depth FILTER costs a batch of 16")
    args = ap.parse_args()
    import torch
    from moped_amd import capi, moped3d, synth
    from moped_amd.pipeline import FramePipeline, ShardedDB
    K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    pool = [gold[f"gray{int(f)}"] for f in gold["frames"]]
    db = synth.make_db(args.models, 5000)
    c0 = capi.Context(0)
    xy, _, desc = c0.sift(pool[0])
    c0.close()
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    all_desc = np.concatenate([db.desc, desc])
    all_xyz = np.concatenate([db.xyz, xyz])
    model_of = np.concatenate([db.model_of, np.full(len(xy), args.models, np.int32)])
    n_models = args.models + 1
    pipe = FramePipeline(0, ShardedDB(all_desc, all_xyz, model_of, n_models), depth=SLOTS, max_queries=B * CAP, batch=B)
    table = moped3d.ratio_table(all_xyz, model_of, n_models, K)
    for c in pipe.ctxs:
        c.frame_set_depth_rules(K, 64, 0.05, 0.01, table)
        c.frame_set_cluster_linkage(capi.default_linkage_params())
    imgs = [torch.from_numpy(np.ascontiguousarray(g)).to(dev) for g in pool]
    raw = torch.from_numpy(np.stack([holed_plane(K, 10 + j) for j in range(B)])).to(dev)          # [B, H, W, 4]
    work = [torch.empty_like(raw) for _ in range(SLOTS)]
    fill = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(SLOTS)]
    torch.cuda.synchronize()
    prm, cam = pipe.params, capi.make_cam(K, CAM0)

    def restore(slot):
        with torch.cuda.stream(pipe.streams[slot]):
            work[slot].copy_(raw)

    def frame_by_frame(groups):
        """groups x 16 frames: group g on slot g % 16, its frames one call sequence each."""
        for g in range(groups):
            s = g % SLOTS
            c = pipe.ctxs[s]
            restore(s)
            for j in range(B):
                d_ptr, f_ptr = work[s][j].data_ptr(), fill[s][j].data_ptr()
                c.depth_fill_dev(d_ptr, W, H, K, f_ptr, 8, False)
                c.frame_set_depth_image(d_ptr, f_ptr, W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
                c.frame_enqueue_image(imgs[(g * B + j) % len(imgs)].data_ptr(), W, H, True, CAP, K, CAM0, prm, g * B + j + 1,
                                      _cam_struct=cam)

    def batched(groups):
        for g in range(groups):
            s = g % SLOTS
            restore(s)
            pipe.enqueue_kinect_batch(s, [imgs[(g * B + j) % len(imgs)].data_ptr() for j in range(B)],
                                      [work[s][j].data_ptr() for j in range(B)], [fill[s][j].data_ptr() for j in range(B)],
                                      W, H, [g * B + j + 1 for j in range(B)], fill_scale=8, max_keypoints=CAP)

    def timed(fn, groups):
        pipe.synchronize()
        t0 = time.perf_counter()
        fn(groups)
        pipe.synchronize()
        return time.perf_counter() - t0

    def found(slot_fetch):
        objs, counts = slot_fetch
        return int(len(objs) > 0 and objs[np.argmax(objs["score"])]["model"] == args.models)

    if args.filter_depth:
        # (c) test points: 300 of every model's own points (the planar model: its keypoints), the map's camera = the image's
        rng = np.random.default_rng(5)
        pts, off = [], [0]
        for m in range(n_models):
            rows = np.nonzero(model_of == m)[0]
            pts.append(all_xyz[rng.choice(rows, min(300, len(rows)), replace=False)])
            off.append(off[-1] + len(pts[-1]))
        pts, off = np.concatenate(pts), np.array(off, np.int32)
        fd_prm = (64.0, 0.1, 0.1)                         # PlausibleSqDistance, DepthFraction, MinKeypointFraction
        for s_ in range(SLOTS):                           # the maps arrive filled: DEPTHFILL once, outside the windows
            restore(s_)
            pipe.ctxs[s_].depth_fill_batch_dev([work[s_][j].data_ptr() for j in range(B)],
                                               [fill[s_][j].data_ptr() for j in range(B)], W, H, K, 8, False)
        pipe.synchronize()

        def filled_batches(groups):
            for g in range(groups):
                s_ = g % SLOTS
                pipe.enqueue_kinect_batch(s_, [imgs[(g * B + j) % len(imgs)].data_ptr() for j in range(B)],
                                          [work[s_][j].data_ptr() for j in range(B)], [fill[s_][j].data_ptr() for j in range(B)],
                                          W, H, [g * B + j + 1 for j in range(B)], fill_scale=None, max_keypoints=CAP)

        def switch(on):
            if on:
                pipe.set_filter_depth(pts, off, f1=fd_prm, f2=fd_prm)
            else:
                pipe.set_filter_depth(None, None)

        print("# Kinect batches of 16 (filled maps): depth FILTER in both slots, 300 test points per model, against off")
        print(f"# {SLOTS} slots, 640x480, {n_models} models, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
        win = {}
        for on in (False, True):
            switch(on)
            filled_batches(2 * SLOTS)
            dt = timed(filled_batches, 2 * SLOTS)
            win[on] = max(SLOTS, int(np.ceil(args.seconds / dt * 2)) * SLOTS)
            hits = sum(found(pipe.ctxs[SLOTS - 1].frame_fetch_slot(j)) for j in range(B))
            print(f"# depth FILTER {'on ' if on else 'off'}: warm; {win[on] * B} frames per window; planted model best in {hits} of {B}")
            if hasattr(capi.load(), "mh_frame_route"):        # (an older library named by MH_LIB_PATH has no such call)
                r_ = pipe.ctxs[SLOTS - 1].frame_route().tolist()
                print(f"# depth FILTER {'on ' if on else 'off'}: last batch: {r_[0]} frames, {'one launch per stage' if r_[1] else 'frame after frame'}, "
                      f"FILTER {'in the POSE tails' if r_[2] else 'as launches of its own'}, depth class bits {r_[3]}")
        rates = {False: [], True: []}
        for r in range(args.rounds):
            for on in (False, True):
                switch(on)
                dt = timed(filled_batches, win[on])
                rates[on].append(win[on] * B / dt)
                print(f"(c) round {r + 1} depth FILTER {'on ' if on else 'off'} {rates[on][-1]:9.1f} frames/s   window {dt:.3f} s")
        for on in (False, True):
            v = rates[on]
            print(f"(c) depth FILTER {'on ' if on else 'off'} min {min(v):.1f} max {max(v):.1f} spread {max(v) - min(v):.1f} frames/s")
        print(f"(c) on / off: {np.median(rates[True]) / np.median(rates[False]):.3f} of the merged, fused batch's rate (medians)")
        # the FILTER launches of one frame alone, stage timing on (both forms then run FILTER as launches of their own)
        c = pipe.ctxs[0]
        c.enable_timing(True)
        c.frame_set_depth_image(work[0][0].data_ptr(), fill[0][0].data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        for on in (False, True):
            switch(on)
            f1, f2 = [], []
            for rep_ in range(-3, 20):
                c.frame_enqueue_image(imgs[0].data_ptr(), W, H, True, CAP, K, CAM0, prm, rep_ + 10, _cam_struct=cam)
                objs, _ = c.frame_fetch()
                t = c.timing()
                if rep_ >= 0:
                    f1.append(t["filter1_ms"])
                    f2.append(t["filter2_ms"])
            print(f"(c) one frame, {'filter_depth_kernel' if on else 'filter_kernel      '}: FILTER median {np.median(f1) * 1e3:.1f} us "
                  f"(min {min(f1) * 1e3:.1f}, max {max(f1) * 1e3:.1f}), FILTER2 median {np.median(f2) * 1e3:.1f} us "
                  f"(min {min(f2) * 1e3:.1f}, max {max(f2) * 1e3:.1f}); {len(objs)} objects delivered (device events, 20 frames)")
        c.enable_timing(False)
        switch(False)
        pipe.close()
        return

    print("# Kinect frames, image + depth map -> objects: frame by frame against batches of 16")
    print(f"# {SLOTS} slots, 640x480, {args.models} synthetic models + the planar model, keypoint capacity {CAP}, "
          f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
    groups = {}
    for name, fn in (("frame_by_frame", frame_by_frame), ("batches_of_16", batched)):
        fn(2 * SLOTS)                                     # warm: every slot twice
        for c in pipe.ctxs:
            c.frame_fetch() if name == "frame_by_frame" else c.frame_fetch_slot(0)
            c.depth_fill_status()
        dt = timed(fn, 2 * SLOTS)
        groups[name] = max(SLOTS, int(np.ceil(args.seconds / dt * 2 * SLOTS / SLOTS)) * SLOTS)
        last = pipe.ctxs[(2 * SLOTS - 1) % SLOTS]
        hits = (found(last.frame_fetch()) if name == "frame_by_frame"
                else sum(found(last.frame_fetch_slot(j)) for j in range(B)))
        print(f"# {name}: warm; {groups[name] * B} frames per window; planted model is the best object in "
              f"{hits} of the {1 if name == 'frame_by_frame' else B} frames fetched")
    rates = {"frame_by_frame": [], "batches_of_16": []}
    for r in range(args.rounds):
        for name, fn in (("frame_by_frame", frame_by_frame), ("batches_of_16", batched)):
            dt = timed(fn, groups[name])
            rate = groups[name] * B / dt
            rates[name].append(rate)
            print(f"(a) round {r + 1} {name:15s} {rate:9.1f} frames/s   window {dt:.3f} s")
    for name, v in rates.items():
        print(f"(a) {name:15s} min {min(v):.1f} max {max(v):.1f} spread {max(v) - min(v):.1f} frames/s")
    a, b = rates["frame_by_frame"], rates["batches_of_16"]
    gain = min(b) > max(a) and min(b) - max(a) >= 3 * (max(a) - min(a))
    loss = min(a) > max(b) and min(a) - max(b) >= 3 * (max(b) - min(b))
    print("(a) verdict under the project's rule (every round above every round of the other side, by at least three "
          "times the other side's spread): " + ("batches of 16 gain" if gain else "frame by frame is faster" if loss else "no claim"))
    for c in pipe.ctxs:
        c.depth_fill_status()

    # (b) DEPTHFILL alone on one context
    c, st = pipe.ctxs[0], pipe.streams[0]
    dp, fp = [work[0][j].data_ptr() for j in range(B)], [fill[0][j].data_ptr() for j in range(B)]

    def fill_single():
        for j in range(B):
            c.depth_fill_dev(dp[j], W, H, K, fp[j], 8, False)

    def fill_batch():
        c.depth_fill_batch_dev(dp, fp, W, H, K, 8, False)

    ms = {"sixteen_mh_depth_fill": [], "one_mh_depth_fill_batch": []}
    for rep in range(-3, 20):                            # (three warm-up rounds)
        for name, fn in (("sixteen_mh_depth_fill", fill_single), ("one_mh_depth_fill_batch", fill_batch)):
            restore(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
    c.depth_fill_status()
    for name, v in ms.items():
        print(f"(b) {name:24s} 16 maps 640x480 factor 8: median {np.median(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  "
              f"({len(v)} rounds, device events)")
    a, b = ms["sixteen_mh_depth_fill"], ms["one_mh_depth_fill_batch"]
    gain = max(b) < min(a) and min(a) - max(b) >= 3 * (max(a) - min(a))
    print("(b) verdict under the same rule: " + ("the batch call gains" if gain else "no claim"))
    pipe.close()


if __name__ == "__main__":
    main()
