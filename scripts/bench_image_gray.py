"""The gray image from what a camera delivers (csrc/image_gray.hip): what the conversion costs, alone and in front of frames.

(a) the conversion alone (mh_image_gray_dev / _batch_dev) at 640 x 480, every format: us per image, one image per call and
    per image in a batch of 16; device events around CALLS back-to-back calls on the stream, ROUNDS rounds, the whole table
    twice (run 1, run 2: the forms alternate, so a drift of the device shows as a difference between the runs).  Beside
    every figure: the bytes the call moves (raw in + gray out) and the time they take at the HBM rate.  A single call is
    bound by its launch, not by its bytes; the table says by how much.
(b) Kinect batches of 16, scene and configuration of scripts/kinect_raw_bench.py (d), 16 slots, maps resident on the device:
      gray   packed gray images, no format set (the existing path)
      bgr8   the cameras' bgr8 buffers with FramePipeline.set_image_format: one more launch per batch
      gold   the bundled gray frames themselves, no format set: the images scripts/kinect_raw_bench.py (d) runs, as a
             control -- gray and bgr8 run colour versions of them (R and B moved by smooth fields), whose gray differs
    alternately, every round printed; gray and bgr8 see the same gray bytes, so their objects are the same.  The keypoints
    FEAT finds per image are printed for both sets of images.

usage: python scripts/bench_image_gray.py [--models 5] [--rounds 5] [--seconds 1.2] > profiles/image_gray.txt
One process on an otherwise idle device; every shape is warmed before it is timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLOTS, B, CAP, W, H = 16, 16, 1024, 640, 480
CALLS, ROUNDS = 50, 10
HBM_TBS = 6.3   # achievable HBM rate of the MI355X (8.0 TB/s on paper)


def colour_of(gray, k):
    """R = clip(g + a smooth field), G = g, B = clip(g - another) -> [H, W, 3] R, G, B."""
    y, x = np.mgrid[0:gray.shape[0], 0:gray.shape[1]].astype(np.float64)
    a = 30.0 * np.sin(x / (50.0 + 7 * k)) * np.cos(y / 70.0)
    b = 25.0 * np.cos(x / 90.0 + k) * np.sin(y / (40.0 + 3 * k))
    g = gray.astype(np.float64)
    return np.stack([np.clip(np.rint(g + a), 0, 255), g, np.clip(np.rint(g - b), 0, 255)], 2).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.2)
    args = ap.parse_args()
    import torch
    import depthmap_ref
    import image_gray_ref as ref
    from kinect_raw_bench import holed_z
    from moped_amd import capi, moped3d, synth
    from moped_amd.pipeline import FramePipeline, ShardedDB
    K = synth.K_DEFAULT
    dev = torch.device("cuda:0")
    print("# The gray image from what a camera delivers (csrc/image_gray.hip); GPU_MAX_HW_QUEUES=" + str(os.environ.get("GPU_MAX_HW_QUEUES")))

    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    pool = [gold[f"gray{int(f)}"] for f in gold["frames"]]
    rgb = [colour_of(g, k) for k, g in enumerate(pool)]

    # ---- (a) the conversion alone ----
    c = capi.Context(0)
    st = torch.cuda.Stream(device=dev)
    c.set_stream(st.cuda_stream)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    out_ptrs = [out[j].data_ptr() for j in range(B)]
    rng = np.random.default_rng(1)
    inputs = {}
    for fmt in ref.FORMATS:
        px = pool[0][:, :, None] if fmt == ref.GRAY8 else ref.from_rgb(rgb[0], fmt)
        raw = ref.pack(px, fmt)
        t = torch.from_numpy(np.stack([np.roll(raw, int(rng.integers(0, raw.size))) for _ in range(B)])).to(dev)
        inputs[fmt] = (t, capi.make_raw_image(fmt, W, H), raw.size)
    torch.cuda.synchronize()
    print(f"(a) {CALLS} back-to-back calls between two device events, {ROUNDS} rounds after 3 warm ones; us per IMAGE; "
          f"'floor' = the call's bytes (raw in + gray out) at {HBM_TBS} TB/s (achievable HBM rate)")
    for run in (1, 2):
        for fmt in ref.FORMATS:
            t, d, nbytes = inputs[fmt]
            in_ptrs = [t[j].data_ptr() for j in range(B)]
            moved = nbytes + W * H
            floor_us = moved / (HBM_TBS * 1e12) * 1e6
            for form in ("one image per call", "batch of 16"):
                us = []
                for rep in range(-3, ROUNDS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    st.synchronize()
                    e0.record(st)
                    for k in range(CALLS):
                        if form == "batch of 16":
                            c.image_gray_batch_dev(in_ptrs, d, out_ptrs)
                        else:
                            c.image_gray_dev(in_ptrs[k % B], d, out_ptrs[k % B])
                    e1.record(st)
                    st.synchronize()
                    if rep >= 0:
                        us.append(e0.elapsed_time(e1) * 1e3 / CALLS / (B if form == "batch of 16" else 1))
                med = float(np.median(us))
                print(f"(a) run {run} {ref.NAMES[fmt]:12s} {form:18s} median {med:7.2f} us  min {min(us):.2f}  max {max(us):.2f}"
                      f"   {moved / 1e6:.2f} MB moved, floor {floor_us:.3f} us = {floor_us / med:.3f} of the time, "
                      f"{moved / (med * 1e-6) / 1e12:.2f} TB/s")
    c.close()

    # ---- (b) Kinect batches of 16: the scene of scripts/kinect_raw_bench.py ----
    grays = [ref.gray(ref.pack(ref.from_rgb(x, ref.BGR8), ref.BGR8), ref.BGR8, W, H) for x in rgb]   # what the device makes of them
    db = synth.make_db(args.models, 5000)
    c0 = capi.Context(0)
    xy, _, desc = c0.sift(grays[0])
    c0.close()
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    all_desc = np.concatenate([db.desc, desc])
    all_xyz = np.concatenate([db.xyz, xyz])
    model_of = np.concatenate([db.model_of, np.full(len(xy), args.models, np.int32)])
    n_models = args.models + 1
    pipe = FramePipeline(0, ShardedDB(all_desc, all_xyz, model_of, n_models), depth=SLOTS, max_queries=B * CAP, batch=B)
    table = moped3d.ratio_table(all_xyz, model_of, n_models, K)
    for c_ in pipe.ctxs:
        c_.frame_set_depth_rules(K, 64, 0.05, 0.01, table)
        c_.frame_set_cluster_linkage(capi.default_linkage_params())
    t_gray = [torch.from_numpy(np.ascontiguousarray(g)).to(dev) for g in grays]
    t_gold = [torch.from_numpy(np.ascontiguousarray(g)).to(dev) for g in pool]
    c0 = capi.Context(0)
    print("# keypoints per image (FEAT, double size): the colour images' gray " + str([len(c0.sift(g)[0]) for g in grays])
          + ", the bundled gray frames " + str([len(c0.sift(g)[0]) for g in pool]))
    c0.close()
    t_bgr = [torch.from_numpy(ref.pack(ref.from_rgb(x, ref.BGR8), ref.BGR8)).to(dev) for x in rgb]
    bgr_fmt = capi.make_raw_image(capi.IMAGE_BGR8, W, H)
    zs = np.stack([holed_z(10 + j) for j in range(B)])
    maps = np.stack([depthmap_ref.depth_map(*depthmap_ref.plain(zs[j]), K, W, H) for j in range(B)])
    raw_dev = torch.from_numpy(maps).to(dev)
    work = [torch.empty_like(raw_dev) for _ in range(SLOTS)]
    fill = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(SLOTS)]
    torch.cuda.synchronize()

    def form(images, fmt):
        def run(groups):
            pipe.set_image_format(fmt)
            for g in range(groups):
                s = g % SLOTS
                with torch.cuda.stream(pipe.streams[s]):
                    work[s].copy_(raw_dev)
                ptrs = [images[(g * B + j) % len(images)].data_ptr() for j in range(B)]
                seeds = [g * B + j + 1 for j in range(B)]
                pipe.enqueue_kinect_batch(s, ptrs, [work[s][j].data_ptr() for j in range(B)],
                                          [fill[s][j].data_ptr() for j in range(B)], W, H, seeds, fill_scale=8, max_keypoints=CAP)
        return run

    def timed(fn, groups):
        pipe.synchronize()
        t0 = time.perf_counter()
        fn(groups)
        pipe.synchronize()
        return time.perf_counter() - t0

    forms = (("gray", form(t_gray, None)), ("bgr8", form(t_bgr, bgr_fmt)), ("gold", form(t_gold, None)))
    groups, heads = {}, {}
    for name, fn in forms:
        fn(2 * SLOTS)
        for c_ in pipe.ctxs:
            c_.frame_fetch_slot(0)
            c_.depth_fill_status()
        dt = timed(fn, 2 * SLOTS)
        groups[name] = max(SLOTS, int(np.ceil(args.seconds / dt * 2)) * SLOTS)
        last = pipe.ctxs[SLOTS - 1]
        heads[name] = [last.frame_fetch_slot(j) for j in range(B)]
        hits = sum(int(len(o) > 0 and o[np.argmax(o["score"])]["model"] == args.models) for o, _ in heads[name])
        print(f"# {name}: warm; {groups[name] * B} frames per window; planted model is the best object in {hits} of the {B} frames fetched")
    same = all(a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) for a, b in zip(heads["gray"], heads["bgr8"]))
    print(f"# gray and bgr8 deliver the same objects and counts for the 16 frames fetched: {same}")
    rates = {n: [] for n, _ in forms}
    for r in range(args.rounds):
        for name, fn in forms:
            dt = timed(fn, groups[name])
            rates[name].append(groups[name] * B / dt)
            print(f"(b) round {r + 1} {name:5s} {rates[name][-1]:9.1f} frames/s   window {dt:.3f} s")
    for name, v in rates.items():
        print(f"(b) {name:5s} min {min(v):.1f} max {max(v):.1f} median {np.median(v):.1f} spread {max(v) - min(v):.1f} frames/s")
    a, b = rates["gray"], rates["bgr8"]
    slower = min(a) > max(b) and min(a) - max(b) >= 3 * (max(b) - min(b)) and min(a) - max(b) >= 3 * (max(a) - min(a))
    faster = min(b) > max(a) and min(b) - max(a) >= 3 * (max(a) - min(a)) and min(b) - max(a) >= 3 * (max(b) - min(b))
    print("(b) gray against bgr8, verdict under the project's rule (every round beyond every round of the other side, by more than three times the "
          "spread): " + ("bgr8 with the format set is slower" if slower else "bgr8 with the format set is faster" if faster else "no claim"))
    pipe.set_image_format(None)
    for c_ in pipe.ctxs:
        c_.depth_fill_status()
    pipe.close()


if __name__ == "__main__":
    main()
