"""Kinect depth maps from raw sensor depth on the device: what the map build costs, and what it saves a host.

(a) the map build alone (mh_depth_map_from_raw_dev / _batch_dev): ms per 640 x 480 map, one map per call and per map in a
    batch of 16, float metres and 16-bit millimetres (the latter also as QVGA resized to 640 x 480); device events around
    CALLS calls on the stream, ROUNDS rounds; against the time the 4.9 MB write alone takes at the HBM rate.
(b) the host loop that builds the same map (moped_amd/host/kinect_depthmap_test --loop), ms per map, and the helper's
    whole call (upload, build, map back to the host) beside it.
(c) Kinect batches of 16 from PINNED HOST memory, scene and configuration of scripts/kinect_image_bench.py, 16 slots:
      upload_xyzn   the host holds finished xyzn maps (4.9 MB per frame go up), FramePipeline.enqueue_kinect_batch
      upload_raw    the host holds raw float z (1.2 MB per frame), FramePipeline.enqueue_kinect_raw_batch
    alternately, every round printed.  Both exclude the host's map build; "host build included" adds (b)'s ms per map
    to upload_xyzn's time per frame (a single-threaded host that builds, then enqueues) and, as the other bound, takes
    the slower of the two (a host that builds the next batch while the device works) -- computed, not measured.
(d) the device-resident batches of profiles/kinect_image_batch.txt (maps restored by one device copy per batch,
    enqueue_kinect_batch) in the same rounds: the existing path, re-measured.

usage: python scripts/kinect_raw_bench.py [--models 5] [--rounds 5] [--seconds 1.2] > profiles/kinect_raw_depth.txt
One process on an otherwise idle device ((b) starts the host program, one more); every shape is warmed before it is timed."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLOTS, B, CAP, W, H = 16, 16, 1024, 640, 480
CALLS, ROUNDS = 50, 20
HBM_TBS = 6.3   # achievable HBM rate of the MI355X (8.0 TB/s on paper)


def holed_z(seed):
    """The z = 0.8 plane [H, W] as a sensor delivers it: NaN shadows beside objects, a dead border, speckle
    (the holes of kinect_image_bench.holed_plane)."""
    rng = np.random.default_rng(seed)
    z = np.full((H, W), 0.8, np.float32)
    yy, xx = np.ogrid[:H, :W]
    for _ in range(25):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 70)
        z[(yy - cy) ** 2 + ((xx - cx) * rng.uniform(0.3, 1.0)) ** 2 < r * r] = np.nan
    z[:, :12] = np.nan
    z[-9:, :] = np.nan
    z[rng.random((H, W)) < 0.01] = np.nan
    return z


def host_program(args):
    exe = os.path.join(ROOT, "moped_amd", "host", "kinect_depthmap_test")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"kinect_depthmap_test {args}: exit {r.returncode}: {r.stdout} {r.stderr[-500:]}")
    t = r.stdout.split()
    return float(t[t.index("HOST_MS") + 1]), float(t[t.index("HIP_MS") + 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.2)
    args = ap.parse_args()
    import torch
    import depthmap_ref as ref
    from moped_amd import capi, moped3d, synth
    from moped_amd.pipeline import FramePipeline, ShardedDB
    K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
    dev = torch.device("cuda:0")
    print("# Kinect depth maps from raw sensor depth (csrc/depthmap.hip); GPU_MAX_HW_QUEUES=" + str(os.environ.get("GPU_MAX_HW_QUEUES")))

    # ---- (b) first: the host program alone on the device ----
    host_ms = {}
    for name, a in (("f32 640x480", ["--format", "f32"]), ("u16 640x480", ["--format", "u16"]),
                    ("cloud 640x480 (point_step 32)", ["--format", "cloud"]),
                    ("u16 320x240 -> 640x480", ["--format", "u16", "--raw", 320, 240, "--map", 640, 480])):
        rows = [host_program(a + ["--loop", 50]) for _ in range(3)]
        hs, ds = [r[0] for r in rows], [r[1] for r in rows]
        host_ms[name] = float(np.median(hs))
        print(f"(b) {name:30s} host loop {np.median(hs):.3f} ms per map (min {min(hs):.3f} max {max(hs):.3f}); "
              f"hipKinectDepthmap, host memory to host memory {np.median(ds):.3f} ms (min {min(ds):.3f} max {max(ds):.3f}); "
              f"3 runs of 50 maps, one thread, 0 differing bytes")

    # ---- the scene of scripts/kinect_image_bench.py ----
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
    zs = np.stack([holed_z(10 + j) for j in range(B)])                                        # [B, H, W] float, NaN holes
    maps = np.stack([ref.depth_map(*ref.plain(zs[j]), K, W, H) for j in range(B)])            # [B, H, W, 4]: the host's build
    pin_xyzn = torch.from_numpy(maps).pin_memory()
    pin_raw = torch.from_numpy(zs).pin_memory()
    raw_dev = torch.from_numpy(maps).to(dev)                       # (d): the maps resident on the device
    work = [torch.empty_like(raw_dev) for _ in range(SLOTS)]
    fill = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(SLOTS)]
    zwork = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(SLOTS)]
    torch.cuda.synchronize()
    fmt32 = capi.make_raw_depth(capi.RAW_DEPTH_F32_M, W, H)

    # ---- (a) the build alone ----
    c, st = pipe.ctxs[0], pipe.streams[0]
    mm = np.where(np.isnan(zs), 0, np.round(zs * 1000)).astype(np.uint16)
    t_z, t_mm = torch.from_numpy(zs).to(dev), torch.from_numpy(mm.view(np.int16)).to(dev)      # (the bits; torch has no uint16 copy everywhere)
    t_qv = torch.from_numpy(np.ascontiguousarray(mm[:, ::2, ::2]).view(np.int16)).to(dev)
    torch.cuda.synchronize()
    out_ptrs = [work[0][j].data_ptr() for j in range(B)]
    cases = (("f32 640x480", t_z, fmt32), ("u16 640x480", t_mm, capi.make_raw_depth(capi.RAW_DEPTH_U16_MM, W, H)),
             ("u16 320x240 -> 640x480", t_qv, capi.make_raw_depth(capi.RAW_DEPTH_U16_MM, W // 2, H // 2)))
    floor_us = W * H * 16 / (HBM_TBS * 1e12) * 1e6
    print(f"(a) the 4.9 MB of a 640x480 map at {HBM_TBS} TB/s (achievable HBM rate): {floor_us:.2f} us")
    for name, t_in, fmt in cases:
        in_ptrs = [t_in[j].data_ptr() for j in range(B)]
        got = {}
        for form in ("one map per call", "batch of 16"):
            ms = []
            for rep in range(-3, ROUNDS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.synchronize()
                e0.record(st)
                for k in range(CALLS):
                    if form == "batch of 16":
                        c.depth_map_from_raw_batch_dev(in_ptrs, fmt, K, out_ptrs, W, H)
                    else:
                        c.depth_map_from_raw_dev(in_ptrs[k % B], fmt, K, out_ptrs[k % B], W, H)
                e1.record(st)
                st.synchronize()
                if rep >= 0:
                    ms.append(e0.elapsed_time(e1) / CALLS / (B if form == "batch of 16" else 1))
            got[form] = ms
            print(f"(a) {name:24s} {form:17s} median {np.median(ms) * 1e3:8.2f} us per map  min {min(ms) * 1e3:.2f}  max {max(ms) * 1e3:.2f}"
                  f"  = {W * H * 16 / (np.median(ms) * 1e-3) / 1e12:.2f} TB/s written, {floor_us / (np.median(ms) * 1e3):.2f} of the rate above"
                  f"  ({ROUNDS} rounds of {CALLS} back-to-back calls, device events)")

    # ---- (c), (d) ----
    def batch_args(g):
        return [imgs[(g * B + j) % len(imgs)].data_ptr() for j in range(B)], [g * B + j + 1 for j in range(B)]

    def resident(groups):
        for g in range(groups):
            s = g % SLOTS
            with torch.cuda.stream(pipe.streams[s]):
                work[s].copy_(raw_dev)
            grays, seeds = batch_args(g)
            pipe.enqueue_kinect_batch(s, grays, [work[s][j].data_ptr() for j in range(B)],
                                      [fill[s][j].data_ptr() for j in range(B)], W, H, seeds, fill_scale=8, max_keypoints=CAP)

    def upload_xyzn(groups):
        for g in range(groups):
            s = g % SLOTS
            with torch.cuda.stream(pipe.streams[s]):
                work[s].copy_(pin_xyzn, non_blocking=True)
            grays, seeds = batch_args(g)
            pipe.enqueue_kinect_batch(s, grays, [work[s][j].data_ptr() for j in range(B)],
                                      [fill[s][j].data_ptr() for j in range(B)], W, H, seeds, fill_scale=8, max_keypoints=CAP)

    def upload_raw(groups):
        for g in range(groups):
            s = g % SLOTS
            with torch.cuda.stream(pipe.streams[s]):
                zwork[s].copy_(pin_raw, non_blocking=True)
            grays, seeds = batch_args(g)
            pipe.enqueue_kinect_raw_batch(s, grays, [zwork[s][j].data_ptr() for j in range(B)], fmt32, W, H, seeds,
                                          fill_scale=8, max_keypoints=CAP)

    def timed(fn, groups):
        pipe.synchronize()
        t0 = time.perf_counter()
        fn(groups)
        pipe.synchronize()
        return time.perf_counter() - t0

    def found(slot_fetch):
        objs, counts = slot_fetch
        return int(len(objs) > 0 and objs[np.argmax(objs["score"])]["model"] == args.models)

    forms = (("resident", resident), ("upload_xyzn", upload_xyzn), ("upload_raw", upload_raw))
    groups, heads = {}, {}
    for name, fn in forms:
        fn(2 * SLOTS)                                     # warm: every slot twice
        for c_ in pipe.ctxs:
            c_.frame_fetch_slot(0)
            c_.depth_fill_status()
        dt = timed(fn, 2 * SLOTS)
        groups[name] = max(SLOTS, int(np.ceil(args.seconds / dt * 2)) * SLOTS)
        last = pipe.ctxs[SLOTS - 1]
        heads[name] = [last.frame_fetch_slot(j) for j in range(B)]
        hits = sum(found(x) for x in heads[name])
        print(f"# {name}: warm; {groups[name] * B} frames per window; planted model is the best object in {hits} of the {B} frames fetched")
    same = all(a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
               for n in ("upload_xyzn", "upload_raw") for a, b in zip(heads["resident"], heads[n]))
    print(f"# the three forms deliver the same objects and counts for the 16 frames fetched: {same}")
    rates = {n: [] for n, _ in forms}
    for r in range(args.rounds):
        for name, fn in forms:
            dt = timed(fn, groups[name])
            rates[name].append(groups[name] * B / dt)
            tag = "(d)" if name == "resident" else "(c)"
            print(f"{tag} round {r + 1} {name:12s} {rates[name][-1]:9.1f} frames/s   window {dt:.3f} s")
    for name, v in rates.items():
        tag = "(d)" if name == "resident" else "(c)"
        print(f"{tag} {name:12s} min {min(v):.1f} max {max(v):.1f} median {np.median(v):.1f} spread {max(v) - min(v):.1f} frames/s")
    a, b = rates["upload_xyzn"], rates["upload_raw"]
    gain = min(b) > max(a) and min(b) - max(a) >= 3 * (max(a) - min(a))
    loss = min(a) > max(b) and min(a) - max(b) >= 3 * (max(b) - min(b))
    print("(c) host build excluded, verdict under the project's rule (every round above every round of the other side, by at "
          "least three times the other side's spread): " + ("upload_raw gains" if gain else "upload_xyzn is faster" if loss else "no claim"))
    hb = host_ms["f32 640x480"]
    per_frame = 1e3 / np.median(a)
    print(f"(c) host build included, computed from (b)'s {hb:.3f} ms per map: upload_xyzn {1e3 / (per_frame + hb):.1f} frames/s if the "
          f"one host thread builds, then enqueues; {1e3 / max(per_frame, hb):.1f} frames/s if it builds beside the device's work; "
          f"upload_raw has no host build: {np.median(b):.1f} frames/s")
    for c_ in pipe.ctxs:
        c_.depth_fill_status()
    pipe.close()


if __name__ == "__main__":
    main()
