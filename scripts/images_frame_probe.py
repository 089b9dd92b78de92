"""Frames with several cameras from device images (mh_frame_enqueue_images[_batch]): what the hand-over on the device
buys and what it costs.  Scene: the planted planar model of tests/test_gpu_image_frame.py.

  images_frame_probe.py                 latency of ONE two-camera frame (gray0 + gray3, ~590 keypoints each), new path
                                        against the host round trip (the only way before: extract, synchronise, concatenate,
                                        upload, mh_frame_set_images, mh_frame_enqueue), the two alternating; then frames/s of
                                        batches of 8 frames x 2 cameras against 16 one-camera images per batch
                                        (mh_frame_enqueue_image_batch: the same FEAT work, no hand-over).
  images_frame_probe.py trace           a few two-camera frames at 2 x ~590 and at 2 x ~3 240 keypoints
                                        (synth.textured_image) -- the program of a `rocprofv3 --kernel-trace --stats` run
  images_frame_probe.py report DIR      reads that run's kernel trace (csv) under DIR: time of the hand-over kernel and of
                                        normalize_kernel per frame, bytes moved (from the shapes) and bytes/s
"""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

TRACE_WARM, TRACE_N = 3, 20
ROW_BYTES = 2 * (128 * 4 + 2 * 4) + 4     # a packed row: descriptor and coordinates read and written, the image index written


def report(where):
    plan = json.load(open(os.path.join(where, "images_frame_probe_plan.json")))
    files = glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {where}")
    pack, norm = [], []
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        if "images_pack_kernel" in name:
            pack.append(dur)
        elif "normalize_kernel" in name and len(pack) > len(norm):   # (the frame's: right behind its hand-over; the DB's come first)
            norm.append(dur)
    per = TRACE_WARM + TRACE_N
    print(f"hand-over kernel (images_pack_kernel) and normalize_kernel per two-camera frame, {TRACE_N} frames per size, from {os.path.basename(files[0])}")
    for k, case in enumerate(plan["cases"]):
        p = pack[k * per + TRACE_WARM:(k + 1) * per]
        n = norm[k * per + TRACE_WARM:(k + 1) * per]
        rows = sum(case["counts"])
        nbytes = rows * ROW_BYTES
        print(f"  {case['name']}: keypoints {case['counts']} (capacity {case['cap']} per image), {nbytes / 1e6:.2f} MB moved: "
              f"hand-over median {statistics.median(p):.2f} us (min {min(p):.2f}, max {max(p):.2f}) = "
              f"{nbytes / statistics.median(p) / 1e3:.1f} GB/s; normalize_kernel median {statistics.median(n):.2f} us "
              f"(reads and writes the same {rows} rows once more)")


if len(sys.argv) > 2 and sys.argv[1] == "report":
    report(sys.argv[2])
    sys.exit(0)

import torch
from moped_amd import capi, synth

gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
dev = torch.device("cuda:0")
H, W = gold["gray0"].shape
prm = capi.default_frame_params()
Ks, cams = [K, K], [CAM0, CAM0]


def make_ctx(rows):
    c = capi.Context(0)
    s = torch.cuda.Stream(device=dev)
    c.set_stream(s.cuda_stream)
    return c, s


def planted_db(c0):
    xy, _, desc = c0.sift(gold["gray0"])
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    bg = synth.make_db(20, 5000)
    return (c0.normalize(np.concatenate([bg.desc, desc])), np.concatenate([bg.model_of, np.full(len(xy), 20, np.int32)]),
            np.concatenate([bg.xyz, xyz]), 21)


if len(sys.argv) > 1 and sys.argv[1] == "trace":
    out = sys.argv[2] if len(sys.argv) > 2 else os.getcwd()   # (where the profiler's run writes: `report` reads the plan there)
    c, s = make_ctx(0)
    c.db_upload(*planted_db(c))
    cases = []
    for name, grays, cap in (("2 x bundled frame", [gold["gray0"], gold["gray3"]], 1024),
                             ("2 x textured image", [synth.textured_image(1), synth.textured_image(2)], 4096)):
        c.reserve(2 * cap)
        g = [torch.from_numpy(x).to(dev) for x in grays]
        torch.cuda.synchronize()
        for i in range(TRACE_WARM + TRACE_N):
            c.frame_enqueue_images([x.data_ptr() for x in g], W, H, True, cap, Ks, cams, prm, seed=i + 1)
            objs, counts = c.frame_fetch()
        cases.append({"name": name, "cap": cap, "counts": c.frame_image_counts().tolist(), "objects": len(objs)})
    json.dump({"cases": cases}, open(os.path.join(out, "images_frame_probe_plan.json"), "w"))
    c.close()
    sys.exit(0)

# ---- one frame alone: latency, the two paths alternating ----------------------------------------------------------
CAP = 1024
c, s = make_ctx(0)
db = planted_db(c)
c.db_upload(*db)
c.reserve(2 * CAP)
imgs = [torch.from_numpy(gold["gray0"]).to(dev), torch.from_numpy(gold["gray3"]).to(dev)]
ptrs = [g.data_ptr() for g in imgs]
with torch.cuda.stream(s):
    st_desc = [torch.empty((CAP, 128), dtype=torch.float32, device=dev) for _ in imgs]
    st_xy = [torch.empty((CAP, 2), dtype=torch.float32, device=dev) for _ in imgs]
    st_n = torch.zeros(2, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def new_path(seed):
    c.frame_enqueue_images(ptrs, W, H, True, CAP, Ks, cams, prm, seed)
    return c.frame_fetch()


def round_trip(seed, through_host):
    """extract each image, synchronise and read the counts, concatenate (on the host: through_host; else with device
    copies), upload, mh_frame_set_images, mh_frame_enqueue, fetch"""
    for i, p in enumerate(ptrs):
        c.sift_dev(p, W, H, True, st_desc[i].data_ptr(), st_xy[i].data_ptr(), 0, CAP, st_n.data_ptr() + 4 * i)
    with torch.cuda.stream(s):
        n = [min(int(x), CAP) for x in st_n.cpu()]          # the synchronisation: the counts cross to the host
        if through_host:
            desc = np.concatenate([st_desc[i][:n[i]].cpu().numpy() for i in range(2)])
            xy = np.concatenate([st_xy[i][:n[i]].cpu().numpy() for i in range(2)])
            q_desc, q_uv = torch.from_numpy(desc).to(dev), torch.from_numpy(xy).to(dev)
        else:
            q_desc = torch.cat([st_desc[i][:n[i]] for i in range(2)])
            q_uv = torch.cat([st_xy[i][:n[i]] for i in range(2)])
        q_img = torch.from_numpy(np.repeat(np.arange(2, dtype=np.int32), n)).to(dev)
    c.frame_set_images(q_img.data_ptr(), Ks, cams)
    c.frame_enqueue(q_desc.data_ptr(), q_uv.data_ptr(), sum(n), K, CAM0, prm, seed)
    out = c.frame_fetch()
    c.frame_set_images(None)
    return out


paths = [("mh_frame_enqueue_images (hand-over on the device)", lambda sd: new_path(sd)),
         ("round trip, lists concatenated on the host", lambda sd: round_trip(sd, True)),
         ("round trip, lists concatenated with device copies", lambda sd: round_trip(sd, False))]
WARM, REPS = 5, 40
times = [[] for _ in paths]
results = []
for r in range(WARM + REPS):
    for k, (_, fn) in enumerate(paths):
        s.synchronize()
        t0 = time.perf_counter()
        res = fn(7)
        dt = time.perf_counter() - t0
        if r >= WARM:
            times[k].append(dt * 1e3)
        if r == WARM:
            results.append(res)
same = all(results[0][0].tobytes() == x[0].tobytes() and np.array_equal(results[0][1], x[1]) for x in results[1:])
print(f"ONE two-camera frame, gray0 + gray3 ({c.frame_keypoints()} keypoints), image on the device to objects on the host, "
      f"{REPS} frames per path, the paths alternating; objects {len(results[0][0])}, identical on all paths: {same}")
for (name, _), t in zip(paths, times):
    q = statistics.quantiles(t, n=4)
    print(f"  {name}: median {statistics.median(t):.3f} ms (quartiles {q[0]:.3f} .. {q[2]:.3f}, min {min(t):.3f})")
c.close()

# ---- batches: 8 frames x 2 cameras against 16 one-camera images, two contexts in flight --------------------------------
DEPTH, BATCHES, BLOCKS = 2, 30, 3
slots = []
for i in range(DEPTH):
    ci, si = make_ctx(0)
    ci.db_upload(*db)
    ci.reserve(16 * CAP)
    slots.append(ci)
batch_ptrs = [ptrs[j % 2] for j in range(16)]
torch.cuda.synchronize()


def rig_batches(k):
    for b in range(k):
        slots[b % DEPTH].frame_enqueue_images_batch(batch_ptrs, 2, W, H, True, CAP, Ks, cams, prm, [b * 8 + f + 1 for f in range(8)])


def image_batches(k):
    for b in range(k):
        slots[b % DEPTH].frame_enqueue_image_batch(batch_ptrs, W, H, True, CAP, K, CAM0, prm, [b * 16 + f + 1 for f in range(16)])


rates = {"rig": [], "image": []}
for blk in range(BLOCKS + 1):                                 # (block 0 warms both up)
    for name, fn in (("rig", rig_batches), ("image", image_batches)):
        for ci in slots:
            ci.synchronize()
        t0 = time.perf_counter()
        fn(BATCHES)
        for ci in slots:
            ci.synchronize()
        dt = time.perf_counter() - t0
        if blk:
            rates[name].append(16 * BATCHES / dt)
    if blk == 0:
        rig_batches(DEPTH)
        n_obj = [len(slots[0].frame_fetch_slot(f)[0]) for f in range(8)]
print(f"batches, {DEPTH} contexts in flight, {BATCHES} batches of 16 images per block, {BLOCKS} blocks per path, alternating "
      f"(objects per two-camera frame of a batch: {n_obj}):")
for name, label in (("rig", "8 frames x 2 cameras (mh_frame_enqueue_images_batch)"), ("image", "16 one-camera images (mh_frame_enqueue_image_batch)")):
    r = rates[name]
    per = " = " + "/".join(f"{x / 2:.0f}" for x in r) + " frames/s" if name == "rig" else ""
    print(f"  {label}: " + "/".join(f"{x:.0f}" for x in r) + f" images/s{per}")
for ci in slots:
    ci.close()
