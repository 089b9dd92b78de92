"""Buffers that grow on a live context (csrc/devbuf.h: every owned device / pinned block is a DevBuf, grown by ensure()).
Each case takes ONE context through small -> large -> small; what every step returns must be bit for bit what a fresh
context returns for that step alone -- so a block that was replaced, kept or handed on wrongly shows as a difference.
The paths here are the ones the rest of the suite does not regrow (it covers the query count of mh_match, a DB
re-upload, the frame capacities and the DB edits)."""
import numpy as np
import pytest

import undistort_ref as ur
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
DB = synth.make_db(3, 500)


def fresh():
    c = capi.Context(0)
    c.db_upload(DB.desc, DB.model_of, DB.xyz, DB.n_models)
    return c


def blob(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def check_regrow(steps, run, setup=None, after=None):
    """steps: [(key, args)]; run(c, args) -> comparable.  One context through all of them, then every distinct step on a
    context of its own.  after(c) -> comparable: one more call on the grown context, against a context that saw only
    the setup."""
    c = fresh()
    keep = setup(c) if setup else None
    got = [run(c, args) for _, args in steps]
    got_after = after(c) if after else None
    c.close()
    want = {}
    for i, (key, args) in enumerate(steps):
        if key not in want:
            f = fresh()
            keep_f = setup(f) if setup else None
            want[key] = run(f, args)
            f.close()
            del keep_f
        assert got[i] == want[key], f"step {i} ({key}) differs from a fresh context"
    if after:
        f = fresh()
        keep_f = setup(f) if setup else None
        want_after = after(f)
        f.close()
        del keep_f
        assert got_after == want_after, "the call after the steps differs from a fresh context"
    del keep
    return got


def set_depth_image_host(c, img, fill, kind=capi.DEPTH_BACKPROJECTION, alpha=0.5, cauchy=0.1):
    h, w = img.shape[:2]
    c._ck(c.L.mh_frame_set_depth_image_host(c.h, capi._ptr(img), capi._ptr(fill), w, h, kind, alpha, cauchy),
          "mh_frame_set_depth_image_host")


def run_host(c, fr, seed=3, Ks=None, cams=None, q_image=None):
    objs, counts = c.frame_run_host(fr.desc.copy(), fr.uv, [K] if Ks is None else Ks, [CAM0] if cams is None else cams,
                                    capi.default_frame_params(), seed, q_image=q_image)
    q, m = c.frame_fetch_matches()
    return objs, counts, q, m


# (a) mh_frame_run_host, two cameras: the frame buffers and the copy of the image indices past their first 4096 rows
def test_host_frames_of_two_cameras_across_the_first_capacity():
    cams = [CAM0, synth.camera_pose(0.12, (0.08, 0.0, 0.0))]
    frames = {q: synth.make_frame_images(DB, cams, n_vis=2 if q > 100 else 1, seed=40 + q, q_per_image=q // 2,
                                         pts_per_obj=120 if q > 1000 else 30) for q in (100, 5000, 300)}
    found = []

    def run(c, q):
        fr = frames[q]
        assert len(fr.desc) == q
        objs, counts, mq, mm = run_host(c, fr, Ks=list(fr.Ks), cams=list(fr.cams), q_image=fr.image)
        found.append(len(objs))
        return blob(objs, counts, mq, mm)

    check_regrow([(q, q) for q in (100, 5000, 300)], run)
    assert max(found) >= 1 and found[1] >= 1


# (b) mh_frame_fetch_batch_async into pageable memory: the staging block behind the delivery grows with max_objects
def test_delivery_staging_grows_with_max_objects():
    import torch
    dev = torch.device("cuda:0")
    B, Q = 2, 600
    frs = [synth.make_frame(DB, n_vis=2, seed=70 + f, Q=Q, pts_per_obj=100) for f in range(B)]
    qd = torch.cat([torch.from_numpy(f.desc) for f in frs]).to(dev)
    uv = torch.cat([torch.from_numpy(f.uv) for f in frs]).to(dev)
    torch.cuda.synchronize()
    prm = capi.default_frame_params()
    totals = []

    def run(c, cap):
        work = qd.clone()   # (MATCH normalises the descriptors in place)
        torch.cuda.synchronize()
        c.frame_enqueue_batch(work.data_ptr(), uv.data_ptr(), Q, B, K, CAM0, prm, [5, 6])
        block = np.zeros(B, capi.frame_block_dtype(cap))   # pageable: the device cannot write it, the copy goes through the staging block
        c.frame_fetch_batch_async(B, cap, block.ctypes.data, 100 + cap)
        c.frame_fetch_wait()
        out = []
        for f in range(B):
            n = int(block[f]["head"]["n_objects"])
            totals.append(n)
            out += [block[f]["head"], block[f]["objects"][:min(n, cap)]]
            objs, _ = c.frame_fetch_slot(f)   # the records are the slots' own objects
            assert n == len(objs) and block[f]["objects"][:min(n, cap)].tobytes() == objs[:cap].tobytes()
        return blob(*out)

    check_regrow([(cap, cap) for cap in (4, 64, 4)], run)
    assert sum(totals) >= 2


# (c) mh_frame_enqueue_images: one camera, two cameras of another size with a larger capacity, one again -- the image
# hand-over's lists, the rebuilt SIFT state, and the views of the cameras / image indices the call points at its own
def test_image_frames_regrow_and_leave_the_callers_camera_table_alone():
    import torch
    from moped_amd.pipeline import _DevMem
    dev = torch.device("cuda:0")
    small = [synth.textured_image(11, 96, 96)]
    large = [synth.textured_image(12, 120, 160), synth.textured_image(13, 120, 160)]
    t_small = [torch.from_numpy(g).to(dev) for g in small]
    t_large = [torch.from_numpy(g).to(dev) for g in large]
    rig = [CAM0, synth.camera_pose(0.1, (0.05, 0.0, 0.0))]
    prm = capi.default_frame_params()
    # the caller's own table (mh_frame_set_images): another rig than the image calls use, for a frame of planted objects
    mine = [CAM0, synth.camera_pose(-0.15, (-0.1, 0.0, 0.0))]
    fr = synth.make_frame_images(DB, mine, n_vis=2, seed=9, q_per_image=400, pts_per_obj=120)
    f_desc, f_uv, f_img = (torch.from_numpy(a).to(dev) for a in (fr.desc, fr.uv, fr.image))
    torch.cuda.synchronize()
    keypoints = []

    def setup(c):
        c.frame_set_images(f_img.data_ptr(), list(fr.Ks), list(fr.cams))

    def run(c, step):
        imgs, w, h, cap, n = step
        c.frame_enqueue_images([t.data_ptr() for t in imgs], w, h, True, cap, [K] * n, rig[:n], prm, 21)
        objs, counts = c.frame_fetch()
        total, per_image = c.frame_keypoints(), c.frame_image_counts()
        keypoints.append(total)
        assert len(per_image) == n and total == int(per_image.sum()) and 0 < total <= n * cap
        d_ptr, u_ptr, _ = c.frame_features_dev()
        get = lambda p, shape: torch.as_tensor(_DevMem(p, shape, "<f4"), device=dev).cpu().numpy()
        mq, mm = c.frame_fetch_matches()
        return blob(objs, counts, per_image, get(d_ptr, (total, 128)), get(u_ptr, (total, 2)), mq, mm)

    def after(c):   # a plain frame of the caller's rig: its image indices and ITS cameras
        work = f_desc.clone()
        torch.cuda.synchronize()
        c.frame_enqueue(work.data_ptr(), f_uv.data_ptr(), len(fr.desc), fr.Ks[0], fr.cams[0], prm, 4)
        objs, counts = c.frame_fetch()
        assert len(objs) >= 1
        return blob(objs, counts, *c.frame_fetch_matches())

    one = (t_small, 96, 96, 256, 1)
    check_regrow([("one", one), ("two", (t_large, 160, 120, 1024, 2)), ("one", one)], run, setup, after)
    assert keypoints[1] > 256   # (the packed rows did outgrow the first call's 256)


# (d) the depth rules: the ratio table for 3 models, 6, none; patch maps of 8 x 6, then 40 x 30 patches
def test_depth_rule_tables_and_patch_maps_regrow():
    fr = synth.make_frame(DB, n_vis=2, seed=21, Q=900, pts_per_obj=140)
    img, fill = synth.depth_image(DB, fr, seed=21, fill_max=0.3)
    rng = np.random.default_rng(3)
    # per model (maxRatioDepth, minRatioDepth, ratioLow, ratioHigh): the ratio falls from High to Low between the two depths
    table6 = np.tile(np.float32([0.7, 1.6, 0.7, 0.85]), (6, 1)) + rng.uniform(-0.05, 0.05, (6, 4)).astype(np.float32)
    sizes = []

    def setup(c):
        set_depth_image_host(c, img, fill)

    def run(c, step):
        table, patch = step
        c.frame_set_depth_rules(K, patch, 0.02, 0.004, table)
        objs, counts, mq, mm = run_host(c, fr)
        pw, ph = -(-640 // patch), -(-480 // patch)
        sizes.append((pw, ph, len(mq)))
        inv = c.depth_rules_debug_fetch("inv_size", 0, pw * ph)
        keep = c.depth_rules_debug_fetch("keep1", 0, len(fr.desc))
        return blob(objs, counts, mq, mm, inv, keep)

    check_regrow([("t3", (table6[:3], 80)), ("t6", (table6, 16)), ("none", (None, 80))], run, setup)
    assert [s[:2] for s in sizes[:3]] == [(8, 6), (40, 30), (8, 6)] and all(s[2] > 0 for s in sizes)


# (e) the context's own copies of a host depth map: one pair of blocks, grown by either of its two callers
def test_own_depth_maps_are_shared_by_both_host_entry_points():
    k = (K * np.float32(0.1)).astype(np.float32)   # the 640 x 480 scene at a tenth of its size
    fr = synth.make_frame(DB, n_vis=2, seed=31, Q=700, pts_per_obj=140)
    world, _ = synth.frame_depth(DB, fr, seed=31)
    fr.uv = np.ascontiguousarray(fr.uv * np.float32(0.1))
    v, u = np.mgrid[0:48, 0:64].astype(np.float64)
    z = 1.5 + 0.05 * np.sin(u / 9.0) * np.cos(v / 7.0)
    small = np.stack([(u + 0.5 - k[2]) / k[0] * z, (v + 0.5 - k[3]) / k[1] * z, z, np.zeros_like(z)], -1)
    rows = np.nonzero((fr.src_point >= 0) & ~fr.is_outlier)[0]   # the planted points in front of that background
    small[np.clip(fr.uv[rows, 1].astype(np.int32), 0, 47), np.clip(fr.uv[rows, 0].astype(np.int32), 0, 63), :3] = world[rows]
    small[..., 3] = np.sqrt((small[..., :3] ** 2).sum(-1))
    small = np.ascontiguousarray(small, np.float32)
    small_fill = np.zeros((48, 64), np.float32)
    rng = np.random.default_rng(8)
    big = synth.depth_image(DB, synth.make_frame(DB, n_vis=1, seed=5, Q=200, pts_per_obj=50), seed=5)[0][::4, ::4].copy()
    big[rng.random(big.shape[:2]) < 0.2, 3] = -1.0   # holes for the fill
    assert big.shape == (120, 160, 4)
    found = []

    def run(c, step):
        if step == "frame":
            set_depth_image_host(c, small, small_fill)
            objs, counts = c.frame_run_host(fr.desc.copy(), fr.uv, [k], [CAM0], capi.default_frame_params(), 3)
            found.append(int(counts[0]))
            print("own depth map: objects", len(objs), "counts", counts.tolist())
            return blob(objs, counts, *c.frame_fetch_matches())
        filled, dist, used = c.depth_fill(big, K * np.float32(0.25), 4)
        return blob(filled, dist, np.int32(used))

    check_regrow([("frame", "frame"), ("fill", "fill"), ("frame", "frame")], run)
    assert found[0] > 0   # (accepted matches: every one looks its depth up in the small map)


# (f) mh_undistort: a map entry, the staging image and the result grow, then a second calibration at the small size
def test_undistort_maps_and_staging_regrow():
    rng = np.random.default_rng(17)
    small = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    large = rng.integers(0, 256, (240, 320), dtype=np.uint8)
    cam_a = ([80.0, 81.0, 32.0, 24.0], [-0.3, 0.1, 1e-3, -1e-3])
    cam_b = ([400.0, 398.0, 161.0, 119.0], [0.2, -0.1, -2e-3, 1e-3])
    cam_c = ([75.0, 75.0, 30.0, 25.0], [0.15, 0.05, 0.0, 2e-3])
    steps = [("a", (small, cam_a)), ("b", (large, cam_b)), ("c", (small, cam_c))]

    def run(c, step):
        img, (k, dist) = step
        return blob(c.undistort(img, k, dist), *c.undistort_map(img.shape[1], img.shape[0], k, dist))

    got = check_regrow(steps, run)
    for (_, (img, (k, dist))), g in zip(steps, got):
        assert g[0] == ur.undistort(img, k, dist).tobytes()
        assert g[0] != img.tobytes()


# (g) the linkage clusterer's similarity-matrix scratch: inside the frame (sized by the frame's queries) and as a step
def test_linkage_scratch_regrows():
    frames, maps = {}, {}
    for q in (200, 1500):
        frames[q] = synth.make_frame(DB, n_vis=2, seed=50 + q, Q=q, pts_per_obj=60 if q == 200 else 140)
        maps[q] = synth.depth_image(DB, frames[q], seed=50 + q, fill_max=0.3)
    rng = np.random.default_rng(23)
    problems = {}
    for n in (50, 600):   # (more than 160 points: the matrices live in the scratch, not in LDS)
        world = np.concatenate([rng.normal(c0, 0.03, (n // 2, 3)) for c0 in ([0.1, 0.0, 0.8], [-0.2, 0.1, 1.1])]).astype(np.float32)
        uv = (world[:, :2] / world[:, 2:] * K[:2] + K[2:]).astype(np.float32)
        problems[n] = (uv, (world + rng.normal(0, 0.002, world.shape)).astype(np.float32), world)
    found = []

    def run(c, q):
        set_depth_image_host(c, *maps[q])
        c.frame_set_cluster_linkage(capi.default_linkage_params())
        objs, counts, mq, mm = run_host(c, frames[q])
        found.append((len(objs), int(counts[1])))
        (clusters, label), = c.cluster_linkage([problems[50 if q == 200 else 600]])
        return blob(objs, counts, mq, mm, label, *clusters)

    check_regrow([(q, q) for q in (200, 1500, 200)], run)
    assert all(n_obj >= 1 and n_cl >= 1 for n_obj, n_cl in found)
