"""moped3d's weighted mean shift through the host plugins.  CLUSTER_WEIGHTED_MEAN_SHIFT_HIP in the CLUSTER slot of the
eleven-step wiring (`moped3d_hip_test --cluster-wms R M MinPts MaxIter HWD`) on the synthetic Kinect scene of
tests/test_gpu_host_moped3d.py: the step's clusters[model] must be what the float32 restatement of the reference's class
(tests/wms_ref.py) and Context.cluster_wms make of the match records DEPTHPROP left -- same clusters, same order, same
members -- and the steps behind it must still report the planted objects.  On the bundled Kinect frame both wirings -- the
eleven steps and the one step FRAME_RESIDENT_3D_HIP with its ClusterWeighted... keys (--resident) -- and the frame composed
through capi give the same clusters and objects.  The header's two compile checks pass."""
import os
import subprocess

import numpy as np
import pytest

import wms_ref
from moped_amd import capi, synth
from test_gpu_host_moped3d import FEATURE_DENSITY, K, CAM0, MATCH_DENSITY, dump_scene, run_harness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
WMS = (0.1, 0.02, 7, 100, 10.0)   # Radius, Merge (metres), MinPts, MaxIterations, halfWeightDistance (pixels)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    db = synth.make_db(4, 600)
    fr = synth.make_frame(db, n_vis=2, seed=5, Q=800)
    img, fill = synth.depth_image(db, fr, seed=5)
    path = str(tmp_path_factory.mktemp("wms") / "scene.bin")
    dump_scene.dump_kinect(path, db.desc, db.xyz, db.model_of, db.n_models, img, K, CAM0, uv=fr.uv, desc=fr.desc,
                           distance=fill, patch_size=64, feature_density=FEATURE_DENSITY, match_density=MATCH_DENSITY,
                           fill_scale=0)
    steps, extra = run_harness(["--cluster-wms"] + [str(v) for v in WMS] + [path])
    # the records DEPTHPROP left, per model in match order: what the CLUSTER step reads
    lists = [([], []) for _ in range(db.n_models)]
    for m, k, valid, x, y, z, depth, dist in steps["DEPTHPROP"]["depth"]:
        assert k == len(lists[m][0])
        lists[m][0].append((x, y, z))
        lists[m][1].append(dist)
    problems = [(np.array(p, np.float32).reshape(-1, 3), np.array(f, np.float32)) for p, f in lists]
    return dict(db=db, fr=fr, steps=steps, extra=extra, problems=problems)


def test_the_step_sits_in_the_cluster_slot(scene):
    assert scene["extra"]["order"] == ["DEPTHFILTER", "MATCH_SIFT", "DEPTHFILTER2", "DEPTHPROP", "CLUSTER", "POSE", "FILTER",
                                       "POSE2", "FILTER2"]
    assert sum(len(p[0]) for p in scene["problems"]) == len(scene["steps"]["CLUSTER"]["matches"]) > 200


def test_clusters_equal_the_restatement_and_the_python_path(ctx, scene):
    got = scene["steps"]["CLUSTER"]["clusters"]
    R, M, min_pts, max_iter, hwd = WMS
    py = ctx.cluster_wms(scene["problems"], capi.mh_wms_params(*WMS))
    n_clusters = 0
    for m, (xyz, fill) in enumerate(scene["problems"]):
        want, _, _, _ = wms_ref.weighted_mean_shift(xyz, wms_ref.cauchy_weight(fill, hwd), R, M, min_pts, max_iter)
        mine = [got[(m, c)] for c in range(sum(1 for key in got if key[0] == m))]
        print(f"model {m}: {len(xyz)} matches, {len(want)} clusters of {[len(w) for w in want]}")
        assert len(mine) == len(want) == len(py[m]), m
        for a, b, c in zip(mine, want, py[m]):
            assert np.array_equal(a, b) and np.array_equal(b, c), m
        n_clusters += len(want)
    for m in scene["fr"].visible:   # the planted objects' matches form clusters
        assert any(key[0] == m for key in got), m
    assert n_clusters == len(got)


def test_the_planted_objects_are_reported(scene):
    objs = scene["steps"]["FILTER2"]["objs"]
    print("objects of models", sorted(o[0] for o in objs), "visible", sorted(scene["fr"].visible))
    assert sorted(o[0] for o in objs) == sorted(scene["fr"].visible.tolist())
    fr = scene["fr"]
    for o in objs:   # the translation bar tests/test_gpu_host_moped3d.py holds the linkage wiring to on this scene: 1 cm
        t = np.array(o[1:4], np.float32)
        true = fr.poses[list(fr.visible).index(o[0])]   # (qx, qy, qz, qw, tx, ty, tz)
        print("model", o[0], "translation error", float(np.linalg.norm(t - true[4:])))
        assert np.linalg.norm(t - true[4:]) < 0.01, (o[0], t, true)


def test_both_wirings_and_the_python_path_agree_on_the_bundled_frame(tmp_path):
    """Scene B of tests/test_gpu_host_moped3d.py (bundled frame 0 as one planar model over the unfilled "blobs" map): the
    eleven-step wiring with the step in the CLUSTER slot, the one step FRAME_RESIDENT_3D_HIP with its ClusterWeighted... keys
    (--resident) and the same frame composed through capi with frame_set_cluster_wms give the same clusters and objects."""
    import torch
    import orclib
    from moped_amd import moped3d
    from test_gpu_depthfill import holes
    from test_gpu_host_moped3d import _bits, moped3d_params
    big = (0.7, 0.05, 7, 100, 10.0)      # a Radius that holds the metre-wide plane
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    gray = np.ascontiguousarray(gold["gray0"])
    H, W, CAP = 480, 640, 1024
    c = capi.Context(0)
    try:
        xy, _, desc = c.sift(gray)
        z = np.float32(0.8)
        xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
        rng = np.random.default_rng(7)
        db_desc = np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(np.float32)])
        db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)])
        model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
        zmap = np.full((H, W), 0.8, np.float32)
        zmap[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = -1.0
        raw = np.zeros((H, W, 4), np.float32)
        u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
        raw[..., 2] = zmap
        raw[..., 0] = (u - K[2]) / K[0] * zmap
        raw[..., 1] = (v - K[3]) / K[1] * zmap
        raw[..., 3] = np.sqrt((raw[..., :3] ** 2).sum(-1))
        path = str(tmp_path / "scene_b.bin")
        dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, K, CAM0, gray=gray, patch_size=64,
                               feature_density=0.8, match_density=0.01, fill_scale=8, max_keypoints=CAP)
        opt = ["--cluster-wms"] + [str(x) for x in big]
        wired, _ = run_harness(opt + [path])
        res, extra = run_harness(["--resident"] + opt + [path])
        got = res["DEPTHFILL"]
        # the same frame composed through capi: the plugin's first frame has seed 1 * 2654435761 + 0
        c.db_upload(c.normalize(db_desc), model_of, db_xyz, 2)
        c.reserve(CAP)
        c.frame_set_depth_rules(K, 64, 0.8, 0.01, moped3d.ratio_table(db_xyz, model_of, 2, K))
        c.frame_set_cluster_wms(capi.mh_wms_params(*big))
        dev = torch.device("cuda:0")
        t_gray, t_map = torch.from_numpy(gray).to(dev), torch.from_numpy(raw).to(dev)
        t_fill = torch.zeros((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        c.depth_fill_dev(t_map.data_ptr(), W, H, K, t_fill.data_ptr(), 8, False)
        c.frame_set_depth_image(t_map.data_ptr(), t_fill.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        c.frame_enqueue_image(t_gray.data_ptr(), W, H, True, CAP, K, CAM0, moped3d_params(), 2654435761)
        objs, counts = c.frame_fetch()
        table = [(m, mem.tolist()) for m, mem in c.frame_debug_fetch_clusters_slot(0)]
        # ... and the restatement on that frame's own records
        pts = c.frame_fetch_match_points()
        mq, mm = c.frame_fetch_matches()
        uv = np.stack([pts["u"], pts["v"]], 1)
        world, _ = orclib.depthmap_prop(t_map.cpu().numpy(), t_fill.cpu().numpy(), uv, 0.1)
        fillv = t_fill.cpu().numpy()[np.clip(uv[:, 1].astype(np.int32), 0, H - 1), np.clip(uv[:, 0].astype(np.int32), 0, W - 1)]
    finally:
        c.frame_set_cluster_wms(None)
        c.close()

    def per_model(clusters):
        return [(m, clusters[(m, k)]) for m in range(2) for k in range(sum(1 for key in clusters if key[0] == m))]
    want = []
    for m in range(2):
        sel = mm == m
        if sel.sum() > big[2]:
            cl, _, _, _ = wms_ref.weighted_mean_shift(world[sel], wms_ref.cauchy_weight(fillv[sel], big[4]), *big[:4])
            want += [(m, x.tolist()) for x in cl]
    print("counts", counts, "harness", extra["counts"], "clusters", [(m, len(x)) for m, x in table])
    assert len(objs) >= 1 and counts[0] > 50 and len(table) >= 1
    assert table == want
    assert per_model(wired["CLUSTER"]["clusters"]) == table          # the eleven-step wiring
    assert per_model(got["clusters"]) == table                       # the one-step wiring
    assert extra["counts"] == counts.tolist()
    assert [g[0] for g in wired["FILTER2"]["objs"]] == [g[0] for g in got["objs"]] == objs["model"].tolist()
    for g, o in zip(got["objs"], objs):                              # the one step IS the capi composition: the same bits
        assert np.array_equal(_bits(g[4:8] + g[1:4]), _bits(o["pose"]))
    best = objs[np.argmax(objs["score"])]                            # the pose bar of tests/test_gpu_kinect_image_batch.py
    assert best["model"] == 0 and np.abs(best["pose"][4:7]).max() < 0.05 and abs(abs(best["pose"][3]) - 1) < 0.01


def test_header_compiles_at_the_references_language_level():
    for target in ("check98_wms", "check_ref_wms"):
        r = subprocess.run(["make", "-s", "-B", "-C", HOST, target], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
