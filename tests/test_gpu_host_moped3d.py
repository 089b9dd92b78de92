"""moped3d's pipeline through its STEP plugins, run for real: moped_amd/host/moped3d_hip_test wires a MopedPipeline as
moped3d/libmoped/src/config.hpp:38-49 with the HIP classes and prints the frame's lists after every step.

Scene A (the step path): synth.make_db(4, 600) + synth.make_frame(n_vis=2, Q=800) over synth.depth_image's map (it arrives
filled, with its distance map).  Every step's lists against the oracle: CONTROL lines, the match lists after MATCH_SIFT and
DEPTHFILTER2 (the recipe of test_gpu_configs_idx4_moped3d.py's _oracle_lists, restated), depthData after DEPTHPROP, the
clusters after CLUSTER, and the objects against the ctypes frame and the project's pose bars.
Densities 0.1 / 0.02 (config.hpp ships 0.05 / 0.01, which keep 99.6 % of this frame's features): on the oracle
DEPTHFILTER keeps 60 % of the features, DEPTHFILTER2 drops 30 of 335 matches, and both planted models keep more than 100
matches -- asserted on the oracle before the device is trusted.

Scene B (--resident): the scene of test_gpu_kinect_image_batch.py -- bundled frame 0's keypoints on a plane are model 0,
500 clutter rows model 1, over the 640x480 "blobs" map, unfilled, fill_scale 8 -- through FRAME_RESIDENT_3D_HIP, bit for
bit against depth_fill_dev -> frame_set_depth_image -> frame_enqueue_image -> fetch through capi with the same seed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orclib
from moped_amd import capi, moped3d, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import dump_scene  # noqa: E402

BIN = os.path.join(ROOT, "moped_amd", "host", "moped3d_hip_test")
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
FEATURE_DENSITY, MATCH_DENSITY = 0.1, 0.02


def _f(tok):
    return np.float32(float.fromhex(tok))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_harness(args):
    """-> {step: dict(matches=[(m, q, u, v, x, y, z)], depth=[...], clusters={(m, c): [..]}, objs=[...])}, extras."""
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    steps, extra, cur = {}, dict(control={}, order=[]), None
    for line in r.stdout.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "STEP":
            cur = steps[t[1]] = dict(matches=[], depth=[], clusters={}, objs=[], features=extra.pop("features", None))
            extra["order"].append(t[1])
        elif t[0] == "FEATURES":
            extra["features"] = int(t[1])          # (printed before the step's name: the count the step left)
        elif t[0] == "MATCH":
            cur["matches"].append((int(t[1]), int(t[2])) + tuple(_f(x) for x in t[3:8]))
        elif t[0] == "DEPTH":
            cur["depth"].append((int(t[1]), int(t[2]), int(t[3])) + tuple(_f(x) for x in t[4:9]))
        elif t[0] == "CLUSTER":
            cur["clusters"][(int(t[1]), int(t[2]))] = [int(x) for x in t[3:]]
        elif t[0] == "OBJ":
            cur["objs"].append((int(t[1]),) + tuple(_f(x) for x in t[2:10]))
        elif t[0] == "CONTROL":
            extra["control"][int(t[1])] = np.array([_f(x) for x in t[2:6]], np.float32)
        elif t[0] == "COUNTS":
            extra["counts"] = [int(x) for x in t[1:5]]
        elif t[0] in ("FPS", "DEPTH_MAP_UPLOADS"):
            extra[t[0]] = t[1]
    return steps, extra


def moped3d_params():
    """The frame parameters of the harness's wiring (config.hpp:46-49 with NHypotheses in place of the test counts)."""
    p = capi.default_frame_params()
    for pose, (align, min_pts, thr) in ((p.pose1, (5, 6, 8.0)), (p.pose2, (6, 8, 5.0))):   # (the LM iteration counts stay)
        pose.n_hypotheses, pose.max_objects_per_cluster = 1024, 4
        pose.n_pts_align, pose.min_n_pts_object, pose.error_threshold = align, min_pts, thr
    p.f1_min_points, p.f1_feature_distance, p.f1_min_score = 6, 4096.0, 2.0
    p.f2_min_points, p.f2_feature_distance, p.f2_min_score = 8, 8192.0, 1e-4
    return p


# ---- scene A -----------------------------------------------------------------------------------------------------------
def _oracle_lists(s, feature_density, match_density, table):
    """The match lists moped3d's rules leave (test_gpu_configs_idx4_moped3d.py:112-131, restated)."""
    db, fr, idx, d1, d2 = s["db"], s["fr"], s["idx"], s["d1"], s["d2"]
    ok = idx >= 0
    if feature_density >= 0:
        ok &= orclib.depthfilter_keep(s["img"], K, 64, feature_density, fr.uv)
    model = np.where(idx >= 0, db.model_of[np.maximum(idx, 0)], -1)
    with np.errstate(all="ignore"):
        q = (d1 / d2).astype(np.float32)
    r, reach = orclib.adaptive_ratio(s["img"], s["fill"], fr.uv, model, table)
    ok &= reach & (q < r)
    qs = np.nonzero(ok)[0]
    qs = qs[np.lexsort((qs, model[qs]))]
    if match_density >= 0:
        off = np.searchsorted(model[qs], np.arange(db.n_models + 1))
        qs = qs[orclib.depthfilter_keep(s["img"], K, 64, match_density, fr.uv[qs], off)]
    return qs.astype(np.int32), model[qs].astype(np.int32)


@pytest.fixture(scope="module")
def scene_a(tmp_path_factory):
    db = synth.make_db(4, 600)
    fr = synth.make_frame(db, n_vis=2, seed=5, Q=800)
    img, fill = synth.depth_image(db, fr, seed=5)
    dbn, qn = orclib.normalize(db.desc), orclib.normalize(fr.desc)
    idx, d1, d2 = orclib.match_2nn(dbn, qn)
    table = np.stack([orclib.adaptive_control_points(db.xyz[db.model_of == m].min(0), db.xyz[db.model_of == m].max(0), K,
                                                     int((db.model_of == m).sum())) for m in range(db.n_models)])
    s = dict(db=db, fr=fr, img=img, fill=fill, idx=idx, d1=d1, d2=d2, table=table)
    # the rules bite and both planted objects survive them, on the oracle
    s["after_match"] = _oracle_lists(s, FEATURE_DENSITY, -1, table)
    s["after_f2"] = _oracle_lists(s, FEATURE_DENSITY, MATCH_DENSITY, table)
    plain = _oracle_lists(s, -1, -1, table)
    assert len(s["after_f2"][0]) < len(s["after_match"][0]) < len(plain[0])
    assert 0.2 < orclib.depthfilter_keep(img, K, 64, FEATURE_DENSITY, fr.uv).mean() < 0.95
    for m in fr.visible:
        assert (s["after_f2"][1] == m).sum() > 100, m
    path = str(tmp_path_factory.mktemp("moped3d") / "scene_a.bin")
    dump_scene.dump_kinect(path, db.desc, db.xyz, db.model_of, db.n_models, img, K, CAM0, uv=fr.uv, desc=fr.desc,
                           distance=fill, patch_size=64, feature_density=FEATURE_DENSITY, match_density=MATCH_DENSITY,
                           fill_scale=0)
    s["steps"], s["extra"] = run_harness([path])
    return s


def test_the_wiring_is_config_hpp(scene_a):
    assert scene_a["extra"]["order"] == ["DEPTHFILTER", "MATCH_SIFT", "DEPTHFILTER2", "DEPTHPROP", "CLUSTER", "POSE", "FILTER",
                                         "POSE2", "FILTER2"]
    assert scene_a["extra"]["DEPTH_MAP_UPLOADS"] == "1"   # the map crossed PCIe once for the frame's four depth steps


def test_control_points_equal_the_oracles(scene_a):
    s, db = scene_a, scene_a["db"]
    got = s["extra"]["control"]
    assert sorted(got) == list(range(db.n_models))
    for m in range(db.n_models):
        lo, hi, n = db.xyz[db.model_of == m].min(0), db.xyz[db.model_of == m].max(0), int((db.model_of == m).sum())
        assert np.array_equal(_bits(got[m]), _bits(moped3d.adaptive_control_points(lo, hi, K, n))), m
        assert np.array_equal(_bits(got[m]), _bits(s["table"][m])), m


@pytest.mark.parametrize("step,key", [("MATCH_SIFT", "after_match"), ("DEPTHFILTER2", "after_f2")])
def test_match_lists_equal_the_oracles(scene_a, step, key):
    s = scene_a
    got = s["steps"][step]["matches"]
    want_q, want_m = s[key]
    print(step, len(got), "matches, oracle", len(want_q))
    assert [g[0] for g in got] == want_m.tolist() and [g[1] for g in got] == want_q.tolist()
    # coord3D = the nearest model point's
    assert np.array_equal(_bits([g[4:7] for g in got]), _bits(s["db"].xyz[s["idx"][want_q]]))


def test_depth_data_equals_the_oracles(scene_a):
    s = scene_a
    want_q, want_m = s["after_f2"]
    got = s["steps"]["DEPTHPROP"]["depth"]
    assert len(got) == len(want_q) > 0
    uv = s["fr"].uv[want_q]
    world, fd = orclib.depthmap_lookup(s["img"], s["fill"], uv)
    valid = s["img"][uv[:, 1].astype(int), uv[:, 0].astype(int), 3] >= 0
    assert [g[0] for g in got] == want_m.tolist()
    assert np.array_equal(np.array([g[2] for g in got]) != 0, valid)
    assert np.array_equal(_bits([g[3:6] for g in got]), _bits(world))
    assert np.array_equal(_bits([g[6] for g in got]), _bits(world[:, 2]))
    assert np.array_equal(_bits([g[7] for g in got]), _bits(fd))


def _oracle_clusters(s):
    want_q, want_m = s["after_f2"]
    out = {}
    for m in range(s["db"].n_models):
        qs = want_q[want_m == m]
        if len(qs) == 0:
            continue
        world, _ = orclib.depthmap_prop(s["img"], s["fill"], s["fr"].uv[qs], 0.1)
        for c, members in enumerate(orclib.cluster_linkage(s["fr"].uv[qs], s["db"].xyz[s["idx"][qs]], world, s["img"], s["fill"])):
            out[(m, c)] = members.tolist()
    return out


def test_clusters_equal_the_oracles(scene_a):
    want = _oracle_clusters(scene_a)
    got = scene_a["steps"]["CLUSTER"]["clusters"]
    print(len(got), "clusters, oracle", len(want))
    assert len(want) >= 2 and got == want


def test_objects_are_the_frames_and_within_the_pose_bars(scene_a):
    s, db, fr = scene_a, scene_a["db"], scene_a["fr"]
    got = s["steps"]["FILTER2"]["objs"]
    c = capi.Context(0)
    try:
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        c.reserve(len(fr.uv))
        c.frame_set_depth_image_host(s["img"], s["fill"])
        c.frame_set_depth_rules(K, 64, FEATURE_DENSITY, MATCH_DENSITY, s["table"])
        c.frame_set_cluster_linkage(capi.default_linkage_params())
        import torch
        dev = torch.device("cuda:0")
        qd, uv = torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev)
        c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), len(fr.uv), K, CAM0, moped3d_params(), 7)
        objs, _ = c.frame_fetch()
    finally:
        c.close()
    assert sorted(g[0] for g in got) == sorted(objs["model"].tolist()) == sorted(fr.visible.tolist())
    want_q, want_m = s["after_f2"]
    clusters = _oracle_clusters(s)
    for g in got:
        m, pose = g[0], np.array(g[4:8] + g[1:4], np.float32)   # (qx, qy, qz, qw, tx, ty, tz)
        qs_m = want_q[want_m == m]
        qs = qs_m[max((v for k, v in clusters.items() if k[0] == m), key=len)]
        uvm, xyz = fr.uv[qs], db.xyz[s["idx"][qs]]
        world, wgt = orclib.depthmap_prop(s["img"], s["fill"], uvm, 0.1)
        ok, op = orclib.ransac_depth(1, uvm, xyz, world, wgt, K, CAM0, 0.5, orclib.POSE1_3D, seed=3)
        assert ok
        _, oinl = orclib.test_all_points(op, uvm, xyz, K, CAM0, 8.0)

        def reproj(p):
            return float(np.sqrt(((orclib.project(p, xyz[oinl], K, CAM0) - uvm[oinl]) ** 2).sum(1)).mean())
        print("model", m, "reprojection", reproj(pose), "oracle", reproj(op))
        assert reproj(pose) <= reproj(op) + 1.0
        j = list(fr.visible).index(m)
        assert np.linalg.norm(pose[4:] - fr.poses[j][4:]) < 0.01


# ---- scene B -----------------------------------------------------------------------------------------------------------
def test_resident_step_equals_the_capi_composition(tmp_path):
    import torch
    from test_gpu_depthfill import holes
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))
    gray = np.ascontiguousarray(gold["gray0"])
    H, W, CAP = 480, 640, 1024
    c = capi.Context(0)
    try:
        xy, _, desc = c.sift(gray)
        z = np.float32(0.8)
        xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
        rng = np.random.default_rng(7)
        clutter = np.abs(rng.normal(size=(500, 128))).astype(np.float32)
        db_desc = np.concatenate([desc, clutter])
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
        filled, dist, _ = orclib.depth_fill(raw, K, 8, False)
        assert (zmap < 0).mean() > 0.05 and not np.array_equal(filled, raw)
        path, maps = str(tmp_path / "scene_b.bin"), str(tmp_path / "maps.bin")
        dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, K, CAM0, gray=gray, patch_size=64,
                               feature_density=0.8, match_density=0.01, fill_scale=8, max_keypoints=CAP)
        steps, extra = run_harness(["--resident", "--maps-out", maps, path])
        got = steps["DEPTHFILL"]
        # the step wiring on the same scene: FEAT on the gray image only (the frame's maps are Images too), the same object
        wired, _ = run_harness([path])
        assert wired["SIFT"]["features"] == len(xy) and wired["DEPTHFILL"]["features"] == 0
        assert [g[0] for g in wired["FILTER2"]["objs"]] == [g[0] for g in got["objs"]]
        # the same frame composed through capi: the plugin's first frame has seed 1 * 2654435761 + 0
        table = moped3d.ratio_table(db_xyz, model_of, 2, K)
        for m in range(2):
            assert np.array_equal(_bits(extra["control"][m]), _bits(table[m])), m
        c.db_upload(c.normalize(db_desc), model_of, db_xyz, 2)
        c.reserve(CAP)
        c.frame_set_depth_rules(K, 64, 0.8, 0.01, table)
        c.frame_set_cluster_linkage(capi.default_linkage_params())
        dev = torch.device("cuda:0")
        t_gray, t_map = torch.from_numpy(gray).to(dev), torch.from_numpy(raw).to(dev)
        t_fill = torch.zeros((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        c.depth_fill_dev(t_map.data_ptr(), W, H, K, t_fill.data_ptr(), 8, False)
        c.frame_set_depth_image(t_map.data_ptr(), t_fill.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        c.frame_enqueue_image(t_gray.data_ptr(), W, H, True, CAP, K, CAM0, moped3d_params(), 2654435761)
        objs, counts = c.frame_fetch()
        mq, mm = c.frame_fetch_matches()
        pts = c.frame_fetch_match_points()
    finally:
        c.close()
    print("counts", counts, "harness", extra["counts"])
    assert len(objs) >= 1 and counts[0] > 50
    assert extra["counts"] == counts.tolist()                                    # matches, clusters, objects x 2
    assert [g[0] for g in got["matches"]] == mm.tolist()
    want = np.stack([pts["u"], pts["v"], pts["x"], pts["y"], pts["z"]], 1)
    assert np.array_equal(_bits([g[2:7] for g in got["matches"]]), _bits(want))
    assert [g[0] for g in got["objs"]] == objs["model"].tolist()
    for g, o in zip(got["objs"], objs):
        assert np.array_equal(_bits(g[4:8] + g[1:4]), _bits(o["pose"]))
        assert np.array_equal(_bits([g[8]]), _bits([o["score"]]))
    # the filled map and its distance map handed back are the oracle's
    back = np.fromfile(maps, np.float32)
    assert back.size == H * W * 5
    assert np.array_equal(back[:H * W * 4].view(np.uint32), filled.reshape(-1).view(np.uint32))
    assert np.array_equal(back[H * W * 4:].view(np.uint32), dist.reshape(-1).view(np.uint32))
