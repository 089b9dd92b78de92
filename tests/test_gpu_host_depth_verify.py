"""DEPTH_VERIFY through the host plugins: moped_amd/host/moped3d_hip_test --depth-verify puts DEPTH_VERIFY_HIP behind FILTER2
in the eleven-step wiring and sets FRAME_RESIDENT_3D_HIP's DepthVerify / Verify... keys in the one-step wiring.  The scene
is tests/test_gpu_depth_verify_frame.py's (a planted object; map (a) confirms it, map (b) shows a surface three times as
far between the keypoints), the maps arrive filled (FillScale 0, a distance map of zeros).  In the step wiring the
objects the step leaves are those the restatement keeps on the lists and objects FILTER2 printed; in the one-step wiring
the objects are those of the same frame composed through the Python interface with the verification on, bit for bit.
And the two syntax checks of the plugin header build."""
import os
import subprocess

import numpy as np
import pytest

import depth_verify_ref as dvr
import test_gpu_depth_verify_frame as tf
import test_gpu_host_moped3d as hm
from moped_amd import capi, moped3d

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = hm.ROOT
K, CAM0, W, H, CAP = tf.K, tf.CAM0, tf.W, tf.H, tf.CAP
PRM = tf.PRM
VERIFY = ["--depth-verify"] + ["%.9g" % v for v in PRM]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    w = tf.World()
    try:
        d = tmp_path_factory.mktemp("depth_verify_host")
        paths = {}
        for n in "ab":
            paths[n] = str(d / ("scene_%s.bin" % n))
            hm.dump_scene.dump_kinect(paths[n], w.db[0], w.db[1], w.db[2], 2, w.maps[n], K, CAM0, gray=tf.kib.GOLD["gray0"],
                                      distance=w.fill, patch_size=64, feature_density=0.8, match_density=0.01, fill_scale=0,
                                      max_keypoints=CAP)
        yield dict(paths=paths, db=w.db, kp_off=w.kp_off, maps=dict(w.maps), fill=w.fill)
    finally:
        w.close()


def _objs(step):
    return [(g[0], np.array(g[4:8] + g[1:4], f32), g[8]) for g in step["objs"]]     # model, pose (q, t), score


def test_step_wiring_leaves_what_the_restatement_keeps(scenes):
    for n, kept in (("a", 1), ("b", 0)):
        plain, _ = hm.run_harness([scenes["paths"][n]])
        steps, extra = hm.run_harness(VERIFY + [scenes["paths"][n]])
        assert extra["order"][-2:] == ["FILTER2", "DEPTH_VERIFY"], extra["order"]
        before = _objs(steps["FILTER2"])
        assert [o[0] for o in before] == [0] and steps["FILTER2"]["objs"] == plain["FILTER2"]["objs"], n
        # the restatement on what FILTER2 left: its match lists (per model, list order) and its objects
        ms = steps["FILTER2"]["matches"]
        mm = np.array([g[0] for g in ms], np.int32)
        assert (np.diff(mm) >= 0).all()
        uv = np.array([g[2:4] for g in ms], f32).reshape(-1, 2)
        xyz = np.array([g[4:7] for g in ms], f32).reshape(-1, 3)
        model_off = np.concatenate([[0], np.cumsum(np.bincount(mm, minlength=2))]).astype(np.int32)
        want = dvr.depth_verify(uv, xyz, model_off, scenes["db"][1], scenes["kp_off"], [o[0] for o in before],
                                np.stack([o[1] for o in before]), K, CAM0, scenes["maps"][n], scenes["fill"], K, CAM0, PRM)
        print("map", n, "QS", float(want[0]["qs"]), "IS", float(want[0]["is"]))
        assert want["keep"].tolist() == [kept], (n, want)
        after = steps["DEPTH_VERIFY"]["objs"]
        assert after == [g for g, k in zip(steps["FILTER2"]["objs"], want["keep"]) if k], n
        assert steps["DEPTH_VERIFY"]["matches"] == ms             # (the step touches the objects only)


def test_one_step_wiring_equals_the_python_path(scenes):
    import torch
    db_desc, db_xyz, model_of = scenes["db"]
    table = moped3d.ratio_table(db_xyz, model_of, 2, K)
    dev = torch.device("cuda:0")
    t_gray = torch.from_numpy(np.ascontiguousarray(tf.kib.GOLD["gray0"])).to(dev)
    t_fill = torch.from_numpy(scenes["fill"]).to(dev)
    for n, kept in (("a", 1), ("b", 0)):
        plain, _ = hm.run_harness(["--resident", scenes["paths"][n]])
        got, extra = hm.run_harness(["--resident"] + VERIFY + [scenes["paths"][n]])
        assert len(plain["DEPTHFILL"]["objs"]) == 1 and len(got["DEPTHFILL"]["objs"]) == kept, n
        c = capi.Context(0)
        try:
            c.db_upload(c.normalize(db_desc), model_of, db_xyz, 2)
            c.reserve(CAP)
            c.frame_set_depth_rules(K, 64, 0.8, 0.01, table)
            c.frame_set_cluster_linkage(capi.default_linkage_params())
            t_map = torch.from_numpy(scenes["maps"][n]).to(dev)
            torch.cuda.synchronize()
            c.frame_set_depth_image(t_map.data_ptr(), t_fill.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
            c.frame_set_depth_verify(PRM, K, CAM0)
            c.frame_enqueue_image(t_gray.data_ptr(), W, H, True, CAP, K, CAM0, hm.moped3d_params(), 2654435761)
            objs, counts = c.frame_fetch()
            rec = c.frame_fetch_verify(0)
        finally:
            c.close()
        assert extra["counts"] == counts.tolist() and len(rec) == 1 and rec["keep"].tolist() == [kept], (n, counts, rec)
        assert [g[0] for g in got["DEPTHFILL"]["objs"]] == objs["model"].tolist()
        for g, o in zip(_objs(got["DEPTHFILL"]), objs):
            assert np.array_equal(hm._bits(g[1]), hm._bits(o["pose"])) and np.array_equal(hm._bits([g[2]]), hm._bits([o["score"]]))


def test_plugin_header_checks_build():
    host = os.path.join(ROOT, "moped_amd", "host")
    for stamp in ("check98_depth_verify",):
        if os.path.exists(os.path.join(host, stamp)):
            os.remove(os.path.join(host, stamp))
    r = subprocess.run(["make", "-C", host, "check98_depth_verify", "check_ref_depth_verify"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "check_ref_depth_verify:" in r.stdout and os.path.exists(os.path.join(host, "check98_depth_verify"))
