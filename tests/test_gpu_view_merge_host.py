"""createMergedModelFromKinectViews_HIP through its harness (moped_amd/host/kinect_model_test.cpp --merge --min-views 2):
the bundled frames 0 and 3 on the plane z = 0.8, identity poses.  The first view is inserted, the second merged
(mh_db_merge_view), then the rows only one view saw are dropped (mh_db_keep_rows).  The model is found in view 0's frame,
its row count is the number of rows with two views, and the rows of the returned SP_Model -- read back from the
.moped.xml the harness writes from them -- re-uploaded equal the store the harness left, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import view_model_ref as ref
from moped_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))


def test_merged_header_is_in_the_cxx98_check():
    """`make check98` compiles kinect_models_hip.hpp, createMergedModelFromKinectViews_HIP in it, under -std=gnu++98."""
    subprocess.check_call(["make", "-s", "-C", HOST, "check98"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    assert '#include "kinect_models_hip.hpp"' in open(os.path.join(HOST, "check98.cpp")).read()
    assert "createMergedModelFromKinectViews_HIP" in open(os.path.join(HOST, "kinect_models_hip.hpp")).read()


@pytest.mark.gpu
def test_two_views_merged_and_pruned_to_one_model_to_frame(tmp_path):
    import torch
    subprocess.check_call(["make", "-s", "-C", HOST, "kinect_model_test"])
    h, w = GOLD["gray0"].shape
    plane = ref.plane_map(0.8, w, h, tuple(synth.K_DEFAULT))
    args = []
    for k in ("gray0", "gray3"):
        np.ascontiguousarray(GOLD[k]).tofile(str(tmp_path / (k + ".gray")))
        plane.tofile(str(tmp_path / (k + ".depth")))
        args += [str(tmp_path / (k + ".gray")), str(tmp_path / (k + ".depth"))]
    out = subprocess.check_output([os.path.join(HOST, "kinect_model_test"), "--merge", "--min-views", "2", *args, str(w), str(h),
                                   "merged", str(tmp_path)], text=True, timeout=120)
    lines = out.splitlines()
    path = str(tmp_path / "merged.moped.xml")
    assert lines[2] == "FILE " + path

    # the Python path on a context of its own
    c = capi.Context(0)
    try:
        dev = torch.device("cuda:0")
        g = [torch.from_numpy(np.ascontiguousarray(GOLD[k])).to(dev) for k in ("gray0", "gray3")]
        m = torch.from_numpy(plane).to(dev)
        torch.cuda.synchronize()
        view = capi.make_view(m.data_ptr(), None, None, synth.K_DEFAULT)
        spec = capi.make_view_spec(merge_ratio=0.8, merge_dist=0.002)
        n0, _, _, d0, x0 = c.db_splice_view(capi.DB_INSERT, 0, g[0].data_ptr(), view, w, h, spec, max_keypoints=8192, want_rows=True)
        n1, nm, _, stats, views, midx, md, mx, d1, x1 = c.db_merge_view(0, g[1].data_ptr(), view, w, h, spec, max_keypoints=8192)
        two = views >= 2
        nk, bbox = c.db_keep_rows(0, two)
        store = {k: c.db_debug_fetch(k) for k in ("desc", "norm", "xyz", "model")}
        # the mirror: patched, appended, pruned
        d0[midx], x0[midx] = md, mx
        mirror_d, mirror_x = np.concatenate([d0, d1])[two], np.concatenate([x0, x1])[two]
    finally:
        c.close()
    assert n0 > 300 and nm > 100 and n1 > 50 and nk == nm == int(two.sum())
    head = lines[0].split(" BBOX ")
    assert head[0] == "MODEL merged INDEX 0 ROWS %d" % nm    # the rows with two views
    assert np.array_equal(np.array([float(v) for v in head[1].split()], np.float32), bbox)
    assert lines[1] == "VIEWS 0 %d" % nm
    assert lines[3] == "STORE ROWS %d MODELS 1" % nm
    for k, dt in (("desc", np.float32), ("xyz", np.float32), ("model", np.int32)):
        got = np.fromfile(str(tmp_path / ("store." + k)), dt)
        assert got.shape == store[k].shape and np.array_equal(got.view(np.uint8), store[k].view(np.uint8)), k
    # the SP_Model's rows, as the harness saved them, are the mirror's ...
    s = capi.ModelSet()
    s.add_rows("merged", mirror_d, mirror_x)
    mine = str(tmp_path / "python.moped.xml")
    s.write_xml(0, mine)
    assert open(path, "rb").read() == open(mine, "rb").read()
    # ... and re-uploaded they are the store
    f = capi.Context(0)
    try:
        mo = np.zeros(nm, np.int32)
        assert f.L.mh_db_upload_raw(f.h, capi._ptr(np.ascontiguousarray(mirror_d)), capi._ptr(mo),
                                    capi._ptr(np.ascontiguousarray(mirror_x)), nm, 1, 0, 1) == 0
        for k in ("desc", "norm", "xyz", "model"):
            assert np.array_equal(f.db_debug_fetch(k).view(np.uint8), store[k].view(np.uint8)), k
    finally:
        f.close()

    # the frame: model frame = camera frame of view 0
    fr = lines[4].split()
    assert fr[:2] == ["FRAME", "KEYPOINTS"] and int(fr[2]) == n0 and int(fr[4]) > 50 and int(fr[6]) >= 1
    objs = [l.split() for l in lines[5:] if l.startswith("OBJ ")]
    best = max(objs, key=lambda o: float(o[2]))
    pose = np.array([float(v) for v in best[4:11]])
    assert int(best[1]) == 0 and np.abs(pose[4:7]).max() < 0.05 and abs(abs(pose[3]) - 1) < 0.01
