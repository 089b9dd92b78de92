"""createModelFromKinectViews_HIP through its harness (moped_amd/host/kinect_model_test.cpp): two views (the bundled
frames 0 and 3 on the plane z = 0.8, identity poses) become one model of an empty store -- the first view inserted, the
second appended without the keypoints the model holds already.  The store the harness leaves equals the Python path's
(Context.db_splice_view + db_append_view) byte for byte, its .moped.xml equals mh_models_write_xml of the Python path's
rows, and view 0 run as a frame finds the model where it was taught."""
import os
import subprocess

import numpy as np
import pytest

import view_model_ref as ref
from moped_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))


def test_header_is_cxx98_clean():
    """`make check98` compiles the step headers, kinect_models_hip.hpp among them, under -std=gnu++98; host code only."""
    subprocess.check_call(["make", "-s", "-C", HOST, "check98"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    assert '#include "kinect_models_hip.hpp"' in open(os.path.join(HOST, "check98.cpp")).read()


@pytest.mark.gpu
def test_two_views_to_one_model_to_frame(tmp_path):
    import torch
    subprocess.check_call(["make", "-s", "-C", HOST, "kinect_model_test"])
    h, w = GOLD["gray0"].shape
    plane = ref.plane_map(0.8, w, h, tuple(synth.K_DEFAULT))
    args = []
    for k in ("gray0", "gray3"):
        np.ascontiguousarray(GOLD[k]).tofile(str(tmp_path / (k + ".gray")))
        plane.tofile(str(tmp_path / (k + ".depth")))
        args += [str(tmp_path / (k + ".gray")), str(tmp_path / (k + ".depth"))]
    out = subprocess.check_output([os.path.join(HOST, "kinect_model_test"), *args, str(w), str(h), "two views", str(tmp_path)],
                                  text=True, timeout=120)
    lines = out.splitlines()
    path = str(tmp_path / "two views.moped.xml")
    assert lines[1] == "FILE " + path

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
        n1, bbox, stats, d1, x1 = c.db_append_view(0, g[1].data_ptr(), view, w, h, spec, max_keypoints=8192, want_rows=True)
        store = {k: c.db_debug_fetch(k) for k in ("desc", "xyz", "model")}
    finally:
        c.close()
    assert n0 > 300 and n1 > 50 and stats[ref.DUP] > 100
    head = lines[0].split(" BBOX ")
    assert head[0] == "MODEL two views INDEX 0 ROWS %d" % (n0 + n1)
    assert np.array_equal(np.array([float(v) for v in head[1].split()], np.float32), bbox)
    assert lines[2] == "STORE ROWS %d MODELS 1" % (n0 + n1)
    for k, dt in (("desc", np.float32), ("xyz", np.float32), ("model", np.int32)):
        got = np.fromfile(str(tmp_path / ("store." + k)), dt)
        assert got.shape == store[k].shape and np.array_equal(got.view(np.uint8), store[k].view(np.uint8)), k
    s = capi.ModelSet()
    s.add_rows("two views", np.concatenate([d0, d1]), np.concatenate([x0, x1]))
    mine = str(tmp_path / "python.moped.xml")
    s.write_xml(0, mine)
    assert open(path, "rb").read() == open(mine, "rb").read()

    # the frame: model frame = camera frame of view 0
    fr = lines[3].split()
    assert fr[:2] == ["FRAME", "KEYPOINTS"] and int(fr[2]) == n0 and int(fr[4]) > 50 and int(fr[6]) >= 1
    objs = [l.split() for l in lines[4:] if l.startswith("OBJ ")]
    best = max(objs, key=lambda o: float(o[2]))
    pose = np.array([float(v) for v in best[4:11]])
    assert int(best[1]) == 0 and np.abs(pose[4:7]).max() < 0.05 and abs(abs(pose[3]) - 1) < 0.01
