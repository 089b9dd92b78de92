"""createPlanarModelsFromImages_HIP through its harness (moped_amd/host/planar_model_test.cpp): a raw gray image becomes
`<name>.moped.xml`, the file is read back with mh_models_add_xml, and the same image run as a frame finds the model.
The file equals, as text, mh_models_write_xml of the rows the Python path (Context.db_splice_image) selected."""
import os
import subprocess

import numpy as np
import pytest

from moped_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sift_ref_frames.npz"))


def test_header_compiles_against_the_reference_types():
    """`make check_ref_planar`: against the reference's moped.hpp and sXML.hpp; skipped where that tree is absent (the
    Makefile says so); host code only."""
    out = subprocess.check_output(["make", "-s", "-C", HOST, "check_ref_planar"], text=True, stderr=subprocess.STDOUT, timeout=300)
    if "check_ref_planar: skipped" in out:
        pytest.skip("the reference tree is absent: nothing to compile against")
    assert "check_ref_planar: createPlanarModelsFromImages_HIP compiles" in out, out


@pytest.mark.gpu
def test_image_to_xml_to_frame(tmp_path):
    import torch
    subprocess.check_call(["make", "-s", "-C", HOST, "planar_model_test"])
    gray = np.ascontiguousarray(GOLD["gray0"])
    h, w = gray.shape
    raw = str(tmp_path / "frame0.gray")
    gray.tofile(raw)
    out = subprocess.check_output([os.path.join(HOST, "planar_model_test"), raw, str(w), str(h), "frame zero", str(tmp_path)],
                                  text=True, timeout=120)
    lines = out.splitlines()
    path = str(tmp_path / "frame zero.moped.xml")
    assert lines[1] == "FILE " + path

    # the rows of the Python path, printed by the model set
    c = capi.Context(0)
    try:
        g = torch.from_numpy(gray).to("cuda:0")
        torch.cuda.synchronize()
        scale = np.float32(0.8) / np.float32(800.0)
        n, bbox, desc, xyz = c.db_splice_image(capi.DB_INSERT, 0, g.data_ptr(), w, h, capi.make_planar_spec(scale=float(scale)),
                                               max_keypoints=4096, want_rows=True)
    finally:
        c.close()
    assert n > 300 and lines[0] == "MODEL frame zero ROWS %d" % n and lines[2] == "LOADED frame zero ROWS %d" % n
    s = capi.ModelSet()
    s.add_rows("frame zero", desc, xyz)
    mine = str(tmp_path / "python.moped.xml")
    s.write_xml(0, mine)
    assert open(path, "rb").read() == open(mine, "rb").read()

    # the frame: the model, where the two parametrisations of the plane put it (tests/test_gpu_planar_model.py, form 0)
    head = lines[3].split()
    assert head[:2] == ["FRAME", "KEYPOINTS"] and int(head[2]) == n and int(head[4]) > 50 and int(head[6]) >= 1
    objs = [l.split() for l in lines[4:] if l.startswith("OBJ ")]
    best = max(objs, key=lambda o: float(o[2]))
    pose = np.array([float(v) for v in best[4:11]])
    t = np.array([-320.0 * scale, -240.0 * scale, 0.8])
    assert int(best[1]) == 0 and np.abs(pose[4:7] - t).max() < 0.05 and abs(abs(pose[3]) - 1) < 0.01
