"""moped3d's STEP plugins and their harness, the parts that need no device: the headers stay -std=gnu++98 clean and compile
against the reference's own moped.hpp where that tree is present, the harness builds, the three new exports of the
library resolve through capi, the harness reads dump_kinect's scene files, and the oracle alone meets the window the
depth-step tests (test_gpu_depth_steps.py) rely on."""
import os
import subprocess
import sys

import numpy as np

import depth_step_cases as dc
import orclib
from moped_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import dump_scene  # noqa: E402


def test_plugin_headers_and_harness_build():
    r = subprocess.run(["make", "-s", "-C", HOST, "check98", "check_ref", "moped3d_hip_test"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(os.path.join(HOST, "moped3d_hip_test"))
    for name in ("check98_depth.cpp", "check_ref_depth.cpp"):
        text = open(os.path.join(HOST, name)).read()
        for header in ("DEPTHFILTER_HIP.hpp", "DEPTHMAP_PROP_HIP.hpp", "FRAME_RESIDENT_3D_HIP.hpp"):
            assert header in text, (name, header)


def test_new_exports_resolve():
    lib = capi.load()
    for name in ("mh_depth_filter", "mh_depth_prop", "mh_frame_run_kinect_host"):
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert capi.DEPTH_INFO_DTYPE.itemsize == 24   # sizeof(mh_depth_info)


def test_harness_refuses_what_is_not_a_scene(tmp_path):
    """Scene files are read before any step is made: a truncated one ends with status 2, with or without a device."""
    db = synth.make_db(2, 40)
    fr = synth.make_frame(db, n_vis=1, seed=1, Q=60, pts_per_obj=20)
    img, fill = synth.depth_image(db, fr, seed=1)
    path = str(tmp_path / "scene.bin")
    dump_scene.dump_kinect(path, db.desc, db.xyz, db.model_of, db.n_models, img, uv=fr.uv, desc=fr.desc, distance=fill)
    want = 36 + 8 + 44 + sum(4 + int((db.model_of == m).sum()) * 131 * 4 for m in range(2)) + 60 * 130 * 4 + 640 * 480 * 5 * 4
    assert os.path.getsize(path) == want
    data = open(path, "rb").read()
    short = str(tmp_path / "short.bin")
    open(short, "wb").write(data[:len(data) // 2])
    subprocess.run(["make", "-s", "-C", HOST, "moped3d_hip_test"], check=True, timeout=600)
    r = subprocess.run([os.path.join(HOST, "moped3d_hip_test"), short], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "not a scene file" in r.stderr
    r = subprocess.run([os.path.join(HOST, "moped3d_hip_test"), "--loop"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_the_oracle_alone_meets_the_depth_steps_window():
    img, fill = dc.depth_map()
    uv = dc.points()
    one, three = dc.oracle_window(orclib, img, uv)      # asserts 20 % .. 95 % kept in every non-empty group
    assert not np.array_equal(one, three)               # counting per group is another filter than counting all
    assert (~dc.inside(uv)).sum() >= 6 and np.isnan(img[..., 2]).any() and (img[..., 2] > 4).any() and (img[..., 3] < 0).any()
    assert np.diff(dc.GROUP_OFF).tolist() == [380, 0, 220]
    # points on the last row, the last column, and in the half patch row at the bottom
    assert (uv[:, 1].astype(int) == dc.H - 1).any() and (uv[:, 0].astype(int) == dc.W - 1).any() and dc.H % dc.PATCH != 0
