"""moped_amd/host/object_hulls_test: getObjectHulls_HIP (object_hulls_hip.hpp) for a libmoped tree, through the C ABI.
The program runs once on a small scene; its OBJHULL lines (MopedBench's format) must name the Python path's hulls."""
import os
import subprocess

import numpy as np
import pytest

import hull_ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moped_amd", "host")
K = np.array([525.0, 525.0, 320.0, 240.0], np.float32)
CAM = synth.camera_pose(0.05, (0.01, -0.02, 0.0)).astype(np.float32)


def _num(v):
    return "%.9g" % float(v)


def test_host_program_prints_the_hulls_of_the_python_path(tmp_path):
    rng = np.random.default_rng(0x40575)
    models = [(rng.uniform(-0.5, 0.5, (n, 3)) * [0.3, 0.2, 0.1]).astype(np.float32) for n in (40, 700, 3)]
    a = np.sort(rng.uniform(0, 2 * np.pi, 40))
    models.append(np.stack([0.1 * np.cos(a), 0.1 * np.sin(a), np.zeros(40)], 1).astype(np.float32))   # a ring: every point a vertex
    objects = [(0, None), (1, None), (1, None), (2, None), (3, None)]
    objects = [(m, np.concatenate([synth.random_quat(rng), [rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)]]).astype(np.float32))
               for m, _ in objects]
    scene = tmp_path / "scene.txt"
    with open(scene, "w") as f:
        f.write("K " + " ".join(_num(v) for v in K) + "\nCAM " + " ".join(_num(v) for v in CAM) + "\n")
        for i, xyz in enumerate(models):
            f.write(f"MODEL model{i} {len(xyz)}\n" + "\n".join(" ".join(_num(v) for v in row) for row in xyz) + "\n")
        for m, pose in objects:
            f.write(f"OBJECT {m} " + " ".join(_num(v) for v in pose) + "\n")
    exe = os.path.join(HOST, "object_hulls_test")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", HOST, "object_hulls_test"])
    out = subprocess.run([exe, str(scene), "9"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ":OBJHULL:" in ln]
    assert len(lines) == len(objects)

    c = capi.Context(0)
    try:
        xyz = np.concatenate(models)
        model_of = np.concatenate([np.full(len(v), i, np.int32) for i, v in enumerate(models)])
        desc = synth.l2_normalize(rng.normal(size=(len(xyz), 128)).astype(np.float32))
        c.db_upload(desc, model_of, xyz, len(models))
        hulls, nv, nb, bb = c.object_hulls([m for m, _ in objects], [p for _, p in objects], K, CAM, 128)
    finally:
        c.close()
    assert max(nv) > 16      # (the program starts with room for 16 vertices: its second round is covered)
    for line, (m, pose), hull in zip(lines, objects, hulls):
        want = f"HULLS:OBJHULL:model{m}" + "".join(f":{_num(x)};{_num(y)}" for x, y in hull)
        assert line == want
        assert hull_ref.same_vertices(hull, hull_ref.object_hull(pose, models[m], K, CAM)[0])
