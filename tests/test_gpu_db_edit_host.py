"""addModel / removeModel between frames through the step plugins (moped_amd/host/db_edit_step_test.cpp): with the
config key IncrementalModels set, MATCH_BRUTE_HIP::Update() edits the resident database; matches and objects are those
of the same run with the key at 0, and all models are uploaded exactly once."""
import os
import subprocess
import sys

import pytest

from moped_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")


@pytest.mark.gpu
def test_incremental_models_through_the_plugins(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dump_scene
    subprocess.check_call(["make", "-s", "-C", HOST, "db_edit_step_test"])
    db = synth.make_db(5, 1500, seed=0xAD0)
    fr = synth.make_frame(db, n_vis=5, seed=2, Q=1500, pts_per_obj=110)
    scene = str(tmp_path / "scene.bin")
    dump_scene.dump(scene, db, fr)
    outs = {}
    for key in ("0", "1"):
        out = subprocess.check_output([os.path.join(HOST, "db_edit_step_test"), scene, key], text=True, timeout=120)
        lines = out.splitlines()
        assert lines[-1].startswith("FULL_UPLOADS ")
        outs[key] = (lines[:-1], [int(w) for w in lines[-1].split()[1::2]])
    frames0, frames1 = outs["0"][0], outs["1"][0]
    assert frames0 == frames1                       # matches (counts, tag of every list entry) and objects, frame by frame
    assert outs["0"][1] == [0, 0]                   # key at 0: today's Update(), nothing counted
    assert outs["1"][1] == [1, 3]                   # one full upload, then a removal, a replace and an append
    heads = [l.split() for l in frames1 if l.startswith("FRAME ")]
    assert [int(h[3]) for h in heads] == [3, 2, 2, 3] and all(int(h[5]) > 100 for h in heads)
    seen = []
    for l in frames1:
        if l.startswith("FRAME "):
            seen.append([])
        elif l.startswith("OBJ "):
            seen[-1].append(l.split()[1])
    seen = [set(s) for s in seen]
    assert len(seen) == 4
    assert "model1" in seen[0] and seen[0] <= {"model0", "model1", "model2"}
    assert "model1" not in seen[1] and seen[1] <= {"model0", "model2"} and seen[1]   # the removed model's object is gone
    assert seen[2] <= {"model0", "model2"} and "model0" in seen[2]                  # "model2" now holds model 3's points
    assert "model4" in seen[3] and "model4" not in seen[2]                          # the appended model is found
