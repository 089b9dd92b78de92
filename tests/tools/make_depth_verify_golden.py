"""Makes tests/golden/depth_verify_ref.npz: objects, matches, models and Kinect maps, and what the reference's own
DEPTH_VERIFY_CPU (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp) prints and keeps for them.

    python tests/tools/make_depth_verify_golden.py [<reference tree>]   (default: $MOPED_REFERENCE or /root/reference)

Builds tests/tools/depth_verify_golden_harness.cpp against the reference headers where they lie, in a temporary directory,
runs it on the cases below and parses what the class wrote to std::cerr (precision 9: decimals that parse back to the same
float32): per object raw QS and IS, the multiplier before the cap, both counts, the adjusted scores; and which objects it
left in the list.  Needed only to remake the golden; no test runs it.

The reference reads outside the map for a keypoint that projects off it, so the maker asserts with the restatement
(tests/depth_verify_ref.py) that EVERY keypoint of every recorded object lands on the map; off-map behaviour rests on the
restatement alone.  It also asserts the coverage listed in main().

Three model sets (0 .. 1 025 keypoints a model), one true pose and three maps each (the surface agrees, refutes, mixed);
the cases walk the maps with several parameter sets.  Coordinates are multiples of 2^-16, depths of 2^-14, so that the
file stays small."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import depth_verify_ref as dvr   # noqa: E402

f32 = np.float32
SETS = ([0, 1, 63, 64, 65], [191, 192, 193, 300], [1025, 40])
MATCHES = ([0, 1, 64, 65, 130], [63, 0, 300, 64], [130, 65])
MODES = ("agree", "refute", "mixed")
KINDS = ("truth", "near", "front", "behind")
# (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction)
PARAMS = ((4096.0, 3.0, 2.0, 0.1), (64.0, 1.0625, 1.0, 0.25), (4.0, 10.0, 0.0, 0.5), (4096.0, 1.5, -1.0, 0.1),
          (0.0, 3.0, 2.0, 0.25), (4096.0, 1.125, 6.0, 0.1))


def cases():
    rng = np.random.default_rng(0xDE97)
    sets, maps, out = [], [], []
    for s, sizes in enumerate(SETS):
        kp, kp_off = dvr.make_models(rng, sizes, spread=(0.16, 0.11))
        truth = dvr.make_truth(rng)
        sets.append(dict(kp_xyz=kp, kp_off=kp_off, truth=truth))
        for mode in MODES:
            depth_img, fill_img = dvr.make_map(rng, truth, mode)
            maps.append([depth_img, fill_img])
            mp = len(maps) - 1
            for k, prm in enumerate(PARAMS):
                rows = [m for m, n in enumerate(sizes) if n > 0]
                obj_model = np.concatenate([rng.permutation(len(sizes)), rng.choice(rows, 2)])[:int(rng.integers(3, 8))]
                kinds = rng.choice(KINDS, len(obj_model), p=[0.4, 0.3, 0.15, 0.15])
                c = dvr.make_verify_case(rng, kp, kp_off, match_sizes=MATCHES[s], kinds=kinds, params=prm, truth=truth,
                                         obj_model=obj_model, maps=maps[mp])
                c["set"], c["map"] = s, mp
                out.append(c)
        # the agreeing map of the set: one pixel gets exactly the putative depth of a keypoint under the true pose
        first = next(c for c in out if c["set"] == s)
        m = max(range(len(sizes)), key=lambda i: sizes[i])
        probe = dict(first, obj_model=np.array([m], np.int32), obj_pose=truth[None].copy())
        assert dvr.plant_equal_depth(probe) is not None
    for c in out:                                     # (an object exactly on the true pose of the planted model)
        if c["params"] == PARAMS[0]:
            m = max(range(len(SETS[c["set"]])), key=lambda i: SETS[c["set"]][i])
            c["obj_model"] = np.concatenate([c["obj_model"], [m]]).astype(np.int32)
            c["obj_pose"] = np.concatenate([c["obj_pose"], sets[c["set"]]["truth"][None]]).astype(f32)
    return sets, maps, out


def run(exe, cs, tmp):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.txt")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cs)).tobytes())
        for c in cs:
            h, w = c["depth_img"].shape[:2]
            for a, t in ((c["params"], f32), (c["K"], f32), (c["cam"], f32), (c["depth_K"], f32), (c["depth_cam"], f32),
                         ([w, h], np.int32), (c["depth_img"], f32), (c["fill_img"], f32), ([len(c["kp_off"]) - 1], np.int32),
                         (c["kp_off"], np.int32), (c["kp_xyz"], f32), (c["model_off"], np.int32),
                         (np.concatenate([c["uv"], c["xyz"]], 1), f32), ([len(c["obj_model"])], np.int32),
                         (c["obj_model"], np.int32), (c["obj_pose"], f32)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    subprocess.check_call([exe, fin, fout])
    num = r"([-+]?(?:nan|inf|[0-9.]+(?:e[-+]?[0-9]+)?))"
    pat = re.compile(r"Examining object; QS = %s; IS = %s\nXPlier: %s; Max = %s\nPlausible Matches: (-?\d+); Used Keypoints: (-?\d+)\n"
                     r"Adjusted QS = %s; IS = %s\n" % ((num,) * 6))
    text = open(fout).read()
    want = []
    blocks = re.split(r"^CASE \d+ \d+\n", text, flags=re.M)[1:]
    assert len(blocks) == len(cs)
    for c, b in zip(cs, blocks):
        body, kept = b.rsplit("KEPT", 1)
        kept = [int(v) for v in kept.split()]
        objs = pat.findall(body)
        assert len(objs) == len(kept) == len(c["obj_model"]) and pat.sub("", body) == "", body
        r = np.zeros(len(objs), dvr.RECORD)
        for o, g in enumerate(objs):
            r[o]["qs_raw"], r[o]["is_raw"], r[o]["multiplier_raw"] = f32(g[0]), f32(g[1]), f32(g[2])
            assert f32(g[3]) == f32(c["params"][1])
            r[o]["plausible"], r[o]["used"] = int(g[4]), int(g[5])
            r[o]["qs"], r[o]["is"] = f32(g[6]), f32(g[7])
            r[o]["keep"] = kept[o]
        want.append(r)
    return want


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOPED_REFERENCE", "/root/reference")
    lib = os.path.join(ref, "moped3d", "libmoped")
    sets, maps, cs = cases()
    # every keypoint of every recorded object on the map (the restatement says so), and the coverage
    cov = dict(at_max=0, above_max=0, nan_depth=0, equal_depth=0)
    for c in cs:
        detail = []
        c["rest"] = dvr.run_ref(c, detail=detail)
        md = f32(c["params"][2])
        for out, _, _, pix, dist, putative in detail:
            assert (pix >= 0).all(), "a keypoint off the map"
            kin = c["depth_img"][pix[:, 1], pix[:, 0], 2]
            cov["at_max"] += int(((out >= 2) & (dist == md) & (md > 0)).sum())
            cov["above_max"] += int(((out == 1) & (dist == np.nextafter(md, f32(np.inf)))).sum())
            cov["nan_depth"] += int(((out == 3) & np.isnan(kin)).sum())
            cov["equal_depth"] += int(((out == 3) & (kin == putative)).sum())
    assert all(v > 0 for v in cov.values()), cov
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "harness")
        subprocess.check_call(["g++", "-O2", "-w", "-std=gnu++98", "-fno-delete-null-pointer-checks",
                               "-I", os.path.join(lib, "include"), "-I", os.path.join(lib, "src", "depthVerify"),
                               os.path.join(HERE, "depth_verify_golden_harness.cpp"), "-o", exe])
        want = run(exe, cs, tmp)
    w = np.concatenate(want)
    r = np.concatenate([c["rest"] for c in cs])
    share = w["keep"].mean()
    assert 0.2 <= share <= 0.8, share                                               # each verdict at least 20 %
    max_of = np.concatenate([np.full(len(c["obj_model"]), c["params"][1], f32) for c in cs])
    assert (w["multiplier_raw"] > max_of).any() and (w["multiplier_raw"] < max_of).any()   # capped and not
    assert (w["used"] == 0).any() and (w["plausible"] == 0).any()
    assert any(c["model_off"][m + 1] == c["model_off"][m] for c in cs for m in c["obj_model"])   # a model without matches
    assert np.isnan(w["is_raw"]).any()
    same = sum(int(np.array_equal(np.nan_to_num(w[k], nan=-7.0), np.nan_to_num(r[k], nan=-7.0)))
               for k in ("qs_raw", "is_raw", "multiplier_raw", "qs", "is", "plausible", "used", "keep"))
    print(f"the restatement agrees on {same} of 8 words")
    set_kp = np.concatenate([[0], np.cumsum([len(s["kp_xyz"]) for s in sets])]).astype(np.int32)
    set_off = np.concatenate([[0], np.cumsum([len(s["kp_off"]) for s in sets])]).astype(np.int32)
    case_moff = np.concatenate([[0], np.cumsum([len(c["model_off"]) for c in cs])]).astype(np.int32)
    case_match = np.concatenate([[0], np.cumsum([len(c["uv"]) for c in cs])]).astype(np.int32)
    case_obj = np.concatenate([[0], np.cumsum([len(c["obj_model"]) for c in cs])]).astype(np.int32)
    path = os.path.join(ROOT, "tests", "golden", "depth_verify_ref.npz")
    np.savez_compressed(
        path, K=cs[0]["K"], cam=cs[0]["cam"], depth_K=cs[0]["depth_K"], depth_cam=cs[0]["depth_cam"],
        kp_xyz_all=np.concatenate([s["kp_xyz"] for s in sets]), kp_off_all=np.concatenate([s["kp_off"] for s in sets]),
        set_kp=set_kp, set_off=set_off, depth_all=np.stack([m[0] for m in maps]), fill_all=np.stack([m[1] for m in maps]),
        case_set=np.array([c["set"] for c in cs], np.int32), case_map=np.array([c["map"] for c in cs], np.int32),
        params=np.array([c["params"] for c in cs], f32), model_off_all=np.concatenate([c["model_off"] for c in cs]),
        case_moff=case_moff[:-1], case_match=case_match[:-1],
        match_all=np.concatenate([np.concatenate([c["uv"], c["xyz"]], 1) for c in cs]).astype(f32), case_obj=case_obj,
        obj_model_all=np.concatenate([c["obj_model"] for c in cs]).astype(np.int32),
        obj_pose_all=np.concatenate([c["obj_pose"] for c in cs]).astype(f32), want=w)
    print(f"{path}: {len(cs)} cases, {len(w)} objects ({int(w['keep'].sum())} kept), {os.path.getsize(path)} bytes; coverage {cov}")


if __name__ == "__main__":
    main()
