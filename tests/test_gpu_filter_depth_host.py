"""The STEP plugin FILTER_PROJECTION_DEPTH_HIP (moped_amd/host) through its stand-alone driver filter_depth_step_test: a
FrameData with matches, objects, a depth map and its ".distance" map goes through the step; the objects left in the frame,
their scores and the rewritten frameData.clusters must be what mh_filter_depth gives when it is called directly with
the points the step has to choose -- all keypoints of a model over its descriptor types in map order when there are at
most TestSampleSize, else the reference's randSample on rand() (FILTER_PROJECTION_DEPTH_CPU.hpp:78-116), replayed here
through the C library's srand / rand."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import filter_depth_ref as fdr
from moped_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moped_amd", "host")
f32 = np.float32


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", HOST, "filter_depth_step_test"])
    return os.path.join(HOST, "filter_depth_step_test")


def _write(path, c, sample_size, seed, with_distance=True, with_depth=True):
    h, w = c["depth_img"].shape[:2]
    n_models = len(c["model_off"]) - 1
    with open(path, "wb") as f:
        f.write(np.array([w, h, n_models, len(c["obj_model"]), sample_size, c["min_points"], seed, int(with_distance),
                          int(with_depth)], np.int32).tobytes())
        f.write(np.concatenate([c["K"], c["cam"], c["depth_K"], c["depth_cam"],
                                [c["fd"], c["psd"], c["min_score"], c["depth_fraction"], c["min_kp_fraction"]]]).astype(f32).tobytes())
        for m in range(n_models):
            kp = c["kp_xyz"][c["kp_off"][m]:c["kp_off"][m + 1]]
            f.write(np.int32(len(kp)).tobytes() + kp.astype(f32).tobytes())
            lo, hi = c["model_off"][m], c["model_off"][m + 1]
            f.write(np.int32(hi - lo).tobytes() + np.concatenate([c["uv"][lo:hi], c["xyz"][lo:hi]], 1).astype(f32).tobytes())
        f.write(c["obj_model"].astype(np.int32).tobytes() + c["obj_pose"].astype(f32).tobytes())
        if with_depth:
            f.write(c["depth_img"].astype(f32).tobytes())
            if with_distance:
                f.write(c["fill_img"].astype(f32).tobytes())


def _blocks(out):
    """The driver's output -> {(frame, slot): (capable, objects, clusters)} ((0, 0) alone without STEP lines)."""
    blocks, key = {}, (0, 0)
    for line in out.splitlines():
        t = line.split()
        if t[0] == "STEP":
            key = (int(t[1]), int(t[2]))
        elif t[0] == "CAPABLE":
            blocks[key] = [int(t[1]), [], {}]
        elif t[0] == "OBJ":
            blocks[key][1].append((int(t[1]), int(t[2], 16)))
        elif t[0] == "CLUSTER":
            blocks[key][2].setdefault(int(t[1]), []).append([int(x) for x in t[3:]])
    return blocks


def _run(driver, path, second=None):
    argv = [driver, path] + ([str(second)] if second else [])
    out = subprocess.run(argv, capture_output=True, text=True, timeout=120, check=True).stdout
    blocks = _blocks(out)
    return blocks if second else tuple(blocks[(0, 0)])


def _rand_sample(seed, counts, sample_size, more=()):
    """selectTestPoints (:94-116) with the C library's generator: model after model, randSample (:78-92) only for a
    model with more than sample_size keypoints: indices sorted by ((Float) rand(), index).  more: the sample sizes of
    further instances of the driver's two-instance mode, instance k seeded with seed + k -> a list of selections then."""
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    out = []
    for k, size in enumerate((sample_size,) + tuple(more)):
        libc.srand(ctypes.c_uint(seed + k))
        chosen = []
        for n in counts:
            if n > size:
                keys = sorted((float(f32(libc.rand())), i) for i in range(n))
                chosen.append([i for _, i in keys[:size]])
            else:
                chosen.append(list(range(n)))
        out.append(chosen)
    return out if more else out[0]


def _case(rng, kp_counts):
    """A generated case whose models carry kp_counts keypoints (make_depth_case's points are the keypoints)."""
    while True:
        c = fdr.make_depth_case(rng, n_obj=int(rng.integers(3, 9)))
        if len(c["model_off"]) - 1 == len(kp_counts) and c["fill_img"] is not None:
            break
    counts = np.array(kp_counts)
    c["kp_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    c["kp_xyz"] = np.concatenate([rng.uniform(-0.55, 0.55, (int(counts.sum()), 2)), rng.uniform(-0.001, 0.001, (int(counts.sum()), 1))], 1).astype(f32)
    c["min_kp_fraction"] = 0.1
    return c


def _direct(ctx, c, chosen, with_distance=True):
    pts = [c["kp_xyz"][c["kp_off"][m]:c["kp_off"][m + 1]][idx] for m, idx in enumerate(chosen)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
    ctx.frame_set_depth_image_host(c["depth_img"], c["fill_img"] if with_distance else None)
    ctx.filter_depth_set_points(np.concatenate(pts) if off[-1] else np.zeros((0, 3), f32), off)
    return ctx.filter_depth(capi.pack_corr(c["uv"], c["xyz"]), c["model_off"], c["obj_model"], c["obj_pose"], c["K"], c["cam"],
                            c["min_points"], c["fd"], c["min_score"], c["depth_K"], c["depth_cam"],
                            (c["psd"], c["depth_fraction"], c["min_kp_fraction"]))


def _check(got, want, c, index=None, tag=None):
    """index: the input-list indices of the objects `want` was computed for (None: all of them)."""
    capable, objs, clusters = got
    score, keep, order, members = want[:4]
    index = np.arange(len(keep)) if index is None else np.asarray(index)
    assert capable == 1, tag
    assert [o for o, _ in objs] == [int(o) for o in index[np.nonzero(keep)[0]]], tag   # the objects left, in list order
    where = {int(o): k for k, o in enumerate(index)}
    for o, bits in objs:
        if not np.isnan(score[where[o]]):
            assert bits == int(f32(score[where[o]]).view(np.uint32)), (tag, o)
    want_cl = {}
    for o, mem in zip(order, members):
        want_cl.setdefault(int(c["obj_model"][index[o]]), []).append([int(i) for i in mem])
    assert clusters == want_cl, tag


@pytest.mark.parametrize("sample_size,kp_counts", [(300, (40, 130, 7)), (64, (200, 64, 65)), (20, (90, 0, 33, 150))])
def test_step_equals_mh_filter_depth_with_the_points_it_must_choose(driver, ctx, tmp_path, sample_size, kp_counts):
    rng = np.random.default_rng([0x4057, sample_size])
    kept = 0
    for trial in range(3):
        c = _case(rng, kp_counts)
        if trial == 2:                                   # every object stays: all their scores are compared
            c["min_points"], c["min_score"] = 0, -1e30
        seed = 1000 + trial
        path = str(tmp_path / f"case{trial}.bin")
        _write(path, c, sample_size, seed)
        chosen = _rand_sample(seed, kp_counts, sample_size)
        assert any(len(ch) == sample_size for ch in chosen) == any(n > sample_size for n in kp_counts)
        want = _direct(ctx, c, chosen)
        _check(_run(driver, path), want, c)
        kept += int(want[1].sum())
        if trial == 0:                                   # without the ".distance" map: every pixel measured
            _write(path, c, sample_size, seed, with_distance=False)
            _check(_run(driver, path), _direct(ctx, c, chosen, with_distance=False), c)
    assert kept >= 1


def test_two_instances_keep_their_own_points_over_two_frames(driver, ctx, tmp_path):
    """FILTER and FILTER2 both the depth class, with different TestSampleSize, share the session's device context: in
    both frames each must run on the sample IT drew, FILTER2 on the
    objects FILTER left."""
    kp_counts, size1, size2 = (200, 90, 150), 64, 20
    rng = np.random.default_rng(0x2172)
    differ = 0
    for trial in range(3):
        c = _case(rng, kp_counts)
        c["min_points"], c["min_score"] = 0, (-1e30 if trial == 0 else c["min_score"])
        seed = 77 + trial
        path = str(tmp_path / f"two{trial}.bin")
        _write(path, c, size1, seed)
        ch1, ch2 = _rand_sample(seed, kp_counts, size1, more=(size2,))
        assert ch1 != ch2
        want1 = _direct(ctx, c, ch1)
        left = np.nonzero(want1[1])[0]
        sub = dict(c, obj_model=c["obj_model"][left], obj_pose=c["obj_pose"][left])
        want2 = _direct(ctx, sub, ch2)
        # (the case bites: on FILTER2's points FILTER would have scored otherwise)
        other = _direct(ctx, c, ch2)
        differ += not np.array_equal(np.nan_to_num(other[0]).view(np.uint32), np.nan_to_num(want1[0]).view(np.uint32))
        blocks = _run(driver, path, second=size2)
        assert sorted(blocks) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for frame in (0, 1):
            _check(blocks[(frame, 0)], want1, c, tag=(trial, frame, "FILTER"))
            _check(blocks[(frame, 1)], want2, c, index=left, tag=(trial, frame, "FILTER2"))
    assert differ >= 1


def test_frame_without_a_depth_map_is_left_alone(driver, tmp_path):
    c = _case(np.random.default_rng(5), (10, 10))
    path = str(tmp_path / "nodepth.bin")
    _write(path, c, 300, 1, with_depth=False)
    capable, objs, clusters = _run(driver, path)
    assert capable == 0 and [o for o, _ in objs] == list(range(len(c["obj_model"])))
