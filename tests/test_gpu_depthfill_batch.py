"""DEPTHFILL of a batch (mh_depth_fill_batch): the maps of B frames through one launch per stage -- one workgroup per
frame replays that frame's FIFO wavefront, the upsampling takes the frame from blockIdx.y.  Every frame's filled map
and distance map must be BIT for bit the oracle's restatement of DEPTH_FILL_EXACT_CPU
(moped3d/libmoped/src/depthfill/DEPTH_FILL_EXACT_CPU.hpp) on that map alone, whatever its neighbours in the batch are
and whatever an earlier batch left in the frame's slice of the context's scratch."""
import re

import numpy as np
import pytest

import orclib
from moped_amd import capi
from test_gpu_depthfill import K, holes

pytestmark = pytest.mark.gpu
KINDS = ["blobs", "none", "all", "one_valid", "nan", "dense", "grid", "sparse"]   # neighbours differ as much as maps can


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def vga():
    """The eight kinds at 640 x 480 and what the oracle makes of them at factor 8: {(kind, bilinear): (map, dist)}."""
    maps = {k: holes(k, 480, 640, np.random.default_rng(100 + i)) for i, k in enumerate(KINDS)}
    want = {(k, b): orclib.depth_fill(maps[k], K, 8, b)[:2] for k in KINDS for b in (False, True)}
    return maps, want


def run_batch(c, torch_dev, maps, w, h, scale, bilinear):
    """-> ([filled map], [distance map]) of the batch, the distance maps pre-set to a pattern the call must overwrite."""
    torch, dev = torch_dev
    t_d = [torch.from_numpy(m).to(dev) for m in maps]
    t_f = [torch.full((h, w), -7.0, dtype=torch.float32, device=dev) for _ in maps]
    torch.cuda.synchronize()
    c.depth_fill_batch_dev([t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f], w, h, K, scale, bilinear)
    c.depth_fill_status()
    return [t.cpu().numpy() for t in t_d], [t.cpu().numpy() for t in t_f]


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("B", [1, 2, 5, 16])
def test_batch_equals_the_oracle_frame_by_frame_and_again_over_stale_scratch(ctx, torch_dev, vga, B, bilinear):
    maps, want = vga
    for rot in (0, 1):   # the second pass: frame f's scratch slice holds frame f's previous result, of another kind
        kinds = [KINDS[(f + rot) % len(KINDS)] for f in range(B)]
        got, got_dist = run_batch(ctx, torch_dev, [maps[k] for k in kinds], 640, 480, 8, bilinear)
        for f, k in enumerate(kinds):
            assert np.array_equal(u32(got_dist[f]), u32(want[k, bilinear][1])), (rot, f, k)
            assert np.array_equal(u32(got[f]), u32(want[k, bilinear][0])), (rot, f, k)


# (the odd shapes of tests/test_gpu_depthfill.py, which names them rows x columns, and the same turned round: either way
#  of reading "100 x 36" is covered)
@pytest.mark.parametrize("h,w,scale", [(100, 36, 3), (36, 100, 3), (483, 642, 8), (642, 483, 8), (60, 80, 1), (80, 60, 1)])
def test_odd_shapes_in_a_batch_of_three(ctx, torch_dev, h, w, scale):
    maps = [holes(k, h, w, np.random.default_rng(h + w + i)) for i, k in enumerate(["blobs", "nan", "sparse"])]
    for bilinear in (False, True):
        got, got_dist = run_batch(ctx, torch_dev, maps, w, h, scale, bilinear)
        for f, m in enumerate(maps):
            want, want_dist, _ = orclib.depth_fill(m, K, scale, bilinear)
            assert np.array_equal(u32(got_dist[f]), u32(want_dist)), (f, bilinear)
            assert np.array_equal(u32(got[f]), u32(want)), (f, bilinear)
            if scale == 1:   # (:336-338: only the distance map is written, the map stays as it came)
                assert np.array_equal(u32(got[f]), u32(m))


def test_refusals_leave_the_maps_and_the_context_as_they_were(ctx, torch_dev, vga):
    torch, dev = torch_dev
    maps, want = vga
    kinds = ["blobs", "dense", "nan"]
    t_d = [torch.from_numpy(maps[k]).to(dev) for k in kinds]
    t_f = [torch.full((480, 640), -7.0, dtype=torch.float32, device=dev) for _ in kinds]
    torch.cuda.synchronize()
    dp, fp = [t.data_ptr() for t in t_d], [t.data_ptr() for t in t_f]
    with pytest.raises(capi.MhError) as e:      # 160 x 120 downscaled pixels: more than the LDS-resident fill holds
        ctx.depth_fill_batch_dev(dp, fp, 640, 480, K, 4)
    assert "-> -3:" in str(e.value)             # MH_ERR_CAPACITY
    with pytest.raises(capi.MhError) as e:      # the automatic factor is one read-back per map
        ctx.depth_fill_batch_dev(dp, fp, 640, 480, K, -1)
    assert "-> -1:" in str(e.value)             # MH_ERR_ARG, and the message names the call that takes -1
    assert re.search(r"mh_depth_fill(?!_)", str(e.value).split(": ", 1)[1])
    for d2, f2 in (([dp[0], dp[1], dp[0]], fp), (dp, [fp[0], fp[1], fp[1]])):   # the frames are filled in place, side by side
        with pytest.raises(capi.MhError) as e:
            ctx.depth_fill_batch_dev(d2, f2, 640, 480, K, 8)
        assert "-> -1:" in str(e.value)
    ctx.depth_fill_status()
    for t, k in zip(t_d, kinds):
        assert np.array_equal(u32(t.cpu().numpy()), u32(maps[k]))
    assert all(bool((t == -7.0).all()) for t in t_f)
    # a batch and a single fill afterwards still give the oracle's bytes
    ctx.depth_fill_batch_dev(dp, fp, 640, 480, K, 8)
    ctx.depth_fill_status()
    for t, f, k in zip(t_d, t_f, kinds):
        assert np.array_equal(u32(t.cpu().numpy()), u32(want[k, False][0]))
        assert np.array_equal(u32(f.cpu().numpy()), u32(want[k, False][1]))
    got, got_dist, used = ctx.depth_fill(maps["grid"], K, 8, True)
    assert used == 8
    assert np.array_equal(u32(got), u32(want["grid", True][0])) and np.array_equal(u32(got_dist), u32(want["grid", True][1]))
