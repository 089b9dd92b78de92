"""The SIFT oracle's stage dump (orclib.SiftRun: the whole pyramid, every scan hit that reached InterpKeyPoint, the
orientation peaks -- one run of the same run_sift that orc_sift calls) against the oracle's own outputs, so that the
GPU stage tests (tests/test_gpu_sift_stages.py) compare against something that is itself pinned: the final list is
the reference's libsiftfast build bit for bit (tests/test_sift_cpu.py)."""
import os

import numpy as np
import pytest

import orclib
from moped_amd import synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_one_run_pyramid_equals_the_per_image_call():
    gray = GOLD["gray0"][200:297, 250:381]
    for dbl in (True, False):
        run = orclib.SiftRun(gray, double_size=dbl)
        assert len(run.octaves) == (4 if dbl else 3)
        for o, (rows, cols) in enumerate(run.octaves):
            for kind, cnt in ((0, 6), (1, 5)):
                for i in range(cnt):
                    want = orclib.sift_image(gray, o, kind, i, double_size=dbl)
                    got = run.level(o, kind, i)
                    assert got.shape == want.shape == (rows, cols)
                    assert np.array_equal(_u32(got), _u32(want)), (dbl, o, kind, i)
        assert orclib.sift_image(gray, len(run.octaves), 0, 0, double_size=dbl) is None


def test_one_run_pyramid_on_a_golden_frame():
    gray = GOLD["gray0"]
    run = orclib.SiftRun(gray)
    assert run.octaves == [(958, 1278), (479, 639), (239, 319), (119, 159), (59, 79), (29, 39), (14, 19)]
    for o, kind, i in ((0, 0, 0), (0, 1, 4), (3, 0, 5), (6, 1, 0)):       # (every image costs a whole run of the old call)
        assert np.array_equal(_u32(run.level(o, kind, i)), _u32(orclib.sift_image(gray, o, kind, i)))
    # DoG i = Gaussian i - Gaussian i + 1, level 0 of octave o + 1 = every second pixel of level 3 of octave o
    for o in range(len(run.octaves)):
        for i in range(5):
            assert np.array_equal(_u32(run.level(o, 1, i)), _u32(run.level(o, 0, i) - run.level(o, 0, i + 1)))
        if o:
            assert np.array_equal(_u32(run.level(o, 0, 0)), _u32(orclib.sift_half(run.level(o - 1, 0, 3))))


@pytest.mark.parametrize("name", ["gray0", "gray3", "textured"])
def test_keys_rebuilt_from_the_hit_dump_equal_the_final_list(name):
    gray = synth.textured_image(0) if name == "textured" else GOLD[name]
    run = orclib.SiftRun(gray)
    xy, so, _ = orclib.sift(gray)
    kx, ks = run.keys()
    assert len(xy) == len(kx) > 500
    assert np.array_equal(_u32(kx), _u32(xy))                 # position
    assert np.array_equal(_u32(ks), _u32(so))                 # scale, orientation
    if name != "textured":
        assert np.array_equal(_u32(xy), _u32(GOLD[f"xy{name[4:]}"]))      # and the list is still libsiftfast's
    h = run.hits
    # the dump's own bookkeeping: generation order, flags, peaks
    order = np.stack([h["octave"], h["index"], h["r0"], h["c0"]], 1)
    assert all(tuple(a) < tuple(b) for a, b in zip(order[:-1], order[1:]))
    assert np.all(h["took"] <= h["passed"]) and h["passed"].sum() >= h["took"].sum() > 0
    if name != "textured":                                    # (the bundled frames have extrema that lose their pixel)
        assert h["passed"].sum() > h["took"].sum()
    assert np.all(h["n_peaks"][h["took"] == 0] == 0) and h["n_peaks"].sum() == len(run.peaks)
    took = h[h["took"] == 1]
    assert len(set(zip(took["octave"].tolist(), took["r"].tolist(), took["c"].tolist()))) == len(took)   # one per pixel
    assert np.array_equal(_u32(took["frow"]), _u32(took["r"].astype(np.float32) + took["x1"]))
    assert np.array_equal(_u32(took["fcol"]), _u32(took["c"].astype(np.float32) + took["x2"]))
    assert np.array_equal(run.peaks["hit"], np.sort(run.peaks["hit"]))
    for k in np.flatnonzero(h["n_peaks"] > 1)[:50]:
        b = run.peaks["bin"][h["first_peak"][k]:h["first_peak"][k] + h["n_peaks"][k]]
        assert np.all(np.diff(b) > 0)


def test_blur_and_half_exports_are_the_runs_own():
    gray = GOLD["gray0"][200:297, 250:381]
    run = orclib.SiftRun(gray, double_size=False)
    fwidth = np.float32(2.0) ** (np.float32(1.0) / np.float32(3.0))
    fincsigma = np.sqrt(fwidth * fwidth - np.float32(1.0), dtype=np.float32)
    sigma = np.float32(1.6)
    for i in range(1, 6):
        assert np.array_equal(_u32(orclib.sift_blur(run.level(0, 0, i - 1), float(fincsigma * sigma))), _u32(run.level(0, 0, i))), i
        sigma = np.float32(sigma * fwidth)
    assert [orclib.sift_taps((n - 0.5) / 8) for n in (3, 5, 11, 13, 17, 21, 25, 33, 35)] == [3, 5, 11, 13, 17, 21, 25, 33, 35]
    assert orclib.sift_half(np.arange(35, dtype=np.float32).reshape(5, 7)).tolist() == [[0, 2, 4], [14, 16, 18]]
