"""The SIFT oracle's stage dump (orclib.SiftRun: the whole pyramid, every scan hit that reached InterpKeyPoint, the
orientation peaks -- one run of the same run_sift that orc_sift calls) against the oracle's own outputs, so that the
GPU stage tests (tests/test_gpu_sift_stages.py) compare against something that is itself pinned: the final list is
the reference's libsiftfast build bit for bit (tests/test_sift_cpu.py).

Descriptors of GIVEN keys (SiftRun.describe) -- what section (f) of the GPU stage tests holds describe_kernel to:
  f32   make_key's own body (one template, T = float): the run's own keys give orc_sift's descriptors bit for bit;
  f64   the samples the float32 tests select, and from there on everything in double on the float32 pixels;
  pert  f32 with every sinf / cosf / expf / gradient atan2f result moved K = FSIZE_ULP_BOUND floats (the project's
        standing allowance for device libm against host libm), all up, all down, or by a hash per result;
  drop  f32 without one selected sample: the mutant that shows the bar bites.
Per key  e_ref = max |f32 - f64|,  e_pert = the largest max |pert - f32| of four perturbation runs (up, down, two hashed
seeds),  bar = 2 (e_ref + e_pert) + 2^-23.  The device does the oracle's operations in the oracle's order, so its
distance from f64 is the oracle's rounding plus the effect of transcendental results at most K floats away; the factor
2 because e_ref is one realisation of the rounding, not a bound on it; 2^-23 = one ulp of the descriptor's norm, for a
key whose e_ref happens to be 0.

Measured (every key of the input; K = 4):
  input             keys   bar median  99 %     max       largest-mag drop / bar, min   row ends detected: first, last
  gray0              586   1.37e-6   2.62e-6  3.44e-6     132                           23 968 / 26 243, 23 990 / 25 963
  gray3              599   1.33e-6   2.48e-6  3.24e-6     171                           24 403 / 26 748, 24 456 / 26 465
  gray0_undoubled    302   1.35e-6   2.91e-6  3.27e-6     145                           12 086 / 13 209, 12 060 / 13 067
  textured         3 240   1.17e-6   1.87e-6  2.40e-6     149                           151 143 / 155 680, 149 947 / 153 689
  crop97x131          95   1.38e-6   2.31e-6  2.48e-6     7.2                           3 578 / 3 829, 3 616 / 3 797
  crop97x131_und      29   1.36e-6   1.88e-6  1.90e-6     158                           1 013 / 1 067, 1 032 / 1 059
  crop60x82_und       17   1.38e-6   2.10e-6  2.15e-6     62                            537 / 567, 555 / 562
  strip33x400         14   1.30e-6   3.17e-6  3.18e-6     396                           425 / 463, 447 / 462
  crop24x40           14   1.36e-6   1.63e-6  1.64e-6     784                           440 / 448, 440 / 446
  crop8x8              1   2.45e-6   2.45e-6  2.45e-6     1 590                         14 / 14, 14 / 14
  mosaic           2 413   1.32e-6   2.54e-6  3.44e-6     58                            99 414 / 108 805, 99 147 / 107 657
e_ref stays below 2.5e-7 and e_pert below 1.5e-6 everywhere.  Losing the sample of largest weighted magnitude moves a
descriptor by at least 7 bars (hard condition, asserted for every key); losing the first or the last selected sample of
a window row -- what an off-by-one in a row interval does -- is detected for 91 % (bundled frames) to 100 % of those
samples: they sit at the window's rim, where the Gaussian and the trilinear weights are smallest.  A slip loses such a
sample in many rows of many keys, and each loss is detected on its own with that share.  The bar is two to three orders of magnitude below the 5e-3 of
tests/test_gpu_sift.py."""
import os

import numpy as np
import pytest

import orclib
from moped_amd import synth
from test_gpu_sift_stages import FSIZE_ULP_BOUND, INPUTS   # the device-libm allowance and the inputs of the GPU stage tests

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


# ---- descriptors of given keys: SiftRun.describe --------------------------------------------------------------------
# Part of the row-end measurement runs on every ROW_END_STRIDE[name]-th key only (a row end costs a whole describe; the
# module docstring has the figures over all keys).
ROW_END_STRIDE = {"textured": 8, "mosaic": 8}
_bars = {}


def _bar_of(name):
    """(run, keys, descriptor_bar) of one input, once per module."""
    if name not in _bars:
        make, dbl = INPUTS[name]
        gray = np.ascontiguousarray(make())
        run = orclib.SiftRun(gray, double_size=dbl)
        keys = run.key_records()
        _bars[name] = (gray, dbl, run, keys, run.descriptor_bar(keys, FSIZE_ULP_BOUND))
    return _bars[name]


@pytest.mark.parametrize("name", list(INPUTS))
def test_describe_f32_is_the_pinned_list_bit_for_bit(name):
    """describe(the run's own keys, 'f32') = orc_sift's descriptors as uint32, and the keys are the list's keys: the new
    export is make_key's body, and the list is pinned to the reference build (tests/test_sift_cpu.py)."""
    gray, dbl, run, keys, q = _bar_of(name)
    xy, so, d = orclib.sift(gray, double_size=dbl)
    assert len(keys) == len(d) >= 1
    fs = run.fscale(keys["octave"])
    assert np.array_equal(_u32(np.stack([fs * keys["fcol"], fs * keys["frow"]], 1)), _u32(xy))
    assert np.array_equal(_u32(np.stack([fs * keys["fsize"], keys["ori"]], 1)), _u32(so))
    assert np.array_equal(_u32(q["f32"]), _u32(d))
    assert np.all(q["totals"] >= 64) and np.all(np.isfinite(q["f64"]))
    # pert with no steps and drop of a sample that does not exist are f32 again
    assert np.array_equal(_u32(run.describe(keys, "pert", ulps=0)), _u32(d))
    assert np.array_equal(_u32(run.describe(keys, "drop", drop=-1)), _u32(d))
    assert np.array_equal(_u32(run.describe(keys, "drop", drop=q["totals"])), _u32(d))
    bad = keys[:1].copy()
    for field, value in (("octave", len(run.octaves)), ("octave", -1), ("index", 0), ("index", 4)):
        k = bad.copy()
        k[field] = value
        with pytest.raises(ValueError):
            run.describe(k, "f32")


@pytest.mark.parametrize("name", list(INPUTS))
def test_descriptor_bar_bites(name):
    """The bar of the module docstring, per key, and the hard condition on it: a descriptor that lost the ONE sample of
    largest weighted magnitude lies further than `bar` from f64 -- for every key of every input.  Measured beside it: the
    share of the first / last selected samples of the window rows whose loss the bar detects."""
    gray, dbl, run, keys, q = _bar_of(name)
    bar = q["bar"]
    assert np.all(bar >= 2.0 ** -23) and np.all(q["e_pert"] > 0)
    lost = run.describe(keys, "drop", drop=-2)
    e_drop = np.abs(lost.astype(np.float64) - q["f64"]).max(axis=1)
    step = ROW_END_STRIDE.get(name, 1)
    tried, det = run.drop_row_ends(keys[::step], q["f64"][::step], bar[::step])
    share = det.sum(axis=0) / np.maximum(tried.sum(axis=0), 1)
    print(f"\n[sift descriptors] {name}: {len(keys)} keys, samples {q['totals'].min()}..{q['totals'].max()}, "
          f"e_ref max {q['e_ref'].max():.3g}, e_pert max {q['e_pert'].max():.3g}, bar median {np.median(bar):.3g} "
          f"99 % {np.quantile(bar, 0.99):.3g} max {bar.max():.3g}; largest-mag drop / bar min {np.min(e_drop / bar):.3g}; "
          f"row ends detected (every {step}. key): first {det[:, 0].sum()}/{tried[:, 0].sum()}, last {det[:, 1].sum()}/{tried[:, 1].sum()}")
    miss = np.flatnonzero(~(e_drop > bar))
    assert len(miss) == 0, (name, [(keys[i].tolist(), int(q["totals"][i]), float(e_drop[i]), float(bar[i])) for i in miss[:5]])
    assert tried.sum() > 0 and np.all(share >= 0.5), (name, tried.sum(axis=0).tolist(), det.sum(axis=0).tolist())


def test_describe_modes_on_one_key():
    """What each mode changes, on the first key of the cropped frame: f64 is close to f32 but not its rounding target
    only; all-up and all-down perturbations differ from f32 and from each other, a hashed one depends on its seed; drop
    of sample t removes exactly that sample (dropping it from a window re-adds up to the f32 descriptor's samples)."""
    gray, dbl, run, keys, q = _bar_of("crop97x131_und")
    k = keys[:1]
    f32 = q["f32"][:1]
    up = run.describe(k, "pert", ulps=FSIZE_ULP_BOUND, direction=1)
    down = run.describe(k, "pert", ulps=FSIZE_ULP_BOUND, direction=-1)
    h1 = run.describe(k, "pert", ulps=FSIZE_ULP_BOUND, direction=0, seed=1)
    h2 = run.describe(k, "pert", ulps=FSIZE_ULP_BOUND, direction=0, seed=2)
    again = run.describe(k, "pert", ulps=FSIZE_ULP_BOUND, direction=0, seed=1)
    assert np.array_equal(_u32(h1), _u32(again))
    for a, b in ((up, f32), (down, f32), (up, down), (h1, h2), (h1, up), (h1, down)):
        assert not np.array_equal(_u32(a), _u32(b))
        assert np.abs(a - b).max() < 1e-5
    assert 0 < q["e_ref"][0] < 1e-6
    total = int(q["totals"][0])
    # every selected sample matters to some entry, and no two drops give the same descriptor
    seen = set()
    for t in (0, 1, total // 2, total - 2, total - 1):
        d = run.describe(k, "drop", drop=t)
        assert not np.array_equal(_u32(d), _u32(f32)), t
        seen.add(d.tobytes())
    assert len(seen) == 5
