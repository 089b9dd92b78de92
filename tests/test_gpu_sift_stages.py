"""FEAT stage by stage: the pyramid, the extrema and the keys the HIP SIFT kernels leave on the device
(mh_sift_debug_*) against the same stages of ONE oracle run (orclib.SiftRun; the oracle's final list is the reference's
libsiftfast build bit for bit, tests/test_sift_cpu.py, and its stage dump is tied to that list by
tests/test_sift_stages_cpu.py).

Prepare, the blur chain, DoG, the 2:1 subsample, the extremum scan, the edge test, the quadratic fit and the
first-claim rule contain no transcendental function on the device (the Gaussian taps come from the host's libm), so
(a), (b), (d) and (e) hold bit for bit; only orient_kernel's powf / expf / atan2f may differ from libm, and (c) says by
how much.  (f) holds the last stage, describe_kernel: every descriptor -- of every key of every input, of several keys
per workgroup, and of synthetic keys at the window's, the orientation's and the 256-sample step's edges run through
mh_sift_debug_describe -- against the float64 descriptor of the same key, within a per-key bar derived from rounding
alone (a few 1e-6; a descriptor that lost one sample misses it: tests/test_sift_stages_cpu.py).  tests/test_gpu_sift.py
keeps its statistical bars on the end-to-end list (count, order, pairing with the reference's keypoints)."""
import os

import numpy as np
import pytest

import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_ref_frames.npz"))


def _mosaic():
    g0, g1 = GOLD["gray0"], GOLD["gray3"]
    return np.block([[g0, g1], [g1[::-1], g0[:, ::-1]]])          # test_hip_sift_many_keypoints' 1280 x 960


# name -> (image, first octave doubled)
INPUTS = {
    "gray0":           (lambda: GOLD["gray0"], True),
    "gray3":           (lambda: GOLD["gray3"], True),
    "gray0_undoubled": (lambda: GOLD["gray0"], False),                      # 30 x 40 = SMALL_OCTAVE_PX exactly: single workgroup
    "textured":        (lambda: synth.textured_image(0), True),
    "crop97x131":      (lambda: GOLD["gray0"][200:297, 250:381], True),
    "crop97x131_und":  (lambda: GOLD["gray0"][200:297, 250:381], False),    # odd width: the c + 1 < cols branch
    "crop60x82_und":   (lambda: GOLD["gray0"][200:260, 250:332], False),    # 30 x 41 = 1 230 px, just above the boundary: tiles
    "strip33x400":     (lambda: GOLD["gray0"][100:133, 0:400], True),       # tiles thinner than their halo, no small octave
    "crop24x40":       (lambda: GOLD["gray0"][200:224, 300:340], True),     # less than one tile wide after the first column
    "crop8x8":         (lambda: GOLD["gray0"][210:218, 300:308], True),     # 14 x 14 only: 3 x 3 scanned pixels
    "mosaic":          (_mosaic, True),                                     # 8 octaves (SIFT_MAX_OCTAVES), > 1 536 keys
}
_VGA2 = [(958, 1278), (479, 639), (239, 319), (119, 159), (59, 79), (29, 39), (14, 19)]
OCTAVES = {
    "gray0": _VGA2, "gray3": _VGA2, "textured": _VGA2,
    "mosaic": [(1918, 2558), (959, 1279), (479, 639), (239, 319), (119, 159), (59, 79), (29, 39), (14, 19)],
    "gray0_undoubled": [(480, 640), (240, 320), (120, 160), (60, 80), (30, 40), (15, 20)],
    "crop97x131": [(192, 260), (96, 130), (48, 65), (24, 32)],
    "crop97x131_und": [(97, 131), (48, 65), (24, 32)],
    "crop60x82_und": [(60, 82), (30, 41), (15, 20)],
    "strip33x400": [(64, 798), (32, 399), (16, 199)],
    "crop24x40": [(46, 78), (23, 39)],
    "crop8x8": [(14, 14)],
}
# oracle keypoints per input (measured on the CPU): every case has something to lose
MIN_KEYS = {"gray0": 586, "gray3": 599, "gray0_undoubled": 302, "textured": 3240, "crop97x131": 95, "crop97x131_und": 29,
            "crop60x82_und": 17, "strip33x400": 14, "crop24x40": 14, "crop8x8": 1, "mosaic": 1537}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_runs = {}


@pytest.fixture(scope="module")
def oracle():
    """One oracle run per input for the whole module."""
    def get(name):
        if name not in _runs:
            make, dbl = INPUTS[name]
            gray = np.ascontiguousarray(make())
            _runs[name] = (gray, dbl, orclib.SiftRun(gray, double_size=dbl))
        return _runs[name]
    yield get
    for _, _, run in _runs.values():
        run.close()
    _runs.clear()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _level_report(what, got, want):
    """'' if the images are equal as uint32, else octave / level, the number of differing pixels, the first (r, c), both values."""
    g, w = _u32(got), _u32(want)
    if g.shape != w.shape:
        return f"{what}: shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    if len(bad) == 0:
        return ""
    r, c = (int(x) for x in bad[0])
    rr, cc = bad[:, 0], bad[:, 1]
    return (f"{what}: {len(bad)} of {g.size} pixels differ, first at (r={r}, c={c}) device {got[r, c]!r} (0x{g[r, c]:08x}) "
            f"oracle {want[r, c]!r} (0x{w[r, c]:08x}); rows {rr.min()}..{rr.max()}, columns {cc.min()}..{cc.max()}")


def _check_pyramid(ctx, run, label):
    n_img, plan = ctx.sift_debug_plan()
    assert n_img == 1 and plan == run.octaves, (label, plan, run.octaves)
    reports = []
    for o, shape in enumerate(plan):
        for kind, kname in ((0, "Gaussian"), (1, "DoG")):
            for i in range(5):
                rep = _level_report(f"{label} octave {o} ({shape[0]}x{shape[1]}) {kname} level {i}",
                                    ctx.sift_debug_level(o, kind, i, shape), run.level(o, kind, i))
                if rep:
                    reports.append(rep)
    assert not reports, "\n".join(reports[:12] + ([f"... and {len(reports) - 12} more images"] if len(reports) > 12 else []))


# ---- (a) the pyramid, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INPUTS))
def test_pyramid_equals_the_oracle_bit_for_bit(ctx, oracle, name):
    """Every stored Gaussian level (0..4) and every DoG level of every octave as uint32, tolerance zero: the products and
    sums are __fmul_rn / __fadd_rn or packed float2 operators without contraction, the taps come from the host."""
    gray, dbl, run = oracle(name)
    assert run.octaves == OCTAVES[name]
    ctx.sift(gray, double_size=dbl)
    _check_pyramid(ctx, run, name)
    with pytest.raises(capi.MhError):                 # Gaussian level 5 is never stored
        ctx.sift_debug_level(0, 0, 5, run.octaves[0])
    with pytest.raises(capi.MhError):
        ctx.sift_debug_level(len(run.octaves), 0, 0, run.octaves[0])
    with pytest.raises(capi.MhError):
        ctx.sift_debug_level(0, 0, 0, run.octaves[0], slot=1)


def _synthetic_images():
    """Images whose pyramid is easy to reason about (octave 0 = the image: not doubled; the blur tile is 64 x 32)."""
    h, w = 100, 150
    pts = np.zeros((h, w), np.uint8)
    for r in (0, h // 2, h - 1):
        for c in (0, w // 2, w - 1):
            if not (r == h // 2 and c == w // 2):
                pts[r, c] = 255                        # the four corners and the middle of each border
    out = [("points", pts), ("points_inverse", (255 - pts).astype(np.uint8))]
    for p in (63, 64, 65, 31, 32, 33):
        v = np.zeros((h, w), np.uint8)
        v[:, p:] = 255
        out.append((f"vertical_step_at_column_{p}", v))
        hz = np.zeros((h, w), np.uint8)
        hz[p:, :] = 255
        out.append((f"horizontal_step_at_row_{p}", hz))
    return out


def test_pyramid_of_synthetic_points_and_steps(ctx):
    for label, img in _synthetic_images():
        for dbl in (False, True):
            run = orclib.SiftRun(img, double_size=dbl)
            ctx.sift(img, double_size=dbl)
            _check_pyramid(ctx, run, f"{label} doubled={dbl}")
            run.close()


# ---- (b) extrema, bit for bit -------------------------------------------------------------------------------------
def _device_candidates(ctx, slot=0):
    cand, won = ctx.sift_debug_candidates(slot)
    order = np.lexsort((cand["key"], cand["octave"]))
    return cand[order], won[order]


def _oracle_candidates(run):
    h = run.hits[run.hits["passed"] == 1]
    rows = np.array([run.octaves[o][0] for o in h["octave"]], np.int64)
    cols = np.array([run.octaves[o][1] for o in h["octave"]], np.int64)
    key = (h["index"] - 1).astype(np.int64) * rows * cols + h["r0"].astype(np.int64) * cols + h["c0"]
    return h, key


@pytest.mark.parametrize("name", list(INPUTS))
def test_extrema_equal_the_oracle_bit_for_bit(ctx, oracle, name):
    """The candidates sorted by (octave, key) are the oracle's scan hits that passed InterpKeyPoint's final test: same
    octave, scale index, start pixel, final pixel, offsets equal as uint32, same winners of the final pixel.  No count
    tolerance, no pairing by distance."""
    gray, dbl, run = oracle(name)
    ctx.sift(gray, double_size=dbl)
    cand, won = _device_candidates(ctx)
    h, key = _oracle_candidates(run)
    assert h["took"].sum() >= 1 and len(run.peaks) >= MIN_KEYS[name], (name, len(run.peaks))
    dev = [(int(q["octave"]), int(q["key"])) for q in cand]
    orc = list(zip(h["octave"].tolist(), key.tolist()))
    missing, extra = sorted(set(orc) - set(dev)), sorted(set(dev) - set(orc))
    assert len(cand) == len(h) and not missing and not extra, (
        f"{name}: device {len(cand)} candidates, oracle {len(h)}; missing (octave, key) {missing[:10]}, extra {extra[:10]}")
    for f, of in (("index", "index"), ("r", "r"), ("c", "c")):
        bad = np.flatnonzero(cand[f] != h[of])
        assert len(bad) == 0, (name, f, [(dev[i], int(cand[f][i]), int(h[of][i])) for i in bad[:10]])
    for f in ("x0", "x1", "x2"):
        bad = np.flatnonzero(_u32(cand[f]) != _u32(h[f]))
        assert len(bad) == 0, (name, f, [(dev[i], float(cand[f][i]), float(h[f][i])) for i in bad[:10]])
    bad = np.flatnonzero(won != (h["took"] == 1))
    assert len(bad) == 0, (name, "won", [(dev[i], bool(won[i])) for i in bad[:10]])


# ---- (c) keys -----------------------------------------------------------------------------------------------------
# fsize = 1.6 powf(2, (index + X0) / 3): the device's powf against libm's.  Largest difference measured over all extrema
# of INPUTS on an MI355X (6 217 extrema; the test prints the figure per input): FSIZE_ULP_MEASURED ulp; the bound is
# twice that, as margin for other libm builds.
FSIZE_ULP_MEASURED = 2
FSIZE_ULP_BOUND = 2 * FSIZE_ULP_MEASURED
BIN_SHARE = 0.005      # extrema per image whose list of histogram bins may differ (test_hip_sift_matches_the_reference_keypoints' 0.5 %)
ANGLE_BOUND = 1e-3     # rad, where the bins agree (the same test's bound)


def _ulp_diff(a, b):
    """|a - b| in units in the last place, for finite positive floats."""
    return np.abs(_u32(a).astype(np.int64) - _u32(b).astype(np.int64))


@pytest.mark.parametrize("name", list(INPUTS))
def test_keys_position_scale_and_peaks(ctx, oracle, name):
    gray, dbl, run = oracle(name)
    ctx.sift(gray, double_size=dbl)
    keys = ctx.sift_debug_keys()
    keys = keys[np.argsort(keys["order"], kind="stable")]
    assert len(np.unique(keys["order"])) == len(keys)
    assert np.array_equal(keys["octave"].astype(np.uint64), keys["order"] >> np.uint64(40))
    group = (keys["order"] >> np.uint64(8)).astype(np.int64)                 # octave << 32 | key
    bins = (keys["order"] & np.uint64(255)).astype(np.int64)
    first = {int(g): i for i, g in reversed(list(enumerate(group)))}
    count = {int(g): int(n) for g, n in zip(*np.unique(group, return_counts=True))}
    h, key = _oracle_candidates(run)
    took = np.flatnonzero(h["took"] == 1)
    ids = {(int(h["octave"][i]) << 32) | int(key[i]) for i in took}
    assert set(count) <= ids, f"{name}: keys of extrema that did not take their pixel: {sorted(set(count) - ids)[:10]}"
    worst_ulp, worst_ang, differ = 0, 0.0, []
    for i in took:
        gid = (int(h["octave"][i]) << 32) | int(key[i])
        want_bins = run.peaks["bin"][h["first_peak"][i]:h["first_peak"][i] + h["n_peaks"][i]].tolist()
        at, n = first.get(gid, 0), count.get(gid, 0)
        got = keys[at:at + n]
        got_bins = bins[at:at + n].tolist()
        where = f"octave {h['octave'][i]} index {h['index'][i]} start ({h['r0'][i]}, {h['c0'][i]}) final ({h['r'][i]}, {h['c'][i]})"
        if n:
            assert np.all(got["index"] == h["index"][i]), where
            assert np.all(_u32(got["frow"]) == _u32(h["frow"][i])) and np.all(_u32(got["fcol"]) == _u32(h["fcol"][i])), (
                name, where, got["frow"].tolist(), float(h["frow"][i]), got["fcol"].tolist(), float(h["fcol"][i]))
            u = int(_ulp_diff(got["fsize"], np.full(n, h["fsize"][i], np.float32)).max())
            worst_ulp = max(worst_ulp, u)
            assert u <= FSIZE_ULP_BOUND, (name, where, got["fsize"].tolist(), float(h["fsize"][i]), u)
        if got_bins != want_bins:
            differ.append(f"{where}: device bins {got_bins}, oracle {want_bins}")
            continue
        if n:
            want_ang = run.peaks["ang"][h["first_peak"][i]:h["first_peak"][i] + n]
            d = float(np.abs(got["ori"].astype(np.float64) - want_ang.astype(np.float64)).max())
            worst_ang = max(worst_ang, d)
            assert d <= ANGLE_BOUND, (name, where, got["ori"].tolist(), want_ang.tolist())
    print(f"\n[sift stages] {name}: {len(took)} extrema, {len(keys)} keys, fsize max {worst_ulp} ulp, "
          f"angle max {worst_ang:.3g} rad, {len(differ)} extrema with other bins")
    assert len(differ) <= BIN_SHARE * len(took), f"{name}: {len(differ)} of {len(took)} extrema:\n" + "\n".join(differ[:20])


# ---- (d) a batch slot equals the image alone ----------------------------------------------------------------------
def _snapshot(ctx, slot, plan):
    levels = [ctx.sift_debug_level(o, kind, i, shape, slot=slot).tobytes()
              for o, shape in enumerate(plan) for kind in (0, 1) for i in range(5)]
    cand, won = _device_candidates(ctx, slot)
    keys = ctx.sift_debug_keys(slot)
    keys = keys[np.argsort(keys["order"], kind="stable")]
    return levels, cand.tobytes(), won.tobytes(), keys.tobytes()


def _compare_snapshots(got, want, plan, label):
    names = [f"octave {o} {'DoG' if kind else 'Gaussian'} level {i}" for o in range(len(plan)) for kind in (0, 1) for i in range(5)]
    for nm, shape, g, w in zip(names, [s for s in plan for _ in range(10)], got[0], want[0]):
        if g != w:
            rep = _level_report(f"{label} {nm}", np.frombuffer(g, np.float32).reshape(shape), np.frombuffer(w, np.float32).reshape(shape))
            raise AssertionError(rep or f"{label} {nm}: bytes differ (NaN payloads?)")
    gc, wc = np.frombuffer(got[1], capi.SIFT_CANDIDATE_DTYPE), np.frombuffer(want[1], capi.SIFT_CANDIDATE_DTYPE)
    assert got[1] == want[1], f"{label}: candidates differ: {len(gc)} in the batch, {len(wc)} alone; first difference at sorted " \
                              f"position {next((i for i, (a, b) in enumerate(zip(gc, wc)) if a != b), min(len(gc), len(wc)))}"
    assert got[2] == want[2], f"{label}: owners of the final pixels differ"
    gk, wk = np.frombuffer(got[3], capi.SIFT_KEY_DTYPE), np.frombuffer(want[3], capi.SIFT_KEY_DTYPE)
    assert got[3] == want[3], f"{label}: keys differ: {len(gk)} in the batch, {len(wk)} alone"


def test_batch_slot_equals_the_image_alone(ctx):
    """Batches of 2, 5 (per-key kernels share workgroups between images from five on) and 16 images of one size -- different
    images in different slots, a blank one in the middle, one image twice: every slot's pyramid, candidates, owners, keys
    and outputs are, as bytes, what the same context gives for the image alone.  Device against device: bit for bit
    including the transcendental stages."""
    import torch
    dev = torch.device("cuda:0")
    g0, g3 = GOLD["gray0"], GOLD["gray3"]
    h, w = 240, 320
    distinct = [g0[0:240, 0:320], g3[240:480, 320:640], g0[120:360, 160:480], np.full((h, w), 128, np.uint8),
                g3[0:240, 320:640], g0[240:480, 0:320], g3[100:340, 100:420]]
    distinct = [np.ascontiguousarray(x) for x in distinct]
    cap = 2048

    def alone(k):
        xy, so, d = ctx.sift(distinct[k])
        n_img, plan = ctx.sift_debug_plan()
        assert n_img == 1
        return plan, _snapshot(ctx, 0, plan), (xy, d)

    singles = {k: alone(k) for k in range(len(distinct))}
    plan = singles[0][0]
    assert plan == [(478, 638), (239, 319), (119, 159), (59, 79), (29, 39), (14, 19)]
    assert all(len(singles[k][2][0]) > 20 for k in singles if k != 3) and len(singles[3][2][0]) == 0   # (image 3 is blank)
    dev_imgs = [torch.from_numpy(x).to(dev) for x in distinct]
    for n, slots in ((2, [0, 1]), (5, [0, 1, 3, 2, 0]), (16, [0, 1, 2, 4, 5, 6, 0, 3, 3, 6, 5, 4, 2, 1, 1, 0])):
        assert len(slots) == n
        desc = torch.zeros((n, cap, 128), dtype=torch.float32, device=dev)
        xy = torch.zeros((n, cap, 2), dtype=torch.float32, device=dev)
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sift_batch_dev([dev_imgs[k].data_ptr() for k in slots], w, h, True, desc.data_ptr(), xy.data_ptr(), cap,
                           counts.data_ptr())
        ctx.synchronize()
        n_img, got_plan = ctx.sift_debug_plan()
        assert n_img == n and got_plan == plan
        with pytest.raises(capi.MhError):
            ctx.sift_debug_keys(slot=n)
        cnt = counts.cpu().numpy()
        for s, k in enumerate(slots):
            label = f"batch of {n}, slot {s} (image {k})"
            _compare_snapshots(_snapshot(ctx, s, plan), singles[k][1], plan, label)
            want_xy, want_d = singles[k][2]
            assert cnt[s] == len(want_xy), label
            assert xy[s, :cnt[s]].cpu().numpy().tobytes() == want_xy.tobytes(), label
            assert desc[s, :cnt[s]].cpu().numpy().tobytes() == want_d.tobytes(), label
    # and a single image again on the same context (its buffers now hold room for sixteen)
    for k in (2, 3, 0):
        p, snap, (want_xy, want_d) = alone(k)
        _compare_snapshots(snap, singles[k][1], plan, f"image {k} alone after the batches")
        assert want_xy.tobytes() == singles[k][2][0].tobytes() and want_d.tobytes() == singles[k][2][1].tobytes()


# ---- (e) blur variants --------------------------------------------------------------------------------------------
ROWS_COLS, LEVEL, JOBS, HALF, SMALL = 0, 1, 2, 3, 4
TAP_COUNTS = (3, 5, 11, 13, 17, 21, 25, 33, 35)      # 33: half-width 16 = the tile kernels' largest; 35: beyond it


def _unit(gray):
    return (gray.astype(np.float32).astype(np.float64) * 1. / 255.).astype(np.float32)


BLUR_SOURCES = {
    "crop97x131": lambda: _unit(GOLD["gray0"][200:297, 250:381]),
    "strip33x400": lambda: _unit(GOLD["gray0"][100:133, 0:400]),
    "crop24x40": lambda: _unit(GOLD["gray0"][200:224, 300:340]),            # fits the single-workgroup chain with its borders
    "crop60x100": lambda: _unit(GOLD["gray0"][100:160, 200:300]),           # fits it only without them (6 000 of 6 912 floats)
}


@pytest.mark.parametrize("src_name", list(BLUR_SOURCES))
def test_blur_variants_equal_the_oracles_blur(ctx, src_name):
    """Every kernel of the blur chain that can take a tap count -- the ones the shipped constants never select included --
    gives the oracle's blur() and source - blurred bit for bit; the ones that cannot refuse it without launching."""
    src = BLUR_SOURCES[src_name]()
    ran = {v: [] for v in (ROWS_COLS, LEVEL, JOBS, SMALL)}
    for taps in TAP_COUNTS:
        sigma = (taps - 0.5) / 8
        assert orclib.sift_taps(sigma) == taps
        want = orclib.sift_blur(src, sigma)
        for variant in (ROWS_COLS, LEVEL, JOBS, SMALL):
            fits = (variant == ROWS_COLS or (variant in (LEVEL, JOBS) and taps // 2 <= 16) or
                    (variant == SMALL and src.size <= 6912))
            if not fits:
                with pytest.raises(capi.MhError, match="variant"):
                    ctx.sift_debug_blur(variant, src, sigma)
                continue
            dst, dog, _ = ctx.sift_debug_blur(variant, src, sigma)
            label = f"{src_name} variant {variant} taps {taps}"
            rep = _level_report(label + " blurred", dst, want) or _level_report(label + " DoG", dog, src - want)
            assert not rep, rep
            ran[variant].append(taps)
        # the job list reading the previous octave: subsample, then blur; the subsampled image is the octave's level 0
        hs = orclib.sift_half(src)
        hw = orclib.sift_blur(hs, sigma)
        if taps // 2 <= 16:
            dst, dog, hd = ctx.sift_debug_blur(JOBS, src, sigma, half=True, want_half=True)
            label = f"{src_name} half job taps {taps}"
            rep = (_level_report(label + " level 0", hd, hs) or _level_report(label + " blurred", dst, hw) or
                   _level_report(label + " DoG", dog, hs - hw))
            assert not rep, rep
        else:
            with pytest.raises(capi.MhError, match="variant"):
                ctx.sift_debug_blur(JOBS, src, sigma, half=True, want_half=True)
    assert ran[ROWS_COLS] == list(TAP_COUNTS) and ran[LEVEL] == ran[JOBS] == list(TAP_COUNTS[:-1])
    assert ran[SMALL] == (list(TAP_COUNTS) if src.size <= 6912 else [])
    dst, _, _ = ctx.sift_debug_blur(HALF, src, 0.0, half=True, want_dog=False)
    rep = _level_report(f"{src_name} half kernel", dst, orclib.sift_half(src))
    assert not rep, rep
    for variant, kw in ((HALF, dict(half=False, want_dog=False)), (ROWS_COLS, dict(half=True)), (LEVEL, dict(half=True)),
                        (SMALL, dict(half=True)), (JOBS, dict(half=True, want_half=False)), (5, {}), (-1, {})):
        with pytest.raises(capi.MhError, match="variant"):
            ctx.sift_debug_blur(variant, src, 1.0, **kw)
    with pytest.raises(capi.MhError, match="variant"):
        ctx.sift_debug_blur(ROWS_COLS, src, 8.0)          # 65 taps: more than the kernels' tap array holds


# ---- (f) descriptors ----------------------------------------------------------------------------------------------
# describe_kernel does make_key's operations in make_key's order; only sinf, cosf, expf and atan2f may differ from libm.
# So a device descriptor's distance from the float64 descriptor of the SAME key (orclib.SiftRun.describe, mode f64: the
# float32 tests select the samples, everything after that in double) is the oracle's own rounding plus the effect of
# transcendental results at most FSIZE_ULP_BOUND floats away: per key
#     bar = 2 (e_ref + e_pert) + 2^-23        (SiftRun.descriptor_bar; derivation and measured figures -- median 1.3e-6,
#                                              largest 3.4e-6 -- in tests/test_sift_stages_cpu.py)
# which a descriptor that lost ONE sample misses (checked there on the CPU for every key of every input).  Every key is
# held to it: no pairing, no percentile, none left out.
F32 = np.float32


def _window_side(fsize):
    """2 win + 1 of make_key's window: win = (int)(3 fSize sqrt2 5 / 2 + 0.5) in float32, as the kernel computes it."""
    return 2 * int(F32(F32(F32(F32(F32(3.0) * F32(fsize)) * F32(1.4142136)) * F32(5.0)) * F32(0.5)) + F32(0.5)) + 1


def _by_order(keys):
    """The output order: place i = the key with i keys of larger `order` (generation order reversed)."""
    return keys[np.argsort(keys["order"], kind="stable")[::-1]]


def _check_descriptors(run, keys, dev, label, names=None):
    """max |device - f64| <= bar for EVERY key (keys in the device's output order); -> the number of descriptors that are
    bit-identical to the oracle's float32 ones, and the largest error / bar."""
    q = run.descriptor_bar(keys, FSIZE_ULP_BOUND)
    assert dev.shape == q["f64"].shape and np.all(np.isfinite(q["f64"])) and np.all(q["totals"] > 0), label
    err = np.abs(dev.astype(np.float64) - q["f64"])
    worst = err.max(axis=1)
    bad = np.flatnonzero(~(worst <= q["bar"]))                        # (a NaN fails)
    lines = []
    for i in bad[:8]:
        k, e = keys[i], int(np.argmax(err[i])) if np.all(np.isfinite(err[i])) else int(np.argmax(~np.isfinite(err[i])))
        lines.append(
            f"{label} key {i}{' [' + names[i] + ']' if names else ''}: octave {k['octave']} index {k['index']} row {k['frow']!r} "
            f"column {k['fcol']!r} fsize {k['fsize']!r} ori {k['ori']!r}, window side {_window_side(k['fsize'])}, "
            f"{q['totals'][i]} samples; worst entry (cell row {e // 32}, cell column {e // 8 % 4}, bin {e % 8}): device "
            f"{dev[i, e]!r} f32 {q['f32'][i, e]!r} f64 {q['f64'][i, e]!r}; error {worst[i]:.3g} > bar {q['bar'][i]:.3g} "
            f"(e_ref {q['e_ref'][i]:.3g}, e_pert {q['e_pert'][i]:.3g})")
    assert len(bad) == 0, f"{len(bad)} of {len(keys)} descriptors beyond their bar\n" + "\n".join(lines)
    same = int(np.sum(np.all(_u32(dev) == _u32(q["f32"]), axis=1)))
    return same, float(np.max(worst / q["bar"]))


@pytest.mark.parametrize("name", list(INPUTS))
def test_descriptors_of_every_key(ctx, oracle, name):
    """(f1) The extraction's own outputs: place i is the key with i keys of larger order, its position / scale /
    orientation are fscale (fcol, frow), fscale fsize and ori as uint32, and its descriptor lies within the key's bar of
    the float64 descriptor of that very key (the device's fsize and ori, whatever they are)."""
    gray, dbl, run = oracle(name)
    xy, so, d = ctx.sift(gray, double_size=dbl)
    keys = _by_order(ctx.sift_debug_keys())
    assert len(keys) == len(d) >= 0.99 * MIN_KEYS[name], (name, len(keys), len(d))
    fs = run.fscale(keys["octave"])
    assert np.array_equal(_u32(xy), _u32(np.stack([fs * keys["fcol"], fs * keys["frow"]], 1))), name
    assert np.array_equal(_u32(so), _u32(np.stack([fs * keys["fsize"], keys["ori"]], 1))), name
    same, ratio = _check_descriptors(run, keys, d, name)
    print(f"\n[sift descriptors] {name}: {len(keys)} keys, {same} descriptors bit-identical to the oracle's float32 ones, "
          f"largest error {ratio:.3g} of its bar")


def test_describe_hook_several_keys_per_workgroup(ctx, oracle):
    """(f2) A workgroup that describes more than one key (the ki += gridDim.x loop: in production only batches of five
    or more images with more than 1 024 keys in one of them): 64 keys of gray0 with the window sizes alternating largest,
    smallest, ... on 1, 3 and 64 workgroups are equal as bytes and within the bar; the mosaic's keys on the batch grid
    (1 024 workgroups, two or three keys each) are the extraction's own outputs as bytes."""
    gray, dbl, run = oracle("gray0")
    ctx.sift(gray, double_size=dbl)
    real = ctx.sift_debug_keys()
    by_size = real[np.argsort(real["fsize"], kind="stable")]
    n = len(by_size)
    alt = np.stack([by_size[::-1][:32], by_size[:32]], 1).reshape(-1)          # largest, smallest, 2nd largest, ...
    assert len(alt) == 64 and n >= 64 and _window_side(alt["fsize"][0]) >= 2 * _window_side(alt["fsize"][1])
    outs = {wg: ctx.sift_debug_describe(alt, workgroups=wg) for wg in (1, 3, 64)}
    for wg in (3, 64):
        for a, b, what in zip(outs[wg], outs[1], ("xy", "scale_ori", "descriptors")):
            assert a.tobytes() == b.tobytes(), f"{what} on {wg} workgroups differ from one workgroup's"
    k = _by_order(alt)
    fs = run.fscale(k["octave"])
    assert np.array_equal(_u32(outs[1][0]), _u32(np.stack([fs * k["fcol"], fs * k["frow"]], 1)))
    assert np.array_equal(_u32(outs[1][1]), _u32(np.stack([fs * k["fsize"], k["ori"]], 1)))
    _check_descriptors(run, k, outs[1][2], "gray0, 64 keys on one workgroup")
    # the hook left the extraction's keys alone
    assert ctx.sift_debug_keys().tobytes() == real.tobytes()

    gray, dbl, run = oracle("mosaic")
    xy, so, d = ctx.sift(gray, double_size=dbl)
    keys = ctx.sift_debug_keys()
    assert len(keys) == len(d) > 1536
    got = ctx.sift_debug_describe(keys, workgroups=1024)
    for a, b, what in zip(got, (xy, so, d), ("xy", "scale_ori", "descriptors")):
        assert a.tobytes() == b.tobytes(), f"mosaic: {what} on 1 024 workgroups differ from the extraction's"
    assert ctx.sift_debug_keys().tobytes() == keys.tobytes()


def test_describe_hook_refuses_what_it_cannot_run(ctx, oracle):
    gray, dbl, run = oracle("crop97x131_und")
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.MhError):                                     # no extraction yet
            fresh.sift_debug_describe(np.zeros(1, capi.SIFT_KEY_DTYPE))
    finally:
        fresh.close()
    ctx.sift(gray, double_size=dbl)
    keys = ctx.sift_debug_keys()
    assert len(keys) >= 2
    ctx.sift_debug_describe(keys[:2])
    with pytest.raises(capi.MhError):
        ctx.sift_debug_describe(keys[:2], slot=1)
    with pytest.raises(capi.MhError):
        ctx.sift_debug_describe(keys[:0])
    with pytest.raises(capi.MhError):
        ctx.sift_debug_describe(keys[:2], workgroups=-1)
    for field, value in (("octave", len(run.octaves)), ("octave", -1), ("index", 0), ("index", 4), ("order", keys["order"][0]),
                         ("fsize", 0.0), ("fsize", np.nan), ("ori", np.inf)):
        k = keys[:2].copy()
        k[field][1] = value
        with pytest.raises(capi.MhError):
            ctx.sift_debug_describe(k)


# Keys found by search on the host with desc_row_interval (moped_amd/csrc/sift_rows.h, as tests/native/sift_rows_check.cpp
# builds it) on a 119 x 159 level -- octave 3 of a doubled 640 x 480 frame: the number of samples describe_kernel WALKS (the
# sum of the rows' intervals; a step takes 256 of them, a wavefront 64) and, of those, the ones KeySample's tests select.
#   (fsize, frow, fcol, ori)                                 walked  selected  window side
STEP_KEYS = [
    ((2.03125, 130.671875, 163.0, -0.607421875),          #      40        21           45   one wavefront, not full
     "walk 40"),
    ((1.640625, 129.28125, 117.890625, -1.361328125),     #      63        41           35   one lane short of a wavefront
     "walk 63"),
    ((3.078125, -7.609375, 169.015625, 2.98828125),       #     255       220           67   one sample short of a step
     "walk 255"),
    ((1.453125, 119.984375, 130.25, 0.880859375),         #     256       201           31   exactly one step
     "walk 256"),
    ((1.875, -1.765625, 156.625, -2.90234375),            #     257       213           41   one sample in the second step
     "walk 257"),
    ((1.484375, 112.328125, 24.34375, 2.166015625),       #     511       420           33
     "walk 511"),
    ((3.75, 119.921875, -11.46875, 1.3046875),            #     512       455           81
     "walk 512"),
    ((1.5, 35.90625, 152.28125, 2.46875),                 #     513       422           33
     "walk 513"),
    ((4.03125, 125.953125, 1.265625, -1.603515625),       #     767       712           87
     "walk 767"),
    ((2.0, 79.625, 35.3125, -1.5556640625),               #   1 023       900           43
     "walk 1023"),
    ((3.40625, 125.5, 82.984375, -0.4560546875),          #   1 024       907           73
     "walk 1024"),
    ((2.1875, 24.203125, 146.203125, -0.0908203125),      #   1 025       943           47
     "walk 1025"),
    ((4.390625, 80.53125, 161.03125, -0.9716796875),      #   2 047     1 881           95
     "walk 2047"),
    ((3.5, 50.625, 115.75, 2.462890625),                  #   3 071     2 758           75
     "walk 3071"),
]
KPI = F32(3.141592654)


def _orientations():
    """What AssignOriHist can emit -- (i + peak) 2 pi / 36 + (pi / 36 - pi) for bins i = 0..35 and peak in [-0.5, 0.5], in
    float32 -- at the ends of that range, and 0, +-pi / 2; each with its two float neighbours."""
    forimult = F32(F32(2) * KPI / F32(36.0))
    foriadd = F32(F32(F32(0.5) * F32(2) * KPI / F32(36.0)) - KPI)
    ends = [F32(F32(F32(-0.5) * forimult) + foriadd), F32(F32(F32(35.5) * forimult) + foriadd)]
    assert abs(float(ends[0]) + np.pi) < 1e-6 and abs(float(ends[1]) - np.pi) < 1e-6
    out = []
    for v in ends + [F32(0.0), F32(KPI / F32(2)), F32(-KPI / F32(2))]:
        out += [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]
    return out


def _synthetic_keys(octaves, with_step_keys):
    """(names, keys) on the first octave of at most 160 columns: SIFT_KEY_DTYPE with descending `order` (the output order
    is the list's order)."""
    o = next(i for i, (r, c) in enumerate(octaves) if c <= 160)
    rows, cols = octaves[o]
    index = 1 + o % 3
    mr, mc = rows // 2 + 0.25, cols // 2 - 0.25
    # fsize = 1.6 powf(2, (index + X0) / 3) with index in 1..3 and |X0| <= 1.5 (InterpKeyPoint's final test)
    smallest, largest = F32(1.6) * F32(2.0) ** F32(-0.5 / 3), F32(1.6) * F32(2.0) ** F32(1.5)
    assert (_window_side(smallest), _window_side(largest)) == (31, 97)    # "side <= 97" in describe_kernel's comment
    items = []
    for a in _orientations():                                             # bin 7 wrapping to bin 0, the while wraps
        items.append((f"ori {a!r}", 2.0, mr, mc, a))
    below = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))
    for label, fr, fc in (
            ("top", 2.25, mc), ("bottom", rows - 3.25, mc), ("left", mr, 2.25), ("right", mr, cols - 3.25),
            ("top left", 2.25, 2.25), ("top right", 2.25, cols - 3.25), ("bottom left", rows - 3.25, 2.25),
            ("bottom right", rows - 3.25, cols - 3.25),
            ("rowstart 0", 0.25, mc), ("colstart cols - 1", mr, cols - 1.25), ("rowstart 0, colstart cols - 1", 0.25, cols - 1.25),
            ("frow .5", rows // 2 + 0.5, mc), ("frow just below .5", below(rows // 2 + 0.5), mc),
            ("fcol .5", mr, cols // 2 + 0.5), ("fcol just below .5", mr, below(cols // 2 + 0.5))):
        items.append((label, 2.0, fr, fc, 0.3))
    # sizes: the key stage's smallest and largest; 5.9 = the widest window the interval walk takes (side 127 <= DESC_MAX_SIDE);
    # 6.0 and 7.52 = the walk over the whole square by division -- ONLY this hook reaches it: no shipped key is that large
    for fsize, side in ((smallest, 31), (largest, 97), (5.9, 127), (6.0, 129), (7.52, 161)):
        assert _window_side(fsize) == side
        items.append((f"side {side}", fsize, mr, mc, -1.1))
        items.append((f"side {side} at the corner", fsize, rows - 3.25, 2.25, 2.0))
    if with_step_keys:
        assert (rows, cols) == (119, 159)
        items += [(label, *k) for k, label in STEP_KEYS]
    keys = np.zeros(len(items), capi.SIFT_KEY_DTYPE)
    keys["octave"], keys["index"] = o, index
    keys["order"] = np.arange(len(items), 0, -1)
    for f, col in (("fsize", 1), ("frow", 2), ("fcol", 3), ("ori", 4)):
        keys[f] = [it[col] for it in items]
    return [it[0] for it in items], keys


@pytest.mark.parametrize("name", ["gray0", "crop8x8", "crop97x131_und"])
def test_describe_hook_synthetic_keys_at_the_edges(ctx, oracle, name):
    """(f3) Keys the bundled frames need not contain, through the hook on this input's pyramid (crop8x8: 14 x 14, every
    window larger than the image), each within its bar, on the production grid and with two workgroups for all of them:
    orientations at the ends of AssignOriHist's range and on the axes, windows cut by every side and corner, rowstart 0,
    colstart cols - 1, centre fractions of .5, the smallest and largest size, walk totals at the edges of a 256-sample
    step, and the whole-square walk of windows wider than DESC_MAX_SIDE."""
    gray, dbl, run = oracle(name)
    ctx.sift(gray, double_size=dbl)
    names, keys = _synthetic_keys(run.octaves, with_step_keys=name == "gray0")
    fs = run.fscale(keys["octave"])
    first = None
    for wg in (0, 2):
        xy, so, d = ctx.sift_debug_describe(keys, workgroups=wg)
        assert np.array_equal(_u32(xy), _u32(np.stack([fs * keys["fcol"], fs * keys["frow"]], 1)))
        assert np.array_equal(_u32(so), _u32(np.stack([fs * keys["fsize"], keys["ori"]], 1)))
        if first is None:
            first = d
            same, ratio = _check_descriptors(run, keys, d, f"{name}, production grid", names)
            print(f"\n[sift descriptors] {name}: {len(keys)} synthetic keys, {same} bit-identical to the oracle's float32 "
                  f"ones, largest error {ratio:.3g} of its bar")
        else:
            assert d.tobytes() == first.tobytes(), f"{name}: two workgroups give other descriptors than {len(keys)}"
