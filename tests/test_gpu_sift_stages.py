"""FEAT stage by stage: the pyramid, the extrema and the keys the HIP SIFT kernels leave on the device
(mh_sift_debug_*) against the same stages of ONE oracle run (orclib.SiftRun; the oracle's final list is the reference's
libsiftfast build bit for bit, tests/test_sift_cpu.py, and its stage dump is tied to that list by
tests/test_sift_stages_cpu.py).

Prepare, the blur chain, DoG, the 2:1 subsample, the extremum scan, the edge test, the quadratic fit and the
first-claim rule contain no transcendental function on the device (the Gaussian taps come from the host's libm), so
(a), (b), (d) and (e) hold bit for bit; only orient_kernel's powf / expf / atan2f may differ from libm, and (c) says by
how much.  tests/test_gpu_sift.py keeps the final list (order, descriptors) with its statistical bars."""
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
