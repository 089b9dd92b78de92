"""POSE's refine arithmetic: the float32 restatement (tests/pose_ref.py) that the device is held to bit for bit
(tests/test_gpu_pose_rows.py) is itself held here, without a GPU, to the oracle's residual functions (which
test_ref_steps_cpu pins to the reference's classes) and to float64.

What is compared, over every non-edge case of tests/pose_cases.py, all six (kind, res) pairs and both phases:
  oracle   phase-1 rows == orclib.residuals / residuals_images / residuals_depth at the same pose given as a
           quaternion, for every entry at least 0.2 m in front of OR behind its camera
  square   phase-0 rows squared (res 1: the three ray-normal rows summed) == the same oracle rows, entries in front
  cd       J == central differences (h = 1e-6) of the float64 twin's rows in (omega, dt), R <- exp(omega) R, entries in front
  pen      J on the penalty rows of entries behind the camera: exactly 0
  twin     float32 rows and J against the float64 twin (rounding only; not a semantic check)
  H, g, cost   against hs J64^T J64, J64^T r64, r64 . r64 formed by numpy from the twin's rows
NORMALISATION.  A row word is divided by the largest magnitude that row index takes in float64 over the whole case set
(for that kind, res, phase); a J word by the largest of its (row, column).  H[(a,b)] by sqrt(H_aa H_bb), g[a] by
sqrt(H_aa cost), cost by cost (Cauchy-Schwarz: what each sum can reach).
BARS are measured, not chosen: RECORDED holds the largest normalised difference of each check over the case set as
measured with this file (python tests/test_pose_ref_cpu.py prints them); a check's bar is 100 x that, and every semantic
mutant of MUTANTS must exceed TEN bars on at least one case of every (kind, res, phase) it touches.

Recorded (float32 restatement, x86-64, numpy): see RECORDED below; smallest multiple of the bar each mutant reached, over
the (kind, res, phase) it touches: see MUTANT_REACH below (written by the same run).  Order mutants: seq_wave_sum first
differs on case n63 (156 case x combination in all), chunked on n65 (132), in cost, H or g words.
Before residual_rows<2> kept the reference's depth row behind the camera (`res2_penalty_row`), `oracle` was red for
(2, 2, phase 1) on the behind cases with weight3D != 0 (alpha 0 and 0.5) -- and for nothing else.

solve6 / rotate_left (not reproducible in numpy: v_rsq_f32, sinf, cosf): bar per output word =
2 (e_ref + e_pert) + 2^-23 max|output| with e_ref = |float32 restatement - float64|, e_pert = the largest
|perturbed restatement - float64| (reciprocal square roots +-1 float, sinf / cosf +-FSIZE_ULP_BOUND floats).  Width of
that bar relative to max|output|, over the 240 steps: see STEP_BAR_RECORDED.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import orclib  # noqa: E402
import pose_cases as pc  # noqa: E402
import pose_ref as pr  # noqa: E402

F = np.float32
FSIZE_ULP_BOUND = 4   # tests/test_gpu_sift_stages.py: the project's bound on the device's transcendentals, in floats
COMBOS = [(k, r, ph) for (k, r) in pr.PAIRS for ph in (0, 1)]
SEMANTIC = [c["name"] for c in pc.CASES if c["family"] != "edge"]
FAR = 0.2   # m: the semantic comparisons leave out what is closer to the camera's plane

# largest normalised difference of each check over the case set, measured (see the docstring)
RECORDED = {"oracle": 2.84e-07, "square": 3.26e-07, "cd": 4.38e-05, "pen": 0.0, "twin_r": 6.14e-07, "twin_J": 4.38e-05,
            "H": 2.77e-04, "g": 1.23e-04, "cost": 1.54e-04}
# the smallest multiple of its check's bar (100 x RECORDED) each semantic mutant reached over the (kind, res, phase) it
# touches (>= 10 asked; inf: a bar of 0 -- the penalty rows' J is exactly 0 -- exceeded)
MUTANT_REACH = {"swap_w": 258, "alpha": 258, "no50": 197, "f50_outside": 1.39e+03, "gw_cross_y": 458, "rc_transposed": 450,
                "iz_missing": 49.7, "tc_kept": 356, "cam0": 1.93e+10, "no2": 115, "pen_grad": float("inf"), "swap_H": 26.1,
                "hs_on_g": 33.3, "hs_depth": 18.1}
STEP_BAR_RECORDED = {"widest dx bar / max|dx|": 4.75e-06, "steps": 240}   # rotate_left alone: 1.1e-7 .. 1.1e-6 (printed)


def args(name, kind):
    c = pc.BY_NAME[name]
    return dict(alpha=c["alpha"], R=c["R"], t=c["t"], cams=pc.devcams(c["cams"]), pts=pc.points(c, kind), lst=c["lst"])


@functools.lru_cache(None)
def oracle_rows(name, kind, res):
    """The oracle's phase-1 rows of every list entry -> float64 [n, 2 | 3]."""
    c = pc.BY_NAME[name]
    lst = c["lst"]
    p7 = pc.pose7(c)
    K0, cam0 = c["cams"][0]
    if res == 3:
        hx = orclib.residuals_images(p7, c["uv3"][lst], c["xyz3"][lst], c["img"][lst], [k for k, _ in c["cams"]],
                                     [m for _, m in c["cams"]])
        return hx.reshape(-1, 2).astype(np.float64)
    if res == 0:
        return orclib.residuals(p7, c["uv"][lst], c["xyz"][lst], K0, cam0).reshape(-1, 2).astype(np.float64)
    W = c["W1"] if res == 1 else c["W2"]
    e = orclib.residuals_depth(res, p7, c["uv"][lst], c["xyz"][lst], W[lst], c["wgt"][lst], K0, cam0, c["alpha"])
    return e.reshape(len(lst), -1).astype(np.float64)


def _exp(w):
    return pr.rodrigues(w)


@functools.lru_cache(None)
def ref(name, kind, res, phase):
    """The float64 twin's rows and J, J by central differences, the normal equations formed by numpy, the masks."""
    a = args(name, kind)
    nr, r, J = pr.residual_rows(kind, res, phase, dtype=np.float64, **a)
    R0, t0 = a["R"].astype(np.float64).reshape(3, 3), a["t"].astype(np.float64)
    h = 1e-6
    cd = np.zeros_like(J)
    for k in range(6):
        e = np.zeros(3)
        e[k % 3] = h
        rr = []
        for s in (1, -1):
            Rk, tk = (_exp(s * e) @ R0, t0) if k < 3 else (R0, t0 + s * e)
            rr.append(pr.residual_rows(kind, res, phase, dtype=np.float64, **dict(a, R=Rk.reshape(9), t=tk))[1])
        cd[:, :, k] = (rr[0] - rr[1]) / (2 * h)
    d = pc.depth64(pc.BY_NAME[name], kind)
    hs = 1.5 if (phase == 1 and res in (0, 3)) else 1.0
    Jf = J[:, :nr].reshape(-1, 6)
    rf = r[:, :nr].reshape(-1)
    with np.errstate(all="ignore"):
        HH = hs * (Jf.T @ Jf)
        gg = Jf.T @ rf
    return dict(nr=nr, r=r, J=J, cd=cd, front=d >= FAR, far=np.abs(d) >= FAR, behind=d <= -FAR,
                H=np.array([HH[i, j] for i, j in pr.H_PAIRS]), g=gg, cost=float(rf @ rf))


@functools.lru_cache(None)
def scales(kind, res, phase):
    """The largest float64 magnitude of every row index / J (row, column) over the semantic cases."""
    Sr, SJ = np.zeros(4), np.zeros((4, 6))
    for name in SEMANTIC:
        q = ref(name, kind, res, phase)
        if q["far"].any():
            Sr = np.maximum(Sr, np.abs(q["r"][q["far"]]).max(axis=0))
        if q["front"].any():
            SJ = np.maximum(SJ, np.abs(q["J"][q["front"]]).max(axis=0))
    Sr[Sr == 0] = 1.0
    SJ[SJ == 0] = 1.0
    return Sr, SJ


@functools.lru_cache(None)
def rows32(name, kind, res, phase, mut=None, legacy=False):
    return pr.residual_rows(kind, res, phase, mut=mut, res2_penalty_row=legacy, **args(name, kind))


def _squares(res, r):
    """Phase-0 rows -> what the phase-1 rows are: their squares (res 1: dxy^2 is the sum of three)."""
    q = r.astype(np.float64) ** 2
    if res == 1:
        return np.stack([q[:, 0] + q[:, 1] + q[:, 2], q[:, 3]], axis=1)
    return q[:, :3 if res == 2 else 2]


def _mx(x):
    x = np.asarray(x)
    return float(np.nanmax(x)) if x.size and not np.all(np.isnan(x)) else (float("nan") if x.size else 0.0)


def row_deviations(name, kind, res, phase, mut=None, legacy=False):
    """check -> largest normalised difference on this case (a NaN where none belongs counts as infinite)."""
    q = ref(name, kind, res, phase)
    nr, r, J = rows32(name, kind, res, phase, mut, legacy)
    Sr, SJ = scales(kind, res, phase)
    S1 = scales(kind, res, 1)[0]
    orc = oracle_rows(name, kind, res)
    m = orc.shape[1]
    out = {}
    with np.errstate(all="ignore"):
        if phase == 1:
            out["oracle"] = _mx(np.abs(r[q["far"], :m] - orc[q["far"]]) / S1[:m])
        else:
            out["square"] = _mx(np.abs(_squares(res, r)[q["front"]] - orc[q["front"]]) / S1[:m])
        out["cd"] = _mx(np.abs(J[q["front"]] - q["cd"][q["front"]]) / SJ)
        pen_rows = nr if res != 2 else 2
        out["pen"] = _mx(np.abs(J[q["behind"], :pen_rows]) / SJ[:pen_rows])
        if mut is None and not legacy:
            out["twin_r"] = _mx(np.abs(r[q["far"]] - q["r"][q["far"]]) / Sr)
            out["twin_J"] = _mx(np.abs(J[q["front"]] - q["J"][q["front"]]) / SJ)
    return {k: (float("inf") if np.isnan(v) else v) for k, v in out.items()}


@functools.lru_cache(None)
def sums32(name, kind, res, phase, mut=None):
    nr, r, J = rows32(name, kind, res, phase)
    H, g = pr.normal_equations(res, phase, nr, r, J, mut)
    return H, g, pr.lm_cost(nr, r, mut)


def sum_deviations(name, kind, res, phase, mut=None):
    q = ref(name, kind, res, phase)
    H, g, cost = sums32(name, kind, res, phase, mut)
    d = np.array([q["H"][k] for k in (0, 6, 11, 15, 18, 20)])
    with np.errstate(all="ignore"):
        sH = np.array([np.sqrt(d[a] * d[b]) for a, b in pr.H_PAIRS])
        out = {"H": _mx(np.abs(H - q["H"]) / sH), "g": _mx(np.abs(g - q["g"]) / np.sqrt(d * q["cost"])),
               "cost": abs(float(cost) - q["cost"]) / q["cost"]}
    return {k: (float("inf") if np.isnan(v) else v) for k, v in out.items()}


def front_only(name):
    return pc.BY_NAME[name]["family"] == "front"


def measure():
    """-> the largest deviation of every check over the case set (the unmutated restatement)."""
    rec = {}
    for name in SEMANTIC:
        for k, r, ph in COMBOS:
            d = row_deviations(name, k, r, ph)
            if front_only(name):   # (sums over penalty rows of 10 .. 11 are not what H, g are for; the GPU holds them bit for bit)
                d.update(sum_deviations(name, k, r, ph))
            for c, v in d.items():
                rec[c] = max(rec.get(c, 0.0), v)
    return rec


def touches(mut, kind, res, phase):
    return {"swap_w": res in (1, 2), "alpha": res in (1, 2), "no50": res == 2, "f50_outside": res == 2 and phase == 0,
            "gw_cross_y": True, "rc_transposed": True, "iz_missing": res in (0, 2, 3), "tc_kept": True, "cam0": kind == 3,
            "no2": phase == 1, "pen_grad": True, "swap_H": True, "hs_on_g": phase == 1 and res in (0, 3),
            "hs_depth": phase == 1 and res in (1, 2)}[mut]


def reach(mut, kind, res, phase):
    """The largest multiple of its bar that any check reaches for this mutant on any case (inf: a bar of 0 exceeded)."""
    best = 0.0
    for name in SEMANTIC:
        if mut in pr.ROW_MUTANTS:
            d = row_deviations(name, kind, res, phase, mut)
        elif front_only(name):
            d = sum_deviations(name, kind, res, phase, mut)
        else:
            continue
        for c, v in d.items():
            bar = 100.0 * RECORDED[c]
            best = max(best, (float("inf") if v > 0 else 0.0) if bar == 0 else v / bar)
    return best


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_case_set_holds_what_it_promises():
    names = [c["name"] for c in pc.CASES]
    assert sorted(len(pc.BY_NAME[f"n{n}"]["lst"]) for n in pc.LENGTHS) == sorted(pc.LENGTHS)
    assert {c["alpha"] for c in pc.CASES} == {0.0, 0.5, 1.0} and {c["px"] for c in pc.CASES} == {0.3, 50.0}
    assert len(set(pc.BY_NAME["repeated65"]["lst"])) < 65 and not np.array_equal(pc.BY_NAME["sparse65"]["lst"], np.arange(65))
    assert not np.array_equal(np.sort(pc.BY_NAME["permuted129"]["lst"]), pc.BY_NAME["permuted129"]["lst"])
    for name in names:
        c = pc.BY_NAME[name]
        for kind in (0, 3):
            d = pc.depth64(c, kind)
            if c["family"] == "front":
                assert d.min() >= 0.29, (name, kind, d.min())
            if c["family"] == "behind":
                assert (d <= -0.29).sum() >= 20 and (d >= 0.29).sum() >= 40 and np.all(np.abs(d) >= 0.29), (name, kind)
        assert set(c["wgt"].tolist()) <= {F(0.0), F(0.3), F(1.0)}


@pytest.mark.parametrize("kind,res,phase", COMBOS)
def test_rows_jacobians_and_sums_against_oracle_and_float64(kind, res, phase):
    worst = {}
    for name in SEMANTIC:
        d = row_deviations(name, kind, res, phase)
        if front_only(name):
            d.update(sum_deviations(name, kind, res, phase))
        for c, v in d.items():
            if not v <= 100.0 * RECORDED[c]:
                worst[(name, c)] = v
    print(kind, res, phase, "largest:", {c: max(row_deviations(n, kind, res, phase).get(c, 0) for n in SEMANTIC)
                                          for c in ("oracle", "square", "cd", "twin_r", "twin_J")})
    assert not worst, f"beyond 100 x the recorded rounding difference: {worst}"


def test_recorded_differences_are_the_measured_ones():
    """RECORDED is what this file measures, not a choice: what a run measures lies between half and 1.5 times each value
    (room for another libm or compiler behind numpy and the oracle; the bars themselves are 100 x)."""
    rec = measure()
    for c, v in RECORDED.items():
        assert v * 0.5 <= rec[c] <= v * 1.5, (c, v, rec[c])


def test_the_form_before_the_fix_is_red_for_res_2_behind_the_camera_and_nothing_else():
    for kind, res, phase in COMBOS:
        for name in SEMANTIC:
            d = row_deviations(name, kind, res, phase, legacy=True)
            c = "oracle" if phase == 1 else "square"
            red = d[c] > 100.0 * RECORDED[c]
            c_ = pc.BY_NAME[name]   # (alpha = 1: weight3D = 0, the third row is 0 in either form)
            assert red == (res == 2 and phase == 1 and c_["family"] == "behind" and c_["alpha"] != 1.0), (kind, res, phase, name, d)


@pytest.mark.parametrize("mut", pr.ROW_MUTANTS + pr.NE_MUTANTS)
def test_semantic_mutants_exceed_ten_bars(mut):
    got = {(k, r, ph): reach(mut, k, r, ph) for k, r, ph in COMBOS if touches(mut, k, r, ph)}
    print(mut, "smallest multiple of the bar:", min(got.values()))
    assert got and all(v >= 10.0 for v in got.values()), {k: v for k, v in got.items() if not v >= 10.0}
    for k, r, ph in COMBOS:   # and leaves alone what it does not touch
        if not touches(mut, k, r, ph):
            assert reach(mut, k, r, ph) <= 1.0, (mut, k, r, ph)


def test_order_mutants_change_words():
    """Only this makes the GPU's bit equality a statement about the tree and the stride."""
    for mut, need_long in (("seq_wave_sum", False), ("chunked", True)):
        differ = []
        for name in SEMANTIC:
            n = len(pc.BY_NAME[name]["lst"])
            if need_long and n <= 64:
                continue
            for k, r, ph in COMBOS:
                a, b = sums32(name, k, r, ph), sums32(name, k, r, ph, mut)
                if not all(pr.same_words(x, y) for x, y in zip(a, b)):
                    differ.append((name, k, r, ph))
        assert differ, mut
        print(mut, "first differs on", differ[0], "and on", len(differ), "case x combination in all")
    for n in (1, 3, 64):   # a list that fits one pass: chunks of one entry ARE the stride
        a, b = sums32(f"n{n}", 0, 0, 1), sums32(f"n{n}", 0, 0, 1, "chunked")
        assert all(pr.same_words(x, y) for x, y in zip(a, b)) == (n != 3 or True)


def test_edge_rows_by_hand():
    """|c[2]| <= 1e-9 (and -0.): the penalty 10 - c[2] times the row's weight, no gradient -- the project's documented
    departure where the reference divides by zero; res 2 keeps its depth row.  The float above 1e-9 takes the ordinary
    branch.  Kind 1 with W = 0: NaN rows."""
    c = pc.BY_NAME["edge"]
    z = c["xyz"][:, 2]
    for kind, res in pr.PAIRS:
        for phase in (0, 1):
            nr, r, J = pr.residual_rows(kind, res, phase, **args("edge", kind))
            w3 = (F(1) - F(c["alpha"])) * c["wgt"] if res in (1, 2) else np.zeros(6, F)
            w2 = F(1) - w3
            for i in range(3):
                pen = -z[i] + F(10)
                for a in range(nr if res != 2 else 2):
                    wgt = w3[i] if (res == 1 and a == nr - 1) else w2[i]
                    want = pen * (np.sqrt(wgt) if phase == 0 else wgt)
                    assert r[i, a].view(np.uint32) == F(want).view(np.uint32), (kind, res, phase, i, a)
                    assert not J[i, a].any()
            if res == 2:
                X = c["xyz"].astype(F)
                W = c["W2"]
                for i in range(3):
                    pw = X[i, 0] * W[i, 0] + X[i, 1] * W[i, 1] + X[i, 2] * W[i, 2] - F(1)
                    n2 = X[i, 0] * X[i, 0] + X[i, 1] * X[i, 1] + X[i, 2] * X[i, 2]
                    want = (np.sqrt(F(50) * w3[i]) * np.sqrt(n2) * pw) if phase == 0 else (F(50) * w3[i] * n2 * pw * pw)
                    assert r[i, 2].view(np.uint32) == F(want).view(np.uint32) and J[i, 2].any(), (phase, i)
            if res in (0, 2, 3):   # just above 1e-9: the projection branch (1 / c[2] = 1e9: enormous, finite)
                K = c["cams"][0][0]
                iz = F(1) / z[3]
                du = c["xyz"][3, 0] * iz * K[0] + K[2] - c["uv"][3, 0]
                s0 = np.sqrt(w2[3]) if phase == 0 else w2[3]
                want = s0 * du if phase == 0 else s0 * du * du
                assert r[3, 0].view(np.uint32) == F(want).view(np.uint32) and np.isfinite(r[3, 0]) and abs(r[3, 0]) > 1e6
            assert np.all(np.isfinite(r[4, :nr])) and np.all(np.isfinite(J[4, :nr]))
            if res == 1:
                assert np.all(np.isnan(r[5, :nr])) and np.all(np.isnan(J[5, :nr]))
            else:
                assert np.all(np.isfinite(r[5, :nr]))


# ---- solve6, rotate_left ------------------------------------------------------------------------------------------------
def step_cases():
    """(label, H, g, mu, R, t): H + mu I of every front case with n >= 6, every (kind, res, phase), the two dampings."""
    out = []
    for name in SEMANTIC:
        c = pc.BY_NAME[name]
        if not front_only(name) or len(set(c["lst"].tolist())) < 6:
            continue
        for k, r, ph in COMBOS:
            H, g, _ = sums32(name, k, r, ph)
            mx = max(F(0), *[H[i] for i in (0, 6, 11, 15, 18, 20)])
            for tau in (F(1e-3), F(1e-7)):
                out.append((f"{name}/{k}{r}{ph}/{tau:g}", H, g, F(tau * mx), c["R"], c["t"]))
    return out


def step_bar(H, g, mu, R, t):
    """-> (f64 words [18], bar [18], restatement words [18]): dx | Rn | tn."""
    def words(x):
        return np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in x[1:]])
    f64 = words((True,) + pr.step_f64(H, g, mu, R, t))
    ref32 = pr.debug_step(H, g, mu, R, t)
    assert ref32[0]
    e_ref = np.abs(words(ref32) - f64)
    e_pert = np.zeros(18)
    for ps in (1, -1):
        for pt in (FSIZE_ULP_BOUND, -FSIZE_ULP_BOUND):
            e_pert = np.maximum(e_pert, np.abs(words(pr.debug_step(H, g, mu, R, t, pert_rsq=ps, pert_trig=pt)) - f64))
    scale = np.concatenate([np.full(6, np.abs(f64[:6]).max()), np.full(9, np.abs(f64[6:15]).max()), np.full(3, np.abs(f64[15:]).max())])
    return f64, 2 * (e_ref + e_pert) + 2.0 ** -23 * scale, words(ref32), scale


def test_solve6_mutants_exceed_the_step_bar_on_every_case():
    widest, noticed = 0.0, 0
    cases = step_cases()
    assert len(cases) >= 200
    for label, H, g, mu, R, t in cases:
        f64, bar, got, scale = step_bar(H, g, mu, R, t)
        assert np.all(np.abs(got - f64) <= bar)
        widest = max(widest, float((bar[:6] / scale[:6]).max()))
        for mut in ("drop_term", "plus_g"):
            ok, dx, _, _ = pr.debug_step(H, g, mu, R, t, mut=mut)
            # (noticed either way: by a flag that differs from the restatement's, or by a dx word beyond its bar)
            assert not ok or np.any(np.abs(dx - f64[:6]) > bar[:6]), (label, mut, np.abs(dx - f64[:6]) / bar[:6])
            noticed += 1
    print("widest dx bar / max|dx|:", widest, "steps:", len(cases), "mutant runs noticed:", noticed)


ROT_MAGNITUDES = (0.0, 5e-5, float(np.nextafter(F(1e-4), F(0))), float(np.nextafter(F(1e-4), F(1))), 1e-3, 0.1, 1.0, 3.0)


def test_rotate_left_at_every_magnitude_and_its_mutants():
    R = pc.BY_NAME["n3"]["R"]
    axis = np.array([0.6, -0.3, 0.74])
    axis /= np.linalg.norm(axis)
    for mag in ROT_MAGNITUDES:
        w = (axis * mag).astype(F)
        f64 = (pr.rodrigues(w.astype(np.float64)) @ R.astype(np.float64).reshape(3, 3)).reshape(9)
        got = pr.rotate_left(w, R)
        e_pert = np.zeros(9)
        for pt in (FSIZE_ULP_BOUND, -FSIZE_ULP_BOUND):
            e_pert = np.maximum(e_pert, np.abs(pr.rotate_left(w, R, pert=pt) - f64))
        bar = 2 * (np.abs(got - f64) + e_pert) + 2.0 ** -23 * np.abs(f64).max()
        assert np.all(np.abs(got - f64) <= bar)
        print(f"|w| = {mag:g}: bar {bar.max():.3g}")
        # the transpose of [w]x is exp(-w): shows wherever w is not 0.  b with th for th2 shows once b [w]x^2 is more than
        # a float of the result and th != th^2: from 0.1 on, not at 1 (and not on the series branch, which has no th)
        if mag > 0:
            assert np.any(np.abs(pr.rotate_left(w, R, mut="transpose_K") - f64) > bar), mag
        if mag in (0.1, 3.0):
            assert np.any(np.abs(pr.rotate_left(w, R, mut="b_th") - f64) > bar), mag
    thf = np.sqrt(F(np.sum((axis * ROT_MAGNITUDES[2]).astype(F) ** 2)))
    assert thf < F(1e-4) <= np.sqrt(F(np.sum((axis * ROT_MAGNITUDES[3]).astype(F) ** 2)))   # the two sides of the branch


def test_solve6_refuses_a_zero_or_negative_pivot():
    H = np.zeros(21, F)
    for k in (0, 6, 11, 15, 18, 20):
        H[k] = 1
    g = np.ones(6, F)
    assert pr.solve6(H, g, F(0))[0]
    for k, name in ((11, "zero"), (15, "negative")):
        Hb = H.copy()
        Hb[k] = 0 if name == "zero" else -2
        assert not pr.solve6(Hb, g, F(0))[0] and not pr.solve6(Hb, g, F(0), dtype=np.float64)[0]
    Hb = H.copy()
    Hb[1] = 2   # |off-diagonal| > diagonal: the second pivot 1 - 4 < 0
    assert not pr.solve6(Hb, g, F(0))[0] and pr.solve6(Hb, g, F(3.5))[0]
    Hn = H.copy()
    Hn[0] = np.nan
    assert not pr.solve6(Hn, g, F(0))[0]


if __name__ == "__main__":
    rec = measure()
    print("RECORDED =", {k: float(f"{v:.3g}") for k, v in rec.items()})
    RECORDED.update(rec)
    for mut in pr.ROW_MUTANTS + pr.NE_MUTANTS:
        got = {c: reach(mut, *c) for c in COMBOS if touches(mut, *c)}
        print(f'    "{mut}": {min(got.values()):.3g},')
