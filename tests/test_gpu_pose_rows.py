"""POSE's LM refine on the device, word for word: what mh_pose_debug_rows returns -- the shipped residual_rows, lm_cost and
lm_refine's own normal equations on one wavefront -- equals the float32 numpy restatement (tests/pose_ref.py) as uint32
words, on every case of tests/pose_cases.py, all six (kind, res) pairs and both phases.  No tolerance: the arithmetic is
IEEE add / multiply / divide / sqrt without contraction, and the order of every sum is restated (lane l takes entries l,
l + 64, ...; wave_sum's tree).  A NaN equals any NaN.  tests/test_pose_ref_cpu.py holds the restatement to the oracle and
to float64, and shows that a sequential wave sum or contiguous chunks per lane would change words on these cases.

mh_pose_debug_step (solve6 with v_rsq_f32, rotate_left with sinf / cosf: not reproducible in numpy) is held to the float64
step within the bar test_pose_ref_cpu.step_bar derives from rounding (measured on an MI355X over the 240 steps: largest
|device - float64| = 0.65 of the bar); tn is t + dx[3..5] bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pose_cases as pc
import pose_ref as pr
import test_pose_ref_cpu as cpu
from moped_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(dev_words, want, what, where):
    got = np.ascontiguousarray(dev_words, np.uint32).view(F)
    want = np.ascontiguousarray(want, F)
    if not pr.same_words(got, want):
        bad = np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{where}: {what} differs in {len(bad)} of {got.size} words, first at {i}: device "
                             f"{got.reshape(-1)[i]!r} ({got.view(np.uint32).reshape(-1)[i]:#010x}), restatement "
                             f"{want.reshape(-1)[i]!r} ({want.view(np.uint32).reshape(-1)[i]:#010x})")


@pytest.mark.parametrize("kind,res,phase", cpu.COMBOS)
def test_rows_jacobians_cost_and_normal_equations_bit_for_bit(ctx, kind, res, phase):
    for c in pc.CASES:
        name = c["name"]
        where = f"{name} kind {kind} res {res} phase {phase}"
        a = cpu.args(name, kind)
        got = ctx.pose_debug_rows(kind, res, phase, a["alpha"], a["R"], a["t"], c["cams"], a["pts"], a["lst"])
        want = pr.debug_rows(kind, res, phase, **a)
        nr, n = want["nrows"], len(a["lst"])
        # the cameras the kernel got are the ones the restatement was given
        dc = np.concatenate(a["cams"], axis=1)
        assert np.array_equal(_u32(got["devcams"]), _u32(dc)), where
        assert np.array_equal(got["nrows"], np.full(n, nr, np.int32)), where
        _same(got["r"][:, :nr], want["r"][:, :nr], "r", where)
        _same(got["J"][:, :nr], want["J"][:, :nr], "J", where)
        assert np.all(got["r"][:, nr:] == capi.POSE_DEBUG_FILL) and np.all(got["J"][:, nr:] == capi.POSE_DEBUG_FILL), where
        _same(np.array([got["cost"]], np.uint32), [want["cost"]], "cost", where)
        _same(got["H"], want["H"], "H", where)
        _same(got["g"], want["g"], "g", where)


def test_step_within_the_rounding_bar_of_float64(ctx):
    cases = cpu.step_cases()
    worst = 0.0
    for label, H, g, mu, R, t in cases:
        f64, bar, _, _ = cpu.step_bar(H, g, mu, R, t)
        ok, dx, Rn, tn, agree = ctx.pose_debug_step(H, g, mu, R, t)
        assert ok == pr.solve6(H, g, mu)[0] and ok and agree, label
        got = np.concatenate([dx, Rn.reshape(9), tn]).astype(np.float64)
        worst = max(worst, float((np.abs(got - f64) / bar).max()))
        assert np.all(np.abs(got - f64) <= bar), (label, (np.abs(got - f64) / bar).max())
        assert np.array_equal(_u32(tn), _u32(np.asarray(t, F) + dx[3:])), label
    print(f"{len(cases)} steps, largest |device - float64| / bar: {worst:.3f}")


def test_rotate_left_on_both_sides_of_its_branch(ctx):
    """rotate_left through the step hook: with H = I and mu = 0 every reciprocal square root is that of 1, which is 1 on any
    hardware, so dx is the restatement's word for word (-g, but for the sign of a zero)."""
    H = np.zeros(21, F)
    H[[0, 6, 11, 15, 18, 20]] = 1
    R, t = pc.BY_NAME["n3"]["R"], pc.BY_NAME["n3"]["t"]
    axis = np.array([0.6, -0.3, 0.74])
    axis /= np.linalg.norm(axis)
    for mag in cpu.ROT_MAGNITUDES:
        w = (axis * mag).astype(F)
        g = np.concatenate([-w, F([0.5, -0.25, 0.125])]).astype(F)
        ok, dx, Rn, tn, agree = ctx.pose_debug_step(H, g, F(0), R, t)
        assert ok and agree and np.array_equal(_u32(dx), _u32(pr.solve6(H, g, F(0))[1])) and np.array_equal(dx, -g), mag
        w = dx[:3]
        f64 = (pr.rodrigues(w.astype(np.float64)) @ R.astype(np.float64).reshape(3, 3)).reshape(9)
        ref = pr.rotate_left(w, R)
        e_pert = np.zeros(9)
        for ptb in (cpu.FSIZE_ULP_BOUND, -cpu.FSIZE_ULP_BOUND):
            e_pert = np.maximum(e_pert, np.abs(pr.rotate_left(w, R, pert=ptb) - f64))
        bar = 2 * (np.abs(ref - f64) + e_pert) + 2.0 ** -23 * np.abs(f64).max()
        assert np.all(np.abs(Rn.reshape(9) - f64) <= bar), (mag, np.abs(Rn.reshape(9) - f64) / bar)
        if np.sqrt(F(np.sum(w * w))) < F(1e-4):   # the series branch has no transcendental in it: bit for bit
            assert np.array_equal(_u32(Rn.reshape(9)), _u32(ref)), mag


def test_step_reports_a_matrix_it_cannot_factor(ctx):
    H = np.zeros(21, F)
    H[[0, 6, 11, 15, 18, 20]] = 1
    g = np.ones(6, F)
    R, t = pc.BY_NAME["n3"]["R"], pc.BY_NAME["n3"]["t"]
    for k, v in ((11, 0.0), (15, -2.0), (1, 2.0), (0, np.nan)):
        Hb = H.copy()
        Hb[k] = v
        assert not pr.solve6(Hb, g, F(0))[0]
        ok, dx, Rn, tn, agree = ctx.pose_debug_step(Hb, g, F(0), R, t)
        assert not ok and agree
        assert np.all(_u32(dx) == capi.POSE_DEBUG_FILL) and np.all(_u32(Rn) == capi.POSE_DEBUG_FILL) and np.all(_u32(tn) == capi.POSE_DEBUG_FILL)


def test_pose_hooks_refuse_what_they_cannot_run(ctx):
    L, h = ctx.L, ctx.h
    c = pc.BY_NAME["n3"]
    P = capi._ptr
    SENT = 0x5A5A5A5A

    def call(kind=0, res=0, phase=1, n_images=3, pts=None, n_pts=None, lst=None, n=None, null=None):
        pts = pc.points(c, kind if kind in (0, 1, 2, 3) else 0) if pts is None else pts
        lst = c["lst"] if lst is None else np.ascontiguousarray(lst, np.int32)
        n_pts = len(pts) if n_pts is None else n_pts
        n = len(lst) if n is None else n
        cams = capi.make_cams([k for k, _ in c["cams"]], [m for _, m in c["cams"]])
        out = {k: np.full(s, SENT, np.uint32) for k, s in (("nrows", 8), ("r", 32), ("J", 192), ("cost", 1), ("H", 21), ("g", 6), ("dc", 128))}
        a = dict(R=P(c["R"]), t=P(c["t"]), cams=C.cast(cams, C.c_void_p), pts=P(pts), lst=P(lst), **{k: P(v) for k, v in out.items()})
        if null:
            a[null] = None
        rc = L.mh_pose_debug_rows(h, kind, res, phase, 0.5, a["R"], a["t"], a["cams"], n_images, a["pts"], n_pts, a["lst"], n,
                                  a["nrows"], a["r"], a["J"], a["cost"], a["H"], a["g"], a["dc"])
        return rc, out

    def refused(**kw):
        rc, out = call(**kw)
        assert rc == capi.MH_ERR_ARG, kw
        assert L.mh_last_error(h).decode().startswith("mh_pose_debug_rows: "), (kw, L.mh_last_error(h))
        assert all(np.all(v == SENT) for v in out.values()), kw

    rc, out = call()
    assert rc == 0 and not np.any(out["H"] == SENT)
    for name in ("R", "t", "cams", "pts", "lst", "nrows", "r", "J", "cost", "H", "g", "dc"):
        refused(null=name)
    for kw in (dict(n_pts=0), dict(n_pts=capi.POSE_MAX_PTS + 1), dict(n=0), dict(n=capi.POSE_MAX_PTS + 1), dict(n=-1),
               dict(lst=[0, 3, 1]), dict(lst=[0, -1, 1]), dict(n_images=0), dict(n_images=9), dict(kind=3, res=3, n_images=2),
               dict(kind=0, res=1), dict(kind=3, res=0), dict(kind=4, res=4), dict(kind=-1, res=-1), dict(kind=1, res=2),
               dict(phase=2), dict(phase=-1)):
        refused(**kw)
    bad = pc.points(c, 3).copy()
    bad[1, 5] = np.int32(-1).view(F)
    refused(kind=3, res=3, pts=bad)
    bad[1, 5] = np.int32(3).view(F)
    refused(kind=3, res=3, pts=bad)

    o = {k: np.full(s, SENT, np.uint32) for k, s in (("ok", 1), ("dx", 6), ("Rn", 9), ("tn", 3), ("agree", 1))}
    H, g = np.ones(21, F), np.ones(6, F)
    for null in ("H", "g", "R", "t", "ok", "dx", "Rn", "tn", "agree"):
        a = dict(H=P(H), g=P(g), R=P(c["R"]), t=P(c["t"]), **{k: P(v) for k, v in o.items()})
        a[null] = None
        assert L.mh_pose_debug_step(h, a["H"], a["g"], 0.5, a["R"], a["t"], a["ok"], a["dx"], a["Rn"], a["tn"], a["agree"]) == capi.MH_ERR_ARG
        assert L.mh_last_error(h).decode().startswith("mh_pose_debug_step: ")
        assert all(np.all(v == SENT) for v in o.values()), null
    assert L.mh_pose_debug_rows(None, 0, 0, 1, 0.5, *([None] * 3), 1, None, 1, None, 1, *([None] * 7)) == capi.MH_ERR_ARG
    # the context still works
    a = cpu.args("n3", 2)
    got = ctx.pose_debug_rows(2, 2, 1, a["alpha"], a["R"], a["t"], c["cams"], a["pts"], a["lst"])
    _same(got["H"], pr.debug_rows(2, 2, 1, **a)["H"], "H", "after the refusals")
