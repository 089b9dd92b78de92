"""Pass C's proof that the ratio test rejects a query (csrc/screen.h: screen_reject_proved, exported as
mh_screen_reject_proved), checked in host arithmetic against the oracle.

The function sees of a query: qq, Dmax, h1 >= every screen value w~ of the DB (or tau, whichever is larger), l2 <= the second
largest w~ over distinct rows, and the ratio.  It may say "rejected" only if no exact arithmetic accepts the query:
the oracle's match_2nn gives (idx1, d1, d2) by the canonical chain, acceptance is `idx1 >= 0 and f32(d1 / d2) < ratio`
(MATCH_ANN_CPU.hpp:165; numpy's float32 division is the correctly rounded one match_accepted uses).

Here the screen values are made from the canonical w = p - dd / 2 (p the f32 fmaf chain the distances come from) by moving
every row's value by the whole proved per-value bound E = (mh_screen_margin - 2e-6 (qq + Dmax^2)) / 2 in the direction
that helps a wrong proof most: the best row's DOWN (the query looks farther from its nearest row than it is), every other
row's UP (the second nearest looks nearer) -- the screen's own error (tests/test_screen_bound_cpu.py holds it inside E) can
do no worse.  h1 and l2 are then the largest and the second largest of these values, as tight as records can make them."""
import numpy as np
import pytest

import accept_model
import orclib
from moped_amd import capi, synth

RATIOS = (0.5, 0.8, 0.99, 1.0, 1.5)


def _chain_f32(q, d):
    """p[i, j] = f32 fmaf chain over k of q[i, k] * d[j, k] (product exact in f64, one rounding per step)."""
    s = np.zeros((q.shape[0], d.shape[0]), np.float32)
    for k in range(q.shape[1]):
        s = (q[:, k:k + 1].astype(np.float64) * d[None, :, k].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def _value_err(qq, dmax):
    L = capi.load()
    m = float(L.mh_screen_margin(np.float32(qq), np.float32(dmax)))
    return 0.5 * (m - 2e-6 * (float(qq) + float(dmax) ** 2))


def _accepted(idx, d1, d2, ratio):
    with np.errstate(all="ignore"):
        return (idx >= 0) & ((d1.astype(np.float32) / d2.astype(np.float32)) < np.float32(ratio))


def _check(name, q, d, ratios=RATIOS):
    """No (query, ratio) is proved rejected that the oracle accepts.  Returns (proved, total) for the caller's floor."""
    q, d = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(d, np.float32)
    idx, d1, d2 = orclib.match_2nn(d, q)
    dd, qq = orclib.row_norms(d), orclib.row_norms(q)
    dmax = float(np.sqrt(dd.max()))
    w = _chain_f32(q, d).astype(np.float64) - 0.5 * dd.astype(np.float64)[None, :]
    proved = total = 0
    for i in range(len(q)):
        E = _value_err(qq[i], dmax)
        best = int(idx[i])
        wt = w[i] + E
        wt[best] = w[i, best] - E
        top2 = np.sort(wt)[-2:]
        h1, l2 = float(top2[1]), float(top2[0])
        margin = float(capi.load().mh_screen_margin(np.float32(qq[i]), np.float32(dmax)))
        for ratio in ratios:
            ok = bool(_accepted(idx[i:i + 1], d1[i:i + 1], d2[i:i + 1], ratio)[0])
            # thresholds: one margin below the second largest value (pass A's rule at its tightest), far below, and --
            # a threshold no row of the best's record exceeds cannot be, so none above l2
            for tau in (l2 - margin, l2 - 0.3, l2):
                # float32 arguments rounded OUTWARD: h1 up, l2 down stay valid bounds of the values above
                a_h1 = np.nextafter(np.float32(h1), np.float32(np.inf)) if np.float32(h1) < h1 else np.float32(h1)
                a_l2 = np.nextafter(np.float32(l2), np.float32(-np.inf)) if np.float32(l2) > l2 else np.float32(l2)
                got = accept_model.reject_proved(qq[i], dmax, a_h1, a_l2, min(tau, float(a_l2)), ratio)
                assert not (got and ok), (name, i, ratio, tau, float(d1[i]), float(d2[i]), h1, l2)
                proved += got
                total += 1
    return proved, total


def _unit(rng, n):
    return orclib.normalize(np.abs(rng.normal(size=(n, 128))).astype(np.float32))


def _at_distance(rng, q, a):
    """A unit row at squared distance ~a from the unit row q: cos = 1 - a / 2, along a random direction orthogonal to q."""
    u = rng.normal(size=128)
    u -= u.dot(q) * q / q.dot(q)
    u /= np.linalg.norm(u)
    c = 1.0 - 0.5 * a
    return (c * q / np.linalg.norm(q) + np.sqrt(max(0.0, 1.0 - c * c)) * u).astype(np.float32)


def test_random_and_near_duplicate_rows():
    base, _, _ = synth.load_sift_fixture()
    rng = np.random.default_rng(3)
    unit = orclib.normalize(base[rng.choice(len(base), 700)])
    p1, t1 = _check("sift-like", unit[:100], unit[100:])
    b = unit[:40]
    rows = [b[k] + 10.0 ** rng.uniform(-5, -2, (12, 1)) * rng.normal(size=(12, 128)) for k in range(40)]
    d = orclib.normalize(np.ascontiguousarray(np.maximum(np.concatenate(rows), 0), np.float32))
    q = orclib.normalize(np.concatenate([b, b + rng.normal(0, 2e-4, b.shape)]).astype(np.float32))
    p2, t2 = _check("near-duplicates", q, d[rng.permutation(len(d))])
    print("proved: sift-like", p1, "of", t1, "near-duplicates", p2, "of", t2)
    assert p1 > 0      # (unrelated rows at ratio 0.5 / 0.8: d1 / d2 is near 1, the proof must find some of them)


@pytest.mark.parametrize("ratio", RATIOS)
def test_planted_ratios_on_either_side(ratio):
    """d1 / d2 planted within +-1e-6 .. +-1e-2 of the ratio, at several distances, the other rows far away."""
    rng = np.random.default_rng(int(ratio * 100))
    rest = _unit(rng, 200)
    qs, rows = [], []
    for a2 in (1e-3, 0.02, 0.3, 0.9):
        for rel in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
            for sign in (-1.0, 1.0):
                a1 = min(a2, a2 * ratio * (1.0 + sign * rel))     # (a ratio above 1 cannot be planted: d1 <= d2)
                q = _unit(rng, 1)[0]
                qs.append(q)
                rows += [_at_distance(rng, q, a1), _at_distance(rng, q, a2)]
    d = np.concatenate([np.asarray(rows, np.float32), rest])
    q = np.asarray(qs, np.float32)
    idx, d1, d2 = orclib.match_2nn(d, q)
    with np.errstate(all="ignore"):
        r = d1 / d2
    if ratio < 1.0:
        near = np.abs(r / ratio - 1.0)
        assert near.min() < 1e-4 and (r < ratio).any() and (r >= ratio).any(), (near.min(), r)   # the cases landed on both sides
    proved, total = _check("planted %g" % ratio, q, d, ratios=(ratio,))
    if ratio >= 1.0:
        assert proved == 0     # d1 <= d2: nothing fails a ratio >= 1 except d1 == d2, and the bounds never pin that


def test_zero_distances_and_scales_away_from_one():
    rng = np.random.default_rng(17)
    q = _unit(rng, 24)
    rest = _unit(rng, 300)
    # d1 = d2 = 0: two exact copies (the quotient is NaN: rejected at every ratio, provably or not); one copy: d1 = 0 accepts
    d = np.concatenate([q[:8], q[:8], q[8:16], rest])
    idx, d1, d2 = orclib.match_2nn(d, q)
    assert (d1[:8] == 0).all() and (d2[:8] == 0).all() and (d1[8:16] == 0).all() and (d2[8:16] > 0).all()
    _check("copies", q, d)
    # qq and Dmax away from 1, either way and both
    for sq, sd in ((0.5, 1.0), (3.0, 1.0), (1.0, 0.25), (1.0, 4.0), (0.3, 2.5), (2e-3, 1.0)):
        dq = (d * np.float32(sd)).astype(np.float32)
        dq[5:9] *= np.float32(0.5)                      # rows of different norms
        _check("scaled %g %g" % (sq, sd), (q * np.float32(sq)).astype(np.float32), dq)


def test_degenerate_arguments_prove_nothing():
    inf, nan = np.inf, np.nan
    p = accept_model.reject_proved
    assert p(1.0, 1.0, 0.1, 0.1, 0.0, 0.8)                      # d1 >= 0.8 - 2E.., d2 <= 0.8 + 2E..: rejected at 0.8
    assert not p(1.0, 1.0, 0.1, 0.1, 0.0, 1.0)                  # ... and not at 1: the bounds overlap
    assert not p(1.0, 1.0, 0.45, 0.1, 0.0, 0.8)                 # d1 may be 0.1
    assert not p(1.0, 1.0, 0.1, 0.1, 0.45, 0.8)                 # rows up to tau may exist outside the records
    for ratio in (0.0, -0.8, nan, inf):
        assert not p(1.0, 1.0, 0.1, 0.1, 0.0, ratio)
    assert not p(1.0, 1.0, 0.1, -inf, 0.0, 0.8)                 # fewer than two records
    assert not p(1.0, 1.0, inf, 0.1, 0.0, 0.8) and not p(1.0, 1.0, nan, 0.1, 0.0, 0.8)
    assert not p(nan, 1.0, 0.1, 0.1, 0.0, 0.8) and not p(1.0, inf, 0.1, 0.1, 0.0, 0.8) and not p(1.0, 1.0, 0.1, 0.1, nan, 0.8)
    assert not p(1.0, 1.0, 0.1, nan, 0.0, 0.8)
    assert not p(1.0, 1.0, 0.6, 0.6, 0.0, 0.8)                  # the upper bound of d2 is not positive


def test_margin_is_twice_the_value_bound_plus_the_norm_slack():
    """The per-value bound was factored out of screen_margin: the margin's bits are what the expression always gave."""
    L = capi.load()
    f = np.float32
    for qq, dmax in ((1.0, 1.0), (0.25, 1.0), (9.0, 2.5), (1e-6, 1.0), (0.0, 1.0), (1.0, 1e-3)):
        nq = np.sqrt(np.maximum(f(qq), f(0)))
        dm = f(dmax)
        E = f(f(f(f(0.000978) * nq) * dm) + f(f(4e-7) * f(nq + dm))) + f(f(3e-5) * f(f(nq * dm) + f(f(f(0.5) * dm) * dm)))
        want = f(f(f(2) * f(E)) + f(f(2e-6) * f(f(qq) + f(dm * dm))))
        got = f(L.mh_screen_margin(f(qq), f(dmax)))
        assert got.view(np.uint32) == want.view(np.uint32), (qq, dmax, float(got), float(want))


def test_share_proved_on_synth_frames():
    """What the early exit is worth on the benchmark's own data (ratio 0.8): printed, and bounded from below so that a
    function that proves nothing does not pass.  tests/test_gpu_accept_reject.py holds the device to 0.8 x this model.
    The floor: on these frames 12% of the queries are accepted and the rest have d1 / d2 near 1 (median d2 0.055); with the
    proved per-value bound (~1.0e-3 at qq = Dmax = 1) about two thirds of all queries are provable, and a bound half as
    large again (1.5e-3) would still leave 56% -- so anything below one half means the function lost more than that."""
    db, dbn, frames = accept_model.synth_frames()
    shares = [accept_model.predicted_share(qn, dbn, 0.8) for qn in frames]
    print("share of queries proved rejected at ratio 0.8, seeds 0..3:", ["%.3f" % s for s in shares])
    assert min(shares) > 0.5, shares
