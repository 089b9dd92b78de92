"""MATCH for a caller that applies the ratio test (mh_match_set_accept; csrc/screen_rescore.hip: rescore_query's ACCEPT form):
pass C answers a query its records prove to fail `d1 / d2 < ratio` with (-1, inf, inf) and skips the search.

mh_match with mh_match_set_accept(0.8) against the same context in full mode, the exact matrix-pipe kernel
(mh_match_set_mode 3) and the oracle:
  (a) every query the full mode accepts at 0.8 has the same bits (idx1, d1, d2);
  (b) every other query has either those bits or (-1, inf, inf);
  (c) the queries answered (-1, inf, inf) that have a neighbour in full mode are exactly as many as mh_match_prerejected says;
  (d) queries planted at d1 / d2 = 0.8 (1 +- 1e-4) are never lost when accepted (a case of (a), on planted rows);
  (e) queries that are incomplete, whose lists overflowed, all-zero and non-finite ones keep the exact triple;
and the launch after it in full mode equals the exact kernel: every slot was left empty, every count zero.

Both record layouts, one after the other on one context: the counted lists of the 16x16x32 passes (12 288 queries, the
smallest launch that takes them -- which needs n_tiles x 12 >= 4 096, so it runs on the 20 x 5 000 DB, not on 16 384 rows)
and the lane-private slots of the 32x32x16 passes (3 000 queries), on the 20 x 5 000 DB and on a DB of 4 models x 4 096 rows.

Absent rows (norm term -1) and rows behind a device-side query count exist only in launches of the image entry points;
mh_match computes the norm terms itself and has no count.  Both leave rescore_query before it looks at a record.

Share: on the 20 x 5 000 DB, frames of seeds 0..3, at least 0.8 x what the host model predicts for the same frames
(tests/accept_model.py; 0.8 covers the records' f16 rounding and blocks that hold both top rows)."""
import numpy as np
import pytest

import accept_model
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
TILE = 128
RATIO = 0.8
Q_LARGE, Q_SMALL = 12288, 3000


def _at_distance(rng, q, a):
    """A unit row at squared distance ~a from the unit row q."""
    u = rng.normal(size=128)
    u -= u.dot(q) * q / q.dot(q)
    u /= np.linalg.norm(u)
    c = 1.0 - 0.5 * a
    return orclib.normalize((c * q / np.linalg.norm(q) + np.sqrt(max(0.0, 1.0 - c * c)) * u).astype(np.float32)[None])[0]


def _bits(r):
    return r[0], r[1].view(np.uint32), r[2].view(np.uint32)


def _same(a, b):
    x, y = _bits(a), _bits(b)
    return (x[0] == y[0]) & (x[1] == y[1]) & (x[2] == y[2])


def _none(r):
    return (r[0] == -1) & np.isposinf(r[1]) & np.isposinf(r[2])


def _match(c, qn, accept, mode=1):
    c.match_set_mode(mode)
    c.match_set_accept(accept)
    with np.errstate(all="ignore"):
        _, raw, d1, d2 = c.match(qn, RATIO)
    c.match_set_accept(0.0)
    c.match_set_mode(-1)
    return raw, d1, d2


def _accepted(r):
    with np.errstate(all="ignore"):
        return (r[0] >= 0) & ((r[1] / r[2]) < np.float32(RATIO))


def _compare(c, dbn, qn, must_be_exact=(), label="", borderline=()):
    """Conditions (a), (b), (c) for one launch shape + the full mode against the exact kernel and the oracle.  Returns the
    mask of the pre-rejected queries."""
    c.match_stats(reset=True)
    full = _match(c, qn, 0.0)
    st_full = c.match_stats()
    exact = _match(c, qn, 0.0, mode=3)
    assert _same(full, exact).all()
    c.match_prerejected(reset=True)
    c.match_incomplete(reset=True)
    c.match_stats(reset=True)
    acc = _match(c, qn, RATIO)
    n_pre = c.match_prerejected()
    st_acc, inc_acc = c.match_stats(), c.match_incomplete()
    same, none = _same(acc, full), _none(acc)
    ok = _accepted(full)
    assert same[ok].all(), (label, np.nonzero(ok & ~same)[0][:10])                       # (a)
    assert (same | none).all(), (label, np.nonzero(~(same | none))[0][:10])              # (b)
    pre = none & (full[0] != -1)
    print(label, "queries", len(qn), "accepted", int(ok.sum()), "pre-rejected", int(pre.sum()), "counter", n_pre,
          "candidate rows per query: full %.2f, accepting %.2f" % (st_full["candidates"] / len(qn), st_acc["candidates"] / len(qn)))
    assert int(pre.sum()) == n_pre, (label, int(pre.sum()), n_pre)                       # (c)
    must = np.asarray(list(must_be_exact), np.int64)
    if len(borderline):                                                                  # the planted pairs landed: both sides of 0.8
        b = np.asarray(list(borderline), np.int64)
        r = full[1][b] / full[2][b]
        assert (np.abs(r / np.float32(RATIO) - 1) < 1e-3).all() and ok[b].any() and not ok[b].all(), (label, r)
    assert same[must].all() and not pre[must].any(), (label, must[~same[must]])          # (d), (e)
    assert st_acc["brute_force_queries"] == st_full["brute_force_queries"]
    # the full mode after it: the slots and counts were left clean
    again = _match(c, qn, 0.0)
    assert _same(again, exact).all(), label
    assert c.match_prerejected() == n_pre                                                # ... and counts nothing
    pick = np.unique(np.concatenate([must[:64], np.random.default_rng(1).choice(len(qn), 64, replace=False)]))
    with np.errstate(all="ignore"):
        oi, o1, o2 = orclib.match_2nn(dbn, qn[pick])
    assert _same([x[pick] for x in again], [oi.astype(np.int32), o1, o2]).all()
    return pre, inc_acc


def _plant_borderline(rng, db, qn, q_at, row_at):
    """Queries q_at[k] get their two nearest rows at d1 / d2 = 0.8 (1 +- 1e-4): rows row_at[k] and row_at[k] + gap."""
    planted = []
    k = 0
    for a2 in (0.02, 0.3):
        for sign in (-1.0, 1.0):
            for gap in (1, 40):                                    # in one record's block, and in two
                qi, r = q_at[k], row_at[k]
                db[r] = _at_distance(rng, qn[qi], a2 * RATIO * (1.0 + sign * 1e-4))
                db[r + gap] = _at_distance(rng, qn[qi], a2)
                planted.append(qi)
                k += 1
    return planted


def _upload(c, db, dbn, Q):
    c.db_upload(dbn, db.model_of, db.xyz, db.n_models)
    c.reserve(Q)
    assert c.match_stats(Q)["two_stage"]


@pytest.fixture(scope="module")
def big():
    """The 20 x 5 000 DB, the frames of seeds 0..3, the host model's share for them (made once, left unchanged)."""
    import torch
    db, dbn, frames = accept_model.synth_frames()
    model = [accept_model.predicted_share(qn, dbn, RATIO, torch_dev=torch.device("cuda:0")) for qn in frames]
    for a in [dbn] + frames:
        a.setflags(write=False)
    return db, dbn, frames, model


def test_both_layouts_on_one_context(big):
    db, dbn0, frames, model = big
    N = len(dbn0)
    plan = capi.screen_launch_plan(Q_LARGE, N)
    assert plan["onesweep"] == 1, plan                              # the 16x16x32 passes, counted lists
    assert capi.screen_launch_plan(Q_SMALL, N)["onesweep"] == 0     # the 32x32x16 passes, lane-private slots
    assert capi.screen_launch_plan(Q_LARGE - 1024, N)["onesweep"] == 0, "12 288 is the smallest launch of the counted lists"
    every, first, n_sel, Sa = plan["tile_stride"], plan["tile_first"], plan["sampled_tiles"], plan["splits_a"]
    sampled = [first + i * every for i in range(n_sel)]
    rng = np.random.default_rng(5)
    dbn = dbn0.copy()
    extra = orclib.normalize(np.abs(rng.normal(size=(Q_LARGE - 4 * Q_SMALL, 128))).astype(np.float32))
    qn = np.concatenate(frames + [extra])
    x0 = 4 * Q_SMALL                                                # the first planted query
    # (d) borderline pairs in unsampled tiles and in sampled ones
    rows = [(sampled[3 + k] + 1) * TILE + 8 for k in range(4)] + [sampled[10 + k] * TILE + 8 for k in range(4)]
    border = _plant_borderline(rng, dbn, qn, list(range(x0, x0 + 8)), rows)
    # (e) an incomplete query that the ratio test rejects and the bounds would prove so: six rows at distances 0.1 ..
    # 0.1025 in six blocks of ONE lane slot of pass A (split 1, quarter 1), which keeps four
    base_a, rem_a = n_sel // Sa, n_sel % Sa
    a0 = 1 * base_a + min(1, rem_a)
    blocks = [(sel, rb) for sel in range(a0, a0 + base_a) for rb in range(4)][:6]
    assert len(blocks) == 6
    q_inc = x0 + 8
    for k, (sel, rb) in enumerate(blocks):
        dbn[sampled[sel] * TILE + rb * 32 + 16 * (k % 2) + 4 * 1 + (k % 4)] = _at_distance(rng, qn[q_inc], 0.1 + 0.0005 * k)
    # (e) a list that overflows: 400 rows at distance 0.1 in 400 blocks of unsampled tiles
    q_ovf = x0 + 9
    uns = [t for t in range(N // TILE - 1) if t not in set(sampled)]
    far = _at_distance(rng, qn[q_ovf], 0.1)
    for k in range(400):
        dbn[uns[40 + k] * TILE + 64 + 5] = far
    # (e) all-zero and non-finite queries
    q_zero, q_inf, q_nan, q_huge = x0 + 10, x0 + 11, x0 + 12, x0 + 13
    qn[q_zero] = 0
    qn[q_inf, 5] = np.inf
    qn[q_nan, 7] = np.nan
    qn[q_huge] *= 1e6
    special = border + [q_inc, q_ovf, q_zero, q_inf, q_nan, q_huge]

    c = capi.Context(0)
    try:
        _upload(c, db, dbn, Q_LARGE)
        pre, inc = _compare(c, dbn, qn, must_be_exact=special, label="counted lists, 20 x 5 000:", borderline=border)
        assert inc >= 1, inc                                        # the planted query did take the bounded sweep
        got = [float(pre[f * Q_SMALL:(f + 1) * Q_SMALL].mean()) for f in range(4)]
        print("share pre-rejected per frame, counted lists:", ["%.3f" % g for g in got], "host model:", ["%.3f" % m for m in model])
        for g, m in zip(got, model):
            assert g >= 0.8 * m, (g, m)
        # the other layout on the same context: frame 0 with the special queries in the place of its last ones
        small = np.concatenate([frames[0][:Q_SMALL - len(special)], qn[special]])
        # (no hand-over in this layout: pass B sweeps the sampled tiles too, the query planted to be incomplete is an
        # ordinary one here, rejected and provably so)
        sp = [Q_SMALL - len(special) + k for k, qi in enumerate(special) if qi != q_inc]
        pre_s, _ = _compare(c, dbn, small, must_be_exact=sp, label="lane-private slots, 20 x 5 000:", borderline=sp[:len(border)])
        assert pre_s[Q_SMALL - len(special) + special.index(q_inc)]
        g = float(pre_s[:Q_SMALL - len(special)].mean())
        m = accept_model.predicted_share(frames[0][:Q_SMALL - len(special)], dbn0, RATIO)
        print("share pre-rejected, lane-private slots: %.3f host model: %.3f" % (g, m))
        assert g >= 0.8 * m, (g, m)
        # ... and back to the counted lists
        _compare(c, dbn, qn, must_be_exact=special, label="counted lists again:")
    finally:
        c.close()


def test_lane_private_slots_on_a_small_db():
    """4 models x 4 096 rows, 3 000 queries: the 32x32x16 passes; the planted cases of the large launch, and a query whose
    sub-lists and overflow list overflow (brute force)."""
    db = synth.make_db(4, 4096)
    dbn = orclib.normalize(db.desc)
    N = len(dbn)
    assert N == 16384 and capi.screen_launch_plan(Q_SMALL, N)["onesweep"] == 0
    qn = orclib.normalize(synth.make_frame(db, n_vis=2, seed=3, Q=Q_SMALL).desc)
    rng = np.random.default_rng(6)
    # (unstructured queries for the planted pairs: a frame's own query may have nearer rows than the planted ones)
    qn[100:108] = orclib.normalize(np.abs(rng.normal(size=(8, 128))).astype(np.float32))
    border = _plant_borderline(rng, dbn, qn, list(range(100, 108)), [t * TILE + 8 for t in range(5, 125, 15)])
    q_ovf, q_zero, q_inf, q_nan = 200, 201, 202, 203
    qn[q_ovf] = orclib.normalize(np.abs(rng.normal(size=(1, 128))).astype(np.float32))[0]
    far = _at_distance(rng, qn[q_ovf], 0.1)
    for k in range(400):
        dbn[(k % 120) * TILE + 32 * (k // 120) + 70 % 32 + 1] = far
    qn[q_zero] = 0
    qn[q_inf, 5] = np.inf
    qn[q_nan, 7] = np.nan
    special = border + [q_ovf, q_zero, q_inf, q_nan]
    c = capi.Context(0)
    try:
        _upload(c, db, dbn, Q_SMALL)
        pre, _ = _compare(c, dbn, qn, must_be_exact=special, label="lane-private slots, 4 x 4 096:", borderline=border)
        assert pre.any()                                            # the exit is taken here as well
        assert c.match_stats()["queries"] > 0
    finally:
        c.close()
