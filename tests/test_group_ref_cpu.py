"""tests/group_ref.py, the reference of tests/test_gpu_group.py, against the oracle's MATCH tail (orc_match_accept:
the reference's ratio test in float, the per-model lists in query order) on every generated case -- and its
generators make what they claim: quotients on the ratio and one ulp below it, the predicates `d1 < ratio * d2` and
`d1 / d2 < ratio` apart, 200 and more distinct pixels of one hash bucket, representatives that differ from the ones
of query order."""
import numpy as np
import pytest

import group_ref as g
import orclib

F32 = np.float32


def _oracle_lists(words, model_of, n_models, ratio, index_base=0):
    idx, d1, d2 = g.merge(words)
    n = len(model_of)
    own = (idx >= index_base) & (idx < index_base + n)
    local = np.where(own, idx - index_base, -1).astype(np.int32)
    q, off = orclib.match_accept(local, d1, d2, ratio, model_of, n_models)
    return q, off


def _check(words, uv, db, ratio, index_base=0):
    e = g.expected(words, uv, db["model_of"], db["xyz"], db["n_models"], ratio, index_base)
    q, off = _oracle_lists(words, db["model_of"], db["n_models"], ratio, index_base)
    assert np.array_equal(e["q"], q) and np.array_equal(e["off"], off)
    assert np.array_equal(e["model"], np.repeat(np.arange(db["n_models"]), np.diff(off)))
    return e


@pytest.mark.parametrize("ratio", [0.8, 0.6, 1.0])
def test_boundary_pairs_are_what_they_claim(ratio):
    r = F32(ratio)
    d1, d2, valid, kind = g.boundary_pairs(ratio)
    with np.errstate(all="ignore"):
        quot = d1 / d2
    assert quot.dtype == F32
    assert np.all(quot[kind == "exact"] == r)
    assert np.all(quot[kind == "ulp_below"] == np.nextafter(r, F32(0)))
    dis = kind == "product_disagrees"
    assert (dis.sum() > 0) == (ratio != 1.0)
    assert np.all((d1[dis] < r * d2[dis]) != (quot[dis] < r))
    assert np.all(np.isnan(quot[kind == "zero_zero"]))
    assert np.all(np.isinf(quot[kind == "d2_zero"]))
    assert np.all(np.isinf(d2[kind == "d2_inf"]))
    sub = d1[kind == "subnormal_d1"]
    assert np.all((sub > 0) & (sub < np.finfo(F32).tiny))
    assert not valid[kind == "no_index"].any() and valid[kind != "no_index"].all()
    # the oracle decides these pairs as the reference does
    db = g.make_db(7, seed=1)
    Q = len(d1)
    rng = np.random.default_rng(2)
    idx = np.where(valid, rng.integers(0, len(db["model_of"]), Q), -1).astype(np.int32)
    uv = rng.integers(0, 640, (Q, 2)).astype(F32)
    e = _check(g.blocks(idx, d1, d2), uv, db, ratio)
    acc = np.zeros(Q, bool)
    acc[e["q"]] = True
    assert not acc[kind == "exact"].any() and acc[kind == "ulp_below"].all()
    assert not acc[(kind == "zero_zero") | (kind == "d2_zero") | (kind == "no_index")].any()
    assert acc[kind == "d2_inf"].all()
    assert acc[kind == "subnormal_d1"].any() and not acc[kind == "subnormal_d1"].all()


def test_adaptive_boundary_pairs_sit_on_each_querys_ratio():
    rs = np.array([0.8, 0.61, 0.0, 0.733, 1.0, 0.55] * 10, F32)
    d1, d2, valid, kind = g.boundary_pairs(rs, n_per_kind=None, seed=3)
    with np.errstate(all="ignore"):
        quot = d1 / d2
    ex, lo = kind == "exact", kind == "ulp_below"
    assert ex.any() and lo.any()
    assert np.all(quot[ex] == rs[ex]) and np.all(quot[lo] == np.nextafter(rs[lo], F32(0)))


def test_colliding_pixels_share_one_bucket():
    uv, b = g.colliding_pixels(260)
    assert len(np.unique(uv, axis=0)) == 260
    assert np.all(g.hash11(uv[:, 0], uv[:, 1]) == b)
    # -0.0 hashes like 0.0 (hash_of adds +0.f)
    assert g.hash11(F32(-0.0), F32(3.5)) == g.hash11(F32(0.0), F32(3.5))
    assert g.reps(np.array([0.0, -0.0], F32), np.array([1.0, 1.0], F32)).tolist() == [0, 0]


@pytest.mark.parametrize("n_models,Q,M", [(1, 4095, 0), (1, 4097, 2047), (2049, 4096, 2048), (5000, 8193, 2049),
                                          (8192, 8193, 6000)])
def test_generated_frames_against_the_oracle(n_models, Q, M):
    db = g.make_db(n_models, seed=n_models)
    words, uv = g.make_frame(db, Q, M, seed=Q + M, n_collide=220)
    e = _check(words, uv, db, 0.8)
    assert e["n"] == M
    if M > 1000:
        assert g.list_vs_query_order(e["rep"], e["q"]) > 0 or n_models == 1   # (one model: list order = query order)
        corr = e["corr"]
        assert np.any((corr["u"] == 0) & np.signbit(corr["u"])) and np.any((corr["u"] == 0) & ~np.signbit(corr["u"]))
        h = g.hash11(corr["u"], corr["v"])
        assert np.bincount(h).max() >= 200


def test_shard_blocks_against_the_oracle():
    rng = np.random.default_rng(5)
    for S in (2, 3, 5, 8):
        db = g.make_db(40, seed=S)
        n = len(db["model_of"])
        base = 3 * n
        Q = 1500
        idx_s = (rng.integers(0, 8 * n, (S, Q))).astype(np.int32)
        idx_s[rng.random((S, Q)) < 0.1] = -1
        d1_s = rng.uniform(0.2, 1.0, (S, Q)).astype(F32)
        d2_s = (d1_s + rng.uniform(0.0, 1.0, (S, Q))).astype(F32)
        words = g.blocks(idx_s, d1_s, d2_s)
        uv = rng.integers(0, 640, (Q, 2)).astype(F32)
        for ratio in (0.8, 1.5):
            e = _check(words, uv, db, ratio, index_base=base)
            assert e["n"] > 0
