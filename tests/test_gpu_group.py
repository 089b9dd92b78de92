"""group_kernel, the tail of MATCH, bit for bit against tests/group_ref.py on injected top-2 blocks: the ratio test at
its boundary (fixed and depth-adaptive ratios), the stable per-model lists, the packed correspondences and every
entry's representative (the key of FILTER's bestPoints map, FILTER_PROJECTION_CPU.hpp:89) -- on all three placement
paths (LDS buckets + hash chains; LDS rank scan for more than 2 048 models; global scans beyond 2 048 matches), the
shards' merge, merged batches and frames with several images.  CLUSTER .. FILTER2 have nothing to do
(ms_min_pts above every list)."""
import numpy as np
import pytest

import group_ref as g
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
F32 = np.float32


def _params(ratio):
    p = capi.default_frame_params()
    p.ratio = float(ratio)
    p.ms_min_pts = 1 << 20
    return p


def _ctx(db, Q, index_base=0, frames=1):
    c = capi.Context(0)
    c.db_upload(db["desc"], db["model_of"], db["xyz"], db["n_models"], index_base)
    if frames > 1:
        c.reserve_batch(Q, frames)
    else:
        c.reserve(Q)
    return c


def _run(c, words, uv, ratio, seed=1):
    import torch
    dev = torch.device("cuda:0")
    S, _, Q = words.shape
    w = torch.from_numpy(np.ascontiguousarray(words).reshape(-1)).to(dev)
    u = torch.from_numpy(np.ascontiguousarray(uv, F32)).to(dev)
    c.frame_enqueue_rest(u.data_ptr(), Q, w.data_ptr(), S, K, CAM0, _params(ratio), seed)
    _, counts = c.frame_fetch()
    return _got(c, counts)


def _got(c, counts, slot=None):
    q, m = c.frame_fetch_matches() if slot is None else c.frame_fetch_matches_slot(slot)
    rep = c.frame_fetch_match_reps(slot)
    return dict(q=q, model=m, rep=rep, n=int(counts[0]),
                corr=c.frame_fetch_match_points() if slot is None else None)


def _same(got, e, what=""):
    assert got["n"] == e["n"], (what, got["n"], e["n"])
    assert np.array_equal(got["q"], e["q"]), what
    assert np.array_equal(got["model"], e["model"]), what
    if got["corr"] is not None:
        assert got["corr"].dtype == capi.CORR_DTYPE
        assert np.array_equal(got["corr"].view(np.uint32).reshape(-1), e["corr"].view(np.uint32).reshape(-1)), what
    assert np.array_equal(got["rep"], e["rep"]), (what, np.nonzero(got["rep"] != e["rep"])[0][:10])


# ---- the ratio test at its boundary ------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.8, 0.6, 1.0])
def test_ratio_boundary(ratio):
    d1, d2, valid, kind = g.boundary_pairs(ratio)
    db = g.make_db(7, seed=1)
    Q = len(d1)
    rng = np.random.default_rng(2)
    idx = np.where(valid, rng.integers(0, len(db["model_of"]), Q), -1).astype(np.int32)
    uv = rng.integers(0, 640, (Q, 2)).astype(F32)
    words = g.blocks(idx, d1, d2)
    e = g.expected(words, uv, db["model_of"], db["xyz"], 7, ratio)
    c = _ctx(db, Q)
    try:
        _same(_run(c, words, uv, ratio), e, ratio)
    finally:
        c.close()
    acc = np.isin(np.arange(Q), e["q"])
    # the cases are reached: quotients on the ratio refused, one ulp below accepted, the predicates apart
    assert (kind == "exact").sum() >= 8 and not acc[kind == "exact"].any() and acc[kind == "ulp_below"].all()
    assert ratio == 1.0 or (kind == "product_disagrees").sum() >= 8
    assert acc[kind == "d2_inf"].all() and acc[kind == "subnormal_d1"].any()


def test_ratio_boundary_through_the_depth_adaptive_ratio():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    n_models = 9
    db = g.make_db(n_models, seed=11)
    h, w = 120, 160
    img = np.zeros((h, w, 4), F32)
    img[..., 2] = rng.uniform(0.1, 4.5, (h, w))
    img[80:, :50, 2] = 5.0                      # beyond MaximumDepth (4 m)
    img[:12, :, 2] = np.nan                     # NaN depths
    fill = rng.uniform(0.0, 0.3, (h, w)).astype(F32)
    table = np.stack([rng.uniform(0.4, 1.0, n_models), rng.uniform(1.2, 2.0, n_models),
                      rng.uniform(0.55, 0.65, n_models), rng.uniform(0.7, 0.85, n_models)], 1).astype(F32)
    Q = 1500
    uv = np.stack([rng.integers(-5, w + 5, Q), rng.integers(-5, h + 5, Q)], 1).astype(F32)
    idx = rng.integers(0, len(db["model_of"]), Q).astype(np.int32)
    r_q, reach = orclib.adaptive_ratio(img, fill, uv, db["model_of"][idx], table)
    d1, d2, valid, kind = g.boundary_pairs(r_q, n_per_kind=None, seed=12)
    idx[~valid] = -1
    words = g.blocks(idx, d1, d2)
    e = g.expected(words, uv, db["model_of"], db["xyz"], n_models, 0.8, ratio_q=r_q, reach=reach)
    c = _ctx(db, Q)
    d_img, d_fill = torch.from_numpy(img).to(dev), torch.from_numpy(fill).to(dev)
    try:
        c.frame_set_depth_image(d_img.data_ptr(), d_fill.data_ptr(), w, h, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        c.frame_set_depth_rules(K, 64, -1.0, -1.0, table)
        _same(_run(c, words, uv, 0.8), e, "adaptive")
    finally:
        c.frame_set_depth_rules(off=True)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()
    acc = np.isin(np.arange(Q), e["q"])
    ex = (kind == "exact") & reach & (r_q > 0)
    assert ex.sum() >= 50 and not acc[ex].any()
    lo = (kind == "ulp_below") & reach & (r_q > 0)
    assert lo.sum() >= 50 and acc[lo].all()
    assert (~reach).sum() >= 20 and not acc[~reach].any()
    nan_px = np.isnan(img[np.clip(uv[:, 1].astype(int), 0, h - 1), np.clip(uv[:, 0].astype(int), 0, w - 1), 2])
    assert (nan_px & valid).sum() >= 20 and acc[nan_px].any()


# ---- the three placement / representative paths and the sizes around them ----------------------------------------
SIZES = {   # n_models -> [(Q, M)]
    1: [(4095, 0), (4096, 1), (4097, 2047), (8193, 6000)],
    2048: [(4096, 2048), (4097, 2049), (8193, 2047)],
    2049: [(4095, 2047), (4096, 2048), (8193, 2049), (4097, 1)],
    5000: [(8193, 2048), (8193, 6000), (4096, 0)],
    8192: [(8193, 2047), (8193, 6000), (4097, 2048)],
}


@pytest.mark.parametrize("n_models", sorted(SIZES))
def test_lists_corr_and_reps_on_every_path(n_models):
    db = g.make_db(n_models, seed=n_models)
    c = _ctx(db, max(q for q, _ in SIZES[n_models]))
    paths = set()
    try:
        for Q, M in SIZES[n_models]:
            words, uv = g.make_frame(db, Q, M, seed=Q + M + n_models, n_collide=220)
            e = g.expected(words, uv, db["model_of"], db["xyz"], n_models, 0.8)
            assert e["n"] == M
            _same(_run(c, words, uv, 0.8), e, (n_models, Q, M))
            paths.add(g.path_of(M, n_models))
            if M > 1000 and n_models > 1:   # the cases are reached: model order is not query order, one long chain
                assert g.list_vs_query_order(e["rep"], e["q"]) > 0
            if M > 1000:
                assert np.bincount(g.hash11(e["corr"]["u"], e["corr"]["v"])).max() >= 200
                assert np.sum((e["corr"]["u"] == 0) & np.signbit(e["corr"]["u"])) >= 1
    finally:
        c.close()
    want = {"global"} | ({"bucket"} if n_models <= g.LDS_M else {"lds_scan"})
    assert paths == want


def test_more_models_than_the_histogram_holds_is_refused():
    db = g.make_db(8193, seed=3, rows_max=1)
    words, uv = g.make_frame(db, 64, 10, seed=3)
    c = _ctx(db, 64)
    try:
        with pytest.raises(capi.MhError, match="-> -3"):   # MH_ERR_CAPACITY
            _run(c, words, uv, 0.8)
    finally:
        c.close()


def test_representatives_hand_made():
    """Duplicates inside one model and across models (the representative is the first entry in MODEL order),
    (-0.0, y) against (0.0, y), on both sides of M = 2048."""
    db = g.make_db(6, seed=4, rows_max=1)      # row r = model r
    for M in (40, 2100):
        Q = M
        idx = np.zeros(Q, np.int32)
        uv = np.stack([np.arange(Q) * F32(0.5) + 100, np.full(Q, 200.0)], 1).astype(F32)
        idx[0], uv[0] = 5, (3.0, 4.0)           # query 0, model 5
        idx[1], uv[1] = 1, (3.0, 4.0)           # query 1, model 1: the representative of query 0's entry
        idx[2], uv[2] = 1, (3.0, 4.0)           # same model, same pixel
        idx[3], uv[3] = 3, (-0.0, 9.0)
        idx[4], uv[4] = 2, (0.0, 9.0)           # model 2 lists before model 3: represents (-0.0, 9)
        idx[5], uv[5] = 4, (7.0, -0.0)
        idx[6], uv[6] = 4, (7.0, 0.0)
        idx[7:] = np.arange(Q - 7) % 6
        d1 = np.full(Q, 0.1, F32)
        d2 = np.ones(Q, F32)
        words = g.blocks(idx, d1, d2)
        e = g.expected(words, uv, db["model_of"], db["xyz"], 6, 0.8)
        ent = {int(q): i for i, q in enumerate(e["q"])}
        assert e["rep"][ent[0]] == ent[1] and e["rep"][ent[2]] == ent[1] and ent[1] < ent[0]
        assert e["rep"][ent[3]] == ent[4] and e["rep"][ent[6]] == ent[5]
        c = _ctx(db, Q)
        try:
            _same(_run(c, words, uv, 0.8), e, M)
        finally:
            c.close()


# ---- shards -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 5, 8])
def test_shard_merge(S):
    rng = np.random.default_rng(20 + S)
    db = g.make_db(60, seed=S)
    n = len(db["model_of"])
    base = 2 * n                                 # this rank's rows: [2n, 3n) of S n + n global rows
    Q = 3000
    idx_s = (np.arange(S)[:, None] * n + rng.integers(0, n, (S, Q))).astype(np.int32)
    d1_s = rng.uniform(0.2, 1.0, (S, Q)).astype(F32)
    d2_s = (d1_s + rng.uniform(0.0, 1.0, (S, Q))).astype(F32)
    if S > 2:
        idx_s[2] = base + rng.integers(0, n, Q)   # the rank's own shard
    # equal best distances in two shards: the lower global index wins (ratio 1.5 accepts the quotient 1)
    tie = rng.random(Q) < 0.3
    d1_s[1, tie] = d1_s[0, tie]
    idx_s[0, tie] = base + rng.integers(0, n, tie.sum())
    idx_s[1, tie] = np.where(rng.random(tie.sum()) < 0.5, idx_s[0, tie] + 1, idx_s[0, tie] - n)
    # a losing best distance becomes the second best
    close = ~tie & (rng.random(Q) < 0.3)
    d1_s[1, close] = d1_s[0, close] * F32(1.1)
    idx_s[rng.random((S, Q)) < 0.1] = -1         # shards without a neighbour (their distances are garbage)
    d1_s[idx_s < 0] = 0.0
    words = g.blocks(idx_s, d1_s, d2_s)
    uv = rng.integers(0, 1280, (Q, 2)).astype(F32) * F32(0.5)
    c = _ctx(db, Q, index_base=base)
    try:
        for ratio in (0.8, 1.5):
            e = g.expected(words, uv, db["model_of"], db["xyz"], 60, ratio, index_base=base)
            _same(_run(c, words, uv, ratio), e, (S, ratio))
            idx, _, _ = g.merge(words)
            assert e["n"] > 0 and np.any((idx >= 0) & ((idx < base) | (idx >= base + n)))
            if ratio == 1.5:
                assert np.isin(np.nonzero(tie)[0], e["q"]).sum() >= 20
    finally:
        c.close()


# ---- merged batches ---------------------------------------------------------------------------------------------
def test_batch_slots_equal_the_reference():
    import torch
    dev = torch.device("cuda:0")
    B, Q = 4, 2600
    db = g.make_db(300, seed=7)
    Ms = [0, 2300, 700, 2049]
    frames = [g.make_frame(db, Q, M, seed=70 + f, n_collide=200 if M > 200 else 0) for f, M in enumerate(Ms)]
    plane = B * Q
    words = np.zeros((1, 3, plane), np.int32)
    uv = np.zeros((B * Q, 2), F32)
    for f, (w, u) in enumerate(frames):
        words[:, :, f * Q:(f + 1) * Q] = w
        uv[f * Q:(f + 1) * Q] = u
    c = _ctx(db, Q, frames=B)
    try:
        wt = torch.from_numpy(words.reshape(-1)).to(dev)
        ut = torch.from_numpy(uv).to(dev)
        c.frame_enqueue_rest_frames(ut.data_ptr(), Q, wt.data_ptr(), 1, 3 * plane, plane, B, K, CAM0, _params(0.8),
                                    [5 + f for f in range(B)])
        for f, (w, u) in enumerate(frames):
            _, counts = c.frame_fetch_slot(f)
            e = g.expected(w, u, db["model_of"], db["xyz"], 300, 0.8)
            assert e["n"] == Ms[f]
            got = _got(c, counts, slot=f)
            if f == B - 1:
                got["corr"] = c.frame_fetch_match_points()
            _same(got, e, f)
        # and each frame alone
        for f, (w, u) in enumerate(frames):
            e = g.expected(w, u, db["model_of"], db["xyz"], 300, 0.8)
            _same(_run(c, w, u, 0.8), e, ("alone", f))
    finally:
        c.close()


# ---- several cameras --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_images", [2, 8])
def test_representatives_per_image(n_images):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(30 + n_images)
    db = g.make_db(40, seed=n_images)
    for Q, M in ((1200, 900), (3000, 2300)):
        words, uv = g.make_frame(db, Q, M, seed=Q + n_images, n_collide=200)
        q_img = rng.integers(0, n_images, Q).astype(np.int32)
        e = g.expected(words, uv, db["model_of"], db["xyz"], 40, 0.8, q_img=q_img)
        plain = g.reps(e["corr"]["u"], e["corr"]["v"])
        assert np.sum(plain != e["rep"]) >= 20    # the same pixel in other images: representatives of their own
        c = _ctx(db, Q)
        qi = torch.from_numpy(q_img).to(dev)
        try:
            c.frame_set_images(qi.data_ptr(), [K] * n_images, [CAM0] * n_images)
            _same(_run(c, words, uv, 0.8), e, (n_images, M))
        finally:
            c.frame_set_images(0)
            c.close()
