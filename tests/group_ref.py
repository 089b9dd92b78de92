"""Plain numpy restatement of `group_kernel` (moped_amd/csrc/group.hip), the tail of MATCH, and the generators of the
inputs its tests inject.

The kernel merges the shards' top-2 blocks, applies the ratio test `ds[0]/ds[1] < Ratio` in float
(MATCH_ANN_CPU.hpp:165; the vendored ANN has `typedef float ANNdist`), builds the stable per-model lists
`matches[model]`, packs (uv of the query, xyz of its row) and finds every entry's representative: the first entry
with the same pixel (and image), the key of FILTER's bestPoints map (FILTER_PROJECTION_CPU.hpp:89).

The accept / lists part is itself pinned to the oracle's `match_accept` by tests/test_group_ref_cpu.py."""
from __future__ import annotations

import numpy as np

import orclib

F32 = np.float32
LDS_M = 2048          # group_kernel's GROUP_LDS_M: matches (and models) its LDS paths hold
PASS_Q = 4096         # queries per compaction super-pass (4 passes of 1 024)


# ---- the reference ----------------------------------------------------------------------------------------------
def blocks(idx_s, d1_s, d2_s):
    """[S][Q] shard top-2 arrays -> the exchange's [S][3][Q] int32 words (index, d1 bits, d2 bits)."""
    idx_s = np.atleast_2d(np.asarray(idx_s, np.int32))
    d1_s = np.atleast_2d(np.asarray(d1_s, F32))
    d2_s = np.atleast_2d(np.asarray(d2_s, F32))
    return np.ascontiguousarray(np.stack([idx_s, d1_s.view(np.int32), d2_s.view(np.int32)], axis=1))


def merge(words):
    """[S][3][Q] words -> (idx, d1, d2) after the shards' merge: the oracle's match_merge."""
    words = np.asarray(words, np.int32)
    return orclib.match_merge(words[:, 0], words[:, 1].view(F32), words[:, 2].view(F32))


def accept(idx, d1, d2, ratio, n_rows, index_base=0, reach=None):
    """Accepted queries: a row of this shard ([index_base, index_base + n_rows)) and the float quotient below the ratio
    (a scalar or one per query); `reach` = the depth rule's "don't even bother searching" (:457-460)."""
    idx = np.asarray(idx, np.int32)
    with np.errstate(all="ignore"):
        q = np.asarray(d1, F32) / np.asarray(d2, F32)
    assert q.dtype == F32
    ok = (idx >= index_base) & (idx < index_base + n_rows) & (q < np.asarray(ratio, F32))
    if reach is not None:
        ok &= reach
    return ok


def lists(ok, model, n_models):
    """Stable per-model lists: (queries in (model, query) order, their models, model_off [n_models + 1])."""
    qs = np.nonzero(ok)[0]
    qs = qs[np.lexsort((qs, model[qs]))]
    mm = model[qs].astype(np.int32)
    off = np.searchsorted(mm, np.arange(n_models + 1)).astype(np.int32)
    return qs.astype(np.int32), mm, off


def reps(u, v, img=None):
    """rep[i] = min{j : u_j == u_i, v_j == v_i (and img_j == img_i)}, compared as floats: -0.0 == 0.0."""
    first = {}
    out = np.empty(len(u), np.int32)
    for i in range(len(u)):
        key = (float(u[i]) + 0.0, float(v[i]) + 0.0, None if img is None else int(img[i]))
        out[i] = first.setdefault(key, i)
    return out


def expected(words, uv, model_of, xyz, n_models, ratio, index_base=0, q_img=None, ratio_q=None, reach=None):
    """Everything group_kernel leaves for a frame: {q, model, corr (CORR_DTYPE), rep, off, n}.
    model_of / xyz: this shard's rows (global model numbers); ratio_q: a ratio per query (depth rules) instead."""
    from moped_amd.capi import CORR_DTYPE
    idx, d1, d2 = merge(words)
    n_rows = len(model_of)
    ok = accept(idx, d1, d2, ratio if ratio_q is None else ratio_q, n_rows, index_base, reach)
    local = np.where(ok, idx - index_base, 0)
    model = np.asarray(model_of, np.int32)[local]
    qs, mm, off = lists(ok, model, n_models)
    corr = np.zeros(len(qs), CORR_DTYPE)
    uv = np.asarray(uv, F32)
    xyz = np.asarray(xyz, F32)
    rows = idx[qs] - index_base
    corr["u"], corr["v"] = uv[qs, 0], uv[qs, 1]
    corr["x"], corr["y"], corr["z"] = xyz[rows, 0], xyz[rows, 1], xyz[rows, 2]
    rep = reps(corr["u"], corr["v"], None if q_img is None else np.asarray(q_img)[qs])
    return dict(q=qs, model=mm, corr=corr, rep=rep, off=off, n=len(qs), idx=idx, d1=d1, d2=d2)


# ---- group_kernel's hash of a pixel (hash_of, group.hip) ----------------------------------------------------------
def hash11(u, v):
    a = (np.asarray(u, F32) + F32(0)).view(np.uint32).astype(np.uint64)
    b = (np.asarray(v, F32) + F32(0)).view(np.uint32).astype(np.uint64)
    h = ((a * 0x9E3779B1) & 0xFFFFFFFF) ^ ((b * 0x85EBCA77) & 0xFFFFFFFF)
    return ((h >> 21) & (LDS_M - 1)).astype(np.int32)


def colliding_pixels(n, bucket=None, seed=0):
    """n distinct pixels (half-pixel steps in a 640 x 480 image) of one 11-bit hash bucket -> (uv [n, 2] float32,
    bucket)."""
    u, v = np.meshgrid(np.arange(0, 640, 0.5, dtype=F32), np.arange(0, 480, 0.5, dtype=F32))
    u, v = u.ravel(), v.ravel()
    h = hash11(u, v)
    if bucket is None:
        bucket = int(np.bincount(h, minlength=LDS_M).argmax())
    sel = np.nonzero(h == bucket)[0]
    assert len(sel) >= n, (len(sel), n)
    sel = np.random.default_rng(seed).choice(sel, n, replace=False)
    return np.stack([u[sel], v[sel]], 1).astype(F32), bucket


# ---- ratio boundary pairs --------------------------------------------------------------------------------------
BOUNDARY_KINDS = ("exact", "ulp_below", "product_disagrees", "zero_zero", "d2_zero", "d2_inf", "subnormal_d1",
                  "no_index")


def _quot(d1, d2):
    with np.errstate(all="ignore"):
        return (np.asarray(d1, F32) / np.asarray(d2, F32)).astype(F32)


def _nudge(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(0))
    return F32(x)


def boundary_pair(r, kind, rng, want=None):
    """One (d1, d2, idx_valid) of `kind` at ratio r.  product_disagrees: want = the quotient's verdict to reach."""
    r = F32(r)
    tiny = np.finfo(F32).smallest_subnormal
    if kind in ("exact", "ulp_below"):
        target = r if kind == "exact" else np.nextafter(r, F32(0))
        for _ in range(100000):
            d2 = F32(rng.uniform(0.05, 2.0))
            for k in (0, -1, 1, -2, 2):
                c = _nudge(F32(target * d2), k)
                if _quot(c, d2) == target:
                    return c, d2, True
        raise AssertionError((r, kind))
    if kind == "product_disagrees":   # (at a ratio of 0.8 only accepting quotients disagree, at 0.6 only rejecting ones)
        for _ in range(1000):
            d2 = rng.uniform(0.05, 2.0, 4096).astype(F32)
            prod = (r * d2).astype(F32)
            for k in range(-3, 4):
                c = prod
                for _ in range(abs(k)):
                    c = np.nextafter(c, F32(np.inf) if k > 0 else F32(0))
                quot_ok = _quot(c, d2) < r
                hit = np.nonzero((quot_ok != (c < prod)) & ((quot_ok == want) if want is not None else True))[0]
                if len(hit):
                    return F32(c[hit[0]]), F32(d2[hit[0]]), True
        raise AssertionError((r, kind, want))
    choice = {
        "zero_zero": [(0.0, 0.0)],
        "d2_zero": [(1e-30, 0.0), (0.5, 0.0), (3.0, 0.0)],
        "d2_inf": [(0.0, np.inf), (1e-30, np.inf), (0.5, np.inf), (3.0e30, np.inf)],
        "subnormal_d1": [(tiny, 1.0), (tiny * 3, tiny * 4), (tiny * 7, tiny * 8), (1e-39, 1.2e-39), (1e-39, 1e-38),
                         (9e-39, 1.1e-38), (1e-39, 0.0), (r * F32(1e-38), 1e-38)],
        "no_index": [(0.1, 1.0), (0.0, 1.0)],
    }[kind]
    d1, d2 = choice[rng.integers(len(choice))]
    return F32(d1), F32(d2), kind != "no_index"


def boundary_pairs(ratios, kinds=BOUNDARY_KINDS, n_per_kind=8, seed=0):
    """(d1, d2, idx_valid, kind) float32 pairs, n_per_kind of every kind at every ratio (`ratios`: one or several),
    or -- `ratios` an array with one ratio per pair wanted and n_per_kind=None -- one pair per ratio, kinds in turn."""
    rng = np.random.default_rng(seed)
    rs = np.atleast_1d(np.asarray(ratios, F32))
    jobs = [(r, k) for r in rs for k in kinds for _ in range(n_per_kind)] if n_per_kind else \
        [(r, kinds[i % len(kinds)]) for i, r in enumerate(rs)]
    out = []
    for j, (r, k) in enumerate(jobs):
        if r <= 0 and k in ("exact", "ulp_below", "product_disagrees"):
            k = "d2_zero"   # (a ratio of 0 rejects every pair: nothing lies below it)
        if r == 1 and k == "product_disagrees":
            k = "exact"     # (1 * d2 is exact: the two predicates agree everywhere)
        out.append(boundary_pair(r, k, rng) + (k,))
    d1, d2, v, kind = zip(*out)
    return np.array(d1, F32), np.array(d2, F32), np.array(v, bool), np.array(kind)


# ---- synthetic DBs and frames ----------------------------------------------------------------------------------
def path_of(M, n_models):
    """Which of group_kernel's placement / representative paths a frame takes."""
    if M > LDS_M:
        return "global"
    return "bucket" if n_models <= LDS_M else "lds_scan"


def make_db(n_models, seed=0, rows_max=3):
    """model_of (1 .. rows_max rows per model, model after model), distinct xyz, descriptors (never searched)."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, rows_max + 1, n_models)
    model_of = np.repeat(np.arange(n_models, dtype=np.int32), per)
    n = len(model_of)
    xyz = (np.arange(3 * n, dtype=F32).reshape(n, 3) * F32(0.001) + rng.uniform(-1, 1, (1, 3)).astype(F32))
    desc = rng.standard_normal((n, 128)).astype(F32)
    return dict(model_of=model_of, xyz=xyz, desc=desc, n_models=n_models)


def make_frame(db, Q, M, seed=0, ratio=0.8, index_base=0, dup_frac=0.25, n_collide=0, neg_zero=True):
    """One frame of Q queries whose M accepted ones (the last query among them) go to every other model with rows
    (empty lists between full ones); the others are refused in every way the kernel tells apart.  Pixels: half-pixel
    steps, with duplicates inside a model and across models, (-0.0, y) beside (0.0, y), and n_collide distinct pixels of
    one hash bucket.  -> (words [1][3][Q], uv [Q, 2])."""
    rng = np.random.default_rng(seed)
    model_of = db["model_of"]
    n = len(model_of)
    idx = np.full(Q, -1, np.int32)
    d1 = np.ones(Q, F32)
    d2 = np.ones(Q, F32)
    acc = np.sort(rng.choice(Q - 1, M - 1, replace=False)) if M > 1 else np.zeros(0, np.int64)
    acc = np.concatenate([acc, [Q - 1]]) if M > 0 else acc
    active = np.nonzero(np.isin(model_of, np.arange(0, db["n_models"], 2)))[0]
    idx[acc] = index_base + rng.choice(active, len(acc))
    d2[acc] = rng.uniform(0.5, 2.0, len(acc)).astype(F32)
    d1[acc] = (d2[acc] * rng.uniform(0.0, 0.9, len(acc)).astype(F32) * F32(ratio)).astype(F32)
    rej = np.setdiff1d(np.arange(Q), acc)
    kind = rng.integers(0, 4, len(rej))
    r_any = index_base + rng.integers(0, n, len(rej))
    idx[rej] = np.where(kind == 0, -1, r_any)                              # no neighbour
    d2[rej] = rng.uniform(0.5, 2.0, len(rej)).astype(F32)
    d1[rej] = np.where(kind == 1, d2[rej], d1[rej])                        # equal distances
    for j in np.nonzero(kind == 2)[0]:                                     # the quotient lands on the ratio exactly
        d1[rej[j]], d2[rej[j]], _ = boundary_pair(ratio, "exact", rng)
    d1[rej] = np.where(kind == 3, np.float32(0.0), d1[rej])                # a row of no shard of this context's
    idx[rej] = np.where(kind == 3, index_base + n + rng.integers(0, 50, len(rej)), idx[rej])
    uv = (rng.integers(0, 1280, (Q, 2)) * F32(0.5)).astype(F32)
    uv[:, 1] %= 480
    if M > 1:
        ndup = int(dup_frac * M)
        src = rng.choice(acc, ndup)
        dst = rng.choice(acc, ndup)
        uv[dst] = uv[src]                                                  # the same pixel, often another model
    if n_collide:
        cu, _ = colliding_pixels(min(n_collide, M), seed=seed)
        uv[acc[:len(cu)]] = cu
    if neg_zero and M > 4:
        k = acc[rng.choice(len(acc), 4, replace=False)]
        uv[k[0]] = (0.0, 7.5)
        uv[k[1]] = (-0.0, 7.5)
        uv[k[2]] = (31.0, -0.0)
        uv[k[3]] = (31.0, 0.0)
    return blocks(idx, d1, d2), uv


def list_vs_query_order(rep, q):
    """Entries whose representative in list order (the reference's) is not the one of the smallest query."""
    first_q = {}
    for i, r in enumerate(rep):
        first_q[r] = min(first_q.get(r, q[i]), q[i])
    return int(sum(q[r] != first_q[r] for r in set(rep.tolist())))
