"""mh_view_merge_dev: the merge of re-seen points on synthetic device arrays, bit for bit against tests/view_merge_ref.py:
the merged rows' indices, sums and points, the full count, the view counts, and the sentinel in everything at and beyond
the count.

The kernels walk the list in chunks of 64 (one wavefront per merged row) and of 1024 (the verdicts), the model's rows in
chunks of 1024: list lengths, model sizes and observation counts sit on those seams.  merge_dist is large, so that MATCH's
answer alone (idx, d1 / d2) decides which keypoint observes which row.  Keypoints behind a list's count would all be
observations of the model's first row if they were read."""
import ctypes as C

import numpy as np
import pytest

import view_merge_ref as mref
import view_model_ref as ref
from moped_amd import capi

pytestmark = pytest.mark.gpu
CAP = 2048
W, H = 64, 48
SENT_BITS = 0x7FC0BEEF   # a NaN no computation here makes
SENT_INT = -77
POSE = ref.trap_pose()
KW = dict(merge_ratio=0.8, merge_dist=100.0)
f = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def dev():
    import torch
    c = capi.Context(0)
    rng = np.random.default_rng(0x3E26E)
    depth = np.concatenate([rng.uniform(-0.5, 1.5, (H, W, 3)), np.ones((H, W, 1))], 2).astype(np.float32)
    depth[10:20, 12:24, 3] = -1.0   # holes
    desc = rng.normal(size=(CAP, 128)).astype(np.float32)   # FEAT's bits: not read by the merge
    qn = unit(np.abs(rng.normal(size=(CAP, 128))))
    d = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    env = dict(c=c, torch=torch, d=d, t=t, depth=depth, depth_d=t(depth), desc_d=t(desc), qn=qn, qn_d=t(qn))
    depth.setflags(write=False)
    qn.setflags(write=False)
    yield env
    c.close()


def keypoints(rng, n):
    """CAP keypoints: most on measured pixels, some outside the map, some in the holes; behind n: all measured."""
    i = np.arange(CAP)
    xy = np.stack([f(0.25) + (i % 10).astype(np.float32), f(0.5) + ((i // 10) % 8).astype(np.float32)], 1).astype(np.float32)
    bad = rng.random(CAP) < 0.1
    bad[n:] = False
    xy[bad & (i % 2 == 0), 0] = f(70.0)          # rule 1
    xy[bad & (i % 2 == 1)] = (f(15.5), f(12.5))  # rule 2
    return xy


def scene(seed, n, rows, row_begin=0, n_db=None, per_row=None, views="random", share=0.6):
    """A store of n_db rows whose rows [row_begin, row_begin + rows) are the model (model 1 when there are rows in front),
    and MATCH's answer for a list of n keypoints.  per_row: {relative row: observations} that are forced; the other
    keypoints observe a random row with probability `share`, are not accepted, or have their nearest row elsewhere."""
    rng = np.random.default_rng(seed)
    n_db = row_begin + rows + 300 if n_db is None else n_db
    row_end = row_begin + rows
    model = 1 if row_begin > 0 else 0
    model_of = np.concatenate([np.zeros(row_begin, np.int32), np.full(rows, model, np.int32),
                               np.full(n_db - row_end, model + 1, np.int32)])
    xy = keypoints(rng, n)
    idx = np.full(CAP, row_begin, np.int32)          # behind the count: observations of the first row, if read
    d1 = np.full(CAP, 0.1, np.float32)
    d2 = np.ones(CAP, np.float32)
    kind = rng.random(CAP)
    for i in range(n):
        if kind[i] < share:
            idx[i] = row_begin + rng.integers(0, rows)
        elif kind[i] < share + 0.15:                 # the model's row, but MATCH does not accept: at and above the ratio
            idx[i] = row_begin + rng.integers(0, rows)
            d1[i] = rng.choice(np.array([0.8, 0.9], np.float32))
        elif kind[i] < share + 0.3 and n_db > rows:  # accepted, another model's row
            other = np.nonzero(model_of != model)[0]
            idx[i] = rng.choice(other)
        else:
            idx[i] = -1
    if per_row:
        # forced rows are nobody else's; their observations take the places given or random free ones
        taken = set()
        forced = set(per_row)
        for i in range(n):
            if idx[i] - row_begin in forced and d1[i] < f(0.5):
                idx[i] = -1
        for r, places in sorted(per_row.items(), key=lambda kv: isinstance(kv[1], int)):   # the given places first
            if isinstance(places, int):
                free = [i for i in rng.permutation(n) if i not in taken][:places]
                places = free
            for i in places:
                assert i < n and i not in taken
                taken.add(int(i))
                idx[i], d1[i] = row_begin + r, f(0.1)
                xy[i] = (f(0.25) + f(i % 10), f(0.5) + f((i // 10) % 8))   # a measured pixel
    if isinstance(views, str):
        views_in = rng.choice(np.array([1, 1, 2, 5, 1 << 24], np.int32), rows)
    else:
        views_in = views
    store_xyz = rng.uniform(-1.0, 1.0, (n_db, 3)).astype(np.float32)
    store_desc = unit(np.abs(rng.normal(size=(n_db, 128))))
    dup = dict(idx=idx, d1=d1, d2=d2, model_of=model_of, xyz=store_xyz, model=model, row_begin=row_begin, row_end=row_end)
    return dict(n=n, xy=xy, dup=dup, store_desc=store_desc, views_in=views_in, rows=rows)


def run(dev, sc, kw=KW, merged_cap=None, cap=CAP):
    """One call -> (merged_idx, merged_desc, merged_xyz, n_merged, views_out) as numpy, outputs pre-filled with sentinels."""
    c, torch, d, t = dev["c"], dev["torch"], dev["d"], dev["t"]
    dup, rows = sc["dup"], sc["rows"]
    merged_cap = rows if merged_cap is None else merged_cap
    xy_d = t(sc["xy"])
    n_d = torch.tensor([sc["n"]], dtype=torch.int32, device=d)
    arrs = [t(np.asarray(dup[k], ty)) for k, ty in (("idx", np.int32), ("d1", np.float32), ("d2", np.float32),
                                                     ("model_of", np.int32), ("xyz", np.float32))]
    dd = capi.mh_view_dup(*[a.data_ptr() for a in arrs], len(dup["model_of"]), dup["model"], dup["row_begin"], dup["row_end"])
    old_d = t(sc["store_desc"])
    vin_d = None if sc["views_in"] is None else t(np.asarray(sc["views_in"], np.int32))
    size = max(rows, 1) + 8
    mi = torch.full((size,), SENT_INT, dtype=torch.int32, device=d)
    md = torch.full((size, 128), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    mx = torch.full((size, 3), SENT_BITS, dtype=torch.int32, device=d).view(torch.float32)
    nm = torch.full((1,), SENT_INT, dtype=torch.int32, device=d)
    vo = torch.full((size,), SENT_INT, dtype=torch.int32, device=d)
    view = capi.make_view(dev["depth_d"].data_ptr(), None, POSE)
    torch.cuda.synchronize()
    c.view_merge_dev(dev["desc_d"].data_ptr(), dev["qn_d"].data_ptr(), xy_d.data_ptr(), n_d.data_ptr(), cap, view, W, H,
                     capi.make_view_spec(**kw), dd, old_d.data_ptr(), None if vin_d is None else vin_d.data_ptr(), mi.data_ptr(),
                     md.data_ptr(), mx.data_ptr(), merged_cap, nm.data_ptr(), vo.data_ptr())
    c.synchronize()
    return mi.cpu().numpy(), md.cpu().numpy(), mx.cpu().numpy(), int(nm.cpu()[0]), vo.cpu().numpy()


def expect(dev, sc, kw=KW, cap=CAP):
    n = max(0, min(sc["n"], cap))
    return mref.merge_view(sc["xy"][:cap], n, dev["depth"], None, POSE, kw, sc["dup"], dev["qn"], sc["store_desc"], sc["views_in"])


def check(got, want, rows, merged_cap=None, what=""):
    mi, md, mx, nm, vo = got
    why, xyz, (widx, ws, wp, wviews) = want
    cap = rows if merged_cap is None else merged_cap
    take = min(len(widx), cap)
    assert nm == len(widx), (what, nm, len(widx))
    assert np.array_equal(mi[:take], widx[:take]), what
    assert np.array_equal(bits(md[:take]), bits(ws[:take])), what
    assert np.array_equal(bits(mx[:take]), bits(wp[:take])), what
    assert np.array_equal(vo[:rows], wviews), what
    # nothing written past the count, the cap or the model's rows
    assert np.all(mi[take:] == SENT_INT) and np.all(bits(md[take:]) == SENT_BITS) and np.all(bits(mx[take:]) == SENT_BITS), what
    assert np.all(vo[rows:] == SENT_INT), what
    return why, widx


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048])
def test_lists_at_the_seams_against_a_model_in_the_middle_of_the_store(dev, n):
    sc = scene(0x100 + n, n, 1000, row_begin=700)
    want = expect(dev, sc)
    why, widx = check(run(dev, sc), want, 1000, what=n)
    if n >= 1023:   # merged, not accepted, another model's, dropped by an earlier rule: all live
        assert len(widx) > 300 and (why == ref.KEEP).sum() > 100 and (why == ref.PIXEL).sum() > 10 and (why == ref.DEPTH).sum() > 10
        obs = mref.observations(why, sc["dup"]["idx"], 700, 1700)
        assert max(len(o) for o in obs.values()) >= 3
    if n == 0:
        assert len(widx) == 0


@pytest.mark.parametrize("rows", [1, 64, 65, 1000, 1025])
def test_models_at_the_seams(dev, rows):
    # the whole store is the model; with one row every accepted keypoint observes it: hundreds of observations
    sc = scene(0x200 + rows, 2048, rows, row_begin=0, n_db=rows)
    want = expect(dev, sc)
    why, widx = check(run(dev, sc), want, rows, what=rows)
    assert len(widx) >= min(rows, 60)
    if rows == 1:
        assert (why == ref.DUP).sum() > 1000
    # without counts every row counts 1
    sc1 = dict(sc, views_in=None)
    check(run(dev, sc1), expect(dev, sc1), rows, what=(rows, "no counts"))


def test_observation_counts_and_chunk_straddles(dev):
    rows = 70
    per_row = {0: 130, 1: 0, 2: 1, 3: 2, 4: 63, 5: 64, 6: 65, 7: [63, 64], 8: [1023, 1024], 9: [0, 2047], 69: 2}
    views = np.ones(rows, np.int32)
    views[[0, 4, 7]] = 2
    views[[5, 8, 69]] = 1 << 24
    sc = scene(0x300, 2048, rows, row_begin=130, per_row=per_row, views=views, share=0.3)
    want = expect(dev, sc)
    why, widx = check(run(dev, sc), want, rows, what="counts")
    obs = mref.observations(why, sc["dup"]["idx"], 130, 200)
    for r, k in per_row.items():
        assert len(obs.get(r, [])) == (k if isinstance(k, int) else len(k)), r
    assert obs[7] == [63, 64] and obs[8] == [1023, 1024] and obs[9] == [0, 2047]
    assert 1 not in widx and widx[0] == 0 and widx[-1] == 69
    # the 130 observations of row 0 lie on both sides of the 1024 seam and in more than two 64-chunks
    assert min(obs[0]) < 1024 <= max(obs[0]) and len({i // 64 for i in obs[0]}) > 2
    assert want[2][3][69] == (1 << 24) + 1 and want[2][3][1] == 1
    # identical bytes on a second run
    a, b = run(dev, sc), run(dev, sc)
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a[:3] + a[4:], b[:3] + b[4:]))
    assert a[3] == b[3]


def test_rule_8_cuts_new_rows_and_not_observations(dev):
    sc = scene(0x400, 2048, 300, row_begin=50)
    kw = dict(KW, max_rows=10)
    want = expect(dev, sc, kw)
    why, widx = check(run(dev, sc, kw), want, 300, what="max_rows")
    tenth = np.nonzero(why == ref.KEEP)[0][9]
    assert ((why == ref.DUP) & (np.arange(len(why)) > tenth)).sum() > 100
    # the duplicate test off: nothing merges, the counts come back as they went in
    for off in (dict(merge_ratio=0.0, merge_dist=100.0), dict(merge_ratio=0.8, merge_dist=-1.0)):
        mi, md, mx, nm, vo = run(dev, sc, off)
        assert nm == 0 and np.all(mi == SENT_INT) and np.array_equal(vo[:300], sc["views_in"])
    # a list capacity below the count
    want = expect(dev, sc, cap=700)
    check(run(dev, sc, cap=700), want, 300, what="n > cap")


@pytest.mark.parametrize("merged_cap", [0, 5, 64])
def test_a_small_merged_cap_gets_the_full_count_and_no_row_beyond_it(dev, merged_cap):
    sc = scene(0x500, 1500, 200, row_begin=10)
    want = expect(dev, sc)
    why, widx = check(run(dev, sc, merged_cap=merged_cap), want, 200, merged_cap=merged_cap, what=merged_cap)
    assert len(widx) > 100


def test_bad_arguments_launch_nothing(dev):
    c, torch, d = dev["c"], dev["torch"], dev["d"]
    L = c.L
    sc = scene(0x600, 500, 100, row_begin=20)
    dup = sc["dup"]
    t = dev["t"]
    arrs = [t(np.asarray(dup[k], ty)) for k, ty in (("idx", np.int32), ("d1", np.float32), ("d2", np.float32),
                                                     ("model_of", np.int32), ("xyz", np.float32))]
    ok_dup = capi.mh_view_dup(*[a.data_ptr() for a in arrs], len(dup["model_of"]), dup["model"], 20, 120)
    xy_d, n_d, old_d = t(sc["xy"]), torch.tensor([500], dtype=torch.int32, device=d), t(sc["store_desc"])
    out = torch.full((1 << 16,), SENT_INT, dtype=torch.int32, device=d)
    p = out.data_ptr()
    ok_spec = capi.make_view_spec(**KW)
    ok_view = capi.make_view(dev["depth_d"].data_ptr(), None, POSE)
    base = dict(desc=dev["desc_d"].data_ptr(), qn=dev["qn_d"].data_ptr(), xy=xy_d.data_ptr(), n=n_d.data_ptr(), cap=CAP,
                view=ok_view, w=W, h=H, spec=ok_spec, dup=ok_dup, old=old_d.data_ptr(), vin=None, mi=p, md=p + 4096, mx=p + 65536,
                mcap=100, nm=p + 2048, vo=p + 3072)

    def call(**kw):
        a = dict(base, **kw)
        ref_ = lambda v: C.byref(v) if v is not None else None
        return L.mh_view_merge_dev(c.h, a["desc"], a["qn"], a["xy"], a["n"], a["cap"], ref_(a["view"]), a["w"], a["h"],
                                   ref_(a["spec"]), ref_(a["dup"]), a["old"], a["vin"], a["mi"], a["md"], a["mx"], a["mcap"],
                                   a["nm"], a["vo"])

    torch.cuda.synchronize()
    for k in ("desc", "qn", "xy", "n", "view", "spec", "dup", "old", "mi", "md", "mx", "nm", "vo"):
        assert call(**{k: None}) == -1, k
    assert "mh_view_merge_dev" in L.mh_last_error(c.h).decode()
    assert call(cap=0) == -1 and call(mcap=-1) == -1 and call(w=0) == -1 and call(h=-1) == -1
    assert call(qn=base["qn"] + 4) == -1 and call(old=base["old"] + 8) == -1 and call(md=p + 4096 + 4) == -1
    assert call(view=capi.make_view(None, None, POSE)) == -1
    pose = np.array(POSE)
    pose[2] = np.nan
    assert call(view=capi.make_view(dev["depth_d"].data_ptr(), None, pose)) == -1
    for bad in (dict(merge_ratio=float("nan")), dict(merge_dist=float("nan")), dict(max_rows=-1), dict(roi=(0.0, float("nan"), 1.0, 1.0))):
        assert call(spec=capi.make_view_spec(**bad)) == -1, bad
    assert call(dup=capi.mh_view_dup(*[a.data_ptr() for a in arrs], len(dup["model_of"]), dup["model"], 20, len(dup["model_of"]) + 1)) == -1
    assert call(dup=capi.mh_view_dup(arrs[0].data_ptr(), None, arrs[2].data_ptr(), arrs[3].data_ptr(), arrs[4].data_ptr(),
                                     len(dup["model_of"]), dup["model"], 20, 120)) == -1
    c.synchronize()
    assert bool((out == SENT_INT).all())   # the outputs were poisoned beforehand and are intact
    # ... and the same arguments, all good, do write
    assert call() == 0
    c.synchronize()
    assert int(out[512]) > 50 and int(out[0]) >= 0   # n_merged at p + 2048 bytes, merged_idx[0]
