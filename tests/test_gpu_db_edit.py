"""mh_db_splice: after any sequence of edits the resident store equals, byte for byte, the store mh_db_upload builds
from the same rows (tests/db_edit_ref.py is the numpy splice both sides start from).

Every comparison is array_equal on raw bytes over everything a fresh upload defines: rows [0, N) of xyz / model, the
whole padded extent of desc, norm, desc_h, neg_h, and ScreenDb's scalars as bit patterns."""
import numpy as np
import pytest

import db_edit_ref as ref
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
INSERT, REPLACE, REMOVE = capi.DB_INSERT, capi.DB_REPLACE, capi.DB_REMOVE
ARRAYS = ("desc", "norm", "xyz", "model", "desc_h", "neg_h")
# six models, 6 036 rows; no model boundary (701, 2200, 3135, 4238, 5015, 6036) on a multiple of 32 or 128
SIZES = (701, 1499, 935, 1103, 777, 1021)
assert all(b % 32 for b in np.cumsum(SIZES))


@pytest.fixture(scope="module")
def pool():
    """Normalised descriptor rows + coordinates to cut models from (computed once, never written)."""
    db = synth.make_db(1, 16000, seed=0xED17)
    d = orclib.normalize(db.desc)
    d.setflags(write=False)
    db.xyz.setflags(write=False)
    return d, db.xyz


@pytest.fixture(scope="module")
def base(pool):
    d, x = pool
    n = sum(SIZES)
    return (d[:n].copy(), x[:n].copy(), np.repeat(np.arange(len(SIZES), dtype=np.int32), SIZES), len(SIZES))


@pytest.fixture(scope="module")
def ctxs():
    """A: the context that is edited; F: the one that gets the fresh upload."""
    a, f = capi.Context(0), capi.Context(0)
    yield a, f
    a.close()
    f.close()


def rows_of(pool, first, n):
    d, x = pool
    return d[first:first + n], x[first:first + n]


def upload(c, db):
    c.db_upload(db[0], db[2], db[1], db[3])


def snapshot(c):
    out = {k: c.db_debug_fetch(k) for k in ARRAYS}
    out["screen"] = c.db_debug_screen()
    out["size"] = c.db_size()
    return out


def assert_same_store(a, f, db, what=""):
    """Context a's store == a fresh upload of `db` into context f, and a's model table == db's."""
    upload(f, db)
    got, want = snapshot(a), snapshot(f)
    assert got["size"] == want["size"] == (len(db[2]), db[3]), what
    assert got["screen"] == want["screen"], (what, got["screen"], want["screen"])
    n_pad = (len(db[2]) + 127) // 128 * 128
    assert want["desc"].size == n_pad * 128 and want["norm"].size == n_pad
    for k in ARRAYS:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)
    assert np.array_equal(got["model"], db[2]), what
    for m in range(db[3]):
        assert a.db_model_rows(m) == ref.model_rows(db, m), (what, m)
    return got


def edit(a, db, op, model, rows=None):
    """The same edit on the device and in numpy."""
    if op == REMOVE:
        a.db_splice(REMOVE, model)
        return ref.remove(db, model)
    a.db_splice(op, model, rows[0], rows[1])
    return ref.splice(db, op, model, rows[0], rows[1])


def queries(db, pool, models, seed):
    """2 048 normalised queries: clutter from the pool's tail + 200 perturbed copies of rows of `models`."""
    rng = np.random.default_rng([0xD8, seed])
    rows = np.nonzero(np.isin(db[2], models))[0]
    pick = rng.choice(rows, 200)
    near = np.maximum(db[0][pick] + rng.normal(0, 0.01, (200, 128)).astype(np.float32), 0)
    far = pool[0][14000 + rng.choice(2000, 1848, replace=False)] + rng.normal(0, 0.02, (1848, 128)).astype(np.float32)
    return orclib.normalize(np.ascontiguousarray(np.concatenate([near, np.maximum(far, 0)]), np.float32))


# ---- every position -----------------------------------------------------------------------------------------------
POSITION_EDITS = [
    ("insert-front", INSERT, 0, 333), ("insert-middle", INSERT, 3, 901), ("insert-end", INSERT, 6, 450),
    ("remove-first", REMOVE, 0, 0), ("remove-middle", REMOVE, 2, 0), ("remove-last", REMOVE, 5, 0),
    ("replace-fewer", REPLACE, 2, 200), ("replace-more", REPLACE, 4, 1300),
]


@pytest.mark.parametrize("name,op,model,n", POSITION_EDITS, ids=[e[0] for e in POSITION_EDITS])
@pytest.mark.parametrize("route", [0, 1], ids=["fused", "copies"])
def test_edit_at_every_position_equals_fresh_upload_and_searches_exactly(ctxs, base, pool, name, op, model, n, route):
    a, f = ctxs
    a.db_debug_route(route)
    try:
        upload(a, base)
        g0 = a.db_generation()
        db = edit(a, base, op, model, rows_of(pool, 7000, n))
        assert a.db_generation() == g0 + 1
    finally:
        a.db_debug_route(0)
    assert_same_store(a, f, db, name)
    # MATCH on the edited store: exact against the oracle on the numpy result, through the two-stage path
    near = [m for m in (model - 1, model, model + 1) if 0 <= m < db[3]]
    q = queries(db, pool, near, model)
    before = a.match_kernel_launches()["screen"]
    acc, raw, d1, d2 = a.match(q)
    assert a.match_kernel_launches()["screen"] == before + 1, "the two-stage path did not run on the edited store"
    oi, o1, o2 = orclib.match_2nn(db[0], q)
    assert np.array_equal(raw, oi) and np.array_equal(d1, o1) and np.array_equal(d2, o2)
    assert np.isin(db[2][raw[:200]], near).mean() > 0.9   # the perturbed copies find their models under the new numbering


def test_chain_of_seeded_edits_stays_equal_after_each_step(ctxs, base, pool):
    a, f = ctxs
    upload(a, base)
    db = base
    rng = np.random.default_rng(0xC4A1)
    for step in range(12):
        op = int(rng.integers(0, 3))
        n = int(rng.choice([0, 1, 127, 128, 700, 1500]))
        model = int(rng.integers(0, db[3] + (1 if op == INSERT else 0)))
        db = edit(a, db, op, model, rows_of(pool, int(rng.integers(6100, 12000)), n))
        assert_same_store(a, f, db, (step, op, model, n))
    assert a.db_generation() == 12


# ---- tile and image edges -----------------------------------------------------------------------------------------
def test_exact_multiple_of_128_rows(ctxs, base, pool):
    a, f = ctxs
    upload(a, base)
    n = 6144 - len(base[2])
    db = edit(a, base, INSERT, 2, rows_of(pool, 9000, n))
    assert len(db[2]) % 128 == 0
    assert_same_store(a, f, db)


def test_dropping_tiles_of_a_reused_buffer_leaves_no_stale_rows(base, pool):
    """Grow, then shrink inside reserved capacity: the sets take turns, so the one an edit fills held an older
    generation's rows beyond the new padded extent's last tile -- and inside it."""
    a, f = capi.Context(0), capi.Context(0)
    try:
        upload(a, base)
        a.db_reserve(8192, 16)
        assert a.db_generation() == 0
        assert_same_store(a, f, base, "reserve keeps the rows")
        db = edit(a, base, INSERT, 6, rows_of(pool, 8000, 500))      # 6 536 rows, 52 tiles
        assert_same_store(a, f, db, "grown")
        db = edit(a, db, REMOVE, 6)                                    # 6 036 rows: the set the base rows were in
        assert_same_store(a, f, db, "shrunk")
        db = edit(a, db, REPLACE, 1, rows_of(pool, 9000, 100))        # 4 637 rows, 37 tiles, in the set that held 6 536
        assert_same_store(a, f, db, "shrunk further")
        db = edit(a, db, INSERT, 0, rows_of(pool, 10000, 27))
        assert_same_store(a, f, db, "and up again")
    finally:
        a.close()
        f.close()


def test_f16_image_disappears_below_4096_rows_and_returns(ctxs, base, pool):
    a, f = ctxs
    upload(a, base)
    db = edit(a, base, REMOVE, 1)
    assert len(db[2]) == 4537 and assert_same_store(a, f, db)["screen"]["has_image"] == 1
    db = edit(a, db, REMOVE, 1)
    got = assert_same_store(a, f, db)
    assert len(db[2]) == 3602 and got["screen"]["has_image"] == 0 and got["desc_h"].size == 0
    q = queries(db, pool, [0, 1], 1)
    acc, raw, d1, d2 = a.match(q)
    oi, o1, o2 = orclib.match_2nn(db[0], q)
    assert np.array_equal(raw, oi) and np.array_equal(d1, o1) and np.array_equal(d2, o2)
    db = edit(a, db, INSERT, 2, rows_of(pool, 8000, 1200))
    assert len(db[2]) == 4802 and assert_same_store(a, f, db)["screen"]["has_image"] == 1


def test_down_to_one_row_to_zero_rows_and_up_again(ctxs, pool):
    a, f = ctxs
    d, x = rows_of(pool, 100, 6)
    db = (d.copy(), x.copy(), np.array([0, 1, 1, 1, 1, 1], np.int32), 2)
    upload(a, db)
    db = edit(a, db, REMOVE, 1)
    assert_same_store(a, f, db, "one row")
    acc, raw, d1, d2 = a.match(pool[0][:3])
    assert np.all(raw == 0) and np.all(np.isinf(d2))     # as test_empty_and_tiny_calls: one row, no second best
    db = edit(a, db, REMOVE, 0)
    assert_same_store(a, f, db, "zero rows")
    assert a.db_size() == (0, 0)
    acc, raw, d1, d2 = a.match(pool[0][:3])
    assert np.all(raw == -1) and np.all(acc == -1)
    db = edit(a, db, INSERT, 0, rows_of(pool, 200, 0))   # an empty model is a model
    assert_same_store(a, f, db, "one empty model")
    db = edit(a, db, INSERT, 1, rows_of(pool, 200, 300))
    assert_same_store(a, f, db, "up again")
    # a context that never had a store edits an empty one
    c = capi.Context(0)
    try:
        c.db_splice(INSERT, 0, *rows_of(pool, 300, 130))
        assert_same_store(c, f, ref.insert(ref.empty(), 0, *rows_of(pool, 300, 130)), "from nothing")
    finally:
        c.close()


def test_raw_rows_are_normalised_like_the_upload_path(ctxs):
    a, f = ctxs
    fx = synth.load_sift_fixture()[0]
    raw = np.ascontiguousarray(np.concatenate([fx, fx[:4500 - len(fx)] * np.float32(1.7)]), np.float32)   # 4 500 raw rows
    xyz = np.random.default_rng(3).standard_normal((4500, 3)).astype(np.float32)
    a.db_upload(np.zeros((0, 128), np.float32), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 0)
    a.db_splice(INSERT, 0, raw, xyz, normalize=True)
    f.L.mh_db_upload_raw(f.h, capi._ptr(raw), capi._ptr(np.zeros(4500, np.int32)), capi._ptr(xyz), 4500, 1, 0, 1)
    got, want = snapshot(a), snapshot(f)
    for k in ARRAYS:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert got["screen"] == want["screen"]
    assert np.array_equal(got["desc"][:4500 * 128].view(np.uint32), orclib.normalize(raw).ravel().view(np.uint32))


# ---- aggregates that must shrink ----------------------------------------------------------------------------------
def special_model(kind, pool):
    d, x = rows_of(pool, 12000, 300)
    d = d.copy()
    if kind == "dmax":
        d *= np.float32(3.0)          # raw rows at 3x norm own dmax
    elif kind == "zero":
        d[17] = 0                     # a zero row owns the zero query's answer
    elif kind == "nan":
        d[5, 40] = np.nan
    elif kind == "huge":
        d[5, 40] = 7e4                # beyond f16's range
    return d, x


@pytest.mark.parametrize("kind", ["dmax", "zero", "nan", "huge"])
@pytest.mark.parametrize("at", [0, 3, 6])
def test_removing_the_model_that_owns_an_aggregate(ctxs, base, pool, kind, at):
    a, f = ctxs
    plain = snapshot_of_fresh(f, base)
    with_it = ref.insert(base, at, *special_model(kind, pool))
    upload(a, with_it)
    got = snapshot(a)["screen"]
    if kind == "dmax":
        assert np.uint32(got["dmax_bits"]).view(np.float32) > 2.9 and got["usable"] == 1
    elif kind == "zero":
        assert got["zero_idx"] == ref.model_rows(with_it, at)[0] + 17 and got["zero_d1_bits"] == 0
    else:
        assert got["usable"] == 0
    db = edit(a, with_it, REMOVE, at)
    assert ref.same(db, base)
    after = assert_same_store(a, f, db, kind)["screen"]
    assert after == plain and after["usable"] == 1 and abs(np.uint32(after["dmax_bits"]).view(np.float32) - 1) < 1e-3
    # and the other way round: the edit that brings the model in ends as the upload of the result does
    db = edit(a, db, INSERT, at, special_model(kind, pool))
    assert assert_same_store(a, f, db, kind + " back")["screen"] == got


def snapshot_of_fresh(f, db):
    upload(f, db)
    return f.db_debug_screen()


# ---- refusals, not faults -----------------------------------------------------------------------------------------
def test_refusals_leave_the_store_as_it_was(base, pool):
    c = capi.Context(0)
    rows = rows_of(pool, 7000, 50)
    try:
        def refused(match, *args, **kw):
            before, gen = snapshot(c), c.db_generation()
            with pytest.raises(capi.MhError, match=match):
                c.db_splice(*args, **kw)
            after = snapshot(c)
            assert c.db_generation() == gen and after["screen"] == before["screen"] and after["size"] == before["size"]
            for k in ARRAYS:
                assert np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)), k

        refused("model index out of range .the store is empty", REMOVE, 0)          # no store at all
        c.db_upload(np.zeros((0, 128), np.float32), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 0)
        refused("model index out of range .the store is empty", REMOVE, 0)          # an empty one
        perm = base[2].copy()
        perm[[10, 3000]] = perm[[3000, 10]]
        c.db_upload(base[0], perm, base[1], base[3])
        refused("not grouped by model", INSERT, 0, *rows)
        with pytest.raises(capi.MhError, match="not grouped by model"):
            c.db_model_rows(1)
        with pytest.raises(capi.MhError, match="not grouped by model"):
            c.db_reserve(8192, 8)
        c.db_upload_blocks(base[0], base[2], base[1], base[3], [0, 9000], [2200, len(base[2]) - 2200])
        refused("uploaded in blocks", REMOVE, 1)
        c.db_upload(base[0], base[2], base[1], base[3], index_base=128)
        refused("index_base is not 0", REPLACE, 1, *rows)
        upload(c, base)
        refused("model index out of range", INSERT, 7, *rows)
        refused("model index out of range", INSERT, -1, *rows)
        refused("model index out of range", REPLACE, 6, *rows)
        refused("model index out of range", REMOVE, 6)
        refused("unknown operation", 3, 0, *rows)
        c.db_splice(REMOVE, 5)      # and the store is still editable
        assert c.db_size() == (len(base[2]) - SIZES[5], 5) and c.db_generation() == 1
    finally:
        c.close()


# ---- frames in flight keep their DB ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """Six models and a frame that sees model 3 (and another one)."""
    db = synth.make_db(6, 1100, seed=0xF11)
    for seed in range(64):
        fr = synth.make_frame(db, n_vis=2, seed=seed, Q=1500, pts_per_obj=140)
        if 3 in fr.visible and fr.visible.max() > 3:
            break
    else:
        raise AssertionError("no seed plants model 3 and a later model")
    dbn = orclib.normalize(db.desc)
    return db, dbn, fr


def run_frame(c, fr, seed=5, fetch=True):
    """Enqueue the frame on context c (its descriptors are normalised in place: a copy per run)."""
    import torch
    dev = torch.device("cuda:0")
    qd, quv = torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev)
    torch.cuda.synchronize()
    c.frame_enqueue(qd.data_ptr(), quv.data_ptr(), qd.shape[0], K, CAM0, capi.default_frame_params(), seed)
    hold = (qd, quv)
    if not fetch:
        return hold
    objs, counts = c.frame_fetch()
    return objs, counts


def same_objects(got, want):
    return np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()


def test_frames_in_flight_keep_their_db(scene):
    db, dbn, fr = scene
    full = (dbn, db.xyz, db.model_of, db.n_models)
    edited = ref.remove(full, 3)
    r, a, b = capi.Context(0), capi.Context(0), capi.Context(0)
    try:
        for c in (r, a, b):
            c.reserve(2048)
        upload(r, full)
        want_full = run_frame(r, fr)
        upload(r, edited)
        want_edited = run_frame(r, fr)
        later = int(fr.visible.max())
        assert sorted(set(want_full[0]["model"].tolist())) == [3, later]
        assert sorted(set(want_edited[0]["model"].tolist())) == [later - 1]    # no old model 3; later models renumbered

        upload(a, full)
        b.db_share(a)
        assert a.db_generation() == b.db_generation() == 0
        hold = run_frame(b, fr, fetch=False)      # in flight on B ...
        a.db_splice(REMOVE, 3)                    # ... while A edits, without synchronising B
        assert (a.db_generation(), b.db_generation()) == (1, 0)
        assert same_objects(b.frame_fetch(), want_full)
        assert same_objects(run_frame(a, fr), want_edited)
        assert b.db_size() == (db.n, 6) and a.db_size() == (db.n - 1100, 5)
        b.db_adopt(a)                             # no synchronize in between
        assert b.db_generation() == 1 and b.db_size() == a.db_size()
        assert same_objects(run_frame(b, fr), want_edited)
        # a second edit while B still holds generation 1
        a.db_splice(INSERT, 3, dbn[3300:4400], db.xyz[3300:4400])
        assert (a.db_generation(), b.db_generation()) == (2, 1)
        hold2 = run_frame(b, fr, fetch=False)
        b.db_adopt(a)                             # behind B's frame in flight on generation 1
        assert same_objects(b.frame_fetch(), want_edited)
        assert same_objects(run_frame(b, fr), want_full)
        del hold, hold2
    finally:
        for c in (b, a, r):
            c.close()


# ---- pipeline -----------------------------------------------------------------------------------------------------
def test_pipeline_add_and_remove_model(scene):
    import torch
    from moped_amd.pipeline import FramePipeline, ShardedDB
    db, dbn, fr = scene
    later = int(fr.visible.max())                 # the planted object that is added and removed again
    keep = db.model_of != later
    lo, hi = later * 1100, (later + 1) * 1100
    dev = torch.device("cuda:0")

    def sharded(mask):
        ids = np.cumsum(np.r_[True, np.diff(db.model_of[mask]) != 0]) - 1
        return ShardedDB(db.desc[mask], db.xyz[mask], ids.astype(np.int32), int(ids[-1]) + 1)

    def frames(pipe):
        out = []
        for slot in range(pipe.depth):
            pipe.enqueue(slot, torch.from_numpy(fr.desc).to(dev), torch.from_numpy(fr.uv).to(dev), seed=9)
        for slot in range(pipe.depth):
            out.append(pipe.fetch(slot))
        return out

    def scratch(mask):
        p = FramePipeline(0, sharded(mask), depth=1, max_queries=1500)
        try:
            return frames(p)[0]
        finally:
            p.close()

    want_without, want_with = scratch(keep), scratch(np.ones(db.n, bool))
    assert later not in want_without[0]["model"]
    # (the planted model moves to the end when it is added: index 5 in the edited pipeline)
    moved = np.r_[np.nonzero(keep)[0], np.arange(lo, hi)]
    want_moved = scratch_order(db, moved, frames, FramePipeline, ShardedDB)
    assert 5 in want_moved[0]["model"]
    pipe = FramePipeline(0, sharded(keep), depth=4, max_queries=1500, db_capacity=(8192, 8))
    try:
        assert all(same_objects(g, want_without) for g in frames(pipe))
        assert pipe.add_model(db.desc[lo:hi], db.xyz[lo:hi], name="planted") == 5
        got = frames(pipe)
        assert all(5 in g[0]["model"] for g in got) and all(same_objects(g, want_moved) for g in got)
        assert [c.db_generation() for c in pipe.ctxs] == [1] * 4 and pipe.db.n_models == 6
        assert pipe.add_model(db.desc[lo:hi], db.xyz[lo:hi], name="planted") == 5       # a known name replaces
        assert all(same_objects(g, want_moved) for g in frames(pipe))
        pipe.remove_model(5)
        assert all(same_objects(g, want_without) for g in frames(pipe))
        assert pipe.db.n_models == 5 and np.array_equal(pipe.db.desc, db.desc[keep])
    finally:
        pipe.close()
    sh = ShardedDB(db.desc, db.xyz, db.model_of, db.n_models, rank=0, world=2)
    with pytest.raises(ValueError):
        sh.splice(REMOVE, 0)


def scratch_order(db, order, frames, FramePipeline, ShardedDB):
    m = db.model_of[order]
    ids = (np.cumsum(np.r_[True, np.diff(m) != 0]) - 1).astype(np.int32)
    p = FramePipeline(0, ShardedDB(db.desc[order], db.xyz[order], ids, int(ids[-1]) + 1), depth=1, max_queries=1500)
    try:
        return frames(p)[0]
    finally:
        p.close()
