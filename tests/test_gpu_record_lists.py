"""The counted record lists of the 16x16x32 MATCH launches on the device (csrc/screen_ab16.hip: the hand-over writes a
query's records from slot 0 and stores their count, pass B's wavefronts append theirs with one atomic add per record when
they write their parked hits out, pass C reads the count and 64 slots, the rest of a longer list in a second trip, and
searches a query whose list overflowed by brute force): (idx1, d1, d2) bit for bit those of match_kernel /
match_mfma_kernel (mh_match_set_mode 2 / 3) and of the oracle, on DBs built so that the rows that matter reach the list
through every writer, fill it past 64 records, past its capacity, and past a wavefront's park buffer.

Launch shapes: the smallest that take launch_passes16<4>, as tests/test_gpu_onesweep.py has them -- 16 384 queries x
32 768 .. 33 000 rows (every 8th tile sampled) and 32 768 queries x 16 384 .. 20 000 rows (every 4th).  The plan -- the
sampled tiles, pass B's splits -- is restated here and held against the library's own (mh_screen_launch_plan): a case
that no longer lands where it was built fails loudly.

How near a planted row is: _near(q, amp) leaves 1 - cos ~ 64 amp^2.  The threshold of a query lies one margin (~2.1e-3 of
the screen value for unit rows) below the second largest value pass A finds in its sample, so with two rows at amp 5e-3
(1 - cos ~ 1.6e-3) in sampled tiles every other row at amp <= 5e-3 is above the threshold (3.7e-3 below 1) and leaves a
record, and no unstructured row (cos ~ 0.64) does."""
import numpy as np
import pytest

import orclib
from moped_amd import capi

pytestmark = pytest.mark.gpu
TILE = 128
CAP = 288            # places in a query's list (SC_SLOT_PITCH)
PARK = 170           # hits a wavefront parks before it appends from the hit path (SC_RECBUF16)
SHAPE_8TH = (16384, 257 * TILE - 37)
SHAPE_4TH = (32768, 141 * TILE - 91)


def _plan(Q, N):
    """launch_passes16<4>'s plan, restated and asserted: sampled tiles, unsampled tiles, pass B's splits as [j0, j1) over the
    unsampled tiles."""
    n_tiles = -(-N // TILE)
    nqb = -(-Q // 1024)
    assert nqb >= 12 and n_tiles * nqb >= 4096, "not a launch_passes16<4> shape"
    every = 4 if n_tiles < 256 else 8
    assert n_tiles >= 4 * every
    n_sel = -(-n_tiles // every)
    first = max(0, min(every // 2, n_tiles - 1 - (n_sel - 1) * every))
    n_b = n_tiles - n_sel
    Sb, best = 1, 1e30
    for c in range(1, min(21, max(1, n_b // 8)) + 1):      # one workgroup per compute unit: least rounds x tiles, the larger of equals
        cost = -(-nqb * c // 256) * -(-n_b // c)
        if cost <= best:
            best, Sb = cost, c
    p = capi.screen_launch_plan(Q, N)
    assert p["onesweep"] == 1, p
    assert (p["tile_stride"], p["tile_first"], p["sampled_tiles"]) == (every, first, n_sel), (p, every, first, n_sel)
    assert (p["tiles_b"], p["splits_b"]) == (n_b, Sb), (p, n_b, Sb)
    sampled = [first + i * every for i in range(n_sel)]
    uns = [t for t in range(n_tiles) if t not in set(sampled)]
    base, rem = n_b // Sb, n_b % Sb
    splits = [(s * base + min(s, rem), s * base + min(s, rem) + base + (1 if s < rem else 0)) for s in range(Sb)]
    return sampled, uns, splits


def _search(c, torch, qn, mode, q_count=None):
    dev = torch.device("cuda:0")
    Q = qn.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(qn)).to(dev)
    with np.errstate(all="ignore"):
        qnorm = torch.from_numpy(orclib.row_norms(qn)).to(dev)
    out = [torch.empty(Q, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32)]
    c.match_set_mode(mode)
    if q_count is None:
        c.match_local_dev(tq.data_ptr(), qnorm.data_ptr(), Q, *[o.data_ptr() for o in out])
    else:
        n_dev = torch.tensor([q_count], dtype=torch.int32, device=dev)
        c.match_local_counted_dev(tq.data_ptr(), qnorm.data_ptr(), Q, n_dev.data_ptr(), 0, *[o.data_ptr() for o in out])
    c.synchronize()
    c.match_set_mode(-1)
    return [o.cpu().numpy() for o in out]


def _diff(a, b):
    return np.nonzero((a[0] != b[0]) | (a[1].view(np.uint32) != b[1].view(np.uint32)) |
                      (a[2].view(np.uint32) != b[2].view(np.uint32)))[0]


def _unit_rows(rng, n):
    return orclib.normalize(np.abs(rng.normal(size=(n, 128))).astype(np.float32))


def _near(rng, q, amp):
    return orclib.normalize(np.maximum(q + amp * rng.normal(size=q.shape), 0).astype(np.float32)[None])[0]


@pytest.fixture(scope="module")
def env():
    """One context; per shape the unstructured rows and queries, made once and left unchanged (the tests plant into copies)."""
    import torch
    c = capi.Context(0)
    base = {}

    def rows(shape):
        if shape not in base:
            rng = np.random.default_rng(shape[1])
            db, qn = _unit_rows(rng, shape[1]), _unit_rows(rng, shape[0])
            db.setflags(write=False)
            qn.setflags(write=False)
            base[shape] = (db, qn)
        return base[shape][0].copy(), base[shape][1].copy()

    yield c, torch, rows
    c.close()


def _upload(c, db, Q):
    n = len(db)
    c.db_upload(db, np.zeros(n, np.int32), np.zeros((n, 3), np.float32), 1)
    c.reserve(Q)
    assert c.match_stats(Q)["two_stage"]


def _run_and_check(c, torch, db, qn, planted=()):
    """Upload, search on the two-stage path, hold the bits against both exact kernels and (planted queries + a sample) the
    oracle.  Returns the result, the statistics and the number of incomplete queries of the two-stage launch."""
    _upload(c, db, len(qn))
    c.match_stats(reset=True)
    c.match_incomplete(reset=True)
    two = _search(c, torch, qn, 1)
    st = c.match_stats()
    inc = c.match_incomplete()
    valu = _search(c, torch, qn, 2)
    mfma = _search(c, torch, qn, 3)
    assert len(_diff(mfma, valu)) == 0
    bad = _diff(two, mfma)
    assert len(bad) == 0, (len(bad), bad[:10], two[0][bad[:10]], mfma[0][bad[:10]])
    pick = np.unique(np.concatenate([np.asarray(planted, np.int64)[:64], np.random.default_rng(1).choice(len(qn), 64, replace=False)]))
    oi, o1, o2 = orclib.match_2nn(db, qn[pick])
    assert len(_diff([x[pick] for x in two], [oi.astype(np.int32), o1, o2])) == 0
    assert st["queries"] == len(qn)
    return two, st, inc


@pytest.mark.parametrize("shape", [SHAPE_8TH, SHAPE_4TH])
def test_unstructured_rows(env, shape):
    c, torch, rows = env
    _plan(*shape)
    db, qn = rows(shape)
    two, st, inc = _run_and_check(c, torch, db, qn)
    print("unstructured", shape, "incomplete", inc, "candidate rows per query", st["candidates"] / st["queries"])
    assert st["brute_force_queries"] == 0, st
    assert inc <= len(qn) // 1000, inc


@pytest.mark.parametrize("shape", [SHAPE_8TH, SHAPE_4TH])
def test_every_writer_reaches_the_list(env, shape):
    """Query i has one row at amp 5e-3 in every (pass B split, quarter) and two in sampled tiles -- 4 Sb + 2 records from 4 Sb
    + 1 writers --, and of these rows number i is the nearest (1e-3) and number i + 7 the second (2e-3): a writer whose
    record did not reach the list loses the query whose nearest row it held.  One more query has exact copies of itself in
    all those places: the lowest row wins, d1 == d2."""
    c, torch, rows = env
    Q, N = shape
    sampled, uns, splits = _plan(Q, N)
    db, qn = rows(shape)
    rng = np.random.default_rng(11)
    W = 4 * len(splits) + 2
    used = set()

    def place(i, w):
        """Row of writer w for query i: (split, quarter) = divmod(w, 4), rows 16 ti + 4 quarter + k of a tile of the split; the
        last two writers are sampled tiles."""
        if w >= 4 * len(splits):
            t = sampled[(3 + 5 * (w - 4 * len(splits)) + i) % (len(sampled) - 1)]      # (not the last tile: it may be padded)
            r = t * TILE + (i * 8 + 3 + i // 16) % TILE
        else:
            s, quarter = divmod(w, 4)
            j0, j1 = splits[s]
            t = uns[j0 + i % (j1 - j0)]
            if t == -(-N // TILE) - 1:
                t = uns[j0]
            blk = i // (j1 - j0)                                  # a different 16-row group for queries that share a tile
            r = t * TILE + 16 * (blk % 8) + 4 * quarter + (i + w) % 4
        assert r < N and r not in used, (i, w, r)
        used.add(r)
        return r

    n_q = W + 1
    want = {}
    for i in range(n_q):
        where = [place(i, w) for w in range(W)]
        for w, r in enumerate(where):
            if i == W:
                db[r] = qn[i]
            else:
                db[r] = _near(rng, qn[i], 1e-3 if w == i else (2e-3 if w == (i + 7) % W else 5e-3))
        want[i] = where
    two, st, inc = _run_and_check(c, torch, db, qn, planted=range(n_q))
    for i in range(W):
        assert two[0][i] == want[i][i], (i, int(two[0][i]), want[i][i])
    assert two[0][W] == min(want[W]) and two[1][W] == two[2][W]
    assert st["brute_force_queries"] == 0, st


def test_more_than_64_records_fewer_than_the_capacity(env):
    """32 queries with 100 rows each inside the margin, in 100 different 8-row blocks of unsampled tiles, and two in sampled
    tiles: 102 records, the second trip.  The two nearest rows sit at places that differ from query to query, and the
    appends land in any order: a list read only up to 64 records loses some of them."""
    c, torch, rows = env
    Q, N = SHAPE_8TH
    sampled, uns, splits = _plan(Q, N)
    db, qn = rows(SHAPE_8TH)
    rng = np.random.default_rng(12)
    n_q, n_r = 32, 100
    assert 64 < n_r + 2 < CAP
    inner = [t for t in uns if t < -(-N // TILE) - 1]
    want = {}
    for i in range(n_q):
        # query i owns the 16-row group i % 8 ... of row block i // 8 of every tile it uses: no two queries share a block
        tiles = [inner[(7 * i + 2 * k) % len(inner)] for k in range(n_r)]
        assert len(set(tiles)) == n_r
        where = [t * TILE + 32 * (i // 8) + 16 * ((i // 4) % 2) + 4 * (i % 4) + k % 4 for k, t in enumerate(tiles)]
        a, b = (13 * i + 5) % n_r, (29 * i + 50) % n_r
        assert a != b
        for k, r in enumerate(where):
            db[r] = _near(rng, qn[i], 1e-3 if k == a else (2e-3 if k == b else 5e-3))
        for k in range(2):
            db[sampled[(2 * i + k) % (len(sampled) - 1)] * TILE + 64 + i] = _near(rng, qn[i], 5e-3)
        want[i] = where[a]
    two, st, inc = _run_and_check(c, torch, db, qn, planted=range(n_q))
    for i in range(n_q):
        assert two[0][i] == want[i], (i, int(two[0][i]), want[i])
    assert st["brute_force_queries"] == 0, st


def test_more_than_the_capacity_then_both_layouts_on_one_context(env):
    """Three queries with 400 exact copies each in 400 different blocks: their lists overflow, pass C searches exactly these
    three by brute force.  The launch after it on the same context (fresh queries) and a 3 000-query launch after that -- the
    32x32x16 passes, lane-private slots in the same memory -- must find every slot empty and every count zero.

    The three queries have eight non-zero coordinates each (cos ~ 0.25 with an unstructured row or query, where those have
    ~ 0.64 among themselves): 400 equal rows that came near ANOTHER query's threshold would overflow that query's list as
    well, and the count of brute-force searches would say nothing."""
    c, torch, rows = env
    Q, N = SHAPE_4TH
    sampled, uns, splits = _plan(Q, N)
    db, qn = rows(SHAPE_4TH)
    n_copies = 400
    assert n_copies > CAP
    inner = [t for t in uns if t < -(-N // TILE) - 1]
    qs = [5, 9000, Q - 1]
    lowest = {}
    for n, qi in enumerate(qs):
        v = np.zeros(128, np.float32)
        v[8 * n + 3:8 * n + 11] = 1.0 + 0.01 * np.arange(8)
        qn[qi] = orclib.normalize(v[None])[0]
        where = [inner[k % len(inner)] * TILE + 32 * (k // len(inner)) + 4 * n + 1 for k in range(n_copies)]
        assert len(set(where)) == n_copies and max(k // len(inner) for k in range(n_copies)) < 4
        db[where] = qn[qi]
        lowest[qi] = min(where)
    two, st, inc = _run_and_check(c, torch, db, qn, planted=qs)
    assert st["brute_force_queries"] == len(qs), st
    for qi in qs:
        assert two[0][qi] == lowest[qi] and two[1][qi] == two[2][qi]
    # fresh queries, the same context and DB
    fresh = _unit_rows(np.random.default_rng(13), Q)
    c.match_stats(reset=True)
    again = _search(c, torch, fresh, 1)
    st2 = c.match_stats()
    exact = _search(c, torch, fresh, 3)
    bad = _diff(again, exact)
    assert len(bad) == 0, (len(bad), bad[:10])
    assert st2["queries"] == Q and st2["brute_force_queries"] == 0, st2
    # ... and a launch of the other layout (a copy of the overflowing queries among its own)
    small = np.concatenate([fresh[:2997], qn[qs]])
    assert capi.screen_launch_plan(len(small), N)["onesweep"] == 0 and c.match_stats(len(small))["two_stage"]
    got = _search(c, torch, small, 1)
    bad = _diff(got, _search(c, torch, small, 3))
    assert len(bad) == 0, (len(bad), bad[:10])
    # ... and back
    bad = _diff(_search(c, torch, fresh, 1), exact)
    assert len(bad) == 0, (len(bad), bad[:10])


@pytest.mark.parametrize("shape,split", [(SHAPE_8TH, 3), (SHAPE_4TH, 0)])
def test_a_full_park_buffer(env, shape, split):
    """The 128 queries of one wavefront (wavefront 5 of the third 1 024-query workgroup) each have their two nearest rows
    inside the tiles of ONE pass B split: 256 hits in one wavefront's sweep against 170 places in its park buffer -- the
    rest is appended from the hit path."""
    c, torch, rows = env
    Q, N = shape
    sampled, uns, splits = _plan(Q, N)
    db, qn = rows(shape)
    rng = np.random.default_rng(14)
    q0 = 2 * 1024 + 5 * 128
    j0, j1 = splits[split]
    tiles = [t for t in uns[j0:j1] if t < -(-N // TILE) - 1]
    assert 2 * 128 > PARK and len(tiles) >= 2
    want, used = {}, set()
    for i in range(128):
        a = tiles[i % len(tiles)] * TILE + (3 * i) % TILE
        b = tiles[(i + 1) % len(tiles)] * TILE + (3 * i + 2) % TILE
        assert a not in used and b not in used and a != b
        used.update((a, b))
        db[a] = _near(rng, qn[q0 + i], 1e-3)
        db[b] = _near(rng, qn[q0 + i], 2e-3)
        want[q0 + i] = a
    two, st, inc = _run_and_check(c, torch, db, qn, planted=range(q0, q0 + 128))
    for qi, r in want.items():
        assert two[0][qi] == r, (qi, int(two[0][qi]), r)
    assert st["brute_force_queries"] == 0, st


def test_queries_that_leave_early(env):
    """A device-side count below the capacity, an all-zero query and non-finite ones among ordinary queries: no records, no
    count left behind -- the answers of the exact kernel, "no neighbour" behind the count, and the full launch after it exact."""
    c, torch, rows = env
    Q, N = SHAPE_8TH
    _plan(Q, N)
    db, qn = rows(SHAPE_8TH)
    qn[100] = 0
    qn[101] *= 1e6
    qn[102, 5] = np.inf
    qn[103, 7] = np.nan
    qn[104] *= 3.0
    _upload(c, db, Q)
    with np.errstate(all="ignore"):
        exact = _search(c, torch, qn, 3)
        n = 15001
        two = _search(c, torch, qn, 1, q_count=n)
        assert (two[0][n:] == -1).all() and np.isposinf(two[1][n:]).all() and np.isposinf(two[2][n:]).all()
        assert len(_diff([x[:n] for x in two], [x[:n] for x in exact])) == 0
        assert len(_diff(_search(c, torch, qn, 1), exact)) == 0


def test_order_does_not_matter(env):
    """The same launch twice: the appends of concurrent wavefronts land in another order, the bits are the same (and those of
    the exact kernel)."""
    c, torch, rows = env
    Q, N = SHAPE_4TH
    _plan(Q, N)
    db, qn = rows(SHAPE_4TH)
    _upload(c, db, Q)
    res, cand = [], []
    for _ in range(2):
        c.match_stats(reset=True)
        res.append(_search(c, torch, qn, 1))
        cand.append(c.match_stats()["candidates"])
    assert len(_diff(res[0], res[1])) == 0
    assert cand[0] == cand[1] > 0
    assert len(_diff(res[0], _search(c, torch, qn, 3))) == 0
