"""Pass C names the rows of a sampled tile's record itself (csrc/screen_rescore.hip, rescore_kernel / sample_pair_values):
screen_handover_kernel knows a block's packed maximum only, so its records say "all 8 rows", and pass C recomputes the 8
screen values of the records that survive its thinning -- by pass A's arithmetic -- and keeps the rows above tau.

Every case compares (idx1, d1, d2) as uint32 against the exact kernels (mh_match_set_mode 2 / 3) and the oracle, on DBs
built so that the mask decides: the two neighbours in ONE 8-row lane block (rows row0 + (b & 3) + 16 (b >> 2)), in two
blocks of one lane slot, a neighbour whose block's other seven rows are far away (the candidate rows of that query are
counted: mh_match_query_candidates), duplicates inside a block, the last, partly padded tile, and a block whose packed
maximum lies between tau - P and tau while none of its rows exceeds tau (an empty mask).  The values the mask is made
from are held against mh_screen_values(shape 2) bit for bit (mh_screen_sample_values).

Launch shapes and the restated plan: as tests/test_gpu_onesweep.py (the smallest launch_passes16<4> launches, every
stride and residue it walks)."""
import numpy as np
import pytest

import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
TILE = 128


def _plan(Q, N):
    """launch_passes16's sampling, restated: stride, sampled tiles, pass A splits -> [sel0, sel1), tiles, identity bits."""
    n_tiles = -(-N // TILE)
    assert -(-Q // 1024) >= 12 and n_tiles * -(-Q // 1024) >= 4096, "not a launch_passes16<4> shape"
    every = 4 if n_tiles < 256 else 8
    assert n_tiles >= 4 * every
    n_sel = -(-n_tiles // every)
    first = max(0, min(every // 2, n_tiles - 1 - (n_sel - 1) * every))
    p = capi.screen_launch_plan(Q, N)
    assert p["onesweep"] == 1, p
    assert (p["tile_stride"], p["tile_first"], p["sampled_tiles"]) == (every, first, n_sel), (p, every, first, n_sel)
    assert p["tiles_b"] == n_tiles - n_sel
    Sa = p["splits_a"]
    base, rem = n_sel // Sa, n_sel % Sa
    splits = [(s * base + min(s, rem), s * base + min(s, rem) + base + (1 if s < rem else 0)) for s in range(Sa)]
    sampled = [first + i * every for i in range(n_sel)]
    return every, sampled, splits, n_tiles, p["pack_bits"]


def _search(c, torch, qn, mode):
    dev = torch.device("cuda:0")
    Q = qn.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(qn)).to(dev)
    qnorm = torch.from_numpy(orclib.row_norms(qn)).to(dev)
    out = [torch.empty(Q, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.float32)]
    c.match_set_mode(mode)
    c.match_local_dev(tq.data_ptr(), qnorm.data_ptr(), Q, *[o.data_ptr() for o in out])
    c.synchronize()
    c.match_set_mode(-1)
    return [o.cpu().numpy() for o in out]


def _same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


@pytest.fixture(scope="module")
def env():
    import torch
    c = capi.Context(0)
    yield c, torch
    c.close()


def _unit_rows(rng, n):
    return orclib.normalize(np.abs(rng.normal(size=(n, 128))).astype(np.float32))


def _near(rng, q, amp):
    return orclib.normalize(np.maximum(q + amp * rng.normal(size=q.shape), 0).astype(np.float32)[None])[0]


def _row0(tile, rb, quarter):
    return tile * TILE + 32 * rb + 4 * quarter


def _block_rows(row0):
    """The 8 rows of a lane's block, by mask bit."""
    return [row0 + (b & 3) + 16 * (b >> 2) for b in range(8)]


def _far_rows(q, n):
    """n unit rows far from q: one coordinate each, where q is smallest (dot = that coordinate of q)."""
    out = np.zeros((n, 128), np.float32)
    out[np.arange(n), np.argsort(q)[:n]] = 1.0
    return out


def _build(rng, Q, N):
    every, sampled, splits, n_tiles, bits = _plan(Q, N)
    is_s = np.zeros(n_tiles, bool)
    is_s[sampled] = True
    uns = np.nonzero(~is_s)[0]
    db = _unit_rows(rng, N)
    qn = _unit_rows(rng, Q)
    cases, used = {}, set()

    def plant(name, qi, rows, amps):
        for r, a in zip(rows, amps):
            assert r < N and r not in used, (name, r)
            used.add(r)
            db[r] = qn[qi] if a == 0 else _near(rng, qn[qi], a)
        cases[name] = (qi, list(rows))

    def far_block(qi, row0, keep):
        rows = [r for b, r in enumerate(_block_rows(row0)) if b not in keep and r < N]
        assert not used.intersection(rows)
        used.update(rows)
        db[rows] = _far_rows(qn[qi], len(rows))

    s = sampled
    # first and second neighbour in the SAME 8-row lane block of a sampled tile (bits 1 and 6)
    b = _block_rows(_row0(s[5], 1, 2))
    plant("same block", 0, [b[1], b[6]], [2e-3, 4e-3])
    # ... the second neighbour the LOWER row of the block (bits 7 and 0)
    b = _block_rows(_row0(s[9], 3, 0))
    plant("same block, second below", 1, [b[7], b[0]], [2e-3, 4e-3])
    # the two neighbours in two blocks of one lane slot (pass A split 1, quarter 1)
    a0, _ = splits[1]
    plant("two blocks of a lane slot", 2, [_block_rows(_row0(s[a0], 0, 1))[2], _block_rows(_row0(s[a0], 3, 1))[5]], [2e-3, 4e-3])
    # a neighbour in a sampled block whose other seven rows are far below the threshold; the other neighbour unsampled
    r0 = _row0(s[3], 2, 3)
    plant("lonely best", 3, [_block_rows(r0)[5], uns[9] * TILE + 5], [2e-3, 4e-3])
    far_block(3, r0, {5})
    r0 = _row0(s[7], 0, 1)
    plant("lonely second", 4, [uns[20] * TILE + 77, _block_rows(r0)[0]], [2e-3, 4e-3])
    far_block(4, r0, {0})
    # both neighbours lonely, in two sampled blocks: every row above tau then lies in a sampled tile
    r0, r1 = _row0(s[2], 1, 0), _row0(s[10], 2, 2)
    plant("lonely pair", 5, [_block_rows(r0)[3], _block_rows(r1)[4]], [2e-3, 4e-3])
    far_block(5, r0, {3})
    far_block(5, r1, {4})
    # exact copies of the query inside one sampled block (bits 2 and 7): the lower row wins, d2 == d1
    b = _block_rows(_row0(s[6], 0, 0))
    plant("duplicates in a block", 6, [b[2], b[7]], [0, 0])
    # ... and copies in a sampled and in an unsampled block, the sampled one's row the higher
    plant("duplicate across", 7, [uns[2] * TILE + 9, _block_rows(_row0(s[8], 1, 1))[4]], [0, 0])
    # the last sampled tile (for some residues the DB's last, partly padded tile): its last real row, and another real
    # row of the same block if the block has one
    last = s[-1]
    n_real = min(N - last * TILE, TILE)
    rl = n_real - 1
    o = rl & 31
    blk = _block_rows(_row0(last, rl >> 5, (o & 15) >> 2))
    assert blk[(o & 3) + 4 * (o >> 4)] == last * TILE + rl
    others = [r for r in blk if r < N and r != last * TILE + rl]
    plant("last sampled tile", 8, [last * TILE + rl, others[0] if others else last * TILE + rl - 1], [2e-3, 4e-3])
    return db, qn, cases, (every, sampled, splits, n_tiles, bits)


def _run_and_check(c, torch, db, qn, cases, index_base=0):
    n = len(db)
    c.db_upload(db, np.zeros(n, np.int32), np.zeros((n, 3), np.float32), 1, index_base=index_base)
    c.reserve(len(qn))
    assert c.match_stats(len(qn))["two_stage"]
    c.match_stats(reset=True)
    two = _search(c, torch, qn, 1)
    st = c.match_stats()
    cand = c.match_query_candidates(16)
    valu = _search(c, torch, qn, 2)
    mfma = _search(c, torch, qn, 3)
    assert _same_bits(mfma, valu)
    bad = np.nonzero((two[0] != mfma[0]) | (two[1].view(np.uint32) != mfma[1].view(np.uint32)) |
                     (two[2].view(np.uint32) != mfma[2].view(np.uint32)))[0]
    names = {qi: name for name, (qi, _) in cases.items()}
    assert len(bad) == 0, (len(bad), [names.get(int(q), int(q)) for q in bad[:10]], two[0][bad[:10]], mfma[0][bad[:10]])
    pick = np.unique(np.concatenate([np.arange(16), np.random.default_rng(1).choice(len(qn), 112, replace=False)]))
    oi, o1, o2 = orclib.match_2nn(db, qn[pick])
    oi = np.where(oi >= 0, oi + index_base, -1).astype(np.int32)
    assert _same_bits([x[pick] for x in two], [oi, o1, o2])
    for name, (qi, rows) in cases.items():
        assert two[0][qi] - index_base in rows, (name, int(two[0][qi]), rows)
    for name in ("duplicates in a block", "duplicate across"):
        qi, rows = cases[name]
        assert two[0][qi] - index_base == min(rows) and two[1][qi] == two[2][qi], name
    assert st["queries"] == len(qn) and st["brute_force_queries"] == 0, st
    # The lonely neighbours: with "all 8 rows" their surviving sampled record alone is 8 candidate rows (9 or 16 with the
    # other neighbour).  Named by value it is the planted row -- the other seven are > 0.3 below a threshold that lies
    # 0.002 below the second neighbour; an unsampled block's mask may add a random row or two (pass B's superset).
    print("candidate rows of the planted queries:", {name: int(cand[qi]) for name, (qi, _) in cases.items()},
          "per query overall:", st["candidates"] / st["queries"])
    for name in ("lonely best", "lonely second"):
        assert 2 <= cand[cases[name][0]] <= 4, (name, cand[:16])
    # every row above tau in a sampled tile: the masks are exact, the two neighbours are all there is
    assert cand[cases["lonely pair"][0]] == 2, cand[:16]
    return two, st


@pytest.mark.parametrize("residue", range(8))
def test_mask_decides_every_8th_tile_sampled(env, residue):
    c, torch = env
    Q = 16384
    n_tiles = 256 + residue
    N = n_tiles * TILE - (0 if residue == 0 else 37)
    rng = np.random.default_rng(140 + residue)
    db, qn, cases, (every, sampled, splits, nt, bits) = _build(rng, Q, N)
    assert every == 8 and nt == n_tiles
    if residue == 5:
        assert sampled[-1] == n_tiles - 1 and N % TILE != 0      # the last, partly padded tile is sampled
    _run_and_check(c, torch, db, qn, cases)


@pytest.mark.parametrize("n_tiles", [128, 129, 130, 131, 255])
def test_mask_decides_every_4th_tile_sampled(env, n_tiles):
    c, torch = env
    Q = 32768
    N = n_tiles * TILE - (0 if n_tiles == 128 else 91)
    rng = np.random.default_rng(1000 + n_tiles)
    db, qn, cases, (every, sampled, splits, nt, bits) = _build(rng, Q, N)
    assert every == 4
    if n_tiles == 131:
        assert sampled[-1] == n_tiles - 1 and N % TILE != 0
    _run_and_check(c, torch, db, qn, cases)


def test_mask_with_index_base(env):
    c, torch = env
    Q, N = 16384, 259 * TILE - 5
    db, qn, cases, _ = _build(np.random.default_rng(17), Q, N)
    _run_and_check(c, torch, db, qn, cases, index_base=123456)


def test_mask_with_more_than_16_pass_a_splits(env):
    """12 query blocks: pass A runs 21 splits, and a thread of screen_handover_kernel holds two splits' lane slots."""
    c, torch = env
    Q, N = 12288, 344 * TILE - 37
    assert capi.screen_launch_plan(Q, N)["splits_a"] > 16
    db, qn, cases, _ = _build(np.random.default_rng(23), Q, N)
    _run_and_check(c, torch, db, qn, cases)


def test_mask_values_are_pass_a_values(env):
    """mh_screen_sample_values (the function rescore_kernel calls) against mh_screen_values(shape 2), bit for bit: blocks of
    every row block and quarter, pairs of different and of equal blocks, the partly padded last tile (-inf rows)."""
    c, torch = env
    Q, N = 16384, 261 * TILE - 37
    rng = np.random.default_rng(5)
    db = _unit_rows(rng, N)
    c.db_upload(db, np.zeros(N, np.int32), np.zeros((N, 3), np.float32), 1)
    nq = 64
    qn = _unit_rows(rng, nq)
    qn[3] = db[_block_rows(_row0(200, 1, 2))[6]]      # a query that IS a row
    vals, _, _ = c.screen_values(qn, 261 * TILE, shape=2)
    tiles = rng.integers(0, 261, size=(nq, 2))
    tiles[0] = (260, 260)
    tiles[1] = (0, 260)
    tiles[3] = (200, 200)
    rb, qu = rng.integers(0, 4, size=(nq, 2)), rng.integers(0, 4, size=(nq, 2))
    rb[0], qu[0] = (2, 2), (2, 3)                      # rows 72.., 76.. and 88.., 92.. of the last tile: real and padding rows
    rb[3], qu[3] = (1, 1), (2, 2)
    row0 = (tiles * TILE + 32 * rb + 4 * qu).astype(np.int32)
    got = c.screen_sample_values(qn, row0)
    for q in range(nq):
        for k in range(2):
            want = vals[q, _block_rows(int(row0[q, k]))]
            assert np.array_equal(got[q, k].view(np.uint32), want.view(np.uint32)), (q, k, row0[q, k], got[q, k], want)
    assert np.isneginf(got[0]).any() and np.isfinite(got[0]).any()


def test_record_with_an_empty_mask(env):
    """A block of a sampled tile whose packed maximum lies in (tau - P, tau] while none of its rows exceeds tau: the
    hand-over writes its record (it tests against tau - P), pass C's thinning keeps it (the query's two neighbours set the
    threshold themselves: both lie in sampled tiles) and the mask is empty.  Built from the hardware's own screen values
    (mh_screen_values) and the library's packing (mh_screen_pack_value): tau is restated here."""
    c, torch = env
    L = capi.load()
    Q, N = 16384, 256 * TILE
    rng = np.random.default_rng(77)
    every, sampled, splits, n_tiles, bits = _plan(Q, N)
    db = _unit_rows(rng, N)
    qn = _unit_rows(rng, Q)
    qi = 9
    q = qn[qi]
    r1, r2 = _row0(sampled[4], 1, 1), _row0(sampled[11], 2, 3)
    r3 = _row0(sampled[20], 0, 2)
    for r0 in (r1, r2, r3):
        db[_block_rows(r0)] = _far_rows(q, 8)
    row_b1, row_b2, row_b3 = _block_rows(r1)[2], _block_rows(r2)[5], _block_rows(r3)[1]
    db[row_b1] = _near(rng, q, 2e-3)
    db[row_b2] = _near(rng, q, 4e-3)

    def upload_and_tau():
        c.db_upload(db, np.zeros(N, np.int32), np.zeros((N, 3), np.float32), 1)
        vals, dmax, _ = c.screen_values(np.repeat(q[None], 32, 0), N, shape=2)
        v = vals[0]
        packed = {}
        for sp, (a0, a1) in enumerate(splits):
            for sel in range(a0, a1):
                for rb in range(4):
                    for qu in range(4):
                        r0 = _row0(sampled[sel], rb, qu)
                        m = max(np.float32(v[_block_rows(r0)].max()), np.float32(-1e38))
                        packed[r0] = np.float32(L.mh_screen_pack_value(m, (sel - a0) * 4 + rb, bits))
        S = np.sort(np.array(list(packed.values()), np.float32))[-2]
        qq = orclib.row_norms(q[None])[0]
        P = np.float32(L.mh_screen_pack_pert(qq, np.float32(dmax), bits))
        tau = np.float32(np.float32(S - P) - np.float32(L.mh_screen_margin(qq, np.float32(dmax))))
        return v, packed, tau, P

    v, packed, tau, P = upload_and_tau()
    assert packed[r2] == np.sort(np.array(list(packed.values()), np.float32))[-2]     # the second neighbour sets the threshold
    # the third row: largest value of its block inside (tau - P + the packing's reach, tau] -- a window of ~1e-6.  Coarse
    # search in an emulation of the screen value (f16 operands, float64 sum); then 8192 rows around the best one go to the
    # device as a DB of their own, which gives their screen values as the hardware accumulates them (a row's value does
    # not depend on where in a DB it lies); the one nearest the window's middle is planted and confirmed in place.
    reach = float(np.float32(abs(tau)) * np.float32(2.0 ** (bits - 23)))
    assert float(P) > 2.5 * reach
    mid = float(tau) - 0.5 * (float(P) - reach)
    qh = q.astype(np.float16).astype(np.float64)
    noise = rng.normal(size=128)

    def cand_rows(amps):
        return orclib.normalize(np.maximum(q[None] + amps[:, None] * noise[None], 0).astype(np.float32))
    amps = np.linspace(2e-3, 4e-2, 20000)
    rows = cand_rows(amps)
    emu = rows.astype(np.float16).astype(np.float64) @ qh - 0.5 * orclib.row_norms(rows).astype(np.float64)
    amp0 = amps[np.argmin(np.abs(emu - mid))]
    rows = cand_rows(np.linspace(0.98 * amp0, 1.02 * amp0, 8192))
    c.db_upload(rows, np.zeros(8192, np.int32), np.zeros((8192, 3), np.float32), 1)
    hw = c.screen_values(np.repeat(q[None], 32, 0), 8192, shape=2)[0][0]
    landed = False
    for j in np.argsort(np.abs(hw.astype(np.float64) - mid))[:4]:
        db[row_b3] = rows[j]
        v, packed, tau, P = upload_and_tau()
        thr = np.float32(tau - P)
        if thr < packed[r3] and v[_block_rows(r3)].max() <= tau:
            landed = True
            break
    assert landed, (mid, np.sort(np.abs(hw.astype(np.float64) - mid))[:4], float(tau), float(P))
    assert (v > tau).sum() == 2 and v[row_b1] > tau and v[row_b2] > tau          # nothing but the two neighbours above tau
    got = c.screen_sample_values(q[None], np.array([[r3, r1]], np.int32))
    assert (got[0, 0] <= tau).all() and (got[0, 1] > tau).sum() == 1
    c.reserve(Q)
    c.match_stats(reset=True)
    two = _search(c, torch, qn, 1)
    cand = c.match_query_candidates(16)
    one = _search(c, torch, qn, 3)
    assert _same_bits(two, one)
    oi, o1, o2 = orclib.match_2nn(db, qn[:16])
    assert _same_bits([x[:16] for x in two], [oi.astype(np.int32), o1, o2])
    assert two[0][qi] == row_b1
    assert cand[qi] == 2, cand[:16]      # the empty record names no row; the two neighbours' masks one each


def test_judged_launch_candidate_rows_and_incomplete_share():
    """bench.py's config-1 launch: same bits as the exact kernel, no brute-force search, at most 0.1 % of the queries in
    the bounded sweep (the cap of tests/test_gpu_onesweep.py); the candidate rows per query are printed."""
    import torch
    db = synth.make_db(20, 5000)
    dbn = orclib.normalize(db.desc)
    n_vis = (2, 2, 5, 1, 2, 3, 0, 2, 4, 2, 0, 1, 2, 2, 3, 2)
    frs = [synth.make_frame(db, n_vis=n, seed=200 + i, Q=3000) for i, n in enumerate(n_vis)]
    qn = np.concatenate([orclib.normalize(f.desc) for f in frs])
    assert capi.screen_launch_plan(len(qn), len(dbn))["onesweep"] == 1
    c = capi.Context(0)
    c.db_upload(dbn, db.model_of, db.xyz, db.n_models)
    c.reserve(len(qn))
    c.match_stats(reset=True)
    c.match_incomplete(reset=True)
    two = _search(c, torch, qn, 1)
    st = c.match_stats()
    inc = c.match_incomplete()
    one = _search(c, torch, qn, 3)
    c.close()
    print("judged launch: incomplete queries", inc, "of", len(qn), "candidate rows per query", st["candidates"] / st["queries"])
    assert _same_bits(two, one)
    assert st["queries"] == len(qn) and st["brute_force_queries"] == 0
    assert inc <= len(qn) // 1000, inc
