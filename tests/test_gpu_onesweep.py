"""The one-sweep MATCH launches on the device (csrc/screen_ab16.hip: pass A of the 16x16x32 passes keeps the identity
of its best blocks and hands the sampled tiles' records over, pass B leaves those tiles out): (idx1, d1, d2) bit for
bit those of match_kernel / match_mfma_kernel (mh_match_set_mode 2 / 3) and of the oracle, on DBs built so that the
rows that matter lie where the hand-over could lose them.

Launch shapes: launch_match_screen takes launch_passes16<4> from 12 query blocks of 1 024 queries and n_tiles x query
blocks >= 4 096; the smallest such launches keep the test short (16 384 queries x >= 256 tiles: every 8th tile
sampled; 32 768 queries x 128..255 tiles: every 4th).  Which tiles pass A samples is restated here from the row count
and held against the library's own plan (mh_screen_launch_plan): a case that no longer lands where it was built to
fails loudly."""
import numpy as np
import pytest

import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
TILE = 128


def _plan(Q, N):
    """launch_passes16's sampling, restated: (stride, first sampled tile, sampled tiles, pass A splits -> [sel0, sel1))."""
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
    return every, sampled, splits, n_tiles


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
    """Non-negative unit rows with no structure: every pair about equally far apart, so that the planted rows decide."""
    return orclib.normalize(np.abs(rng.normal(size=(n, 128))).astype(np.float32))


def _near(rng, q, amp):
    return orclib.normalize(np.maximum(q + amp * rng.normal(size=q.shape), 0).astype(np.float32)[None])[0]


def _build(rng, Q, N):
    """A DB of N unit rows and Q queries; the first queries have their nearest rows planted by position.
    Returns db, queries, {case name: (query index, planted rows)}."""
    every, sampled, splits, n_tiles = _plan(Q, N)
    is_s = np.zeros(n_tiles, bool)
    is_s[sampled] = True
    uns = np.nonzero(~is_s)[0]
    db = _unit_rows(rng, N)
    qn = _unit_rows(rng, Q)
    cases = {}
    used = set()

    def plant(name, qi, rows, amps):
        for r, a in zip(rows, amps):
            assert r < N and r not in used, (name, r)
            used.add(r)
            db[r] = qn[qi] if a == 0 else _near(rng, qn[qi], a)
        cases[name] = (qi, list(rows))

    s = sampled
    # the two nearest rows both in sampled tiles (different tiles, different quarters)
    plant("both sampled", 0, [s[3] * TILE + 17, s[7] * TILE + 101], [2e-3, 4e-3])
    # both in one 8-row block of a sampled tile: rows row0 + r and row0 + 16 + r of one quarter
    plant("one block", 1, [s[5] * TILE + 32 + 8 + 1, s[5] * TILE + 32 + 16 + 8 + 2], [2e-3, 4e-3])
    # one sampled, one not -- either way round
    plant("sampled best", 2, [s[2] * TILE + 64, uns[9] * TILE + 5], [2e-3, 4e-3])
    plant("sampled second", 3, [uns[20] * TILE + 77, s[6] * TILE + 3], [2e-3, 4e-3])
    def slot_rows(split, quarter, n):
        """One row in each of n different 8-row blocks of the lane slot (split, quarter): rows 16 i + 4 quarter .. + 3 of
        the split's sampled tiles, a block = those rows of one 32-row group."""
        a0, a1 = splits[split]
        blocks = [(sel, rb) for sel in range(a0, a1) for rb in range(4)]
        assert len(blocks) >= n, (split, a0, a1, n)
        return [s[sel] * TILE + rb * 32 + 16 * (k % 2) + 4 * quarter + (k % 4) for k, (sel, rb) in enumerate(blocks[:n])]
    # >= 6 near-ties inside the margin in ONE lane slot (pass A split 1, quarter 1): it keeps four blocks
    plant("near-ties in a lane slot", 4, slot_rows(1, 1, 6), [1e-5 * (k + 1) for k in range(6)])
    # ... and seven EXACT copies in one lane slot, an eighth in an unsampled tile before them: the lowest row wins
    lowest_uns = int(uns[uns < s[splits[2][0]]][-1]) * TILE + 90
    plant("copies in a lane slot", 5, [lowest_uns] + slot_rows(2, 2, 7), [0] * 8)
    # duplicates of the best row across a sampled and an unsampled tile, either order (lowest row wins)
    plant("duplicate, sampled first", 6, [s[1] * TILE + 50, uns[30] * TILE + 50], [0, 0])
    plant("duplicate, unsampled first", 7, [uns[2] * TILE + 9, s[8] * TILE + 9], [0, 0])
    # the first and the last sampled tile, the last rows of the DB
    plant("first sampled tile", 8, [s[0] * TILE + 0, s[0] * TILE + 127], [2e-3, 4e-3])
    plant("last rows", 9, [N - 1, N - 2], [2e-3, 4e-3])
    plant("last sampled tile", 10, [min(s[-1] * TILE + 1, N - 3), s[-2] * TILE + 120], [2e-3, 4e-3])
    # the tiles next to a sampled one (pass B's walk must neither skip nor repeat them)
    plant("neighbours of a sampled tile", 11, [(s[4] - 1) * TILE + 127, (s[4] + 1) * TILE + 0], [2e-3, 4e-3])
    plant("first and last unsampled tile", 12, [uns[0] * TILE + 1, min(uns[-1] * TILE + 2, N - 4)], [2e-3, 4e-3])
    return db, qn, cases, (every, sampled, n_tiles)


def _run_and_check(c, torch, db, qn, cases, index_base=0, want_incomplete=True):
    n = len(db)
    c.db_upload(db, np.zeros(n, np.int32), np.zeros((n, 3), np.float32), 1, index_base=index_base)
    c.reserve(len(qn))
    assert c.match_stats(len(qn))["two_stage"]
    c.match_stats(reset=True)
    c.match_incomplete(reset=True)
    two = _search(c, torch, qn, 1)
    st = c.match_stats()
    inc = c.match_incomplete()
    valu = _search(c, torch, qn, 2)
    mfma = _search(c, torch, qn, 3)
    assert _same_bits(mfma, valu)
    bad = np.nonzero((two[0] != mfma[0]) | (two[1].view(np.uint32) != mfma[1].view(np.uint32)) |
                     (two[2].view(np.uint32) != mfma[2].view(np.uint32)))[0]
    assert len(bad) == 0, (len(bad), bad[:10], two[0][bad[:10]], mfma[0][bad[:10]])
    # the oracle on the planted queries and a sample of the rest
    pick = np.unique(np.concatenate([np.arange(16), np.random.default_rng(1).choice(len(qn), 112, replace=False)]))
    oi, o1, o2 = orclib.match_2nn(db, qn[pick])
    oi = np.where(oi >= 0, oi + index_base, -1).astype(np.int32)
    assert _same_bits([x[pick] for x in two], [oi, o1, o2])
    # the cases landed where they were built to: the planted rows are what the search finds
    for name, (qi, rows) in cases.items():
        assert two[0][qi] - index_base in rows, (name, int(two[0][qi]), rows)
    for name in ("copies in a lane slot", "duplicate, sampled first", "duplicate, unsampled first"):
        qi, rows = cases[name]
        assert two[0][qi] - index_base == min(rows) and two[1][qi] == two[2][qi], name
    assert st["queries"] == len(qn) and st["brute_force_queries"] == 0, st
    if want_incomplete:
        assert inc >= 1, inc       # the near-ties and the copies overfill their lane slots: pass C's bounded sweep ran
    return st, inc


@pytest.mark.parametrize("residue", range(8))
def test_planted_neighbours_every_8th_tile_sampled(env, residue):
    """Tile counts of every residue mod the stride; residues 1..7 end in a partly padded tile, and for residue 5 that
    tile (number 260 = 4 + 32 x 8) is a sampled one."""
    c, torch = env
    Q = 16384
    n_tiles = 256 + residue
    N = n_tiles * TILE - (0 if residue == 0 else 37)
    rng = np.random.default_rng(40 + residue)
    db, qn, cases, (every, sampled, nt) = _build(rng, Q, N)
    assert every == 8 and nt == n_tiles
    if residue == 5:
        assert sampled[-1] == n_tiles - 1 and N % TILE != 0      # the last, partly padded tile is sampled
    _run_and_check(c, torch, db, qn, cases)


@pytest.mark.parametrize("n_tiles", [128, 129, 130, 131, 255])
def test_planted_neighbours_every_4th_tile_sampled(env, n_tiles):
    """A sharded launch's shape: fewer than 256 tiles, every 4th sampled -- the repeated share was a quarter."""
    c, torch = env
    Q = 32768
    N = n_tiles * TILE - (0 if n_tiles == 128 else 91)
    rng = np.random.default_rng(n_tiles)
    db, qn, cases, (every, sampled, nt) = _build(rng, Q, N)
    assert every == 4
    if n_tiles == 131:
        assert sampled[-1] == n_tiles - 1 and N % TILE != 0
    _run_and_check(c, torch, db, qn, cases)


def test_shard_with_index_base(env):
    c, torch = env
    Q, N = 16384, 259 * TILE - 5
    rng = np.random.default_rng(7)
    db, qn, cases, _ = _build(rng, Q, N)
    _run_and_check(c, torch, db, qn, cases, index_base=123456)


def test_queries_the_screen_cannot_vouch_for_and_short_frames(env):
    """Zero, huge and non-finite queries between ordinary ones at a one-sweep shape: no hand-over for them, the same
    answers as the exact kernels."""
    c, torch = env
    Q, N = 16384, 262 * TILE
    rng = np.random.default_rng(8)
    db, qn, cases, _ = _build(rng, Q, N)
    qn[100] = 0
    qn[101] *= 1e6
    qn[102, 5] = np.inf
    qn[103] *= 3.0
    n = len(db)
    c.db_upload(db, np.zeros(n, np.int32), np.zeros((n, 3), np.float32), 1)
    c.reserve(Q)
    two = _search(c, torch, qn, 1)
    one = _search(c, torch, qn, 3)
    assert _same_bits(two, one)


def test_judged_launch_incomplete_share_is_capped():
    """bench.py's config-1 launch (16 frames x 3 000 queries, the 20-model DB, as tests/test_gpu_judged_shape.py builds
    it): at most 0.1 % of the queries may take the bounded sweep, none the brute-force search; same bits as the exact
    kernel."""
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
