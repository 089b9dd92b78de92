"""Completeness of pass A's hand-over in the one-sweep MATCH launches (csrc/screen_ab16.hip, "pass A of the
one-sweep launches"), as a restatement in numpy against the direct definition.

A lane slot (split x quarter) of pass A folds the largest screen value of every 8-row block it sees into a sorted list
of the K = 4 largest PACKED values (the block's number in the low mantissa bits) plus the fifth largest;
screen_handover_kernel makes the query's threshold from the lists and turns every listed block above it into a record,
or marks the query incomplete for the lane slots whose fifth value is above it too.  What must hold:

    every block whose largest screen value exceeds tau is a record, or lies in a lane slot marked incomplete

whatever the values: ties, more than K hits in one slot, -inf blocks (padding rows), slots with fewer than K blocks.
The packing and its bound are the library's own host arithmetic (mh_screen_pack_value / mh_screen_pack_pert)."""
import numpy as np
import pytest

from moped_amd import capi

K = 4
FLOOR = np.float32(-1e38)


def _pack(v, blk, bits):
    return np.float32(capi.load().mh_screen_pack_value(np.float32(v), int(blk), int(bits)))


def _med3(a, b, c):
    return np.float32(sorted((a, b, c))[1])


def _lane_slot_list(values, bits):
    """The kernel's branch-free insertion, block by block: level k <- med3(level k - 1, level k, new), top <- max."""
    p = [np.float32(-np.inf)] * (K + 1)
    for blk, v in enumerate(values):
        m = _pack(max(np.float32(v), FLOOR), blk, bits)
        for k in range(K, 0, -1):
            p[k] = _med3(p[k - 1], p[k], m)
        p[0] = max(p[0], m)
    return p


def _handover(lists, pert, margin, bits, n_slots_cap=32):
    """screen_handover_kernel for one query: lists[ls] = the K + 1 values of lane slot ls = 4 split + quarter.
    Returns tau, the records {(ls, block)}, the incomplete (split mask, quarter mask)."""
    def val(ls, k):
        v = lists[ls][k]
        return np.float32(-np.inf) if v < np.float32(0.5) * FLOOR else v
    B = S = np.float32(-np.inf)
    for ls in range(len(lists)):
        p1, p2 = val(ls, 0), val(ls, 1)
        S = max(min(B, p1), max(S, p2))
        B = max(B, p1)
    tau = np.float32(np.float32(S - pert) - margin)
    recs, sm, qm = set(), 0, 0
    if not tau > -np.inf:
        return tau, None, (0, 0)      # pass B's lists overflow: brute force
    thr = np.float32(tau - pert)
    for ls in range(len(lists)):
        if val(ls, K) > thr:
            sm |= 1 << (ls >> 2)
            qm |= 1 << (ls & 3)
    full = False
    for ls in range(len(lists)):
        if (sm >> (ls >> 2)) & 1 and (qm >> (ls & 3)) & 1:
            continue
        for k in range(K):
            v = val(ls, k)
            if not v > thr:
                break
            if len(recs) == n_slots_cap:
                full = True
                break
            recs.add((ls, int(np.float32(v).view(np.uint32)) & ((1 << bits) - 1)))
        if full:
            break
    if full:
        recs, sm, qm = set(), (1 << (len(lists) // 4)) - 1, 0xF
    return tau, recs, (sm, qm)


def _check(table, bits=7, qq=1.0, dmax=1.0, cap=32):
    """table[ls] = the true block maxima of lane slot ls (float32, -inf allowed)."""
    L = capi.load()
    pert = np.float32(L.mh_screen_pack_pert(np.float32(qq), np.float32(dmax), bits))
    margin = np.float32(L.mh_screen_margin(np.float32(qq), np.float32(dmax)))
    lists = [_lane_slot_list(v, bits) for v in table]
    tau, recs, (sm, qm) = _handover(lists, pert, margin, bits, cap)
    allv = np.sort(np.concatenate([np.asarray(v, np.float64) for v in table]))[::-1]
    # the threshold's basis never exceeds the true second largest block maximum
    if len(allv) >= 2 and np.isfinite(allv[1]):
        assert float(tau) + float(margin) <= allv[1], (float(tau) + float(margin), allv[1])
    if recs is None:
        return tau, recs, (sm, qm)
    for ls, v in enumerate(table):
        swept = (sm >> (ls >> 2)) & 1 and (qm >> (ls & 3)) & 1
        for blk, x in enumerate(v):
            if np.float64(x) > np.float64(tau):
                assert swept or (ls, blk) in recs, (ls, blk, float(x), float(tau))
        if swept:
            assert not any(r[0] == ls for r in recs)    # a swept slot leaves no record: pass C sees its rows once
    # a record names a block that exists, and no block twice
    for ls, blk in recs:
        assert blk < len(table[ls])
    return tau, recs, (sm, qm)


def _random_table(rng, n_slots=20, n_blocks=80, hot=0):
    t = [rng.uniform(-0.45, 0.2, n_blocks).astype(np.float32) for _ in range(n_slots)]
    for _ in range(hot):
        t[rng.integers(n_slots)][rng.integers(n_blocks)] = np.float32(rng.uniform(0.3, 0.5))
    return t


@pytest.mark.parametrize("seed", range(20))
def test_random_tables(seed):
    rng = np.random.default_rng(seed)
    _check(_random_table(rng, hot=int(rng.integers(0, 12))))


def test_more_equal_maxima_in_one_lane_slot_than_it_keeps():
    rng = np.random.default_rng(1)
    for n_equal in (K, K + 1, K + 2, 9):
        t = _random_table(rng)
        t[5][rng.choice(80, n_equal, replace=False)] = np.float32(0.4)
        tau, recs, (sm, qm) = _check(t)
        if n_equal > K:
            assert (sm >> 1) & 1 and (qm >> 1) & 1      # lane slot 5 = split 1, quarter 1: incomplete
        else:
            assert sm == 0 and sum(1 for r in recs if r[0] == 5) == K


def test_all_hits_in_one_quarter():
    rng = np.random.default_rng(2)
    t = _random_table(rng)
    for split in range(5):
        t[4 * split + 2][rng.choice(80, 3, replace=False)] = rng.uniform(0.3995, 0.4, 3).astype(np.float32)   # (all within the margin of each other)
    tau, recs, (sm, qm) = _check(t)
    assert sm == 0 and len(recs) >= 15
    # ... and with six in every slot of that quarter: all of them incomplete, nothing else
    for split in range(5):
        t[4 * split + 2][rng.choice(80, 6, replace=False)] = np.float32(0.4)
    tau, recs, (sm, qm) = _check(t)
    assert sm == 0b11111 and qm == 0b0100


def test_padding_blocks_and_short_splits():
    rng = np.random.default_rng(3)
    t = _random_table(rng)
    t[19] = np.full(3, -np.inf, np.float32)                       # a lane slot of padding rows only, fewer than K blocks
    t[18] = np.array([0.41, -np.inf, 0.4], np.float32)            # fewer than K blocks, two of them hits
    t[17][10:] = -np.inf
    tau, recs, (sm, qm) = _check(t)
    assert (18, 0) in recs and (18, 2) in recs and not any(r[0] == 19 for r in recs)
    # nothing but padding anywhere: no threshold, no hand-over
    tau, recs, _ = _check([np.full(8, -np.inf, np.float32)] * 8)
    assert recs is None and tau == -np.inf


def test_more_records_than_slots_marks_everything():
    rng = np.random.default_rng(4)
    t = _random_table(rng)
    for ls in range(20):
        t[ls][:3] = np.float32(0.4)
    tau, recs, (sm, qm) = _check(t, cap=32)
    assert recs == set() and sm == 0b11111 and qm == 0xF


@pytest.mark.parametrize("bits", [2, 7, 10])
def test_negative_tiny_and_wide_identities(bits):
    rng = np.random.default_rng(bits)
    n_blocks = min(1 << bits, 300)
    t = [(-rng.uniform(0, 0.5, n_blocks) * 10.0 ** rng.uniform(-42, 0, n_blocks)).astype(np.float32) for _ in range(8)]
    t[3][: min(6, n_blocks)] = np.float32(-1e-40)                  # subnormal near-ties
    _check(t, bits=bits)


def _pass_b_walk(n_tiles, first, stride, n_splits):
    """screen16_kernel's pass B over the tiles pass A did not sample (skip_first + i * skip_stride), split by split: the
    one division in front of the loop, then the running tile number and the count-down to the next tile to jump over."""
    n_sel_a = -(-n_tiles // stride)
    n_sel = n_tiles - n_sel_a
    base, rem = n_sel // n_splits, n_sel % n_splits
    out = []
    for split in range(n_splits):
        sel_begin = split * base + min(split, rem)
        sel_end = min(sel_begin + base + (1 if split < rem else 0), n_sel)
        d = stride - 1
        if sel_begin < first:
            tile, gap = sel_begin, first - sel_begin
        else:
            jj = sel_begin - first
            tile, gap = sel_begin + 1 + jj // d, d - jj % d
        for _ in range(sel_begin, sel_end):
            out.append(tile)
            tile, gap = tile + 1, gap - 1
            if gap == 0:
                tile, gap = tile + 1, d
    return out


@pytest.mark.parametrize("stride", [2, 3, 4, 6, 8])
def test_pass_b_walks_exactly_the_unsampled_tiles(stride):
    for n_tiles in list(range(4 * stride, 4 * stride + 40)) + [782, 783, 7813]:
        n_sel_a = -(-n_tiles // stride)
        first = max(0, min(stride // 2, n_tiles - 1 - (n_sel_a - 1) * stride))      # launch_passes16's tile_first
        sampled = {first + i * stride for i in range(n_sel_a)}
        assert max(sampled) < n_tiles
        want = [t for t in range(n_tiles) if t not in sampled]
        for n_splits in (1, 2, 5, 16, 21):
            if n_splits <= len(want):
                assert _pass_b_walk(n_tiles, first, stride, n_splits) == want, (n_tiles, stride, n_splits)
