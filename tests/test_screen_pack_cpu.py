"""The packed identity of the one-sweep MATCH launches, checked in float64 (host arithmetic of the library, as
tests/test_screen_bound_cpu.py checks the margin).

Pass A replaces the low `bits` mantissa bits of a block's largest screen value by the block's number.  What the
exactness argument needs from that (csrc/match_screen.hip, csrc/screen.h):
  1. |packed - value| <= mh_screen_pack_pert(qq, Dmax, bits) for every screen value a query can have
     (|value| <= |q_h| |d_h| + dd / 2 + accumulation), negative and subnormal values included;
  2. hence T = (second largest packed value) - pert <= the second largest value over distinct blocks;
  3. the (lo, hi) pass C derives from a sampled block's record (f16 of packed - tau) bracket the block's value."""
import numpy as np
import pytest

import orclib
from moped_amd import capi, synth
import test_screen_bound_cpu as T


def _pert(qq, dmax, bits):
    return float(capi.load().mh_screen_pack_pert(np.float32(qq), np.float32(dmax), int(bits)))


def _pack(v, ids, bits):
    keep = np.uint32(~((1 << bits) - 1) & 0xFFFFFFFF)
    u = (np.asarray(v, np.float32).view(np.uint32) & keep) | (np.asarray(ids, np.uint32) & ~keep)
    return u.view(np.float32)


def test_python_packing_is_the_librarys():
    L = capi.load()
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 0.3, 200), [0.0, -0.0, 1e-40, -1e-40, -1e38, 3.0]]).astype(np.float32)
    for bits in (0, 2, 7, 10):
        ids = rng.integers(0, 1 << 10, len(v))
        mine = _pack(v, ids, bits)
        lib = np.array([L.mh_screen_pack_value(np.float32(x), int(i), bits) for x, i in zip(v, ids)], np.float32)
        assert np.array_equal(mine.view(np.uint32), lib.view(np.uint32))
        assert np.all(np.isfinite(mine))          # the floor -1e38 stays a finite number with any identity


@pytest.mark.parametrize("name,q,d", list(T._cases()), ids=[c[0] for c in T._cases()])
@pytest.mark.parametrize("bits", [2, 7, 10])
def test_perturbation_bound_on_real_screen_values(name, q, d, bits):
    dd = orclib.row_norms(d)
    dmax = float(np.sqrt(dd.max()))
    qq = (q.astype(np.float64) ** 2).sum(1)
    wt = T._screen_f32(q, d, dd)                                     # the screen values, f32
    rng = np.random.default_rng(bits)
    for ids in (np.zeros(wt.shape, np.uint32), np.full(wt.shape, (1 << bits) - 1, np.uint32),
                rng.integers(0, 1 << bits, wt.shape).astype(np.uint32)):
        pk = _pack(wt, ids, bits)
        err = np.abs(pk.astype(np.float64) - wt.astype(np.float64)).max(1)
        bound = np.array([_pert(x, dmax, bits) for x in qq])
        assert np.all(err <= bound), (name, bits, float((err / bound).max()))
    # the bound's premise: |value| <= W, with W = pert * 2^(23 - bits)
    W = np.array([_pert(x, dmax, 0) for x in qq]) * 2.0 ** 23
    assert np.all(np.abs(wt.astype(np.float64)).max(1) <= W)
    # and it is not a second margin: at the widest identity it stays below a tenth of the margin for unit rows
    if name == "sift-like unit rows":
        assert _pert(1.0, 1.0, 10) < 0.1 * T._margin(1.0, 1.0)
        assert _pert(1.0, 1.0, 7) < 0.02 * T._margin(1.0, 1.0)


def test_negative_and_subnormal_values():
    rng = np.random.default_rng(3)
    v = np.concatenate([-10.0 ** rng.uniform(-45, 0, 4000), 10.0 ** rng.uniform(-45, 0, 4000), [0.0, -0.0]]).astype(np.float32)
    v = v[np.abs(v) <= 1.5]
    for bits in (2, 7, 10):
        ids = rng.integers(0, 1 << bits, len(v)).astype(np.uint32)
        err = np.abs(_pack(v, ids, bits).astype(np.float64) - v.astype(np.float64))
        assert err.max() <= _pert(1.0, 1.0, bits)                   # W(1, 1) = 1.5: covers every |v| here
        # (relative to the value itself where it is normal: 2^(bits - 23))
        normal = np.abs(v) >= 1.2e-38
        assert np.all(err[normal] <= 2.0 ** (bits - 23) * np.abs(v[normal].astype(np.float64)))


def test_threshold_basis_stays_below_the_second_largest_value():
    rng = np.random.default_rng(4)
    for bits in (2, 7, 10):
        P = np.float32(_pert(1.0, 1.0, bits))
        for _ in range(200):
            v = rng.uniform(-0.5, 0.5, 64).astype(np.float32)
            v[rng.integers(64)] = v.max()                           # ties at the top as well
            pk = _pack(v, rng.permutation(64).astype(np.uint32), bits)
            t = np.float32(np.sort(pk)[-2] - P)
            assert float(t) <= float(np.sort(v)[-2])


def test_sample_record_bounds_bracket_the_blocks_value():
    L = capi.load()
    rng = np.random.default_rng(5)
    for bits in (7, 10):
        for qq, dmax in ((1.0, 1.0), (0.25, 3.0), (4.0, 0.5)):
            P = _pert(qq, dmax, bits)
            W = P * 2.0 ** (23 - bits)
            for _ in range(300):
                tau = np.float32(rng.uniform(-W, W))
                v = np.float32(tau + rng.choice([1e-7, 1e-5, 1e-3, 0.05, 0.5]) * rng.uniform(-0.2, 1) * W)
                v = np.float32(np.clip(v, -W, W))
                pk = _pack(np.array([v]), np.array([rng.integers(1 << bits)], np.uint32), bits)[0]
                bits16 = L.mh_screen_record_value(np.float32(pk), tau)      # f16(packed - tau), the kernel's expression
                lo, hi = capi.screen_sample_bounds(bits16, tau, P, dmax)
                assert lo <= float(v) <= hi, (bits, qq, dmax, float(tau), float(v), lo, hi)
                assert hi - lo <= 4 * P + 2.1e-3 * abs(float(pk) - float(tau)) + 1e-5 + 2e-6 * (abs(float(tau)) + dmax * dmax)


def test_launch_plan_of_the_judged_shapes():
    """bench.py's config 1 / config 2 launches: which tiles pass A samples and what is left for pass B."""
    p = capi.screen_launch_plan(48000, 100000)
    assert p == {"onesweep": 1, "tile_first": 4, "tile_stride": 8, "sampled_tiles": 98, "splits_a": 5, "pack_bits": 7,
                 "splits_b": 16, "tiles_b": 684}
    # 47 query blocks x 16 splits = 3 rounds of ceil(684 / 16) = 43 tiles: 129 tile steps per compute unit (147 with all 782)
    assert -(-p["tiles_b"] // p["splits_b"]) * -(-47 * p["splits_b"] // 256) == 129
    p2 = capi.screen_launch_plan(48000, 1000000)
    assert p2["onesweep"] == 1 and p2["pack_bits"] == 10 and p2["tiles_b"] == 7813 - 977
    assert capi.screen_launch_plan(3000, 100000)["onesweep"] == 0      # single frames stay on the 32x32x16 passes
    # fewer than 4 x stride tiles cannot occur on the 16x16x32 passes (they need >= 86 tiles); a sharded launch below 256
    # tiles samples every 4th
    p3 = capi.screen_launch_plan(96000, 15000)
    assert p3["onesweep"] == 1 and p3["tile_stride"] == 4
